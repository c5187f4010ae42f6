"""Every output of the four conjugate-gradient entry points on the cases the tests use, in one process, on the library PA_LIB names
(default: the shipped one), written to an .npz: x, exit reason, iterations and relative residual of
  pa_conjugated_gradient       every case of tests/cg_twin.py (preconditioner on and off), iterates m = 1..8 through iterate_call;
  pa_conjugated_gradient_patch every case of tests/patch_pcg_twin.py, iterates m = 1..8 through iterate_call;
  pa_conjugated_gradient_rows  one rank, cg_twin's systems of 257, 4097 and 65537 rows (4097: a second trip of the one-block sum over
                               the SpMV partials; 65537: over the vector partials), the same iterates;
  pa_obstacle_block_solve      the meshes and active sets of tests/test_gpu_obstacle_solve.py (up to 48 x 48), face degrees 0 and 1.
Two libraries compute the same bits if their files compare equal:
    PA_LIB=<library> python tools/cg_bits_dump.py OUT.npz
    python tools/cg_bits_dump.py --compare A.npz B.npz [--skip C.npz D.npz]      (no GPU; one line per case; exit status 1 if a case differs)
--skip: the cases in which C and D differ -- two runs of one library -- are listed as not reproducible and not compared."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROWS_SIZES = (257, 4097, 65537)
FIELDS = ("x", "exit", "rr")


def dump(out):
    import torch

    import cg_twin as T
    import patch_pcg_twin as P
    import proton_amd as pa
    from proton_amd.batch import BatchAssembler
    from test_gpu_obstacle_solve import BLOCK_CASES, active_set
    asm = BatchAssembler(0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(asm.device)
    res = {}

    def put(name, x, reason, iters, rr):
        asm.synchronize()
        res[name + "/x"] = x.cpu().numpy()
        res[name + "/exit"] = np.array([reason, iters], dtype=np.int64)
        res[name + "/rr"] = np.array([rr], dtype=np.float64)

    for case in T.case_table():
        sy = T.system(case)
        dv = [dev(a) for a in (sy.rowptr, sy.colind, sy.values, sy.b)]
        for m in range(1, len(T.truth(case).rr) + 1):
            kw, _ = T.iterate_call(case, m)
            put("cg/%s/m%d" % (T.case_id(case), m), *asm.conjugated_gradient(*dv, precond=case.precond, **kw))
    for case in P.case_table():
        sy, pt = P.system(case), P.patches(case)
        dv, dp = [dev(a) for a in (sy.rowptr, sy.colind, sy.values, sy.b)], (dev(pt.ptr), dev(pt.rows))
        for m in range(1, len(P.truth(case).rr) + 1):
            kw, _ = P.iterate_call(case, m)
            put("patch/%s/m%d" % (P.case_id(case), m), *asm.conjugated_gradient_patch(*dv, dp, x=torch.full_like(dv[3], float("nan")), **kw))
    for case in [T.Case(n, precond, arrow) for n in ROWS_SIZES for arrow in (False, True) for precond in (True, False)]:
        sy = T.system(case)
        dv = [dev(a) for a in (sy.rowptr, sy.colind, sy.values, sy.b)]
        for m in range(1, len(T.truth(case).rr) + 1):
            kw, _ = T.iterate_call(case, m)
            x = torch.full_like(dv[3], float("nan"))
            r = asm.ctx.conjugated_gradient_rows(None, 0, case.n, *(t.data_ptr() for t in dv), x.data_ptr(), precond=case.precond, **kw)
            put("rows/%s/m%d" % (T.case_id(case), m), x, *r[:3])
    for Nx, Ny, kind in BLOCK_CASES:
        for fd in (0, 1):
            asm.generate_mesh(Nx, Ny, (-1.0, -1.0), (1.0, 1.0))
            lc = asm.local_ops(0, fd, pa.QUAD_TENSOR, pa.STAB_FANCY, want=("lc",))["lc"]
            rhs = asm.cell_rhs(0, pa.capi.FN_OBSTACLE_RHS, pa.QUAD_TENSOR, dinc=1)
            g = asm.dirichlet_data(fd, pa.capi.FN_OBSTACLE_SOL)
            gamma = dev(0.1 * np.random.default_rng(Nx + fd).standard_normal(asm.ncells))
            in_A = dev(active_set(Nx, Ny, kind).astype(np.uint8))
            A_ct, B_ct, num_I, num_A = asm.obstacle_tables(in_A)
            system = asm.obstacle_csr_assemble(fd, lc, rhs, g, gamma, in_A, A_ct, B_ct, num_I)
            put("obstacle/%dx%d-%s-fd%d" % (Nx, Ny, kind, fd), *asm.obstacle_block_solve(fd, *system, in_A, A_ct, B_ct, num_I))
    np.savez(out, **res)
    print("%d cases written to %s (library %s)" % (len(res) // len(FIELDS), out, pa.capi.LIB_PATH))


def differing(a, b):
    """the cases of two files in which an array of one is not numpy.array_equal to the other's"""
    assert sorted(a.files) == sorted(b.files), "the two files hold different cases"
    cases = sorted({k.rsplit("/", 1)[0] for k in a.files})
    return cases, {c for c in cases if not all(np.array_equal(a[c + "/" + f], b[c + "/" + f]) for f in FIELDS)}


def compare(argv):
    a, b = np.load(argv[0]), np.load(argv[1])
    skip = differing(np.load(argv[3]), np.load(argv[4]))[1] if len(argv) > 2 and argv[2] == "--skip" else set()
    cases, bad = differing(a, b)
    for c in cases:
        it = int(a[c + "/exit"][1])
        if c in skip:
            print("%-44s not reproducible between two runs of one library: left to the twin's gate" % c)
        else:
            print("%-44s %s (%d rows, exit %d after %d iterations)" % (c, "DIFFERS" if c in bad else "equal", a[c + "/x"].size, int(a[c + "/exit"][0]), it))
    bad -= skip
    print("%d cases, %d not reproducible, %d of the others differ" % (len(cases), len(skip), len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2:]))
    dump(sys.argv[1])
