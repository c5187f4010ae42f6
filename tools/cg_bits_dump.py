"""Every output of the conjugate-gradient entry points and of the preconditioners' table builders on the cases the tests use, in one
process, on the library PA_LIB names (default: the shipped one), written to an .npz: x, exit reason, iterations and relative residual of
  pa_conjugated_gradient       every case of tests/cg_twin.py (preconditioner on and off), iterates m = 1..8 through iterate_call;
  pa_conjugated_gradient_patch every case of tests/patch_pcg_twin.py, iterates m = 1..8 through iterate_call;
  pa_conjugated_gradient_rows  one rank, cg_twin's systems of 257, 4097 and 65537 rows (4097: a second trip of the one-block sum over
                               the SpMV partials; 65537: over the vector partials), the same iterates;
  pa_obstacle_block_solve      the meshes and active sets of tests/test_gpu_obstacle_solve.py (up to 48 x 48), face degrees 0 and 1;
  pa_conjugated_gradient_patch_coarse        every case of tests/coarse_twin.py, iterates m = 1..8 through iterate_call;
  pa_conjugated_gradient_rows_patch_coarse   no transport, the generic system of tests/rows_pcg_twin.py, both levels and patches only;
the status, the text of pa_last_error and x (untouched) of both of those on a refused patch table, a refused coarse table and an
indefinite patch (the defects of tests/test_gpu_coarse_pcg.py and tests/test_gpu_rows_pcg.py); and ptr, rows or cols, and vals of
  pa_condensed_patches, pa_condensed_coarse (one part and by side), pa_condensed_rows_patches, pa_condensed_rows_coarse,
  pa_interface_condensed_patches / _coarse, pa_interface_rows_patches / _coarse (one slab of the whole mesh, and the interior slab
  of three) on the smallest meshes of their tests.
Two libraries compute the same bits if their files compare equal:
    PA_LIB=<library> python tools/cg_bits_dump.py OUT.npz [--only GROUP,GROUP..]     (groups: the first word of a case's name)
    python tools/cg_bits_dump.py --compare A.npz B.npz [--skip C.npz D.npz]      (no GPU; one line per case; exit status 1 if a case differs)
--skip: the cases in which C and D differ -- two runs of one library -- are listed as not reproducible and not compared."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROWS_SIZES = (257, 4097, 65537)
GROUPS = ("cg", "patch", "rows", "obstacle", "coarse", "rowspc", "refused", "table")
IF_MESH = (12, ((0, 12), (3, 8)))          # circle-12 of tests/interface_rows_pcg_twin.py: the one slab, the interior slab of (0, 3, 8, 12)


def dump(out, only=GROUPS):
    import torch

    import cg_twin as T
    import coarse_twin as CT
    import patch_pcg_twin as P
    import proton_amd as pa
    import rows_pcg_twin as RT
    from proton_amd.batch import BatchAssembler
    from proton_amd.capi import ProtonAmdError
    from test_gpu_coarse_pcg import _bad_tables
    from test_gpu_obstacle_solve import BLOCK_CASES, active_set
    asm = BatchAssembler(0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(asm.device)
    res = {}

    def put(name, x, reason, iters, rr):
        asm.synchronize()
        res[name + "/x"] = x.cpu().numpy()
        res[name + "/exit"] = np.array([reason, iters], dtype=np.int64)
        res[name + "/rr"] = np.array([rr], dtype=np.float64)

    def put_table(name, a, t):
        a.synchronize()
        for f, v in zip(("ptr", "idx", "vals", "ncoarse"), t):
            res[name + "/" + f] = v.cpu().numpy() if hasattr(v, "cpu") else np.array([v], dtype=np.int64)

    def put_refusal(name, call, x):
        """a call that must fail: its status, the text of pa_last_error, and x as it was"""
        try:
            call()
            status, text = 0, ""
        except ProtonAmdError as e:
            status, text = e.status, str(e)
        asm.synchronize()
        res[name + "/x"] = x.cpu().numpy()
        res[name + "/status"] = np.array([status], dtype=np.int64)
        res[name + "/text"] = np.frombuffer(text.encode(), dtype=np.uint8)

    if "coarse" in only:
        for case in CT.case_table():
            sy, pt, tb = P.system(CT.base(case)), P.patches(CT.base(case)), CT.coarse(case)
            dv, dp = [dev(a) for a in (sy.rowptr, sy.colind, sy.values, sy.b)], (dev(pt.ptr), dev(pt.rows))
            dc = (dev(tb.ptr.astype(np.int64)), dev(tb.cols.astype(np.int32)), dev(tb.vals.astype(np.float64)), tb.ncoarse)
            for m in range(1, len(CT.truth(case).rr) + 1):
                kw, _ = CT.iterate_call(case, m)
                put("coarse/%s/m%d" % (CT.case_id(case), m),
                    *asm.conjugated_gradient_patch_coarse(*dv, dp, dc, x=torch.full_like(dv[3], float("nan")), **kw))
    if "rowspc" in only or "refused" in only:
        sy, n = RT.generic_system(), RT.CASE.n
        dv = [dev(a) for a in (sy.rowptr, sy.colind, sy.values, sy.b)]
        _, pt, tb = RT.generic_tables((0, n))
        dp = (dev(pt.ptr), dev(pt.rows))
        dc = (dev(tb.ptr.astype(np.int64)), dev(tb.cols.astype(np.int32)), dev(tb.vals.astype(np.float64)), tb.ncoarse)
    if "rowspc" in only:
        for coarse in (True, False):
            for m in range(1, len(RT.truth((0, n), coarse).rr) + 1):
                kw, _ = RT.iterate_call((0, n), m, coarse)
                put("rowspc/%s/m%d" % ("two-level" if coarse else "patches", m),
                    *asm.conjugated_gradient_rows_patch_coarse(None, 0, n, *dv, dp, dc if coarse else None, x=torch.full_like(dv[3], float("nan")), **kw))
    if "refused" in only:
        rows = dp[1].clone(); rows[5] = n                                # tests/test_gpu_coarse_pcg.py: a row outside the system
        bad = _bad_tables(tb)[1]                                        # a column = ncoarse
        dbad = (dev(bad[1].astype(np.int64)), dev(bad[2].astype(np.int32)), dev(bad[3].astype(np.float64)), bad[4])
        for what, v, p, c in (("patch-table", dv[2], (dp[0], rows), dc), ("coarse-table", dv[2], dp, dbad), ("indefinite-patch", -dv[2], dp, dc)):
            x = torch.full_like(dv[3], 7.0)
            put_refusal("refused/one-rank/" + what, lambda: asm.conjugated_gradient_patch_coarse(dv[0], dv[1], v, dv[3], p, c, x=x), x)
            x = torch.full_like(dv[3], 7.0)
            put_refusal("refused/rows/" + what, lambda: asm.conjugated_gradient_rows_patch_coarse(None, 0, n, dv[0], dv[1], v, dv[3], p, c, x=x), x)
        x = torch.full_like(dv[3], 7.0)
        put_refusal("refused/patch/indefinite-patch", lambda: asm.conjugated_gradient_patch(dv[0], dv[1], -dv[2], dv[3], dp, x=x), x)
    if "table" in only:
        for N, H, parts in ((4, 2, (0, 1, 2, 3, 4)), (9, 3, (0, 2, 5, 9))):       # tests/test_gpu_rows_pcg.py
            for k in (0, 2):
                w = BatchAssembler(0)
                w.generate_mesh(N, N)
                for kind in ("face", "cell"):
                    put_table("table/condensed_patches/%d-k%d-%s" % (N, k, kind), w, w.condensed_patches(k + 1, k, kind))
                put_table("table/condensed_coarse/%d-k%d-H%d" % (N, k, H), w, w.condensed_coarse(k + 1, k, H))
                for r0, r1 in zip(parts[:-1], parts[1:]):
                    a = BatchAssembler(0)
                    a.generate_mesh(N, N, rows=(r0, r1))
                    for kind in ("face", "cell"):
                        put_table("table/condensed_rows_patches/%d-k%d-%s-rows%d-%d" % (N, k, kind, r0, r1), a, a.condensed_rows_patches(k + 1, k, kind))
                    put_table("table/condensed_rows_coarse/%d-k%d-H%d-rows%d-%d" % (N, k, H, r0, r1), a, a.condensed_rows_coarse(k + 1, k, H))
        w = BatchAssembler(0)
        w.cut_preprocess(12, refsteps=3, line_y=0.47)                         # tests/test_gpu_coarse_pcg.py: line12
        for k in (0, 2):
            for H in (2, 4):
                for where in (0, 1):
                    put_table("table/condensed_coarse/line12-k%d-H%d-side%d" % (k, H, where), w, w.condensed_coarse(k + 1, k, H, "side", where))
        N, slabs = IF_MESH
        w = BatchAssembler(0)
        w.cut_preprocess(N)
        for k in (0, 2):
            for kind in ("face", "cell"):
                put_table("table/interface_condensed_patches/%d-k%d-%s" % (N, k, kind), w, w.interface_condensed_patches(k, kind))
            for H in (3, 4):
                for parts in ("one", "side"):
                    put_table("table/interface_condensed_coarse/%d-k%d-H%d-%s" % (N, k, H, parts), w, w.interface_condensed_coarse(k, H, parts))
        for r0, r1 in slabs:
            a = BatchAssembler(0)
            a.cut_preprocess(N, rows=(r0, r1))
            for k in (0, 2):
                for kind in ("face", "cell"):
                    put_table("table/interface_rows_patches/%d-k%d-%s-rows%d-%d" % (N, k, kind, r0, r1), a, a.interface_rows_patches(k, kind))
                for H in (3, 4):
                    for parts in ("one", "side"):
                        put_table("table/interface_rows_coarse/%d-k%d-H%d-%s-rows%d-%d" % (N, k, H, parts, r0, r1), a, a.interface_rows_coarse(k, H, parts))
    for case in T.case_table() if "cg" in only else ():
        sy = T.system(case)
        dv = [dev(a) for a in (sy.rowptr, sy.colind, sy.values, sy.b)]
        for m in range(1, len(T.truth(case).rr) + 1):
            kw, _ = T.iterate_call(case, m)
            put("cg/%s/m%d" % (T.case_id(case), m), *asm.conjugated_gradient(*dv, precond=case.precond, **kw))
    for case in P.case_table() if "patch" in only else ():
        sy, pt = P.system(case), P.patches(case)
        dv, dp = [dev(a) for a in (sy.rowptr, sy.colind, sy.values, sy.b)], (dev(pt.ptr), dev(pt.rows))
        for m in range(1, len(P.truth(case).rr) + 1):
            kw, _ = P.iterate_call(case, m)
            put("patch/%s/m%d" % (P.case_id(case), m), *asm.conjugated_gradient_patch(*dv, dp, x=torch.full_like(dv[3], float("nan")), **kw))
    for case in [T.Case(n, precond, arrow) for n in ROWS_SIZES for arrow in (False, True) for precond in (True, False)] if "rows" in only else ():
        sy = T.system(case)
        dv = [dev(a) for a in (sy.rowptr, sy.colind, sy.values, sy.b)]
        for m in range(1, len(T.truth(case).rr) + 1):
            kw, _ = T.iterate_call(case, m)
            x = torch.full_like(dv[3], float("nan"))
            r = asm.ctx.conjugated_gradient_rows(None, 0, case.n, *(t.data_ptr() for t in dv), x.data_ptr(), precond=case.precond, **kw)
            put("rows/%s/m%d" % (T.case_id(case), m), x, *r[:3])
    for Nx, Ny, kind in BLOCK_CASES if "obstacle" in only else ():
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
    print("%d cases written to %s (library %s)" % (len({k.rsplit("/", 1)[0] for k in res}), out, pa.capi.LIB_PATH))


def differing(a, b):
    """the cases of two files in which an array of one is not numpy.array_equal to the other's"""
    assert sorted(a.files) == sorted(b.files), "the two files hold different cases"
    cases = sorted({k.rsplit("/", 1)[0] for k in a.files})
    return cases, {c for c in cases if not all(np.array_equal(a[k], b[k]) for k in a.files if k.rsplit("/", 1)[0] == c)}


def describe(a, c):
    if c + "/exit" in a.files:
        return "%d rows, exit %d after %d iterations" % (a[c + "/x"].size, int(a[c + "/exit"][0]), int(a[c + "/exit"][1]))
    if c + "/status" in a.files:
        return "status %d, x as it was: %s; %s" % (int(a[c + "/status"][0]), bool((a[c + "/x"] == 7.0).all()), a[c + "/text"].tobytes().decode())
    return "%d rows or patches, %d entries" % (a[c + "/ptr"].size - 1, a[c + "/idx"].size) + \
        (", %d columns" % int(a[c + "/ncoarse"][0]) if c + "/ncoarse" in a.files else "")


def compare(argv):
    a, b = np.load(argv[0]), np.load(argv[1])
    skip = differing(np.load(argv[3]), np.load(argv[4]))[1] if len(argv) > 2 and argv[2] == "--skip" else set()
    cases, bad = differing(a, b)
    for c in cases:
        if c in skip:
            print("%-62s not reproducible between two runs of one library: left to the twin's gate" % c)
        else:
            print("%-62s %s (%s)" % (c, "DIFFERS" if c in bad else "equal", describe(a, c)))
    bad -= skip
    print("%d cases, %d not reproducible, %d of the others differ" % (len(cases), len(skip), len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2:]))
    dump(sys.argv[1], tuple(sys.argv[3].split(",")) if len(sys.argv) >= 4 and sys.argv[2] == "--only" else GROUPS)
