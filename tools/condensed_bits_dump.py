"""Every output of the cut cells' condensation and recovery (ifd_dense.hpp) on small cases the tests use, in one process, on the
library PA_LIB names (default: the shipped one), written to an .npz: cond, cond_cut, info, info_cut and the recovered vector of
  pa_fictdom_condensed_ops_batch / _recover     the seven CASES of tests/test_gpu_fictdom_condensed.py (the synthetic POSITIVE case
                                                included), recovery from a seeded random xF, on the line cases with both kinds of
                                                boundary data; the matrix with a failed pivot of test_a_failed_pivot_is_reported;
  pa_interface_condensed_ops_batch / _recover   the circle at (10, 0), (10, 1), (20, 1), (20, 2), the line level set at N = 12,
                                                k = 0..2, and face degree 3 on the mesh (N = 16) of the tests' synthetic case --
                                                not that case itself, whose random records reach only the CSR fill, but seeded
                                                positive definite operators, so that records and recovery run at that degree;
  pa_interface_rows_ops_batch / _recover        every slab of circle-12-thin (an empty slab, a one-row slab) and line-12 of
                                                tests/test_gpu_interface_rows.py, k = 0..2.
Two libraries compute the same bits if their files compare equal:
    PA_LIB=<library> python tools/condensed_bits_dump.py OUT.npz
    python tools/condensed_bits_dump.py --compare A.npz B.npz          (no GPU; one line per case; exit status 1 if a case differs)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FIELDS = ("cond", "cond_cut", "info", "info_cut", "recovered")
IF_CIRCLES = ((10, 0), (10, 1), (20, 1), (20, 2))
IF_LINE = dict(line_y=0.43)


def random_vector(n, seed, device):
    import torch
    gen = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(n, generator=gen, dtype=torch.float64) - 0.5).to(device)


def dump(out):
    import torch

    import proton_amd as pa
    import test_gpu_fictdom_condensed as F
    from interface_helpers import real_ops
    from proton_amd.batch import BatchAssembler
    from test_gpu_interface_rows import MESHES
    asm = BatchAssembler(0)
    res = {}
    empty = torch.empty(0, dtype=torch.float64)

    def put(name, rec, recovered):
        asm.synchronize()
        for f in FIELDS[:4]:
            res[name + "/" + f] = rec.get(f, empty).cpu().numpy()
        res[name + "/recovered"] = recovered.cpu().numpy()

    # ---- the fictitious domain: the cond of pa_fictdom_condensed_ops_batch holds the cut cells' rows (no cond_cut)
    for case in F.CASES:
        N, k, where, kw = case
        for g_kind in ("sol", "cos") if "line_y" in kw else ("sol",):
            asm.cut_preprocess(N, **kw)
            op = F.operators(asm, k, where, g_kind)
            xF = F.random_faces(asm, k, seed=17 + N + k)
            put("fictdom/%s-%s" % (F.case_id(case), g_kind), F.records(asm, k, where, op), F.recover(asm, k, where, op, xF))
    asm.cut_preprocess(10, refsteps=4)
    op = F.operators(asm, 1, F.NEG)
    op["cut_lc"] = op["cut_lc"].clone()
    op["cut_lc"][5, 2, 2] = -1.0
    put("fictdom/failed-pivot-10-k1", F.records(asm, 1, F.NEG, op), empty)

    # ---- the interface problem, whole mesh
    def interface(name, k, ops, g, seed):
        rec = asm.interface_condensed_ops(k, ops)
        xF = random_vector(asm.ctx.interface_condensed_query(k).system_size, seed, asm.device)
        put(name, rec, asm.interface_condensed_recover(k, ops, xF, g))

    for N, k in IF_CIRCLES:
        ops, g = real_ops(asm, N, k)
        interface("interface/circle-%d-k%d" % (N, k), k, ops, g, 17 + N + k)
    for k in (0, 1, 2):
        ops, g = real_ops(asm, 12, k, **IF_LINE)
        interface("interface/line-12-k%d" % k, k, ops, g, 29 + k)
    # face degree 3: the interface operators stop at 2.  The tests' case at this degree (synthetic_records(16, 3, seed=13)) holds
    # random records and reaches the CSR fill alone, so here seeded symmetric positive definite matrices (synthetic_spd of
    # tests/test_gpu_fictdom_condensed.py) stand in for the operators on that mesh: records and recovery run at degree 3
    N, k = 16, 3
    asm.cut_preprocess(N, refsteps=4)
    cbs, ms = (k + 3) * (k + 2) // 2, (k + 3) * (k + 2) // 2 + 4 * (k + 1)
    spd = lambda n, M, seed: torch.from_numpy(F.synthetic_spd(np.random.default_rng(seed), n, M)).to(asm.device)      # noqa: E731
    ops = {"lc": spd(asm.ncells, ms, 13), "rhs": random_vector(asm.ncells * cbs, 14, asm.device),
           "lc_cut": spd(asm.ncut, 2 * ms, 15), "rhs_cut": random_vector(asm.ncut * 2 * cbs, 16, asm.device)}
    interface("interface/synthetic-16-k3", k, ops, random_vector(2 * N * (N + 1) * (k + 1), 18, asm.device), 19)

    # ---- the interface problem by row slabs
    for mesh in ("circle-12-thin", "line-12"):
        N, bounds, kw = MESHES[mesh]
        for k in (0, 1, 2):
            for rows in zip(bounds[:-1], bounds[1:]):
                ops, g = real_ops(asm, N, k, rows=rows, **kw)
                i = asm.interface_rows_info(k)
                xF = random_vector(i.col_end - i.row_begin, 41 + k + rows[0], asm.device)
                put("rows/%s-k%d-rows%d-%d" % (mesh, k, rows[0], rows[1]), asm.interface_rows_ops(k, ops), asm.interface_rows_recover(k, ops, xF, g))
    np.savez(out, **res)
    print("%d cases written to %s (library %s)" % (len(res) // len(FIELDS), out, pa.capi.LIB_PATH))


def same_bits(x, y):
    """numpy.array_equal, and the same bits where it cannot tell: the NaNs behind a failed pivot, the sign of a zero"""
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() and np.array_equal(x, y, equal_nan=True)


def compare(argv):
    a, b = np.load(argv[0]), np.load(argv[1])
    assert sorted(a.files) == sorted(b.files), "the two files hold different cases"
    cases = sorted({k.rsplit("/", 1)[0] for k in a.files})
    bad = 0
    for c in cases:
        differ = [f for f in FIELDS if not same_bits(a[c + "/" + f], b[c + "/" + f])]
        bad += bool(differ)
        sizes = " ".join("%s %d" % (f, a[c + "/" + f].size) for f in FIELDS)
        nonzero = int(np.count_nonzero(a[c + "/info"])) + int(np.count_nonzero(a[c + "/info_cut"]))
        print("%-40s %s (%s; %d nonzero infos)" % (c, "DIFFERS in " + ", ".join(differ) if differ else "equal", sizes, nonzero))
    print("%d cases, %d differ" % (len(cases), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2:]))
    dump(sys.argv[1])
