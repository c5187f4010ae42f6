"""Every output of the two cut-cell kernels (cut_device.hpp, cut_interface_device.hpp) on small meshes the tests use, in one
process, on the library PA_LIB names (default: the shipped one), written to an .npz:
  pa_cut_local_ops_batch        the circle at (N, k, refsteps) = (10, 0, 4), (10, 1, 4), (20, 2, 4), (16, 1, 2), (12, 2, 5) -- the
                                last with more than 64 interface points per cell, the second chunk of the interface moments -- and
                                the line level sets (10, 1, 0.53), (12, 2, 0.47), (9, 0, 0.5); each on both sides; the output sets
                                all / lc + rhs / stab alone (the stabilization-only path of the interface problem) / data without
                                rhs; and pa_cut_rhs_sampled_batch with caller-sampled source and boundary values;
  pa_cut_interface_ops_batch    the (N, k, refsteps, kappa) of test_interface_operators_match_oracle and the line cases, with
                                oper and data and without (data to the context's scratch).
Two libraries compute the same bits if their files compare equal:
    PA_LIB=<library> python tools/cut_bits_dump.py OUT.npz
    python tools/cut_bits_dump.py --compare A.npz B.npz          (no GPU; one line per case; exit status 1 if a case differs)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CIRCLES = ((10, 0, 4), (10, 1, 4), (20, 2, 4), (16, 1, 2), (12, 2, 5))
LINES = ((10, 1, 0.53), (12, 2, 0.47), (9, 0, 0.5))
IF_CIRCLES = ((10, 0, 4, (1.0, 1.0)), (10, 1, 4, (1.0, 1.0)), (20, 2, 4, (1.0, 1.0)), (12, 1, 3, (1.0, 7.5)), (10, 2, 5, (2.0, 0.5)))
WANTS = (("all", ("oper", "data", "stab", "lc", "rhs", "info")), ("lc-rhs", ("lc", "rhs")), ("stab", ("stab",)), ("data", ("data", "info")))


def dump(out):
    import torch

    import proton_amd as pa
    from proton_amd.batch import BatchAssembler
    asm = BatchAssembler(0)
    res = {}

    def put(case, arrays):
        asm.synchronize()
        for name, t in arrays.items():
            res[case + "/" + name] = t.cpu().numpy()

    def one_sided(label, k):
        for where in (pa.capi.LOC_NEGATIVE, pa.capi.LOC_POSITIVE):
            for tag, want in WANTS:
                put("cut/%s-where%d-%s" % (label, where, tag), asm.cut_local_ops(k, where=where, want=want))
            # the built-in source and boundary functions sampled by the caller at the kernel's own points
            xyw0 = asm.ctx.cut_quadrature_points(k, where, 0)[1]
            off1 = asm.ctx.cut_quadrature_points(k, where, 1)[0]
            xyw2 = asm.ctx.cut_quadrature_points(k, where, 2)[1]
            f = torch.from_numpy(2 * np.pi ** 2 * np.sin(np.pi * xyw0[:, 0]) * np.sin(np.pi * xyw0[:, 1])).to(asm.device)
            b = torch.from_numpy(np.sin(np.pi * xyw2[:, 0]) * np.sin(np.pi * xyw2[:, 1])).to(asm.device)
            got = torch.empty((asm.ncut, (k + 3) * (k + 2) // 2), dtype=torch.float64, device=asm.device)
            asm.ctx.cut_rhs_sampled(k, asm.level_set, where, f.data_ptr(), b.data_ptr(), got.data_ptr())
            put("cut/%s-where%d-sampled" % (label, where), {"rhs": got})
            print("cut/%s where %d: %d cut cells, at most %d interface points per cell" % (label, where, asm.ncut, int(np.diff(off1).max())))

    def two_sided(label, k, kappa):
        for want_oper in (True, False):
            o = asm.interface_local_ops(k, kappa=kappa, want_oper=want_oper)
            put("interface/%s-%s" % (label, "oper" if want_oper else "lc"), {n: t for n, t in o.items() if n.endswith("_cut")})

    for N, k, r in CIRCLES:
        asm.cut_preprocess(N, refsteps=r)
        one_sided("circle-%d-k%d-r%d" % (N, k, r), k)
    for N, k, y in LINES:
        asm.cut_preprocess(N, line_y=y)
        one_sided("line-%d-k%d-y%g" % (N, k, y), k)
        two_sided("line-%d-k%d-y%g" % (N, k, y), k, (1.0, 1.0))
    for N, k, r, kappa in IF_CIRCLES:
        asm.cut_preprocess(N, refsteps=r)
        two_sided("circle-%d-k%d-r%d-kappa%g-%g" % (N, k, r, kappa[0], kappa[1]), k, kappa)
    np.savez(out, **res)
    print("%d cases, %d arrays written to %s (library %s)" % (len({n.rsplit("/", 1)[0] for n in res}), len(res), out, pa.capi.LIB_PATH))


def same_bits(x, y):
    """numpy.array_equal, and the same bits where it cannot tell: the NaNs behind a failed pivot, the sign of a zero"""
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() and np.array_equal(x, y, equal_nan=True)


def compare(argv):
    a, b = np.load(argv[0]), np.load(argv[1])
    assert sorted(a.files) == sorted(b.files), "the two files hold different cases"
    cases = sorted({n.rsplit("/", 1)[0] for n in a.files})
    bad = 0
    for c in cases:
        fields = sorted(n.rsplit("/", 1)[1] for n in a.files if n.rsplit("/", 1)[0] == c)
        differ = [f for f in fields if not same_bits(a[c + "/" + f], b[c + "/" + f])]
        bad += bool(differ)
        sizes = " ".join("%s %d" % (f, a[c + "/" + f].size) for f in fields)
        nonzero = sum(int(np.count_nonzero(a[c + "/" + f])) for f in fields if f.startswith("info"))
        print("%-52s %s (%s; %d nonzero infos)" % (c, "DIFFERS in " + ", ".join(differ) if differ else "equal", sizes, nonzero))
    print("%d cases, %d differ" % (len(cases), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2:]))
    dump(sys.argv[1])
