"""The double-double and cross-lane primitives of proton_amd/csrc/dd_arith.hpp, each on its own ON THE DEVICE, as the shipped flags
compile them (tests/hip/dd_probe.hip -> proton_amd/lib/probe/libpa_dd_probe.so, built by proton_amd/_build.py; nothing is compiled
here).  The cut-cell tests see these functions only end to end and on well-conditioned meshes: a primitive degraded from 1e-32 to
1e-20 -- both of the losses the header's comments record were of that kind -- passes there.

Every arithmetic op is held to its published bound against the exact result (fractions.Fraction; the square roots against 80-digit
mpmath) and, the sharp check, must equal tests/dd_twin.py's IEEE-strict restatement bit for bit, hi and lo, on every element: a
contraction or a reassociation changes bits long before it breaks a bound.  Bounds (u = 2^-53; Joldes, Muller, Popescu 2017):
dd_add / dd_sub 3u^2 + 13u^3 relative, dd_mul 7u^2, dd_mul_d 2u^2, dd_add_fast / dd_sub_fast 2^-104 (|a| + |b|) absolute (the
header's contract); two_sum, quick_two_sum, two_prod error-free with a correctly rounded hi.  The square roots: 8 x the twin's
worst relative error from seeds off by up to 2^-20, recomputed here from the twin on these inputs.

Measured on an MI355X (the flags of proton_amd/_build.py), 6144 elements per op, 2048 per square root; the device was
bit for bit the twin on every element of every op, so the twin's worst errors on these inputs are the same figures:
    op                       device worst            twin worst              bound
    two_sum / quick_two_sum  0 (error-free)          0                       0, hi correctly rounded
    two_prod                 0 (error-free)          0                       0, hi correctly rounded
    dd_add, dd_sub           1.28 u^2                1.28 u^2                3 u^2 + 13 u^3
    dd_add_fast, dd_sub_fast 0.321 x 2^-104 (|a|+|b|) 0.321 x                2^-104 (|a| + |b|)
    dd_mul                   3.04 u^2                3.04 u^2                7 u^2
    dd_mul_d                 1.11 u^2                1.11 u^2                2 u^2
    dd_round                 equal                   equal                   hi + lo in double
    dd_rsqrt                 2.57e-32                2.51e-32 (seeds 2^-20)  2.01e-31 = 8 x the twin's
    dd_rsqrt_1               4.71e-32                5.33e-32 (seeds 2^-20)  4.26e-31 = 8 x the twin's
(the hardware's seed was off by up to 4.5e-8 = 2^-24.4; from it the twin reproduces the device's square roots bit for bit).
lanes_transpose_reduce<N, 32>, N = 1, 2, 3, 5, 6, 7, 9, 10, 13, 15, 21, 28, 33, 64: double-double at most 0.063 of 7 x 2^-104 sum |v|,
double at most 0.32 of 7 u sum |v| and exact on integers, both bit for bit the restated butterfly; the lane moves bit-exact.
"""
import ctypes as C
import os

import numpy as np
import pytest

import dd_twin as T

pytestmark = pytest.mark.gpu

NWAVES = 8                       # two blocks of four waves


@pytest.fixture(scope="module")
def probe():
    import torch
    from proton_amd import _build
    assert torch.cuda.is_available()
    assert os.path.exists(_build.PROBE_LIB_PATH), "the build makes the probe library: no kernel is compiled by a test"
    lib = C.CDLL(_build.PROBE_LIB_PATH)
    lib.pa_probe_dd.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 7
    lib.pa_probe_transpose_reduce.argtypes = [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5
    lib.pa_probe_lane_moves.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 6
    for f in (lib.pa_probe_dd, lib.pa_probe_transpose_reduce, lib.pa_probe_lane_moves):
        f.restype = C.c_int
    return lib


def to_dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def run_dd(lib, op, a, b, d):
    """one launch of `op` over the pairs a, b and the doubles d: the device's list of pairs"""
    import torch
    n = len(a)
    cols = [to_dev(np.array(c, dtype=np.float64)) for c in ([x[0] for x in a], [x[1] for x in a], [x[0] for x in b], [x[1] for x in b], d)]
    oh, ol = (torch.full((n,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    st = lib.pa_probe_dd(T.OPS.index(op), n, *[t.data_ptr() for t in cols], oh.data_ptr(), ol.data_ptr())
    assert st == 0, "hipError_t %d" % st
    return list(zip(oh.cpu().tolist(), ol.cpu().tolist()))


@pytest.mark.parametrize("op", [op for op in T.OPS if op in T.BOUNDS] + ["dd_round"])
def test_arithmetic_op(probe, op):
    inp = T.binary_inputs()
    a, b = T.operands(op, inp)
    got = run_dd(probe, op, list(a), list(b), inp["d"])
    worst, bad = T.check(op, inp, got)
    diff = T.same_bits(got, T.run(op, inp))
    print("%s: device worst %.4f of its bound over %d elements; %d differ from the twin in a bit" % (op, worst, len(got), len(diff)))
    assert not bad, bad[:3]
    assert worst <= 1.0
    assert not diff, [(i, inp["a"][i], inp["b"][i], inp["d"][i], got[i]) for i in diff[:3]]


@pytest.mark.parametrize("op", ["dd_rsqrt", "dd_rsqrt_1"])
def test_reciprocal_square_root(probe, op):
    inp = T.rsqrt_inputs()
    a = inp["a"]
    seeds = [s for s, _ in run_dd(probe, "rsq_seed", a, a, [0.0] * len(a))]
    got = run_dd(probe, op, a, a, [0.0] * len(a))
    bar, twin_worst = T.rsqrt_bar(op)
    worst = max(T.rsqrt_errors(inp, got))
    with T.mp.workdps(80):
        seed_worst = max(float(abs(T.mp.mpf(s) * T.mp.sqrt(T.mp.mpf(x[0])) - 1)) for s, x in zip(seeds, a))
    diff = T.same_bits(got, T.run(op, inp, seeds=seeds))
    print("%s: device worst relative error %.3g (hardware seed off by up to %.3g), twin from emulated seeds %.3g, bar %.3g; %d differ "
          "from the twin started from the device's seed" % (op, worst, seed_worst, twin_worst, bar, len(diff)))
    assert seed_worst <= T.RSQRT_SEED_SPREAD            # the emulation drew seeds at least as bad as the hardware's
    assert all(g[0] == g[0] + g[1] for g in got)
    assert worst < bar
    assert not diff, [(i, a[i], seeds[i], got[i]) for i in diff[:3]]


# ---- lanes_transpose_reduce ---------------------------------------------------------------------------------------------------------
def transpose_inputs(n):
    """v[wave][lane][m], pairs: waves 0-1 general values of every scale and sign, 2-3 neighbouring lanes that cancel to 2^-10 .. 2^-70
    (b = -a (1 + delta)), 4 a single lane that holds anything, 5 neighbouring lanes with opposite hi and unrelated lo, 6-7
    integers below 2^20"""
    inp = T.binary_inputs()
    by_cls = {c: [(x, y) for x, y, k in zip(inp["a"], inp["b"], inp["cls"]) if k == c] for c in (1, 2, 3)}
    rng = np.random.default_rng(1000 + n)
    v = []
    for w in range(NWAVES):
        rows = [[(0.0, 0.0)] * n for _ in range(64)]
        for l in range(64):
            for m in range(n):
                k = (w * 4099 + l * 67 + m * 131)
                if w < 2:
                    rows[l][m] = by_cls[1][k % 1024][l & 1]
                elif w < 4:
                    rows[l][m] = by_cls[2][(w * 331 + (l // 2) * 64 + m) % 1024][l & 1]
                elif w == 4:
                    if l == (7 * n) % 64:
                        rows[l][m] = by_cls[1][k % 1024][0]
                elif w == 5:
                    rows[l][m] = by_cls[3][((l // 2) * 64 + m) % 1024][l & 1]
                else:
                    rows[l][m] = (float(rng.integers(-2 ** 20 + 1, 2 ** 20)), 0.0)
        v.append(rows)
    return v


@pytest.mark.parametrize("is_dd", [True, False], ids=["dd", "double"])
@pytest.mark.parametrize("n", T.TRANSPOSE_COUNTS)
def test_transpose_reduce(probe, n, is_dd):
    import torch
    v = transpose_inputs(n)
    if not is_dd:
        v = [[[(x[0], 0.0) for x in row] for row in wave] for wave in v]
    flat = np.array(v, dtype=np.float64)                                     # [wave][lane][m][2]
    dev_in = to_dev(flat if is_dd else flat[..., 0])
    nt = NWAVES * 64
    idx, okt = (torch.full((nt,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    oh, ol = (torch.full((nt,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    st = probe.pa_probe_transpose_reduce(n, int(is_dd), NWAVES, dev_in.data_ptr(), idx.data_ptr(), okt.data_ptr(), oh.data_ptr(), ol.data_ptr())
    assert st == 0, "hipError_t %d" % st
    idx, okt = idx.cpu().numpy().reshape(NWAVES, 64), okt.cpu().numpy().reshape(NWAVES, 64)
    oh, ol = oh.cpu().numpy().reshape(NWAVES, 64), ol.cpu().numpy().reshape(NWAVES, 64)

    # (index, ok) is the lane's alone: the restated bookkeeping's, in every wave of every block
    add = T.dd_add_fast if is_dd else (lambda x, y: (x[0] + y[0], 0.0))
    want_idx, want_ok, _ = T.lanes_transpose_reduce([[0] * n] * 64, n, 32, lambda x, y: 0, 0)
    for w in range(NWAVES):
        assert idx[w].tolist() == want_idx and okt[w].tolist() == [int(o) for o in want_ok], w
    assert sorted(set(i for i, o in zip(want_idx, want_ok) if o)) == list(range(n))
    worst = 0.0
    for w in range(NWAVES):
        _, _, twin = T.lanes_transpose_reduce(v[w], n, 32, add, (0.0, 0.0))
        for m in range(n):
            lanes = [l for l in range(64) if want_ok[l] and want_idx[l] == m]
            assert lanes
            got = (float(oh[w, lanes[0]]), float(ol[w, lanes[0]]))
            for l in lanes:                                                  # all of them store to one address in cut_device.hpp
                assert T.bits(float(oh[w, l])) == T.bits(got[0]) and T.bits(float(ol[w, l])) == T.bits(got[1]), (w, m, l)
            want = sum((T.exact(v[w][l][m]) for l in range(64)), T.F(0))
            mass = sum((abs(T.exact(v[w][l][m])) for l in range(64)), T.F(0))
            err = abs(T.exact(got) - want)
            if not is_dd and w >= 6:
                assert err == 0, (w, m, got)                                 # integers: every partial sum is exact
            bound = 7 * (T.F(1, 2 ** 104) if is_dd else T.U) * mass          # six levels of dd_add_fast's contract / of rounding
            assert err <= bound, (w, m, got, float(err / bound))
            if mass:
                worst = max(worst, float(err / bound))
            assert not T.same_bits([got], [twin[lanes[0]]]), (w, m, got, twin[lanes[0]])
    print("lanes_transpose_reduce<%d, 32> %s: worst error %.4f of the bound" % (n, "dd" if is_dd else "double", worst))


# ---- dd_readlane, dd_shfl_xor -------------------------------------------------------------------------------------------------------
def lane_patterns():
    """a bit pattern per thread for hi and another for lo: -0.0, subnormals, infinities, quiet and signalling NaNs with payloads,
    spread over the lanes, the rest random bits"""
    rng = np.random.default_rng(64)
    special = [0x8000000000000000, 0x0000000000000001, 0x000FFFFFFFFFFFFF, 0x800FFFFFFFFFFFFE, 0x7FF0000000000000, 0xFFF0000000000000,
               0x7FF8000000000001, 0x7FF80000DEADBEEF, 0xFFF8000012345678, 0x7FF0000000000001, 0x7FF4000000ABCDEF, 0xFFF00000CAFE0001,
               0x0000000000000000, 0x3FF0000000000000]
    hi = rng.integers(0, 2 ** 64, size=NWAVES * 64, dtype=np.uint64)
    lo = rng.integers(0, 2 ** 64, size=NWAVES * 64, dtype=np.uint64)
    for w in range(NWAVES):
        for k, s in enumerate(special):
            hi[w * 64 + (5 * k + 9 * w) % 64] = s
            lo[w * 64 + (5 * k + 9 * w + 3) % 64] = special[(k + 1 + w) % len(special)] ^ 0x0000000100000000
    return hi, lo


def test_lane_moves_are_bit_exact(probe):
    import torch
    hi, lo = lane_patterns()
    dh, dl = to_dev(hi.view(np.float64)), to_dev(lo.view(np.float64))
    rl = [torch.zeros(NWAVES * 64 * 64, dtype=torch.float64, device="cuda") for _ in range(2)]
    sx = [torch.zeros(NWAVES * 6 * 64, dtype=torch.float64, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    st = probe.pa_probe_lane_moves(NWAVES, -1, dh.data_ptr(), dl.data_ptr(), rl[0].data_ptr(), rl[1].data_ptr(), sx[0].data_ptr(), sx[1].data_ptr())
    assert st == 0, "hipError_t %d" % st
    lane = np.arange(64)
    for src, r, s in ((hi, rl[0], sx[0]), (lo, rl[1], sx[1])):
        src = src.reshape(NWAVES, 64)
        r = r.cpu().numpy().view(np.uint64).reshape(NWAVES, 64, 64)                      # [wave][j][lane]: lane j's value on every lane
        assert np.array_equal(r, np.broadcast_to(src[:, :, None], r.shape))
        s = s.cpu().numpy().view(np.uint64).reshape(NWAVES, 6, 64)
        for k in range(6):
            assert np.array_equal(s[:, k, :], src[:, lane ^ (1 << k)]), k
    # the lane index as a kernel argument
    one = [torch.zeros(NWAVES * 64, dtype=torch.float64, device="cuda") for _ in range(2)]
    for j in range(64):
        torch.cuda.synchronize()
        st = probe.pa_probe_lane_moves(NWAVES, j, dh.data_ptr(), dl.data_ptr(), one[0].data_ptr(), one[1].data_ptr(), 0, 0)
        assert st == 0, "hipError_t %d" % st
        for src, r in ((hi, one[0]), (lo, one[1])):
            r = r.cpu().numpy().view(np.uint64).reshape(NWAVES, 64)
            assert np.array_equal(r, np.broadcast_to(src.reshape(NWAVES, 64)[:, j:j + 1], r.shape)), j
