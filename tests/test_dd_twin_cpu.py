"""The IEEE-strict twin of dd_arith.hpp (tests/dd_twin.py) on the inputs the device test uses, without a device: the twin meets
every bound the device is held to, two degraded twins -- the two losses of accuracy dd_arith.hpp records -- miss theirs on the same
inputs, the transposed butterfly's bookkeeping delivers every entry once for every count, and the build leaves the probe library."""
import ctypes
import os
import subprocess

import pytest

import dd_twin as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITH = [op for op in T.OPS if op in T.BOUNDS] + ["dd_round"]


def test_inputs_are_normalised_and_cover_the_classes():
    inp = T.binary_inputs()
    assert [inp["cls"].count(c) for c in range(1, 7)] == [1024] * 6
    for x in inp["a"] + inp["b"] + T.rsqrt_inputs()["a"]:
        assert x[0] == x[0] + x[1]
    for x, y, c in zip(inp["a"], inp["b"], inp["cls"]):
        if c == 2:
            assert 2.0 ** -71 < abs(float((T.exact(x) + T.exact(y)) / T.exact(x))) < 2.0 ** -9
        if c == 3:
            assert y[0] == -x[0]
        if c == 4:
            assert T.exact(x) + T.exact(y) == 0 and x[0] != 0.0
        if c == 6:
            assert x[0] == 0.0 or y[0] == 0.0
    assert any(T.bits(x[0]) == T.bits(-0.0) for x in inp["a"]) and any(T.bits(z) == T.bits(-0.0) for z in inp["d"])
    assert all(x[0] > 0.0 for x in T.rsqrt_inputs()["a"])


@pytest.mark.parametrize("op", ARITH)
def test_twin_meets_the_bound(op):
    inp = T.binary_inputs()
    worst, bad = T.check(op, inp, T.run(op, inp))
    print("%s: twin worst %.3f of its bound" % (op, worst))
    assert not bad, bad[:3]
    assert worst <= 1.0


def test_twin_error_levels_are_the_published_ones():
    """(the worst errors in u^2: AccurateDWPlusDW is attained to ~2.25 u^2, DWTimesDW1 to ~4 u^2, DWTimesFP3 to ~1.5 u^2 in the
    paper; inputs that stayed far below those would not be trying)"""
    inp = T.binary_inputs()
    for op, least in (("dd_add", 0.5), ("dd_mul", 1.5), ("dd_mul_d", 0.7)):
        worst, _ = T.check(op, inp, T.run(op, inp))
        assert float(worst * T.BOUNDS[op][1] / T.U ** 2) > least, op


@pytest.mark.parametrize("op", ["dd_rsqrt", "dd_rsqrt_1"])
def test_twin_square_roots_from_emulated_seeds(op):
    bar, worst = T.rsqrt_bar(op)
    print("%s: twin worst relative error %.3g from seeds off by 2^-20, bar %.3g" % (op, worst, bar))
    assert worst < 1e-31                 # ~2^-104: what a double-double holds; the historical failures sat at 1e-20 and 1e-16
    # ... and from seeds as good as the hardware's (2^-26) no worse than the bar
    inp = T.rsqrt_inputs()
    seeds = [s * (1.0 + (2.0 ** -26 if i % 2 else -2.0 ** -26)) for i, s in
             enumerate(float(1 / T.mp.sqrt(T.mp.mpf(x[0]))) for x in inp["a"])]
    assert max(T.rsqrt_errors(inp, T.run(op, inp, seeds=seeds))) < bar


def test_contracted_product_misses_the_bound():
    """dd_mul with two_prod's error term dropped: ~u instead of ~u^2"""
    inp = T.binary_inputs()
    worst, bad = T.check("dd_mul", inp, T.run("dd_mul", inp, fn=T.dd_mul_contracted))
    assert worst > 1e10 and len(bad) > 1000
    assert len(T.same_bits(T.run("dd_mul", inp, fn=T.dd_mul_contracted), T.run("dd_mul", inp))) > 1000


def test_single_step_square_root_misses_the_bar():
    """dd_rsqrt as one double-double Newton step from a 2^-26 seed"""
    inp = T.rsqrt_inputs()
    bar, _ = T.rsqrt_bar("dd_rsqrt")
    seeds = [s * (1.0 + (2.0 ** -26 if i % 2 else -2.0 ** -26)) for i, s in
             enumerate(float(1 / T.mp.sqrt(T.mp.mpf(x[0]))) for x in inp["a"])]
    errs = T.rsqrt_errors(inp, T.run("dd_rsqrt", inp, seeds=seeds, fn=T.dd_rsqrt_one_step))
    assert min(errs) > 1e6 * bar and max(errs) > 1e-16


@pytest.mark.parametrize("n", range(1, 65))
def test_butterfly_delivers_every_entry_once(n):
    """the bookkeeping of lanes_transpose_reduce<n, 32>, values carried as sets of (lane, entry) contributions: a lane that is `ok`
    holds entry `index` of all 64 lanes, each once; a lane that is not holds padding only; the lanes that end with the same entry are
    one aligned group, and the groups that are `ok` deliver 0 .. n - 1 once each"""
    def add(x, y):
        assert not (x & y)
        return x | y

    v = [[frozenset([(l, m)]) for m in range(n)] for l in range(64)]
    index, ok, out = T.lanes_transpose_reduce(v, n, 32, add, frozenset())
    for l in range(64):
        if ok[l]:
            assert 0 <= index[l] < n and out[l] == frozenset((k, index[l]) for k in range(64)), (l, index[l])
        else:
            assert out[l] == frozenset(), (l, index[l])      # (its index may well be a valid one: callers must look at ok)
    group = 64 >> (n - 1).bit_length()
    delivered = []
    for g0 in range(0, 64, group):
        assert len({(index[l], ok[l]) for l in range(g0, g0 + group)}) == 1
        if ok[g0]:
            delivered.append(index[g0])
    assert sorted(delivered) == list(range(n))


def test_build_leaves_the_probe_library():
    from proton_amd import _build
    assert os.path.realpath(_build.PROBE_LIB_PATH) == os.path.join(ROOT, "proton_amd", "lib", "probe", "libpa_dd_probe.so")
    assert os.path.exists(_build.PROBE_LIB_PATH), "run the build: the GPU tests compile nothing"
    lib = ctypes.CDLL(_build.PROBE_LIB_PATH)
    for name in ("pa_probe_dd", "pa_probe_transpose_reduce", "pa_probe_lane_moves"):
        assert getattr(lib, name) is not None
    out = subprocess.run(["nm", "-D", "--defined-only", _build.PROBE_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(w.split()[-1] for w in out.splitlines() if " T pa_" in w) == ["pa_probe_dd", "pa_probe_lane_moves", "pa_probe_transpose_reduce"]
    # the probe is compiled with the library's flags, nothing added, and is no part of what bench.py's build stamp covers
    with open(os.path.join(os.path.dirname(_build.PROBE_LIB_PATH), "dd_probe.o.flags")) as f:
        assert f.read() == " ".join(_build.FLAGS)
    assert not os.path.exists(os.path.join(_build.CSRC, "dd_probe.hip"))
