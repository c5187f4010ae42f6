"""An IEEE-strict twin of proton_amd/csrc/dd_arith.hpp, the inputs the primitives are tried on, and the checks of their results.

Every function restates the header's function of the same name operation by operation in Python floats: IEEE doubles, rounded to
nearest, never contracted, never reassociated.  fma() is the correctly rounded one (exact in fractions.Fraction, rounded once).  The
reciprocal square roots take their seed as an argument: the device's comes from an approximate instruction, the emulated one is the
exact value off by up to 2^-20.  A (hi, lo) pair is a tuple of two floats.

check(op, inputs, hi, lo) holds a set of results -- the twin's (tests/test_dd_twin_cpu.py) or the device's
(tests/test_gpu_dd_primitives.py) -- to the bounds of Joldes, Muller and Popescu, "Tight and rigorous error bounds for basic
building blocks of double-word arithmetic" (ACM TOMS 44, 2017): AccurateDWPlusDW 3u^2 + 13u^3, DWTimesDW1 7u^2, DWTimesFP3 2u^2,
u = 2^-53; dd_add_fast to the contract dd_arith.hpp states, 2^-104 (|a| + |b|) absolute.
"""
import functools
import math
import random
from fractions import Fraction as F

import mpmath as mp

U = F(1, 2 ** 53)
# the numbering of tests/hip/dd_probe.hip
OPS = ("two_sum", "quick_two_sum", "two_prod", "dd_add", "dd_add_fast", "dd_sub", "dd_sub_fast", "dd_mul", "dd_mul_d",
       "dd_rsqrt", "dd_rsqrt_1", "dd_round", "rsq_seed")
# the error an op may make, and against what: "rel": |got - exact| <= bound |exact|; "abs": <= bound (|a| + |b|); 0: exact
BOUNDS = {
    "two_sum": ("rel", F(0)), "quick_two_sum": ("rel", F(0)), "two_prod": ("rel", F(0)),
    "dd_add": ("rel", 3 * U ** 2 + 13 * U ** 3), "dd_sub": ("rel", 3 * U ** 2 + 13 * U ** 3),
    "dd_add_fast": ("abs", F(1, 2 ** 104)), "dd_sub_fast": ("abs", F(1, 2 ** 104)),
    "dd_mul": ("rel", 7 * U ** 2), "dd_mul_d": ("rel", 2 * U ** 2),
}
RSQRT_MARGIN = 8                      # the bar of the square roots: this many times the twin's worst error from emulated seeds
RSQRT_SEED_SPREAD = 2.0 ** -20        # ... which are off by up to this (the hardware's is good to ~2^-26 on paper)
TRANSPOSE_COUNTS = (1, 2, 3, 5, 6, 7, 9, 10, 13, 15, 21, 28, 33, 64)      # PA_PROBE_COUNTS of tests/hip/dd_probe.hip


# ---- the header, restated -----------------------------------------------------------------------------------------------------------
def fma(a, b, c):
    r = F(a) * F(b) + F(c)
    if r == 0:                        # the sign of an exact zero: that of the sum of two zeros, else +0 (round to nearest)
        return a * b + c if (a == 0.0 or b == 0.0) else 0.0
    return float(r)                   # int / int: correctly rounded


def two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def quick_two_sum(a, b):
    s = a + b
    return s, b - (s - a)


def two_prod(a, b):
    p = a * b
    return p, fma(a, b, -p)


def dd_add(a, b):
    sh, sl = two_sum(a[0], b[0])
    th, tl = two_sum(a[1], b[1])
    sl = sl + th
    sh, sl = quick_two_sum(sh, sl)
    sl = sl + tl
    return quick_two_sum(sh, sl)


def dd_add_fast(a, b):
    sh, sl = two_sum(a[0], b[0])
    sl = sl + (a[1] + b[1])
    return quick_two_sum(sh, sl)


def dd_neg(a):
    return -a[0], -a[1]


def dd_sub(a, b):
    return dd_add(a, dd_neg(b))


def dd_sub_fast(a, b):
    return dd_add_fast(a, dd_neg(b))


def dd_mul(a, b):
    ph, pl = two_prod(a[0], b[0])
    pl = pl + (a[0] * b[1] + a[1] * b[0])
    return quick_two_sum(ph, pl)


def dd_mul_d(a, b):
    ph, pl = two_prod(a[0], b)
    pl = fma(a[1], b, pl)
    return quick_two_sum(ph, pl)


def _newton_double(ah, x):
    t = ah * x
    e = fma(-t, x, 1.0)
    return fma(0.5 * x, e, x)


def _newton_dd(a, y):
    r = dd_sub((1.0, 0.0), dd_mul(dd_mul(a, y), y))
    return dd_add(y, dd_mul(dd_mul_d(r, 0.5), y))


def dd_rsqrt(a, seed):
    y = (_newton_double(a[0], seed), 0.0)
    for _ in range(2):
        y = _newton_dd(a, y)
    return y


def dd_rsqrt_1(a, seed):
    x = _newton_double(a[0], _newton_double(a[0], seed))
    t = dd_mul_d(dd_mul_d(a, x), x)
    r = (1.0 - t[0]) - t[1]
    return quick_two_sum(x, (0.5 * x) * r)


def dd_round(a):
    return a[0] + a[1]


# ---- the two losses of accuracy dd_arith.hpp records, restated: the inputs and the bars must see them --------------------------------
def dd_mul_contracted(a, b):
    """two_prod's error term gone (what fusing p = a * b into the addition after it amounts to)"""
    ph, pl = a[0] * b[0], 0.0
    pl = pl + (a[0] * b[1] + a[1] * b[0])
    return quick_two_sum(ph, pl)


def dd_rsqrt_one_step(a, seed):
    """a single double-double Newton step from the raw seed, no step in double"""
    return _newton_dd(a, (seed, 0.0))


def lanes_transpose_reduce(v, n, off, add, zero):
    """lanes_transpose_reduce<n, off> on the 64 lanes at once: v[lane][m] -> (index[lane], ok[lane], out[lane])"""
    if n == 1:
        s = [v[l][0] for l in range(64)]
        while off >= 1:
            s = [add(s[l], s[l ^ off]) for l in range(64)]
            off >>= 1
        return [0] * 64, [True] * 64, s
    assert off >= 1, "more values than lanes"
    h = (n + 1) // 2
    keep = [[None] * h for _ in range(64)]
    send = [[None] * h for _ in range(64)]
    for l in range(64):
        up = (l & off) != 0
        for m in range(h):
            lo, hi = v[l][m], (v[l][m + h] if m + h < n else zero)
            send[l][m], keep[l][m] = (lo, hi) if up else (hi, lo)
    w = [[add(keep[l][m], send[l ^ off][m]) for m in range(h)] for l in range(64)]
    index, ok, out = lanes_transpose_reduce(w, h, off // 2, add, zero)
    for l in range(64):
        up = (l & off) != 0
        if up and index[l] + h >= n:
            ok[l] = False
        index[l] += h if up else 0
    return index, ok, out


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
EDGE_MANTISSAS = (1.0, 1.0 + 2.0 ** -52, 2.0 - 2.0 ** -52, 1.5, 1.0 + 2.0 ** -26)


def ulp(x):
    return math.ldexp(1.0, math.frexp(abs(x))[1] - 53)


def exact(a):
    return F(a[0]) + F(a[1])


def _from_exact(x):
    hi = float(x)
    return two_sum(hi, float(x - F(hi)))


def _sign(rng):
    return -1.0 if rng.random() < 0.5 else 1.0


def _lo_for(rng, hi, kind):
    """0 / just under +-ulp(hi)/2 / uniform in +-ulp(hi)/2 / that scaled by 2^-1 .. 2^-40"""
    half = 0.5 * ulp(hi)
    if kind == 0:
        return 0.0
    if kind == 1:
        return _sign(rng) * math.nextafter(half, 0.0)
    lo = rng.uniform(-1.0, 1.0) * half
    return lo if kind == 2 else math.ldexp(lo, -rng.randint(1, 40))


def _general(rng, e, kind):
    hi = _sign(rng) * math.ldexp(rng.uniform(1.0, 2.0), e)
    return two_sum(hi, _lo_for(rng, hi, kind))


def _edge(rng, e, which):
    hi = _sign(rng) * math.ldexp(EDGE_MANTISSAS[which % 5], e)
    return two_sum(hi, _sign(rng) * math.ldexp(hi, -rng.randint(54, 60)))


def _near(rng, e, spread):
    return max(-100, min(100, e + rng.randint(-spread, spread)))


@functools.lru_cache(maxsize=None)
def binary_inputs(per_class=1024, seed=20260):
    """the operands of the two-operand ops: lists a, b (pairs), d (doubles), cls (1 .. 6), per_class elements of each class"""
    rng = random.Random(seed)
    a, b, d, cls = [], [], [], []

    def put(c, x, y, z):
        a.append(x); b.append(y); d.append(z); cls.append(c)

    def dbl():
        return _sign(rng) * math.ldexp(rng.uniform(1.0, 2.0), rng.randint(-100, 100))

    for i in range(per_class):                           # 1: general; three in four with exponents close enough to interact
        e = rng.randint(-100, 100)
        eb = _near(rng, e, 64) if i % 4 != 3 else rng.randint(-100, 100)
        put(1, _general(rng, e, i % 4), _general(rng, eb, (i // 4) % 4), dbl())
    for i in range(per_class):                           # 2: cancellation, b = -a (1 + delta), |delta| = 2^-10 .. 2^-70
        x = _general(rng, rng.randint(-100, 100), i % 4)
        delta = F(_sign(rng)) / 2 ** (10 + i % 61)
        put(2, x, _from_exact(-exact(x) * (1 + delta)), dbl())
    for i in range(per_class):                           # 3: b.hi = -a.hi exactly, an unrelated lo
        x = _general(rng, rng.randint(-100, 100), i % 4)
        put(3, x, two_sum(-x[0], _lo_for(rng, x[0], 1 + (i // 4) % 3)), dbl())
    for i in range(per_class):                           # 4: b = -a exactly
        x = _general(rng, rng.randint(-100, 100), i % 4) if i % 2 else _edge(rng, rng.randint(-100, 100), i // 2)
        put(4, x, dd_neg(x), -x[0] if i % 4 == 0 else dbl())
    for i in range(per_class):                           # 5: binade edges, lo at 2^-54 .. 2^-60 of hi
        e = rng.randint(-100, 100)
        eb = _near(rng, e, 3) if i % 2 == 0 else rng.randint(-100, 100)
        put(5, _edge(rng, e, i), _edge(rng, eb, i // 5), _sign(rng) * math.ldexp(EDGE_MANTISSAS[(i // 25) % 5], rng.randint(-100, 100)))
    zeros = [(0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0)]
    for i in range(per_class):                           # 6: one or both operands zero, -0.0 included
        x = _general(rng, rng.randint(-100, 100), i % 4)
        y = _edge(rng, rng.randint(-100, 100), i)
        z0, z1 = zeros[(i // 3) % 4], zeros[(i // 12) % 4]
        x, y = ((z0, y), (x, z0), (z0, z1))[i % 3]
        put(6, x, y, (0.0, -0.0, dbl())[(i // 3) % 3])
    return {"a": a, "b": b, "d": d, "cls": cls}


@functools.lru_cache(maxsize=None)
def rsqrt_inputs(per_class=1024, seed=20261):
    """the operands of the reciprocal square roots: a.hi > 0 over 2^-200 .. 2^200, general and binade-edge mantissas"""
    rng = random.Random(seed)
    a = []
    for i in range(per_class):
        hi = math.ldexp(rng.uniform(1.0, 2.0), rng.randint(-200, 200))
        a.append(two_sum(hi, _lo_for(rng, hi, i % 4)))
    for i in range(per_class):
        hi = math.ldexp(EDGE_MANTISSAS[i % 5], rng.randint(-200, 200))
        a.append(two_sum(hi, _sign(rng) * math.ldexp(hi, -rng.randint(54, 60))))
    return {"a": a}


@functools.lru_cache(maxsize=None)
def emulated_seeds(per_class=1024, seed=20262):
    """1 / sqrt(a.hi) off by a relative error drawn from +-2^-20, the two ends included"""
    rng = random.Random(seed)
    out = []
    with mp.workdps(80):
        for i, x in enumerate(rsqrt_inputs(per_class)["a"]):
            eps = (RSQRT_SEED_SPREAD, -RSQRT_SEED_SPREAD, rng.uniform(-1.0, 1.0) * RSQRT_SEED_SPREAD)[min(i % 8, 2)]
            out.append(float((1 / mp.sqrt(mp.mpf(x[0]))) * (1 + mp.mpf(eps))))
    return out


def operands(op, inp):
    """the (a, b) an op sees: quick_two_sum wants |a| >= |b|; the subtractions get -b, so that the classes cancel for them too"""
    if op in ("dd_sub", "dd_sub_fast"):
        return inp["a"], [dd_neg(y) for y in inp["b"]]
    if op == "quick_two_sum":
        return zip(*[(x, y) if abs(x[0]) >= abs(y[0]) else (y, x) for x, y in zip(inp["a"], inp["b"])])
    return inp["a"], inp["b"]


def run(op, inp, seeds=None, fn=None):
    """the twin's results of `op` on the inputs: a list of pairs (fn: another implementation of the same op, e.g. a degraded one)"""
    a, b = operands(op, inp) if "b" in inp else (inp["a"], None)
    if op in ("dd_rsqrt", "dd_rsqrt_1"):
        f = fn or globals()[op]
        return [f(x, s) for x, s in zip(a, seeds)]
    if op == "dd_round":
        return [(dd_round(x), 0.0) for x in a]
    if op in ("two_sum", "quick_two_sum", "two_prod"):
        return [globals()[op](x[0], y[0]) for x, y in zip(a, b)]
    if op == "dd_mul_d":
        return [(fn or dd_mul_d)(x, z) for x, z in zip(a, inp["d"])]
    f = fn or globals()[op]
    return [f(x, y) for x, y in zip(a, b)]


# ---- checks -------------------------------------------------------------------------------------------------------------------------
def want_exact(op, x, y, z):
    if op in ("two_sum", "quick_two_sum"):
        return F(x[0]) + F(y[0])
    if op == "two_prod":
        return F(x[0]) * F(y[0])
    if op in ("dd_add", "dd_add_fast"):
        return exact(x) + exact(y)
    if op in ("dd_sub", "dd_sub_fast"):
        return exact(x) - exact(y)
    if op == "dd_mul":
        return exact(x) * exact(y)
    assert op == "dd_mul_d"
    return exact(x) * F(z)


def check(op, inp, got):
    """`got` (a list of pairs) against the exact results: (worst error as a multiple of the op's bound -- of u^2 for the exact
    ops --, problems found).  Normalisation, the exact zeros and, for the error-free transformations, the correctly rounded hi."""
    a, b = operands(op, inp)
    bad, worst = [], F(0)
    if op == "dd_round":
        for i, (x, g) in enumerate(zip(a, got)):
            if not (g[0] == x[0] + x[1] and math.copysign(1.0, g[0]) == math.copysign(1.0, x[0] + x[1])):
                bad.append((i, "dd_round", x, g))
        return 0.0, bad
    kind, bound = BOUNDS[op]
    for i, (x, y, z, g) in enumerate(zip(a, b, inp["d"], got)):
        want, have = want_exact(op, x, y, z), exact(g)
        if g[0] != g[0] + g[1]:
            bad.append((i, "not normalised", x, y, g))
        err = abs(have - want)
        if want == 0 and (g[0] != 0.0 or g[1] != 0.0) and kind == "rel":
            bad.append((i, "exact zero missed", x, y, g))
        scale = abs(want) if kind == "rel" else abs(exact(x)) + abs(exact(y))
        if bound == 0:
            if err != 0 or (want != 0 and g[0] != float(want)):
                bad.append((i, "not error-free / hi not the rounded result", x, y, g))
        elif scale != 0:
            if err > bound * scale:
                bad.append((i, "error %.3g of the bound" % float(err / (bound * scale)), x, y, g))
            worst = max(worst, err / (bound * scale))
        elif err != 0:
            bad.append((i, "nonzero from zeros", x, y, g))
        if op in ("dd_add", "dd_add_fast", "dd_sub", "dd_sub_fast") and inp["cls"][i] == 4 and (g[0] != 0.0 or g[1] != 0.0):
            bad.append((i, "b = -a: not (0, 0)", x, y, g))
    return float(worst), bad


def rsqrt_errors(inp, got):
    """the relative errors of `got` against 1 / sqrt(hi + lo) in 80-digit arithmetic"""
    out = []
    with mp.workdps(80):
        for x, g in zip(inp["a"], got):
            w = 1 / mp.sqrt(mp.mpf(x[0]) + mp.mpf(x[1]))
            out.append(float(abs((mp.mpf(g[0]) + mp.mpf(g[1]) - w) / w)))
    return out


@functools.lru_cache(maxsize=None)
def rsqrt_bar(op, per_class=1024):
    """(the bar a device result is held to, the twin's own worst error): RSQRT_MARGIN times the worst relative error of the twin
    from the emulated seeds on these inputs"""
    inp = rsqrt_inputs(per_class)
    worst = max(rsqrt_errors(inp, run(op, inp, seeds=emulated_seeds(per_class))))
    return RSQRT_MARGIN * worst, worst


def bits(x):
    import struct
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def same_bits(got, want):
    """indices at which two lists of pairs differ in any bit"""
    return [i for i, (g, w) in enumerate(zip(got, want)) if bits(g[0]) != bits(w[0]) or bits(g[1]) != bits(w[1])]
