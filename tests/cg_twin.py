"""A twin of the conjugate gradient (solver_cg.hpp:63-144, proton_amd/csrc/solver.hip) that judges it iterate by iterate.

CG corrects itself: a dot product that loses a partial, a product that drops an entry of a row, a preconditioner applied in one place
only -- all of them still converge, a few iterations later.  So the converged solution says little; the m-th iterate says everything,
and it is observable through the public entry point because the exit tests run in the reference's order (rr < tol, iter > max_iter,
rr > div): div = 0 returns x_1 (reason 1, iterations 0), max_iter = m - 2 with tol = 0 returns x_m (reason 2, iterations m - 1).

No device here.  This module holds
  * system(case): a deterministic SPD CSR system from a seed (band {1, 5, 17}, optional arrowhead, fixed row lengths, symmetric
    scaling over four decades so that Jacobi and no preconditioner give different iterates, the last row carrying weight);
  * truth(case): the recurrences in mpmath at 50 digits (n <= 4097) or numpy.longdouble (above) -> x_1..x_M and |r_j| / |r_0|;
  * recurrences(...): the same recurrences in IEEE double in two summation orders -- sequential (the reference's) and the device's
    stated order restated in numpy (16 lanes per row with stride-16 assignment and a butterfly, 64-lane butterfly, four wave sums, the
    strided loop over the per-block partials) -- with switches that plant the defects the case table is there to catch;
  * e_ref(case): the error of those against truth, worst of the two orders, in the norm  max |dx_i| sqrt(A_ii) / max |x_i| sqrt(A_ii)
    (a plain max-norm would let the large-scale components hide the small ones);
  * the gate max(FLOOR, 10 e_ref), the cap e_ref <= 1e-10 below which a pair is judged, and the exit thresholds."""
import functools
import math
from collections import namedtuple

import numpy as np

RB, ROW_LANES = 256, 16                   # cg.hpp
M_MAX = 8                                 # iterates judged per case: m = 1..min(M_MAX, n)
CAP = 1e-10                               # a (case, m) pair is judged where e_ref <= CAP: beyond, double has left the exact trajectory
MARGIN = 10.0                             # the project's margin over e_ref (tests/test_gpu_hard_cells.py)
# The largest e_ref of the preconditioned (case, m) pairs, rounded up to a power of two.  Measured on the CPU from the double
# recurrences, never from the device: tests/test_cg_twin_cpu.py recomputes it from the whole table and asserts this figure; it is
# written next to that table in profiles/cg_twin_parity.txt.
FLOOR = 2.0 ** -45                       # 2.84e-14; the largest is 1.56e-14: sequential sums of 65537 terms, arrowhead, m = 1
MP_ROWS = 4097                            # truth in mpmath up to here, in longdouble above
EXACT = 1e-40                             # a truth residual below this is the exact termination of CG (n steps; 1 for a diagonal matrix)

SIZES = (1, 2, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 65536, 65537)
ROW_LENGTHS = (1, 15, 16, 17, 33)

Case = namedtuple("Case", "n precond arrow L reverse")
Case.__new__.__defaults__ = (False, None, False)


def case_id(c):
    kind = "L%d" % c.L if c.L else ("arrow" if c.arrow else "band")
    return "n%d-%s%s-%s" % (c.n, kind, "-rev" if c.reverse else "", "jacobi" if c.precond else "plain")


def case_table():
    """n in SIZES x preconditioner on / off x band with / without the arrowhead; at n = 257 also every row of exactly L entries and the
    band with the column indices of each row reversed"""
    out = []
    for n in SIZES:
        for arrow in (False, True):
            for precond in (True, False):
                out.append(Case(n, precond, arrow))
    for precond in (True, False):
        for L in ROW_LENGTHS:
            out.append(Case(257, precond, False, L))
        out.append(Case(257, precond, False, None, True))
        out.append(Case(257, precond, True, None, True))
    return out


# ---- the systems ---------------------------------------------------------------------------------------------------------------
System = namedtuple("System", "n rowptr colind values b diag scale")


def _pairs(n, arrow, L):
    """the off-diagonal pattern: (i, j) with i < j, each once; and the rows that store one explicit zero"""
    ii, jj, zero_rows = [], [], []
    if L is None:
        for o in (1, 5, 17):
            if n > o:
                ii.append(np.arange(n - o)); jj.append(np.arange(o, n))
        if arrow and n > 2:
            j = np.arange(2, n)                    # (0, 1) is in the band already
            j = j[(j != 5) & (j != 17)]
            ii.append(np.zeros(j.size, dtype=np.int64)); jj.append(j)
    else:
        # circulant offsets 1..h on both sides: 2 h + 1 entries per row.  An even L needs one more per row: the matching
        # k <-> k + n // 2, k < n // 2, which leaves the last row (n is odd) alone -- that row stores an explicit zero instead
        # (a symmetric pattern with an odd number of odd rows does not exist)
        h = (L - 1) // 2
        assert n % 2 == 1 and 2 * h + 2 < n // 2
        i = np.arange(n)
        for o in range(1, h + 1):
            j = (i + o) % n
            ii.append(np.minimum(i, j)); jj.append(np.maximum(i, j))
        if L % 2 == 0:
            k = np.arange(n // 2)
            ii.append(k); jj.append(k + n // 2)
            zero_rows.append(n - 1)
    if not ii:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), zero_rows
    return np.concatenate(ii).astype(np.int64), np.concatenate(jj).astype(np.int64), zero_rows


@functools.lru_cache(maxsize=None)
def _system(n, arrow, L, reverse):
    rng = np.random.default_rng([20240613, n, int(arrow), L or 0])
    i, j, zero_rows = _pairs(n, arrow, L)
    w = rng.uniform(0.25, 1.0, i.size) * rng.choice([-1.0, 1.0], i.size)
    absrow = np.zeros(n)
    np.add.at(absrow, i, np.abs(w)); np.add.at(absrow, j, np.abs(w))
    dw = 1.25 * absrow + rng.uniform(0.5, 1.0, n)                  # strictly dominant
    # s = 10^U(-e, e), e = 2: the diagonal spans eight decades.  With few rows e = n / 8: there x_n is the solve itself, and the
    # last steps of a terminating CG without preconditioner amplify rounding by the condition number -- at n = 2 and four decades
    # the double recurrences leave the trajectory at m = 2 (e_ref 9e-9), and no pair with m <= 3 may be left out
    e = min(2.0, n / 8.0)
    # (rounded to float32 and back: a power function that differs by an ulp from one machine to the next gives the same systems)
    s = (10.0 ** rng.uniform(-e, e, n)).astype(np.float32).astype(np.float64)
    z = rng.standard_normal(n)
    # the last row carries weight: the largest scale and |b| >= 1, so that a partial or a lane lost at the tail changes every
    # dot product by a share that is not negligible
    s[n - 1] = float(np.float32(10.0 ** e))
    if abs(z[n - 1]) < 1.0:
        z[n - 1] = math.copysign(1.0 + abs(z[n - 1]), z[n - 1])
    b = s * z
    v = (s[i] * s[j]) * w                                          # the same double for (i, j) and (j, i)
    diag = (s * s) * dw
    rows = np.concatenate([i, j, np.arange(n)])
    cols = np.concatenate([j, i, np.arange(n)])
    vals = np.concatenate([v, v, diag])
    for r in zero_rows:
        rows = np.append(rows, r); cols = np.append(cols, (r + n // 2) % n); vals = np.append(vals, 0.0)
    order = np.lexsort((-cols if reverse else cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=rowptr[1:])
    if L is not None:
        assert (np.diff(rowptr) == L).all()
    for a in (rowptr, cols, vals, b, diag, s):
        a.setflags(write=False)
    return System(n, rowptr, cols.astype(np.int32), vals, b, diag, s)


def system(case):
    """the CSR system of a case (shared, read-only): rowptr int64, colind int32, values, b, the diagonal and the scaling s"""
    return _system(case.n, bool(case.arrow), case.L, bool(case.reverse))


def scaled_error(x, ref, diag):
    """max |x_i - ref_i| sqrt(A_ii) / max |ref_i| sqrt(A_ii)"""
    w = np.sqrt(np.asarray(diag, dtype=np.longdouble))
    ref = np.asarray(ref, dtype=np.longdouble)
    return float((np.abs(np.asarray(x, dtype=np.longdouble) - ref) * w).max() / (np.abs(ref) * w).max())


# ---- truth ---------------------------------------------------------------------------------------------------------------------
Truth = namedtuple("Truth", "x rr")        # x[j - 1] = x_j as longdouble, rr[j - 1] = |r_j| / |r_0| as float, j = 1..M


def _truth_mp(sy, m, precond):
    import mpmath
    with mpmath.workdps(50):
        mpf = mpmath.mpf
        obj = lambda a: np.array([mpf(float(t)) for t in a], dtype=object)
        vals, b = obj(sy.values), obj(sy.b)
        n, starts = sy.n, sy.rowptr[:-1]
        iA = np.array([mpf(1) / mpf(float(t)) for t in sy.diag], dtype=object) if precond else None
        dot = lambda u, v: mpmath.fsum(u * v)
        x = np.array([mpf(0)] * n, dtype=object)
        r = b.copy()
        d = iA * r if precond else r.copy()
        nr0 = mpmath.sqrt(dot(r, r))
        xs, rrs = [], []
        for _ in range(m):
            y = np.add.reduceat(vals * d[sy.colind], starts)
            z = iA * r if precond else r
            rho = dot(r, z)
            alpha = rho / dot(d, y)
            x = x + alpha * d
            r = r - alpha * y
            rr = mpmath.sqrt(dot(r, r)) / nr0
            xs.append(np.array([np.longdouble(mpmath.nstr(t, 25)) for t in x]))
            rrs.append(float(rr))
            if rr < EXACT:
                break
            z = iA * r if precond else r
            d = z + (dot(r, z) / rho) * d
        return Truth(xs, rrs)


def _truth_ld(sy, m, precond):
    ld = np.longdouble
    vals, b = sy.values.astype(ld), sy.b.astype(ld)
    starts = sy.rowptr[:-1]
    iA = ld(1) / sy.diag.astype(ld) if precond else None
    x = np.zeros(sy.n, dtype=ld)
    r = b.copy()
    d = iA * r if precond else r.copy()
    nr0 = np.sqrt(np.sum(r * r))
    xs, rrs = [], []
    for _ in range(m):
        y = np.add.reduceat(vals * d[sy.colind], starts)
        z = iA * r if precond else r
        rho = np.sum(r * z)
        alpha = rho / np.sum(d * y)
        x = x + alpha * d
        r = r - alpha * y
        rr = np.sqrt(np.sum(r * r)) / nr0
        xs.append(x.copy())
        rrs.append(float(rr))
        if rr < 1e-17:                             # the exact termination as this route sees it
            break
        z = iA * r if precond else r
        d = z + (np.sum(r * z) / rho) * d
    return Truth(xs, rrs)


@functools.lru_cache(maxsize=None)
def _truth(case, route):
    sy = system(case)
    m = min(M_MAX, case.n)
    return (_truth_mp if route == "mp" else _truth_ld)(sy, m, case.precond)


def truth(case, route=None):
    """x_1..x_M and |r_j| / |r_0| of the exact recurrences of solver_cg.hpp:76-131 on the case's double inputs; M = min(8, n), or
    the step at which CG terminates exactly if that comes first (a diagonal matrix under Jacobi: one step)"""
    return _truth(case, route or ("mp" if case.n <= MP_ROWS else "ld"))


# ---- the double recurrences, in two orders, with planted defects -------------------------------------------------------------------
def _seq_sum(a):
    return float(np.cumsum(a)[-1]) if a.size else 0.0


def _butterfly(v, width):
    idx = np.arange(width)
    o = width // 2
    while o:
        v = v + v[..., idx ^ o]
        o >>= 1
    return v[..., 0]


def _block_sums(t):
    """block_sum (cg.hpp) of every block of RB consecutive thread values: 64-lane butterfly, then the four wave sums in order"""
    nb = -(-t.size // RB)
    p = np.zeros(nb * RB)
    p[:t.size] = t
    w = _butterfly(p.reshape(nb, RB // 64, 64), 64)
    s = np.zeros(nb)
    for k in range(RB // 64):
        s = s + w[:, k]
    return s


def _strided_sum(parts, limit=None):
    """the one-block sum of per-block partials: thread t adds parts[t], parts[t + RB], ... in order, then block_sum"""
    if limit is not None:
        parts = parts[:limit]
    nt = -(-parts.size // RB)
    p = np.zeros(nt * RB)
    p[:parts.size] = parts
    acc = np.zeros(RB)
    for k in range(nt):
        acc = acc + p[k * RB:(k + 1) * RB]
    return float(_block_sums(acc)[0])


def _dot_device(u, v, limit=None):
    return _strided_sum(_block_sums(u * v), limit)


def _spmv_seq(sy, d, row_cap=None):
    """every row summed entry by entry in its stored order"""
    prod = sy.values * d[sy.colind]
    starts, lens = sy.rowptr[:-1], np.diff(sy.rowptr)
    if row_cap is not None:
        lens = np.minimum(lens, row_cap)
    y = np.zeros(sy.n)
    long_rows = np.nonzero(lens > 64)[0]
    short = lens.copy()
    short[long_rows] = 0
    for p in range(int(short.max()) if sy.n else 0):
        act = np.nonzero(short > p)[0]
        y[act] = y[act] + prod[starts[act] + p]
    for r in long_rows:
        y[r] = _seq_sum(prod[starts[r]:starts[r] + lens[r]])
    return y


def _spmv_device(sy, d, row_cap=None):
    """cg_spmv_kernel: lane sub of a row adds its entries sub, sub + 16, ... in order, then the 16-lane butterfly"""
    prod = sy.values * d[sy.colind]
    starts, lens = sy.rowptr[:-1], np.diff(sy.rowptr)
    if row_cap is not None:
        lens = np.minimum(lens, row_cap)
    lanes = np.zeros((sy.n, ROW_LANES))
    sub = np.arange(ROW_LANES)
    for t in range(-(-int(lens.max()) // ROW_LANES) if sy.n else 0):
        act = np.nonzero(lens > t * ROW_LANES)[0]
        pos = t * ROW_LANES + sub[None, :]
        ok = pos < lens[act][:, None]
        k = np.where(ok, starts[act][:, None] + pos, 0)
        lanes[act] = lanes[act] + np.where(ok, prod[k], 0.0)
    return _butterfly(lanes, ROW_LANES)


def _dy_device(d, y, limit=None):
    """the partial of d . y per SpMV block (16 rows, the value in the row's lane 0), then the strided sum"""
    t = np.zeros(d.size * ROW_LANES)
    t[::ROW_LANES] = d * y
    return _strided_sum(_block_sums(t), limit)


def recurrences(case, order, vec_parts=None, spmv_parts=None, row_cap=None, precond_in_d=True, m=None):
    """The recurrences of solver_cg.hpp:76-131 in IEEE double -> (x_1..x_M, rr_1..rr_M).  order "seq": every sum entry by entry;
    "dev": the device's stated order.  The switches plant defects (device order only for the first two): vec_parts / spmv_parts = sum
    only that many of the vector / SpMV per-block partials; row_cap = stop each row at that entry; precond_in_d = False applies
    1 / diag in rho and not in the search direction."""
    sy = system(case)
    tr = truth(case)
    m = len(tr.rr) if m is None else m
    pre = case.precond
    if order == "seq":
        dot = lambda u, v: _seq_sum(u * v)
        dy = dot
        spmv = lambda d: _spmv_seq(sy, d, row_cap)
    else:
        dot = lambda u, v: _dot_device(u, v, vec_parts)
        dy = lambda d, y: _dy_device(d, y, spmv_parts)
        spmv = lambda d: _spmv_device(sy, d, row_cap)
    iA = 1.0 / sy.diag
    x = np.zeros(sy.n)
    r = sy.b.copy()
    z = iA * r if pre else r
    d = (z if precond_in_d else r).copy()
    nr0 = math.sqrt(dot(r, r))
    rho = dot(r, z)
    xs, rrs = [], []
    with np.errstate(all="ignore"):
        for _ in range(m):
            y = spmv(d)
            alpha = rho / dy(d, y)
            x = x + alpha * d
            r = r - alpha * y
            xs.append(x.copy())
            rrs.append(math.sqrt(dot(r, r)) / nr0)
            z = iA * r if pre else r
            rho_new = dot(r, z)
            d = (z if precond_in_d else r) + (rho_new / rho) * d
            rho = rho_new
    return xs, rrs


def errors(case, xs):
    """the scaled error of x_1.. against truth"""
    tr, diag = truth(case), system(case).diag
    return [scaled_error(x, t, diag) for x, t in zip(xs, tr.x)]


@functools.lru_cache(maxsize=None)
def e_ref(case):
    """per m: the error of the double recurrences against truth, worst of the sequential and the device's order"""
    return tuple(max(a, b) for a, b in zip(errors(case, recurrences(case, "seq")[0]), errors(case, recurrences(case, "dev")[0])))


def gate(e):
    return max(FLOOR, MARGIN * e)


def judged(case):
    """the m (1-based) of the case whose pair is judged: e_ref <= CAP"""
    return [j + 1 for j, e in enumerate(e_ref(case)) if e <= CAP]


def pow2_ceil(v):
    return 2.0 ** math.ceil(math.log2(v))


# ---- exits ---------------------------------------------------------------------------------------------------------------------
HUGE = 1e300


def expected_exit(rr, tol, div, max_iter):
    """(reason, iterations, index of the iterate returned) the exit order of solver_cg.hpp:113-126 gives on the residual history rr;
    None if the history ends first"""
    it = 0
    for j, v in enumerate(rr):
        if v < tol:
            return 0, it, j
        if it > max_iter:
            return 2, it, j
        if v > div:
            return 1, it, j
        it += 1
    return None


def iterate_call(case, m):
    """the thresholds that return x_m, and the (reason, iterations) they give on truth's history"""
    rr = truth(case).rr
    if m == 1:
        # div = 0: out after the first update.  Where CG has terminated exactly there (n = 1, a diagonal matrix under Jacobi) the
        # device's residual is rounding noise or zero, and `rr > 0` is no safe comparison: leave on the convergence test instead
        kw = dict(tol=0.5, div=HUGE, max_iter=1000) if rr[0] < EXACT else dict(tol=0.0, div=0.0, max_iter=1000)
    else:
        kw = dict(tol=0.0, div=HUGE, max_iter=m - 2)
    want = expected_exit(rr, **kw)
    assert want is not None and want[2] == m - 1
    return kw, want[:2]


def threshold_calls(case):
    """exits on tol and on div at geometric means of two successive truth residuals (no comparison within rounding of a threshold;
    thresholds_clear says so), with max_iter as the backstop where the history ends"""
    # (only as far as the pairs are judged: beyond, the double recurrences have left truth's residuals too)
    er = e_ref(case)
    M = next((j for j, e in enumerate(er) if e > CAP), len(er))
    rr = truth(case).rr[:M]
    out = []
    if M < 2 or rr[M - 1] < EXACT and M < 3:
        return out
    last = M - 1 if rr[M - 1] >= EXACT else M - 2           # the last residual that is not the exact zero
    for a in sorted({0, last - 1}):
        gm = math.sqrt(rr[a] * rr[a + 1])
        out.append(dict(tol=gm, div=HUGE, max_iter=M - 2))
        out.append(dict(tol=0.0, div=gm, max_iter=M - 2))
    return [(kw, expected_exit(rr, **kw)) for kw in out]


def thresholds_clear(case, kw):
    """every residual of the history the call can see is a factor 1.001 away from both thresholds"""
    rr = truth(case).rr[:kw["max_iter"] + 2]
    return all(abs(math.log(v / t)) > 1e-3 for v in rr if v >= EXACT for t in (kw["tol"], kw["div"]) if 0.0 < t < HUGE)


# ---- the report ----------------------------------------------------------------------------------------------------------------
HEADER = """tests/test_gpu_cg_twin.py on one MI355X (CG_TWIN_PROFILE=this file python -m pytest tests/test_gpu_cg_twin.py -m gpu -s).
Every case of tests/cg_twin.py and every iterate x_m the test takes from pa_conjugated_gradient, m = 1..min(8, n).  e_ref = the error
of the recurrences of solver_cg.hpp:76-131 in IEEE double against the truth (mpmath at 50 digits up to 4097 rows, longdouble above),
worst of the sequential and the device's summation order, computed on the CPU (tests/test_cg_twin_cpu.py); device = the kernel's
error against the same truth; both in the norm max |dx_i| sqrt(A_ii) / max |x_i| sqrt(A_ii).  Cases: n rows, band {1, 5, 17} with or
without the arrowhead row / column 0, L = every row of exactly L entries, rev = columns of a row descending, jacobi / plain =
preconditioner on / off.
"""


def table_lines(device=None, device_rr=None):
    """e_ref (and, given device[(case, m)] = error, the device's error and its share of the gate) for every case and m;
    device_rr[(case, m)] = the share of the gate the relative residual's error takes"""
    lines, dropped, worst, worst_pre = [], [], (0.0, None), 0.0
    npairs = 0
    for c in case_table():
        er = e_ref(c)
        for j, e in enumerate(er):
            npairs += 1
            kept = e <= CAP
            if not kept:
                dropped.append((c, j + 1, e))
            if c.precond:
                worst_pre = max(worst_pre, e)
            s = "  %-28s m %d  e_ref %9.3e  gate %9.3e%s" % (case_id(c), j + 1, e, gate(e), "" if kept else "  (left out: e_ref > 1e-10)")
            if device is not None and (c, j + 1) in device:
                eg = device[(c, j + 1)]
                s += "  device %9.3e  device/gate %6.3f" % (eg, eg / gate(e))
                if kept and eg / gate(e) > worst[0]:
                    worst = (eg / gate(e), "%s m %d" % (case_id(c), j + 1))
            lines.append(s)
    head = ["pairs %d, left out %d (%.1f %%), largest kept e_ref %.3e" % (npairs, len(dropped), 100.0 * len(dropped) / npairs,
                                                                        max(e for c in case_table() for e in e_ref(c) if e <= CAP)),
            "largest e_ref of the preconditioned pairs %.3e -> floor 2^%d = %.3e; gate = max(floor, 10 e_ref)" %
            (worst_pre, round(math.log2(pow2_ceil(worst_pre))), pow2_ceil(worst_pre)),
            "left out: " + (", ".join("%s m %d (%.1e)" % (case_id(c), m, e) for c, m, e in dropped) or "none")]
    if device is not None:
        head.append("worst device error / gate of the judged pairs: %.3f (%s)" % worst)
    if device_rr:
        k = max(device_rr, key=device_rr.get)
        head.append("worst error of the reported relative residual / gate of the judged pairs: %.3f (%s m %d)" % (device_rr[k], case_id(k[0]), k[1]))
    return HEADER.split("\n")[:-1] + head + lines
