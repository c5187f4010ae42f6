"""A twin of the smoothed coarse levels and the multilevel conjugate gradient (proton_amd/csrc/multilevel_precond.hip; the
recurrences of solver_cg.hpp:63-144 with
  z = sum_p R_p^T A_p^-1 R_p r + sum_l P_l diag(P_l^T A P_l)^-1 P_l^T r + P_c (P_c^T A P_c)^-1 P_c^T r),
written the way tests/coarse_twin.py is, which it imports and leaves alone.

No device here.  This module holds
  * table(...): coarse_twin.table's hats -- the same 1-D hats (coarse_twin.hats), the same products, modes and column order -- face by
    face instead of dense over (face, node), and without the refusal above 4096 columns: the tables of smoothed levels;
  * seeded cases: coarse_twin's systems and tables, a table of 5000 columns of 1 to 70 entries on 20 011 rows (every length next to
    a multiple of 16 is there) and a table with one column of 5000 entries;
  * diagonal / apply / pcg over the number type: numpy.longdouble (the truth) and IEEE double in the kernels' order -- entry e of a
    column to slot e mod 64, a slot's entries ascending, the halving tree 32 .. 1; a row's gather in entry order -- with switches
    that plant the defects the tests are there to catch.  (The kernels fuse every multiply-add; the restatement rounds twice.  That
    is inside what e_ref measures.);
  * e_ref: the error of the double restatement against the truth in cg_twin's norm, the gate max(2^-45, 10 e_ref);
  * multilevel_iterations: a plain double PCG that counts iterations on the oracle's condensed systems."""
import functools
import math
from collections import namedtuple

import numpy as np

import cg_twin as T
import coarse_twin as CT
import patch_pcg_twin as PT

MAX_NODES, MAX_LEVELS = 1 << 24, 8         # PA_SMOOTHED_MAX_NODES, PA_MULTILEVEL_MAX_LEVELS
FLOOR, MARGIN, CAP, M_MAX = T.FLOOR, T.MARGIN, T.CAP, 8
Table = CT.Table


# ---- the table of the face-only numbering, any number of columns ----------------------------------------------------------------------
def table(Nx, Ny, H, fbs, compress, face_pts, num_other, face_side=None, where=0, max_nodes=MAX_NODES):
    """coarse_twin.table (its arguments, its Table) face by face -> Table, or None without an interior node or beyond max_nodes"""
    hx, hy = CT.hats(Nx, H)[1:-1], CT.hats(Ny, H)[1:-1]               # interior lines only
    nix, niy = hx.shape[0], hy.shape[0]
    if nix < 1 or niy < 1:
        return None
    nn = nix * niy
    nzx = [np.nonzero(hx[:, i])[0] for i in range(Nx + 1)]
    nzy = [np.nonzero(hy[:, i])[0] for i in range(Ny + 1)]
    fp = np.asarray(face_pts, dtype=np.int64)
    comp = np.asarray(compress, dtype=np.int64)
    live = np.nonzero(comp >= 0)[0]
    live = live[np.argsort(comp[live])]
    assert live.size == num_other
    per_face = []
    for f in live:
        ax, ay, bx, by = fp[f, 0] % (Nx + 1), fp[f, 0] // (Nx + 1), fp[f, 1] % (Nx + 1), fp[f, 1] // (Nx + 1)
        nodes, v0, v1 = [], [], []
        for jy in np.union1d(nzy[ay], nzy[by]):
            for jx in np.union1d(nzx[ax], nzx[bx]):
                fa, fb = hy[jy, ay] * hx[jx, ax], hy[jy, by] * hx[jx, bx]
                if fa != 0.0 or fb != 0.0:
                    nodes.append(jy * nix + jx); v0.append(0.5 * (fa + fb)); v1.append(0.5 * (fb - fa))
        per_face.append((np.asarray(nodes, dtype=np.int64), np.asarray(v0), np.asarray(v1)))
    if face_side is None:
        index, ncoarse = np.arange(2 * nn) % nn, nn
        part = np.zeros(live.size, dtype=np.int64)
    else:
        side = np.asarray(face_side)[live]
        part = ((side != 2) & (side != where)).astype(np.int64)
        used = np.zeros(2 * nn, dtype=bool)
        for q, (nodes, _, _) in enumerate(per_face):
            used[part[q] * nn + nodes] = True
        index = np.full(2 * nn, -1, dtype=np.int64)
        index[used] = np.arange(int(used.sum()))
        ncoarse = int(used.sum())
    if ncoarse < 1 or ncoarse > max_nodes:
        return None
    ptr = np.zeros(num_other * fbs + 1, dtype=np.int64)
    cols, vals = [np.zeros(0, dtype=np.int64)], [np.zeros(0)]
    for q, (nodes, v0, v1) in enumerate(per_face):
        col = index[part[q] * nn + nodes]
        cols.append(col); vals.append(v0)
        ptr[q * fbs + 1] = nodes.size
        if fbs >= 2:
            odd = v1 != 0.0
            cols.append(col[odd]); vals.append(v1[odd])
            ptr[q * fbs + 2] = int(odd.sum())
    np.cumsum(ptr, out=ptr)
    return Table(ptr, np.concatenate(cols).astype(np.int32), np.concatenate(vals), ncoarse)


def level_tables(hs, build):
    """the tables of a level set: build(H) for every H of hs, each H dividing the next"""
    assert all(b % a == 0 for a, b in zip(hs, hs[1:])) and len(hs) <= MAX_LEVELS
    return [build(h) for h in hs]


# ---- the generic cases ----------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "n ncoarse kind")           # kind "ct": coarse_twin.coarse; "wide", "long": the two tables beyond it
WIDE, LONG = Case(20011, 5000, "wide"), Case(5003, 3, "long")
EDGE_LENGTHS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 70)


def case_id(c):
    return "n%d-c%d%s" % (c.n, c.ncoarse, "" if c.kind == "ct" else "-" + c.kind)


def case_table():
    return [Case(c.n, c.ncoarse, "ct") for c in CT.case_table()] + [WIDE, LONG]


def system(case):
    return PT.system(PT.Case(case.n))


def _from_pairs(n, nc, rows, cols, vals):
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=ptr[1:])
    assert np.diff(ptr).max() <= CT.MAX_ROW
    out = Table(ptr, cols.astype(np.int32), vals, nc)
    for a in out[:3]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def level(case):
    """the table of a case.  wide: column j holds 1 to 70 rows out of the 160 around j n / ncoarse, every length of EDGE_LENGTHS
    among them, a row in at most 4 columns.  long: column 1 holds rows 0 .. 4999, columns 0 and 2 a few rows at the two ends"""
    n, nc, kind = case
    if kind == "ct":
        return CT.coarse(CT.Case(n, nc))
    rng = np.random.default_rng([20260114, n, nc])
    if kind == "long":
        rows = np.concatenate([[0, 1], np.arange(5000), [1, 7, 5000, 5001]])          # (row 1 in all three, row 5002 in none)
        cols = np.concatenate([[0, 0], np.ones(5000, dtype=np.int64), [2, 2, 2, 2]])
    else:
        lens = rng.integers(1, 21, nc)
        lens[np.arange(len(EDGE_LENGTHS)) * 331 + 200] = EDGE_LENGTHS
        count = np.zeros(n, dtype=np.int64)
        rows, cols = [], []
        for j in range(nc):
            c = j * n // nc
            win = np.arange(max(0, c - 80), min(n, c + 80))
            win = win[count[win] < CT.MAX_ROW]
            pick = rng.choice(win, size=int(lens[j]), replace=False)
            count[pick] += 1
            rows.append(pick); cols.append(np.full(pick.size, j))
        rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = rng.uniform(0.25, 1.0, rows.size) * rng.choice([-1.0, 1.0], rows.size)
    return _from_pairs(n, nc, rows.astype(np.int64), cols.astype(np.int64), vals)


def column_lengths(tb):
    return np.bincount(tb.cols, minlength=tb.ncoarse)


def lanes_per_column(tb):
    """the host's choice (pa_smoothed_level_info.lanes_per_column)"""
    return 16 if tb.ptr[-1] <= 32 * tb.ncoarse else 64


# ---- a column's sum -------------------------------------------------------------------------------------------------------------------
def _ft(mode):
    return np.longdouble if mode == "ld" else np.float64


@functools.lru_cache(maxsize=None)
def _transposed(key):
    tb = _TABLES[key]
    rows = np.repeat(np.arange(tb.ptr.size - 1), np.diff(tb.ptr))
    order = np.lexsort((rows, tb.cols))                                # by column, fine rows ascending
    start = np.zeros(tb.ncoarse + 1, dtype=np.int64)
    np.cumsum(np.bincount(tb.cols, minlength=tb.ncoarse), out=start[1:])
    local = np.arange(order.size) - start[tb.cols[order]]
    return order, rows[order], tb.cols[order].astype(np.int64), local


_TABLES = {}


def transposed(tb):
    """-> (entry of P per entry of P^T, its fine row, its column, its place within the column)"""
    key = id(tb.ptr)
    _TABLES[key] = tb
    return _transposed(key)


def column_sums(tb, contrib, mode):
    """sum of contrib (one per entry of P^T, in P^T's order) per column: "ld" in longdouble; "f64" slot e mod 64, a slot's entries
    ascending, then the tree 32, 16, 8, 4, 2, 1"""
    _, _, col, local = transposed(tb)
    if mode == "ld":
        out = np.zeros(tb.ncoarse, dtype=np.longdouble)
        np.add.at(out, col, contrib.astype(np.longdouble))
        return out
    acc = np.zeros((tb.ncoarse, 64))
    for k in range(int(local.max()) // 64 + 1 if local.size else 0):
        sel = local // 64 == k
        acc[col[sel], local[sel] % 64] += contrib[sel]                 # (one entry per (column, slot) in a round)
    for o in (32, 16, 8, 4, 2, 1):
        acc[:, :o] = acc[:, :o] + acc[:, o:2 * o]
    return acc[:, 0].copy()


def diagonal(sy, tb, mode, from_A=False):
    """d_j = sum_i P_ij t_ij, t_ij = sum_k A_ik P_kj over row i of A in its entry order.  Defect: from_A = the diagonal of A at the
    column's first row instead"""
    ft = _ft(mode)
    order, row, col, _ = transposed(tb)
    if from_A:
        first = np.full(tb.ncoarse, -1, dtype=np.int64)
        first[col[::-1]] = row[::-1]
        return sy.diag.astype(ft)[first]
    av, pv = sy.values.astype(ft), tb.vals.astype(ft)
    look = {}
    rows = np.repeat(np.arange(tb.ptr.size - 1), np.diff(tb.ptr))
    for q in range(tb.cols.size):
        look[(int(rows[q]), int(tb.cols[q]))] = pv[q]
    contrib = np.zeros(order.size, dtype=ft)
    for e in range(order.size):
        i, j = int(row[e]), int(col[e])
        t = ft(0)
        for m in range(sy.rowptr[i], sy.rowptr[i + 1]):
            p = look.get((int(sy.colind[m]), j))
            if p is not None:
                t = t + av[m] * p
        contrib[e] = pv[order[e]] * t
    return column_sums(tb, contrib, mode)


def apply(tb, d, r, mode, z0=None, twice=False):
    """z = z0 + P D^-1 P^T r: the restriction by column_sums, u = (1 / d) * sum, the gather of a row in entry order onto z0.
    Defect: twice = the level applied twice"""
    ft = _ft(mode)
    n = tb.ptr.size - 1
    order, row, _, _ = transposed(tb)
    pv, rv = tb.vals.astype(ft), r.astype(ft)
    u = (ft(1) / d.astype(ft)) * column_sums(tb, pv[order] * rv[row], mode)
    z = np.zeros(n, dtype=ft) if z0 is None else z0.astype(ft).copy()
    sizes = np.diff(tb.ptr)
    for _ in range(2 if twice else 1):
        for l in range(CT.MAX_ROW):
            act = np.nonzero(sizes > l)[0]
            q = tb.ptr[act] + l
            z[act] = z[act] + pv[q] * u[tb.cols[q]]
    return z


@functools.lru_cache(maxsize=None)
def diag_of(case, mode):
    return diagonal(system(case), level(case), mode)


def test_vectors(case):
    return PT.test_vectors(PT.Case(case.n))


@functools.lru_cache(maxsize=None)
def apply_truth(case, which, accumulate=False):
    r = test_vectors(case)[which]
    return apply(level(case), diag_of(case, "ld"), r, "ld", test_vectors(case)[1 - which] if accumulate else None)


def apply_double(case, which, accumulate=False, d=None, **defect):
    r = test_vectors(case)[which]
    return apply(level(case), diag_of(case, "f64") if d is None else d, r, "f64", test_vectors(case)[1 - which] if accumulate else None,
                 **defect)


def scaled_error(case, z, ref):
    return T.scaled_error(z, ref, system(case).diag)


@functools.lru_cache(maxsize=None)
def apply_e_ref(case):
    return max(scaled_error(case, apply_double(case, w, acc), apply_truth(case, w, acc)) for w in (0, 1) for acc in (False, True))


def dinv_error(case, dinv):
    """max |dinv_j d_j - 1| against the truth's d_j"""
    return float(np.max(np.abs(np.asarray(dinv, dtype=np.longdouble) * diag_of(case, "ld") - 1)))


@functools.lru_cache(maxsize=None)
def dinv_e_ref(case):
    return dinv_error(case, 1.0 / diag_of(case, "f64"))


def gate(e):
    return max(FLOOR, MARGIN * e)


# ---- the recurrences ------------------------------------------------------------------------------------------------------------------
Truth = namedtuple("Truth", "x rr")
Solve = namedtuple("Solve", "n levels exact")         # ncoarse of the smoothed levels' tables, of the exact table or None


def solve_id(s):
    return "n%d-l%s-e%s" % (s.n, "+".join(map(str, s.levels)) or "0", s.exact)


def solve_table():
    """0, 1 and 3 smoothed levels, with and without an exact level, on coarse_twin's 257 rows; one case of several blocks"""
    return [Solve(257, (), None), Solve(257, (), 33), Solve(257, (65,), None), Solve(257, (65,), 31), Solve(257, (65, 33, 31), None),
            Solve(257, (65, 33, 31), 2), Solve(4097, (1025,), 257)]


def solve_levels(s):
    return [level(Case(s.n, nc, "ct")) for nc in s.levels], (level(Case(s.n, s.exact, "ct")) if s.exact else None)


def preconditioner(sy, pt, pfac, levels, exact, mode, order=None, **defect):
    """r -> z: the patch sum, the levels in `order` (default: as given), the exact level.  **defect: those of diagonal (from_A) and of
    apply (twice), planted in level 0"""
    ds = [diagonal(sy, tb, mode, from_A=(k == 0 and defect.get("from_A", False))) for k, tb in enumerate(levels)]
    cfac = CT.factor(CT.galerkin(sy, exact, mode), mode) if exact is not None else None

    def M(r):
        z = PT.apply(pt, pfac, r, mode)
        for k in (order if order is not None else range(len(levels))):
            z = apply(levels[k], ds[k], r, mode, z, twice=(k == 0 and defect.get("twice", False)))
        return CT.apply(exact, cfac, r, mode, z) if exact is not None else z
    return M


def pcg(s, mode, m=None, order=None, **defect):
    """solver_cg.hpp:76-131 with the multilevel z -> (x_1..x_m, |r_j| / |r_0|), as coarse_twin.pcg"""
    b = PT.Case(s.n)
    sy = PT.system(b)
    m = min(M_MAX, s.n) if m is None else m
    levels, exact = solve_levels(s)
    M = preconditioner(sy, PT.patches(b), PT.factors(b, mode), levels, exact, mode, order, **defect)
    starts = sy.rowptr[:-1]
    if mode == "ld":
        dot = dy = lambda u, v: np.sum(u * v)
        root = np.sqrt
        vals = sy.values.astype(np.longdouble)
        spmv = lambda d: np.add.reduceat(vals * d[sy.colind], starts)
    else:
        dot, dy, root = T._dot_device, T._dy_device, math.sqrt
        spmv = lambda d: T._spmv_device(sy, d)
    x = np.zeros(s.n, dtype=_ft(mode))
    r = sy.b.astype(_ft(mode)).copy()
    z = M(r)
    d = z.copy()
    nr0 = root(dot(r, r))
    rho = dot(r, z)
    xs, rrs = [], []
    with np.errstate(all="ignore"):
        for _ in range(m):
            y = spmv(d)
            alpha = rho / dy(d, y)
            x = x + alpha * d
            r = r - alpha * y
            rr = root(dot(r, r)) / nr0
            xs.append(x.copy())
            rrs.append(float(rr))
            if mode == "ld" and rr < 1e-17:
                break
            z = M(r)
            rho_new = dot(r, z)
            d = z + (rho_new / rho) * d
            rho = rho_new
    return Truth(xs, rrs)


@functools.lru_cache(maxsize=None)
def truth(s):
    return pcg(s, "ld")


def errors(s, xs):
    diag = PT.system(PT.Case(s.n)).diag
    return [T.scaled_error(x, t, diag) for x, t in zip(xs, truth(s).x)]


@functools.lru_cache(maxsize=None)
def e_ref(s):
    return tuple(errors(s, pcg(s, "f64", len(truth(s).rr)).x))


def judged(s):
    return [j + 1 for j, e in enumerate(e_ref(s)) if e <= CAP]


def iterate_call(s, m):
    """the thresholds that make the solver return x_m (tests/cg_twin.py) and the (reason, iterations) the truth's history gives"""
    rr = truth(s).rr
    if m == 1:
        kw = dict(tol=0.5, div=T.HUGE, max_iter=1000) if rr[0] < T.EXACT else dict(tol=0.0, div=0.0, max_iter=1000)
    else:
        kw = dict(tol=0.0, div=T.HUGE, max_iter=m - 2)
    want = T.expected_exit(rr, **kw)
    assert want is not None and want[2] == m - 1
    return kw, want[:2]


def dense_preconditioner(s):
    """M as a matrix, in longdouble rounded to double: column k is M e_k"""
    b = PT.Case(s.n)
    levels, exact = solve_levels(s)
    M = preconditioner(PT.system(b), PT.patches(b), PT.factors(b, "ld"), levels, exact, "ld")
    eye = np.eye(s.n)
    return np.stack([np.asarray(M(eye[k]), dtype=np.float64) for k in range(s.n)], axis=1)


# ---- iteration counts on the oracle's condensed systems --------------------------------------------------------------------------------
def multilevel_iterations(sysm, pt, levels, exact, tol=1e-13, max_iter=20000):
    """textbook PCG in double from x = 0 to |r| / |r_0| < tol with z = (patch sum) + sum_l P_l D_l^-1 P_l^T r + (the exact level's
    term, exact None: none), as coarse_twin.two_level_iterations"""
    import scipy.linalg as sl
    import scipy.sparse as sp
    n = sysm.b.size
    A = sp.csr_matrix((sysm.values, sysm.colind, sysm.rowptr), shape=(n, n))
    mats = [sp.csr_matrix((tb.vals, tb.cols, tb.ptr), shape=(n, tb.ncoarse)) for tb in levels]
    dinv = [1.0 / np.asarray((Pm.multiply(A @ Pm)).sum(axis=0)).ravel() for Pm in mats]
    if exact is not None:
        Pe = sp.csr_matrix((exact.vals, exact.cols, exact.ptr), shape=(n, exact.ncoarse))
        cho = sl.cho_factor((Pe.T @ A @ Pe).toarray())
    Ap = PT.patch_matrices(sysm.rowptr, sysm.colind, sysm.values, pt)
    inv = np.linalg.inv(Ap)
    sizes = np.diff(pt.ptr)
    Pw = Ap.shape[1]
    live = np.arange(Pw)[None, :] < sizes[:, None]
    ent = np.where(live, pt.ptr[:-1, None] + np.arange(Pw)[None, :], 0)
    idx = pt.rows[ent].astype(np.int64)

    def M(r):
        zp = np.einsum("pij,pj->pi", inv, np.where(live, r[idx], 0.0))
        z = np.zeros(n)
        np.add.at(z, idx[live], zp[live])
        for Pm, di in zip(mats, dinv):
            z = z + Pm @ (di * (Pm.T @ r))
        return z + Pe @ sl.cho_solve(cho, Pe.T @ r) if exact is not None else z
    x = np.zeros(n)
    r = sysm.b.copy()
    z = M(r)
    d = z.copy()
    rho = r @ z
    nr0 = math.sqrt(r @ r)
    for it in range(1, max_iter + 1):
        y = A @ d
        alpha = rho / (d @ y)
        x += alpha * d
        r -= alpha * y
        if math.sqrt(r @ r) / nr0 < tol:
            return it
        z = M(r)
        rho_new = r @ z
        d = z + (rho_new / rho) * d
        rho = rho_new
    return max_iter
