"""A twin of the two-level conjugate gradient on the ROW-PARTITIONED system (proton_amd/csrc/rows_precond.hip; the recurrences of
solver_cg.hpp:63-144 with  z = sum_p R_p^T A_p^-1 R_p r + P (P^T A P)^-1 P^T r  where every rank holds a range of rows, its own
patches and its own rows of P), built on tests/patch_pcg_twin.py and tests/coarse_twin.py, which it imports and does not restate.

No device here.  This module holds
  * the tables of a slab: bounds (the rows a slab of cell rows owns, in closed form), truncate_patches (pa_condensed_rows_patches'
    rule: a patch belongs to one slab and loses every row outside it; keep_foreign plants the defect), split_patches (for the
    generic cases, whose patches belong to nobody: every patch cut at the slab boundaries), slab_coarse (rows of P, pointer rebased);
  * galerkin_rows: A_c as the ranks form it, sum over the ranks of P_r^T (A_r P_window), against coarse_twin.galerkin's P^T A P;
    drop_ghosts plants the defect of a window that holds the rank's own rows of P only;
  * pcg: the recurrence over the number type, by two routes: global (one table, one sum per dot product) and by ranks (bounds given:
    every sum grouped by rank and added in rank order, the coarse matrix from galerkin_rows, the restriction rank by rank).  In exact
    arithmetic the two are the same sequence: the partition enters through the patch table alone;
  * truth / e_ref / gate as the other twins have them: truth in longdouble, e_ref the by-ranks route in IEEE double with cg_twin's
    restatement of the device's reductions, gate max(2^-45, 10 e_ref)."""
import functools
import math
from collections import namedtuple

import numpy as np

import cg_twin as T
import coarse_twin as CT
import patch_pcg_twin as PT

FLOOR, MARGIN, CAP, M_MAX = T.FLOOR, T.MARGIN, T.CAP, T.M_MAX
# two longdouble routes to a judged iterate: double's own error there is at most CAP, longdouble carries 11 more bits
ROUTES_AGREE = 2.0 * CAP * 2.0 ** -11

# the generic case of the device tests and its partitions into 2, 3 and 4 ranks: uneven, no boundary on a multiple of 256, every
# rank with more rows than the 17 its neighbours read of it
CASE = CT.Case(257, 33)
PARTITIONS = ((0, 100, 257), (0, 60, 130, 257), (0, 50, 120, 200, 257))
# the mesh of the device's comparison with the point Jacobi: (N, k, H, slabs), pair (k + 1, k); tests/test_rows_pcg_cpu.py says why
SOLVE_MESH = (24, 1, 4, (0, 10, 24))


# ---- the tables of a slab -------------------------------------------------------------------------------------------------------------
def bounds(Nx, Ny, parts, fbs):
    """the rows [row_begin, row_end) of the slabs of cell rows parts[s] .. parts[s + 1] (structured_mesh.hpp: the non-Dirichlet faces
    below face row j number Nx - 1 + (j - 1) (2 Nx - 1), j >= 1)"""
    first = lambda j: 0 if j == 0 else (Nx - 1) + (j - 1) * (2 * Nx - 1)
    return [(first(a) * fbs, first(b) * fbs) for a, b in zip(parts[:-1], parts[1:])]


def cell_owner(Nx, parts, npatches):
    """the slab of every cell patch of a mesh whose cells all have a non-Dirichlet face (Nx, Ny >= 2): patch p is cell p"""
    rows = np.arange(npatches) // Nx
    return np.searchsorted(np.asarray(parts), rows, side="right") - 1


def row_owner(pt, bnds):
    """the slab that owns the first row of every patch (a face patch lies in one slab)"""
    return np.searchsorted(np.asarray([b[1] for b in bnds]), pt.rows[pt.ptr[:-1]], side="right")


def _table(plist):
    ptr = np.zeros(len(plist) + 1, dtype=np.int64)
    if plist:
        np.cumsum([p.size for p in plist], out=ptr[1:])
    rows = np.concatenate(plist).astype(np.int32) if plist else np.zeros(0, dtype=np.int32)
    return PT.Patches(ptr, rows)


def truncate_patches(pt, owner, bnds, keep_foreign=False):
    """per slab: its patches in the table's order, every row outside the slab deleted (a patch left empty is dropped), the rows as
    global indices.  keep_foreign: nothing is deleted (the defect: a cell patch that keeps the row of the slab above)"""
    out = []
    for s, (r0, r1) in enumerate(bnds):
        plist = []
        for p in np.nonzero(np.asarray(owner) == s)[0]:
            rows = pt.rows[pt.ptr[p]:pt.ptr[p + 1]]
            if not keep_foreign:
                rows = rows[(rows >= r0) & (rows < r1)]
            if rows.size:
                plist.append(rows)
        out.append(_table(plist))
    return out


def split_patches(pt, bnds):
    """per slab: the part of every patch that lies in it, in the table's order (the generic cases)"""
    out = []
    for r0, r1 in bnds:
        plist = []
        for p in range(pt.ptr.size - 1):
            rows = pt.rows[pt.ptr[p]:pt.ptr[p + 1]]
            rows = rows[(rows >= r0) & (rows < r1)]
            if rows.size:
                plist.append(rows)
        out.append(_table(plist))
    return out


def concat(tables):
    return _table([t.rows[t.ptr[p]:t.ptr[p + 1]] for t in tables for p in range(t.ptr.size - 1)])


def slab_coarse(tb, r0, r1):
    """rows [r0, r1) of P: the same columns, the pointer rebased to 0"""
    a, b = tb.ptr[r0], tb.ptr[r1]
    return CT.Table(tb.ptr[r0:r1 + 1] - a, tb.cols[a:b], tb.vals[a:b], tb.ncoarse)


def slab_rows(sy, r0, r1):
    """rows [r0, r1) of the CSR system with global columns, the pointer rebased -> (rowptr, colind, values, b)"""
    a, b = sy.rowptr[r0], sy.rowptr[r1]
    return sy.rowptr[r0:r1 + 1] - a, sy.colind[a:b], sy.values[a:b], sy.b[r0:r1]


# ---- the coarse matrix as the ranks form it -------------------------------------------------------------------------------------------
def _ft(mode):
    return np.longdouble if mode == "ld" else np.float64


def galerkin_rows(sy, tb, bnds, mode, drop_ghosts=False):
    """sum over the ranks, in rank order, of P_r^T (A_r P_window): per rank coarse_twin.galerkin's loops over its rows, the lower
    triangle; mirrored after the sum.  drop_ghosts: the window holds the rank's own rows of P only (the defect)"""
    ft = _ft(mode)
    nc = tb.ncoarse
    vals, pv = sy.values.astype(ft), tb.vals.astype(ft)
    total = np.zeros((nc, nc), dtype=ft)
    for r0, r1 in bnds:
        Ac = np.zeros((nc, nc), dtype=ft)
        for i in range(r0, r1):
            w = {}
            for e in range(sy.rowptr[i], sy.rowptr[i + 1]):
                c = sy.colind[e]
                if drop_ghosts and not (r0 <= c < r1):
                    continue
                for q in range(tb.ptr[c], tb.ptr[c + 1]):
                    j = tb.cols[q]
                    v = vals[e] * pv[q]
                    w[j] = w[j] + v if j in w else v
            for q in range(tb.ptr[i], tb.ptr[i + 1]):
                j = tb.cols[q]
                for c, wv in w.items():
                    if c <= j:
                        Ac[j, c] = Ac[j, c] + pv[q] * wv
        total = total + Ac
    return np.tril(total) + np.tril(total, -1).T


# ---- the recurrence -------------------------------------------------------------------------------------------------------------------
Truth = namedtuple("Truth", "x rr")


def _coarse_apply(tb, fac, r, z, mode, bnds):
    """z + P W^T W P^T r; bnds: the restriction rank by rank, added in rank order"""
    ft = _ft(mode)
    n = tb.ptr.size - 1
    rows = np.repeat(np.arange(n), np.diff(tb.ptr))
    pv = tb.vals.astype(ft)
    prod = pv * r.astype(ft)[rows]
    rc = np.zeros(tb.ncoarse, dtype=ft)
    for r0, r1 in (bnds or [(0, n)]):
        part = np.zeros(tb.ncoarse, dtype=ft)
        a, b = tb.ptr[r0], tb.ptr[r1]
        np.add.at(part, tb.cols[a:b], prod[a:b])
        rc = rc + part
    u = fac.W.T @ (fac.W @ rc)
    out = z.astype(ft).copy()
    np.add.at(out, rows, pv * u[tb.cols])
    return out


def pcg(sy, pt, tb, mode, m=M_MAX, bnds=None, Ac=None):
    """solver_cg.hpp:76-131 with z = (patch sum over pt) + (coarse term of tb; None: patches only) -> (x_1..x_m, |r_j| / |r_0|).
    mode "ld": longdouble; "f64": cg_twin's restatement of the device's reductions.  bnds: the route by ranks (every sum grouped by
    rank and added in rank order; A_c from galerkin_rows).  Ac: another coarse matrix (a planted defect's)"""
    ft = _ft(mode)
    n = sy.n
    groups = bnds or [(0, n)]
    if mode == "ld":
        one_dot = one_dy = lambda u, v: np.sum(u * v)
        root = np.sqrt
        vals = sy.values.astype(ft)
        spmv = lambda d: np.add.reduceat(vals * d[sy.colind], sy.rowptr[:-1])
    else:
        one_dot, one_dy, root = T._dot_device, T._dy_device, math.sqrt
        spmv = lambda d: T._spmv_device(sy, d)

    def grouped(f):
        def g(u, v):
            s = f(u[groups[0][0]:groups[0][1]], v[groups[0][0]:groups[0][1]])
            for r0, r1 in groups[1:]:
                s = s + f(u[r0:r1], v[r0:r1])
            return s
        return g
    dot, dy = grouped(one_dot), grouped(one_dy)
    pfac = PT.factor(PT.patch_matrices(sy.rowptr, sy.colind, sy.values, pt), mode)
    cfac = None
    if tb is not None:
        if Ac is None:
            Ac = galerkin_rows(sy, tb, bnds, mode) if bnds else CT.galerkin(sy, tb, mode)
        cfac = CT.factor(Ac, mode)
        assert cfac.pivot == 0

    def M(r):
        z = PT.apply(pt, pfac, r, mode)
        return z if tb is None else _coarse_apply(tb, cfac, r, z, mode, bnds)
    x = np.zeros(n, dtype=ft)
    r = sy.b.astype(ft).copy()
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


def errors(sy, xs, truth_xs):
    return [T.scaled_error(x, t, sy.diag) for x, t in zip(xs, truth_xs)]


def gate(e):
    return max(FLOOR, MARGIN * e)


# ---- the generic case, partitioned ----------------------------------------------------------------------------------------------------
def generic_system():
    return PT.system(CT.base(CASE))


def generic_bounds(parts):
    return list(zip(parts[:-1], parts[1:]))


@functools.lru_cache(maxsize=None)
def generic_tables(parts, coarse=True):
    """-> (the slabs' patch tables, their concatenation, P or None)"""
    slabs = split_patches(PT.patches(CT.base(CASE)), generic_bounds(parts))
    return slabs, concat(slabs), CT.coarse(CASE) if coarse else None


@functools.lru_cache(maxsize=None)
def truth(parts, coarse=True):
    """the exact iterates of the partition's preconditioner: the global route in longdouble"""
    _, pt, tb = generic_tables(parts, coarse)
    return pcg(generic_system(), pt, tb, "ld")


@functools.lru_cache(maxsize=None)
def by_ranks(parts, mode, coarse=True):
    _, pt, tb = generic_tables(parts, coarse)
    return pcg(generic_system(), pt, tb, mode, bnds=generic_bounds(parts))


@functools.lru_cache(maxsize=None)
def e_ref(parts, coarse=True):
    return tuple(errors(generic_system(), by_ranks(parts, "f64", coarse).x, truth(parts, coarse).x))


def iterate_call(parts, m, coarse=True):
    """the thresholds that make the solver return x_m (tests/cg_twin.py) and the (reason, iterations) the truth's history gives"""
    rr = truth(parts, coarse).rr
    kw = dict(tol=0.0, div=0.0, max_iter=1000) if m == 1 else dict(tol=0.0, div=T.HUGE, max_iter=m - 2)
    want = T.expected_exit(rr, **kw)
    assert want is not None and want[2] == m - 1
    return kw, want[:2]
