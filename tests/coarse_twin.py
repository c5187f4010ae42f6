"""A twin of the Galerkin coarse level and the two-level conjugate gradient (proton_amd/csrc/coarse_precond.hip; the recurrences of
solver_cg.hpp:63-144 with  z = sum_p R_p^T A_p^-1 R_p r + P (P^T A P)^-1 P^T r), written the way tests/patch_pcg_twin.py is.

No device here.  This module holds
  * table(...): the coarse table of pa_condensed_coarse restated in numpy from the assembler's numbering (the inputs of
    patch_pcg_twin.numbering_patches plus the faces' end points and sides), dense over (face, node) -- the device decides per face
    which lines can matter; here every hat is evaluated at every vertex.  The values are the definition's, operation by operation,
    so the device's table is compared bit for bit.  shift = (node, lines): one hat moved by that many lines (a planted defect);
  * seeded generic cases: the SPD band systems and patch tables of patch_pcg_twin with a random P of 0 to 4 entries per row,
    ncoarse in NCOARSE;
  * galerkin / factor / apply / pcg in one restatement over the number type: numpy.longdouble (the truth: 11 bits more than double)
    and IEEE double (W = A P and A_c summed in the device's stated order; the dot products of the Cholesky factor, of L^-1 and of
    the two triangular products in numpy's order) -- with switches that plant the defects the tests are there to catch;
  * e_ref: the error of the double restatement against the truth in cg_twin's norm, the gate max(2^-45, 10 e_ref);
  * the oracle's condensed Poisson and fictitious-domain systems with their tables, and a plain double PCG that counts iterations."""
import functools
import math
from collections import namedtuple

import numpy as np

import cg_twin as T
import patch_pcg_twin as PT

MAX_ROW, MAX_NODES = 4, 4096               # PA_COARSE_MAX_ROW_ENTRIES, PA_COARSE_MAX_NODES
FLOOR, MARGIN, CAP, M_MAX = T.FLOOR, T.MARGIN, T.CAP, 8
NCOARSE = (1, 2, 31, 32, 33, 63, 64, 65, 257, 1025)

Table = namedtuple("Table", "ptr cols vals ncoarse")  # int64 [n + 1], int32, float64, int


# ---- the table of the face-only numbering ---------------------------------------------------------------------------------------------
def lines(N, H):
    """the coarse lines of a direction with N cells: 0, H, 2 H, .. below N, and N"""
    return list(range(0, N, H)) + [N]


def hats(N, H):
    """hat[j, i]: the 1-D hat of line j at vertex index i (one division each)"""
    ln = lines(N, H)
    out = np.zeros((len(ln), N + 1))
    for j, lj in enumerate(ln):
        out[j, lj] = 1.0
        if j > 0:
            for i in range(ln[j - 1] + 1, lj):
                out[j, i] = float(i - ln[j - 1]) / float(lj - ln[j - 1])
        if j + 1 < len(ln):
            for i in range(lj + 1, ln[j + 1]):
                out[j, i] = float(ln[j + 1] - i) / float(ln[j + 1] - lj)
    return out


def table(Nx, Ny, H, fbs, compress, face_pts, num_other, face_side=None, where=0, shift=None):
    """pa_condensed_coarse: face_pts [nfaces, 2] point ids (point p = vertex (p % (Nx + 1), p // (Nx + 1))), compress [nfaces]
    (-1 Dirichlet), face_side None (one part) or [nfaces] in {0, 1, 2 = cut} -> Table, or None where the entry refuses (no
    interior node, more than MAX_NODES columns)"""
    hx, hy = hats(Nx, H)[1:-1], hats(Ny, H)[1:-1]                     # interior lines only
    nix, niy = hx.shape[0], hy.shape[0]
    nn = nix * niy
    if nix < 1 or niy < 1:
        return None
    fp = np.asarray(face_pts, dtype=np.int64)
    comp = np.asarray(compress, dtype=np.int64)
    live = np.nonzero(comp >= 0)[0]
    live = live[np.argsort(comp[live])]
    assert live.size == num_other
    ax, ay = fp[live, 0] % (Nx + 1), fp[live, 0] // (Nx + 1)
    bx, by = fp[live, 1] % (Nx + 1), fp[live, 1] // (Nx + 1)

    def phi(x, y):                                                     # [face, jy, jx] = wx * wy, one rounding
        hxx, hyy = hx[:, x].T, hy[:, y].T
        out = hyy[:, :, None] * hxx[:, None, :]
        if shift is not None:
            jy, jx = divmod(shift[0], nix)
            out[:, jy, jx] = hyy[:, jy] * hx[(jx + shift[1]) % nix][x]
        return out.reshape(live.size, nn)

    fa, fb = phi(ax, ay), phi(bx, by)
    mask = (fa != 0.0) | (fb != 0.0)
    v0, v1 = 0.5 * (fa + fb), 0.5 * (fb - fa)
    if face_side is None:
        column = np.arange(nn)[None, :].repeat(live.size, axis=0)
        ncoarse = nn
    else:
        side = np.asarray(face_side)[live]
        part = ((side != 2) & (side != where)).astype(np.int64)
        used = np.zeros((2, nn), dtype=bool)
        for p in (0, 1):
            used[p] = mask[part == p].any(axis=0)
        index = np.full(2 * nn, -1, dtype=np.int64)
        flat = used.reshape(-1)
        index[flat] = np.arange(int(flat.sum()))
        ncoarse = int(flat.sum())
        column = index.reshape(2, nn)[part]
    if ncoarse < 1 or ncoarse > MAX_NODES:
        return None
    ptr = np.zeros(num_other * fbs + 1, dtype=np.int64)
    cols, vals = [], []
    for q in range(live.size):
        nodes = np.nonzero(mask[q])[0]
        cols.append(column[q, nodes]); vals.append(v0[q, nodes])
        ptr[q * fbs + 1] = nodes.size
        if fbs >= 2:
            odd = nodes[v1[q, nodes] != 0.0]
            cols.append(column[q, odd]); vals.append(v1[q, odd])
            ptr[q * fbs + 2] = odd.size
    np.cumsum(ptr, out=ptr)
    return Table(ptr, np.concatenate(cols).astype(np.int32), np.concatenate(vals), ncoarse)


def dense(tb):
    n = tb.ptr.size - 1
    P = np.zeros((n, tb.ncoarse))
    rows = np.repeat(np.arange(n), np.diff(tb.ptr))
    P[rows, tb.cols] = tb.vals
    return P


# ---- the generic cases ----------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "n ncoarse")


def case_id(c):
    return "n%d-c%d" % c


def case_table():
    return [Case(4097 if nc >= 257 else 257, nc) for nc in NCOARSE]


def base(case):
    return PT.Case(case.n)


@functools.lru_cache(maxsize=None)
def coarse(case):
    """random P: 0 to 4 entries per row, columns ascending, values in +-[0.25, 1].  Row i draws its columns from the five around
    i ncoarse / n: the system's rows reach 17 rows to either side, so a row of A P meets at most 14 columns (the device keeps 16).
    The first row of every column's own stretch holds that column alone, so that P has full column rank."""
    n, nc = case
    rng = np.random.default_rng([20251020, n, nc])
    centre = np.arange(n) * nc // n
    lo, hi = np.maximum(centre - 2, 0), np.minimum(centre + 3, nc)
    sizes = np.minimum(rng.integers(0, MAX_ROW + 1, n), hi - lo)
    own = -(-np.arange(nc) * n // nc)
    assert np.array_equal(centre[own], np.arange(nc))
    sizes[own] = 1
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(sizes, out=ptr[1:])
    cols = np.zeros(ptr[-1], dtype=np.int32)
    for i in range(n):
        cols[ptr[i]:ptr[i + 1]] = np.sort(lo[i] + rng.choice(hi[i] - lo[i], size=sizes[i], replace=False))
    cols[ptr[own]] = np.arange(nc)
    vals = rng.uniform(0.25, 1.0, ptr[-1]) * rng.choice([-1.0, 1.0], ptr[-1])
    for a in (ptr, cols, vals):
        a.setflags(write=False)
    return Table(ptr, cols, vals, nc)


# ---- Galerkin product, factor, apply --------------------------------------------------------------------------------------------------
def _ft(mode):
    return np.longdouble if mode == "ld" else np.float64


def galerkin(sy, tb, mode):
    """A_c = P^T (A P): W = A P row by row in the row's entry order, then every (j, c) summed over the fine rows ascending; the lower
    triangle mirrored"""
    ft = _ft(mode)
    n, nc = sy.n, tb.ncoarse
    vals, pv = sy.values.astype(ft), tb.vals.astype(ft)
    Ac = np.zeros((nc, nc), dtype=ft)
    for i in range(n):
        w = {}
        for e in range(sy.rowptr[i], sy.rowptr[i + 1]):
            c = sy.colind[e]
            for q in range(tb.ptr[c], tb.ptr[c + 1]):
                j = tb.cols[q]
                v = vals[e] * pv[q]
                w[j] = w[j] + v if j in w else v
        for q in range(tb.ptr[i], tb.ptr[i + 1]):
            j = tb.cols[q]
            for c, wv in w.items():
                if c <= j:
                    Ac[j, c] = Ac[j, c] + pv[q] * wv
    low = np.tril(Ac)
    return low + np.tril(Ac, -1).T


Factor = namedtuple("Factor", "L W pivot")


def factor(Ac, mode):
    """left-looking Cholesky and W = L^-1 by forward substitution -> Factor (pivot: first non-positive pivot + 1 or 0)"""
    ft = _ft(mode)
    nc = Ac.shape[0]
    A = Ac.astype(ft)
    L = np.zeros((nc, nc), dtype=ft)
    for j in range(nc):
        s = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not (float(s[0]) > 0.0):
            return Factor(L, None, j + 1)
        d = np.sqrt(s[0])
        L[j, j] = d
        L[j + 1:, j] = s[1:] / d
    W = np.zeros((nc, nc), dtype=ft)
    for i in range(nc):
        row = -(L[i, :i] @ W[:i, :])
        row[i] = row[i] + 1
        W[i, :] = row / L[i, i]
    return Factor(L, np.tril(W), 0)


def apply(tb, fac, r, mode, z0=None, linv_for_linvt=False, drop=False):
    """z = z0 + P W^T W P^T r.  Defects: linv_for_linvt = L^-1 applied where L^-T belongs; drop = the coarse term left out"""
    ft = _ft(mode)
    n = tb.ptr.size - 1
    z = np.zeros(n, dtype=ft) if z0 is None else z0.astype(ft).copy()
    if drop:
        return z
    rows = np.repeat(np.arange(n), np.diff(tb.ptr))
    pv = tb.vals.astype(ft)
    rc = np.zeros(tb.ncoarse, dtype=ft)
    np.add.at(rc, tb.cols, pv * r.astype(ft)[rows])
    t = fac.W @ rc
    u = (fac.W if linv_for_linvt else fac.W.T) @ t
    np.add.at(z, rows, pv * u[tb.cols])
    return z


@functools.lru_cache(maxsize=None)
def matrix(case, mode):
    return galerkin(PT.system(base(case)), coarse(case), mode)


@functools.lru_cache(maxsize=None)
def factors(case, mode):
    return factor(matrix(case, mode), mode)


def test_vectors(case):
    return PT.test_vectors(base(case))


@functools.lru_cache(maxsize=None)
def apply_truth(case, which, accumulate=False):
    r = test_vectors(case)[which]
    z0 = test_vectors(case)[1 - which] if accumulate else None
    return apply(coarse(case), factors(case, "ld"), r, "ld", z0)


def apply_double(case, which, accumulate=False, **defect):
    r = test_vectors(case)[which]
    z0 = test_vectors(case)[1 - which] if accumulate else None
    return apply(coarse(case), factors(case, "f64"), r, "f64", z0, **defect)


def scaled_error(case, z, ref):
    return T.scaled_error(z, ref, PT.system(base(case)).diag)


@functools.lru_cache(maxsize=None)
def apply_e_ref(case):
    return max(scaled_error(case, apply_double(case, w, acc), apply_truth(case, w, acc)) for w in (0, 1) for acc in (False, True))


def matrix_error(case, Ac):
    """max |dA_jc| / sqrt(A_jj A_cc) against the truth"""
    ref = matrix(case, "ld")
    d = np.sqrt(np.diag(ref))
    return float(np.max(np.abs(np.asarray(Ac, dtype=np.longdouble) - ref) / (d[:, None] * d[None, :])))


@functools.lru_cache(maxsize=None)
def matrix_e_ref(case):
    return matrix_error(case, matrix(case, "f64"))


def gate(e):
    return max(FLOOR, MARGIN * e)


# ---- the recurrences ------------------------------------------------------------------------------------------------------------------
Truth = namedtuple("Truth", "x rr")


def pcg(case, mode, m=None, tb=None, **defect):
    """solver_cg.hpp:76-131 with z = (patch sum) + (coarse term) explicit -> (x_1..x_m, |r_j| / |r_0|); "ld": exact-order sums in
    longdouble; "f64": cg_twin's restatement of the device's reductions.  tb: another coarse table; **defect: those of apply"""
    b = base(case)
    sy = PT.system(b)
    m = min(M_MAX, case.n) if m is None else m
    pt, pfac = PT.patches(b), PT.factors(b, mode)
    if tb is None:
        tb, cfac = coarse(case), factors(case, mode)
    else:
        cfac = factor(galerkin(sy, tb, mode), mode)
    starts = sy.rowptr[:-1]
    if mode == "ld":
        dot = dy = lambda u, v: np.sum(u * v)
        root = np.sqrt
        vals = sy.values.astype(np.longdouble)
        spmv = lambda d: np.add.reduceat(vals * d[sy.colind], starts)
    else:
        dot, dy, root = T._dot_device, T._dy_device, math.sqrt
        spmv = lambda d: T._spmv_device(sy, d)
    M = lambda r: apply(tb, cfac, r, mode, PT.apply(pt, pfac, r, mode), **defect)
    x = np.zeros(case.n, dtype=_ft(mode))
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
def truth(case):
    return pcg(case, "ld")


def errors(case, xs):
    diag = PT.system(base(case)).diag
    return [T.scaled_error(x, t, diag) for x, t in zip(xs, truth(case).x)]


@functools.lru_cache(maxsize=None)
def e_ref(case):
    return tuple(errors(case, pcg(case, "f64", len(truth(case).rr)).x))


def judged(case):
    return [j + 1 for j, e in enumerate(e_ref(case)) if e <= CAP]


def iterate_call(case, m):
    """the thresholds that make the solver return x_m (tests/cg_twin.py) and the (reason, iterations) the truth's history gives"""
    rr = truth(case).rr
    if m == 1:
        kw = dict(tol=0.5, div=T.HUGE, max_iter=1000) if rr[0] < T.EXACT else dict(tol=0.0, div=0.0, max_iter=1000)
    else:
        kw = dict(tol=0.0, div=T.HUGE, max_iter=m - 2)
    want = T.expected_exit(rr, **kw)
    assert want is not None and want[2] == m - 1
    return kw, want[:2]


# ---- the oracle's condensed systems ---------------------------------------------------------------------------------------------------
Condensed = namedtuple("Condensed", "rowptr colind values b face cell one side N fbs")


def _schur(K, RHS, c0, cbs, nc):
    import scipy.sparse as sp
    KTT, KTF, KFT, KFF = K[:c0, :c0], K[:c0, c0:], K[c0:, :c0], K[c0:, c0:]
    blocks = np.stack([KTT[c * cbs:(c + 1) * cbs, c * cbs:(c + 1) * cbs].toarray() for c in range(nc)])
    iTT = sp.block_diag(list(np.linalg.inv(blocks)), format="csr")
    S = (KFF - KFT @ iTT @ KTF).tocsr()
    S = ((S + S.T) * 0.5).tocsr()
    S.sort_indices()
    return S, RHS[c0:] - KFT @ (iTT @ RHS[:c0])


def _assembled(asm, local, nc):
    import scipy.sparse as sp
    rows, cols, vals = [], [], []
    RHS = np.zeros(asm.system_size)
    for c in range(nc):
        tr, tc, tv, rr, rv = asm.assemble_cell(c, *local[c])
        rows.append(tr); cols.append(tc); vals.append(tv)
        ok = rr >= 0
        np.add.at(RHS, rr[ok], rv[ok])
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(asm.system_size,) * 2), RHS


@functools.lru_cache(maxsize=None)
def oracle_fictdom(N, k, H):
    """patch_pcg_twin.oracle_condensed(N, k) with the coarse tables of H: one part, and by side of the circle"""
    import oracle_lib as o
    sy = PT.oracle_condensed(N, k)
    msh = o.CutMesh(N, refsteps=4)
    di = o.degrees(k + 1, k)
    asm = o.Assembler(o.MeshParams(N, N, 0.0, 1.0, 0.0, 1.0), msh.points, msh.ptids, di, bf_id=2)
    one = table(N, N, H, di.fbs, asm.compress, asm.faces, asm.num_other)
    side = table(N, N, H, di.fbs, asm.compress, asm.faces, asm.num_other, msh.face_loc, 0)
    return Condensed(sy.rowptr, sy.colind, sy.values, sy.b, sy.face, sy.cell, one, side, N, di.fbs)


@functools.lru_cache(maxsize=None)
def oracle_poisson(N, k, H):
    """The Schur complement on the face unknowns of the oracle's Poisson system, pair (k + 1, k), tensor quadrature, the
    HHO stabilization, with a random right-hand side (seed 1), its patch tables and the coarse table of H"""
    import oracle_lib as o
    mp, points, ptids = o.make_mesh(N, N)
    di = o.degrees(k + 1, k)
    asm = o.Assembler(mp, points, ptids, di)
    st, out = o.local_ops_batch(points, ptids, di, o.QUAD_TENSOR, o.STAB_FANCY, fn=1, want=("lc",))
    assert st == 0
    local = [(out["lc"][c], out["rhs"][c]) for c in range(ptids.shape[0])]
    K, RHS = _assembled(asm, local, ptids.shape[0])
    S, _ = _schur(K, RHS, di.cbs * ptids.shape[0], di.cbs, ptids.shape[0])
    b = np.random.default_rng(1).standard_normal(S.shape[0])
    face, cell = PT.numbering_patches(asm.compress, asm.cell_faces, asm.num_other, di.fbs)
    one = table(N, N, H, di.fbs, asm.compress, asm.faces, asm.num_other)
    return Condensed(S.indptr.astype(np.int64), S.indices.astype(np.int32), S.data.copy(), b, face, cell, one, None, N, di.fbs)


def two_level_iterations(sysm, pt, tb, tol=1e-13, max_iter=20000):
    """textbook PCG in double from x = 0 to |r| / |r_0| < tol with z = (patch sum) + P (P^T A P)^-1 P^T r (tb None: patches alone)"""
    import scipy.linalg as sl
    import scipy.sparse as sp
    if tb is None:
        return PT.pcg_iterations(sysm, pt, tol, max_iter)
    n = sysm.b.size
    A = sp.csr_matrix((sysm.values, sysm.colind, sysm.rowptr), shape=(n, n))
    Pm = sp.csr_matrix((tb.vals, tb.cols, tb.ptr), shape=(n, tb.ncoarse))
    cho = sl.cho_factor((Pm.T @ A @ Pm).toarray())
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
        return z + Pm @ sl.cho_solve(cho, Pm.T @ r)
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
