"""A twin of the patch preconditioner and the conjugate gradient that uses it (proton_amd/csrc/patch_precond.hip; the recurrences
of solver_cg.hpp:63-144 with  z = sum_p R_p^T (R_p A R_p^T)^-1 R_p r  as an explicit vector), written the way tests/cg_twin.py is.

No device here.  This module holds
  * system(case) / patches(case): the seeded SPD band systems of cg_twin (diagonal over eight decades, so a patch of neighbouring
    rows is badly scaled) with a random overlapping patch table: a cover of chunks of 1..maxm rows in shuffled order, a patch across
    every multiple of 256 rows (the block edge of the row kernels), random extra patches so that rows lie in 1 to 4 patches, the
    patch order shuffled; `hard` adds the 16-row patch of the widest scale spread (condition beyond 1e8);
  * factor / apply / pcg in one generic restatement over the number type: mpmath at 50 digits (the truth), numpy.longdouble (the
    second route to it), and IEEE double in the device's stated order (lane sums ascending, a row's contributions in ascending patch
    order, cg_twin's dot products) or sequentially -- with switches that plant the defects the tests are there to catch;
  * e_ref: the error of the double restatements against the truth, in cg_twin's norm  max |dx_i| sqrt(A_ii) / max |x_i| sqrt(A_ii);
  * the gate max(2^-45, 10 e_ref) and the cap e_ref <= 1e-10 on judged iterates, as cg_twin has them;
  * the condensed fictitious-domain system of the oracle (Schur complement of tests/cuthho_driver.py's assembly) with its face and
    cell patch tables, and a plain double PCG that counts iterations on it."""
import functools
import math
from collections import namedtuple

import numpy as np

import cg_twin as T

PMAX = 16                                  # PA_PATCH_MAX_ROWS
FLOOR, MARGIN, CAP, M_MAX = T.FLOOR, T.MARGIN, T.CAP, T.M_MAX
RB = T.RB

Case = namedtuple("Case", "n maxm hard")
Case.__new__.__defaults__ = (16, False)
SIZES = (1, 2, 255, 256, 257, 4097)


def case_id(c):
    return "n%d-m%d%s" % (c.n, c.maxm, "-hard" if c.hard else "")


def case_table():
    """every size with patches of up to 16 rows; at 257 rows also the tables whose largest patch holds 4 and 8 rows (the kernels
    give a patch 4, 8 or 16 lanes) and the table with the badly conditioned patch"""
    return [Case(n) for n in SIZES] + [Case(257, 4), Case(257, 8), Case(257, 16, True)]


@functools.lru_cache(maxsize=None)
def system(case):
    """cg_twin's band system; `hard`: rescaled symmetrically by another decade, so that the diagonal spans ten"""
    sy = T.system(T.Case(case.n, True, False))
    if not case.hard:
        return sy
    rng = np.random.default_rng([31, case.n])
    t = (10.0 ** rng.uniform(-0.5, 0.5, case.n)).astype(np.float32).astype(np.float64)
    rows = np.repeat(np.arange(case.n), np.diff(sy.rowptr))
    out = T.System(sy.n, sy.rowptr, sy.colind, sy.values * t[rows] * t[sy.colind], sy.b * t, sy.diag * t * t, sy.scale * t)
    for a in out[1:]:
        a.setflags(write=False)
    return out


# ---- the patch tables -------------------------------------------------------------------------------------------------------------
Patches = namedtuple("Patches", "ptr rows")          # int64 [npatches + 1], int32 [ptr[-1]]


@functools.lru_cache(maxsize=None)
def patches(case):
    n, maxm = case.n, case.maxm
    sy = system(case)
    rng = np.random.default_rng([20250117, n, maxm, int(case.hard)])
    count = np.zeros(n, dtype=np.int64)
    plist = []

    def add(rows):
        rows = np.asarray(rows, dtype=np.int64)
        rows = rows[count[rows] < 4]
        if rows.size:
            count[rows] += 1
            plist.append(rows)

    if case.hard:                                     # eight rows of the largest and eight of the smallest scale within 48 rows
        best = max(range(0, max(1, n - 48)), key=lambda s: sy.scale[s:s + 48].max() / sy.scale[s:s + 48].min())
        order = best + np.argsort(sy.scale[best:best + 48])
        add(rng.permutation(np.concatenate([order[:8], order[-8:]])))
    i, first = 0, True
    while i < n:                                      # the cover; its first patch is a full one
        m = maxm if first else int(rng.integers(1, maxm + 1))
        first = False
        add(rng.permutation(np.arange(i, min(n, i + m))))
        i += m
    add([n - 1])                                      # a patch of one row
    for b in range(RB, n, RB):                        # across every block edge of the row kernels
        add(rng.permutation(np.arange(b - 2, min(n, b + 2))))
    for _ in range(max(3, n // 6)):                   # overlapping extras out of windows of 2 maxm rows
        s = int(rng.integers(0, n))
        win = np.arange(s, min(n, s + 2 * maxm))
        add(rng.choice(win, size=int(rng.integers(1, min(maxm, win.size) + 1)), replace=False))
    assert count.min() >= 1 and count.max() <= 4
    plist = [plist[k] for k in rng.permutation(len(plist))]
    ptr = np.zeros(len(plist) + 1, dtype=np.int64)
    np.cumsum([p.size for p in plist], out=ptr[1:])
    rows = np.concatenate(plist).astype(np.int32)
    ptr.setflags(write=False); rows.setflags(write=False)
    return Patches(ptr, rows)


def jacobi_patches(n):
    """one patch per row: the point Jacobi as a patch table"""
    return Patches(np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32))


def order_preserving_permutation(pt):
    """a permutation of the patches (new position -> old patch) that swaps neighbours sharing no row: every row still meets its
    patches in the same order -> (permutation, the permuted table)"""
    npat = pt.ptr.size - 1
    perm = np.arange(npat)
    k = 0
    while k + 1 < npat:
        a, b = pt.rows[pt.ptr[k]:pt.ptr[k + 1]], pt.rows[pt.ptr[k + 1]:pt.ptr[k + 2]]
        if np.intersect1d(a, b).size == 0:
            perm[k], perm[k + 1] = k + 1, k
            k += 2
        else:
            k += 1
    plist = [pt.rows[pt.ptr[p]:pt.ptr[p + 1]] for p in perm]
    ptr = np.zeros(npat + 1, dtype=np.int64)
    np.cumsum([p.size for p in plist], out=ptr[1:])
    return perm, Patches(ptr, np.concatenate(plist).astype(np.int32))


def patch_matrices(rowptr, colind, values, pt, P=None):
    """A_p = R_p A R_p^T of every patch as float64 [npatches, P, P], padded by the identity; absent entries are zero"""
    import scipy.sparse as sp
    n = rowptr.size - 1
    A = sp.csr_matrix((values, colind, rowptr), shape=(n, n))
    npat = pt.ptr.size - 1
    P = P or int(np.diff(pt.ptr).max())
    out = np.zeros((npat, P, P))
    out[:, np.arange(P), np.arange(P)] = 1.0
    for p in range(npat):
        r = pt.rows[pt.ptr[p]:pt.ptr[p + 1]].astype(np.int64)
        out[p, :r.size, :r.size] = A[r][:, r].toarray()
    return out


# ---- the number types ---------------------------------------------------------------------------------------------------------------
MP_ROWS = 257                              # truth in mpmath at 50 digits up to here, in longdouble above (2^-11 of double's error)


def _mp50(fn):
    """run fn at 50 digits of mpmath (the other number types do not notice)"""
    @functools.wraps(fn)
    def wrapped(*a, **kw):
        import mpmath
        with mpmath.workdps(50):
            return fn(*a, **kw)
    return wrapped


def truth_mode(case):
    return "mp" if case.n <= MP_ROWS else "ld"


def _mp_array(a):
    import mpmath
    flat = np.array([mpmath.mpf(float(t)) for t in np.asarray(a).reshape(-1)], dtype=object)
    return flat.reshape(np.asarray(a).shape)


def _convert(a, mode):
    if mode == "mp":
        return _mp_array(a)
    return np.asarray(a, dtype=np.longdouble if mode == "ld" else np.float64)


def _sqrt(a, mode):
    if mode == "mp":
        import mpmath
        return np.frompyfunc(mpmath.sqrt, 1, 1)(a)
    return np.sqrt(a)


def _zeros(shape, mode):
    if mode == "mp":
        import mpmath
        z = np.empty(shape, dtype=object)
        z.fill(mpmath.mpf(0))
        return z
    return np.zeros(shape, dtype=np.longdouble if mode == "ld" else np.float64)


# ---- factor and apply ---------------------------------------------------------------------------------------------------------------
Factors = namedtuple("Factors", "L W pivots")         # [npatches, P, P] each (lower triangles); first non-positive pivot + 1 or 0


@_mp50
def factor(Ap, mode):
    """Cholesky of every patch matrix and W = L^-1, the steps of patch_factor_kernel in the number type of `mode`"""
    A = _convert(Ap, mode).copy()
    npat, P = A.shape[0], A.shape[1]
    L, W = _zeros(A.shape, mode), _zeros(A.shape, mode)
    pivots = np.zeros(npat, dtype=np.int64)
    with np.errstate(all="ignore"):
        for j in range(P):
            bad = np.array([not (float(v) > 0.0) for v in A[:, j, j]])
            pivots[(pivots == 0) & bad] = j + 1
            if mode == "mp":
                A[bad, j, j] = A[bad, j, j] * 0 + 1           # (the truth is never asked about a failed patch)
            ljj = _sqrt(A[:, j, j], mode)
            L[:, j, j] = ljj
            for i in range(j + 1, P):
                L[:, i, j] = A[:, i, j] / ljj
            for k in range(j + 1, P):
                for i in range(k, P):
                    A[:, i, k] = A[:, i, k] - L[:, i, j] * L[:, k, j]
        for l in range(P):
            for i in range(l, P):
                s = _zeros(npat, mode) + (1 if i == l else 0)
                for k in range(l, i):
                    s = s - L[:, i, k] * W[:, k, l]
                W[:, i, l] = s / L[:, i, i]
    return Factors(L, W, pivots)


def _slots(pt, n):
    """per row its entries of patch_rows in ascending order (= ascending patch order): (order, start, count)"""
    order = np.argsort(pt.rows, kind="stable")
    count = np.bincount(pt.rows, minlength=n)
    start = np.zeros(n, dtype=np.int64)
    np.cumsum(count[:-1], out=start[1:])
    return order, start, count


@_mp50
def apply(pt, fac, r, mode, first_slot_only=False, lt_for_linvt=False):
    """z = sum_p R_p^T W_p^T W_p R_p r: t = W r_p with every lane's sum ascending, z_p = W^T t likewise, the patches' results in a
    patch-major buffer, every row's contributions added in ascending patch order.  Defects: first_slot_only = a shared row takes
    the contribution of its first patch only; lt_for_linvt = L^T applied where L^-T belongs"""
    n = r.size
    npat, P = fac.W.shape[0], fac.W.shape[1]
    sizes = np.diff(pt.ptr)
    rp = _zeros((npat, P), mode)
    lane = np.arange(P)[None, :]
    live = lane < sizes[:, None]
    ent = np.where(live, pt.ptr[:-1, None] + lane, 0)
    rp[live] = r[pt.rows[ent[live]]]
    t = _zeros((npat, P), mode)
    for i in range(P):
        for j in range(i + 1):
            t[:, i] = t[:, i] + fac.W[:, i, j] * rp[:, j]
    zp = _zeros((npat, P), mode)
    B = fac.L if lt_for_linvt else fac.W
    for l in range(P):
        for i in range(l, P):
            zp[:, l] = zp[:, l] + B[:, i, l] * t[:, i]
    zbuf = _zeros(pt.rows.size, mode)
    zbuf[ent[live]] = zp[live]
    order, start, count = _slots(pt, n)
    z = _zeros(n, mode)
    for k in range(1 if first_slot_only else int(count.max())):
        act = np.nonzero(count > k)[0]
        z[act] = z[act] + zbuf[order[start[act] + k]]
    return z


@functools.lru_cache(maxsize=None)
def factors(case, mode):
    sy, pt = system(case), patches(case)
    return factor(patch_matrices(sy.rowptr, sy.colind, sy.values, pt), mode)


def max_patch_condition(case):
    sy, pt = system(case), patches(case)
    return max(np.linalg.cond(a) for a in patch_matrices(sy.rowptr, sy.colind, sy.values, pt, PMAX))


def _to_ld(a):
    import mpmath
    return np.array([np.longdouble(mpmath.nstr(t, 25)) for t in a]) if a.dtype == object else np.asarray(a, dtype=np.longdouble)


def test_vectors(case):
    """the two residuals the apply is judged on: the system's right-hand side and a seeded vector of the same scaling"""
    sy = system(case)
    rng = np.random.default_rng([77, case.n])
    return sy.b.copy(), sy.scale * rng.standard_normal(case.n)


@functools.lru_cache(maxsize=None)
@_mp50
def apply_truth(case, which, mode=None):
    """M r of test_vectors(case)[which] as longdouble"""
    mode = mode or truth_mode(case)
    return _to_ld(apply(patches(case), factors(case, mode), _convert(test_vectors(case)[which], mode), mode))


def apply_double(case, which, **defect):
    return apply(patches(case), factors(case, "f64"), test_vectors(case)[which], "f64", **defect)


def scaled_error(case, z, ref):
    return T.scaled_error(z, ref, system(case).diag)


@functools.lru_cache(maxsize=None)
def apply_e_ref(case):
    """the error of the double restatement of factor + apply against the truth, worst of the two test vectors"""
    return max(scaled_error(case, apply_double(case, w), apply_truth(case, w)) for w in (0, 1))


def symmetry_defect(case, z1, z2):
    """|r1 . M r2 - r2 . M r1| / sqrt((r1 . M r1) (r2 . M r2)) for z1 = M r1, z2 = M r2, summed in longdouble"""
    ld = np.longdouble
    r1, r2 = (v.astype(ld) for v in test_vectors(case))
    z1, z2 = np.asarray(z1, dtype=ld), np.asarray(z2, dtype=ld)
    return float(abs(np.sum(r1 * z2) - np.sum(r2 * z1)) / np.sqrt(np.sum(r1 * z1) * np.sum(r2 * z2)))


def gate(e):
    return max(FLOOR, MARGIN * e)


# ---- the recurrences ----------------------------------------------------------------------------------------------------------------
Truth = namedtuple("Truth", "x rr")


@_mp50
def pcg(case, mode, m=None, order="dev", pt=None, rho_rr=False, **defect):
    """The recurrences of solver_cg.hpp:76-131 with z = M r explicit -> (x_1..x_M, |r_j| / |r_0|).  mode "mp" / "ld": exact sums;
    "f64": order "seq" (every sum entry by entry) or "dev" (cg_twin's restatement of the device's reductions).  rho_rr: r . r used
    for rho (a defect); **defect: those of apply.  pt: another table for the same system (default: the case's)."""
    sy = system(case)
    m = min(M_MAX, case.n) if m is None else m
    if pt is None:
        pt, fac = patches(case), factors(case, mode)
    else:
        fac = factor(patch_matrices(sy.rowptr, sy.colind, sy.values, pt), mode)
    starts = sy.rowptr[:-1]
    if mode == "mp":
        import mpmath
        dot = dy = lambda u, v: mpmath.fsum(u * v)
        root = mpmath.sqrt
        vals = _mp_array(sy.values)
        spmv = lambda d: np.add.reduceat(vals * d[sy.colind], starts)
        small = T.EXACT
    elif mode == "ld":
        dot = dy = lambda u, v: np.sum(u * v)
        root = np.sqrt
        vals = sy.values.astype(np.longdouble)
        spmv = lambda d: np.add.reduceat(vals * d[sy.colind], starts)
        small = 1e-17
    elif order == "seq":
        dot = dy = lambda u, v: T._seq_sum(u * v)
        root, small = math.sqrt, 0.0
        spmv = lambda d: T._spmv_seq(sy, d)
    else:
        dot, dy = T._dot_device, T._dy_device
        root, small = math.sqrt, 0.0
        spmv = lambda d: T._spmv_device(sy, d)
    M = lambda r: apply(pt, fac, r, mode, **defect)
    x = _zeros(case.n, mode)
    r = _convert(sy.b, mode).copy()
    z = M(r)
    d = z.copy()
    nr0 = root(dot(r, r))
    rho = dot(r, r) if rho_rr else dot(r, z)
    xs, rrs = [], []
    with np.errstate(all="ignore"):
        for _ in range(m):
            y = spmv(d)
            alpha = rho / dy(d, y)
            x = x + alpha * d
            r = r - alpha * y
            rr = root(dot(r, r)) / nr0
            xs.append(_to_ld(x) if mode != "f64" else x.copy())
            rrs.append(float(rr))
            if mode != "f64" and rr < small:
                break
            z = M(r)
            rho_new = dot(r, r) if rho_rr else dot(r, z)
            d = z + (rho_new / rho) * d
            rho = rho_new
    return Truth(xs, rrs)


@functools.lru_cache(maxsize=None)
def truth(case, mode=None):
    return pcg(case, mode or truth_mode(case))


def errors(case, xs):
    tr, diag = truth(case), system(case).diag
    return [T.scaled_error(x, t, diag) for x, t in zip(xs, tr.x)]


@functools.lru_cache(maxsize=None)
def e_ref(case):
    """per m: the error of the double recurrences against the truth, worst of the sequential and the device's order"""
    m = len(truth(case).rr)
    return tuple(max(a, b) for a, b in zip(errors(case, pcg(case, "f64", m, "seq").x), errors(case, pcg(case, "f64", m, "dev").x)))


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


# ---- the oracle's condensed fictitious-domain system ----------------------------------------------------------------------------------
Condensed = namedtuple("Condensed", "rowptr colind values b face cell")


def numbering_patches(compress, cell_faces, num_other, fbs):
    """the two tables of pa_condensed_patches restated from the assembler's numbering (compressed face q owns rows q fbs ..):
    face = one patch per non-Dirichlet face; cell = one per cell with such a face, rows in the cell's face order"""
    face = Patches(np.arange(num_other + 1, dtype=np.int64) * fbs, np.arange(num_other * fbs, dtype=np.int32))
    plist = []
    for c in range(cell_faces.shape[0]):
        q = [int(compress[int(f)]) for f in cell_faces[c] if compress[int(f)] >= 0]
        if q:
            plist.append(np.concatenate([np.arange(v * fbs, (v + 1) * fbs) for v in q]))
    ptr = np.zeros(len(plist) + 1, dtype=np.int64)
    if plist:
        np.cumsum([p.size for p in plist], out=ptr[1:])
    rows = np.concatenate(plist).astype(np.int32) if plist else np.zeros(0, dtype=np.int32)
    return face, Patches(ptr, rows)


@functools.lru_cache(maxsize=None)
def oracle_condensed(N, k):
    """The Schur complement on the face unknowns of the system tests/cuthho_driver.py assembles for `-f` (the cell blocks are
    block diagonal: eliminated block by block), and its patch tables from the assembler's numbering: face = the fbs rows of a
    non-Dirichlet face; cell = the rows of a cell's non-Dirichlet faces in the order bottom, right, top, left"""
    import scipy.sparse as sp

    import cuthho_driver as drv
    import oracle_lib as o
    msh = o.CutMesh(N, refsteps=4)
    di = o.degrees(k + 1, k)
    asm = o.Assembler(o.MeshParams(N, N, 0.0, 1.0, 0.0, 1.0), msh.points, msh.ptids, di, bf_id=2)
    local = drv.oracle_cut_provider(msh, di)
    rows, cols, vals = [], [], []
    RHS = np.zeros(asm.system_size)
    for c in range(msh.nc):
        tr, tc, tv, rr, rv = asm.assemble_cell(c, *local[c])
        rows.append(tr); cols.append(tc); vals.append(tv)
        ok = rr >= 0
        np.add.at(RHS, rr[ok], rv[ok])
    K = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(asm.system_size,) * 2)
    cbs, fbs = di.cbs, di.fbs
    c0 = cbs * msh.nc
    KTT, KTF, KFT, KFF = K[:c0, :c0], K[:c0, c0:], K[c0:, :c0], K[c0:, c0:]
    blocks = np.stack([KTT[c * cbs:(c + 1) * cbs, c * cbs:(c + 1) * cbs].toarray() for c in range(msh.nc)])
    iTT = sp.block_diag(list(np.linalg.inv(blocks)), format="csr")
    S = (KFF - KFT @ iTT @ KTF).tocsr()
    S = ((S + S.T) * 0.5).tocsr()
    S.sort_indices()
    b = RHS[c0:] - KFT @ (iTT @ RHS[:c0])
    face, cell = numbering_patches(asm.compress, asm.cell_faces, asm.num_other, fbs)
    return Condensed(S.indptr.astype(np.int64), S.indices.astype(np.int32), S.data.copy(), b, face, cell)


def pcg_iterations(sysm, pt, tol=1e-13, max_iter=20000):
    """textbook PCG in double from x = 0 to |r| / |r_0| < tol -> iterations.  pt None: no preconditioner; "jacobi": 1 / diag"""
    import scipy.sparse as sp
    n = sysm.b.size
    A = sp.csr_matrix((sysm.values, sysm.colind, sysm.rowptr), shape=(n, n))
    if pt is None:
        M = lambda r: r
    elif isinstance(pt, str):
        iA = 1.0 / A.diagonal()
        M = lambda r: iA * r
    else:
        Ap = patch_matrices(sysm.rowptr, sysm.colind, sysm.values, pt)
        inv = np.linalg.inv(Ap)
        sizes = np.diff(pt.ptr)
        P = Ap.shape[1]
        live = np.arange(P)[None, :] < sizes[:, None]
        ent = np.where(live, pt.ptr[:-1, None] + np.arange(P)[None, :], 0)
        idx = pt.rows[ent].astype(np.int64)

        def M(r):
            zp = np.einsum("pij,pj->pi", inv, np.where(live, r[idx], 0.0))
            z = np.zeros(n)
            np.add.at(z, idx[live], zp[live])
            return z
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
