"""The judge of the fictitious-domain problem's condensed records and recovery: a cut cell's local matrix eliminated at 50 digits
(mpmath), and the measure the tests hold a candidate to.

A local matrix lc is [A_TT A_TF; A_FT A_FF] with n = cbs cell unknowns first, row-major numpy [M, M]; f is the cell right-hand
side.  The record is the upper triangle of S = A_FF - A_FT A_TT^-1 A_TF, column-packed (entry (i, j), i <= j, at j (j + 1) / 2 + i),
then g = -A_FT A_TT^-1 f: pa_condensed_ops_batch's layout.

The matrix judged is the symmetric one the kernels read: the lower triangle of A_TT, A_TF (A_FT is its transpose) and the upper
triangle of A_FF.  The device's cut matrices are symmetric bit for bit; the oracle's are symmetric to rounding only, and an
asymmetry of one ulp is amplified by cond(A_TT) in S, so a judge that read the other copies would measure that, not the
elimination."""
import numpy as np

DPS = 50
RECORD_GATE = 1e-13          # of the record's largest entry: the gate test_cut_records_against_mpmath holds ifd_records_kernel to
RECOVER_GATE = 1e-13         # of the cell's largest |u_T|


def _solve_mp(lc, cols, n, mp):
    """X = A_TT^-1 cols at mp's precision: Gaussian elimination without pivoting (A_TT is SPD) and back substitution.
    cols: n rows of mp numbers."""
    A = [[mp.mpf(float(lc[max(i, j), min(i, j)])) for j in range(n)] for i in range(n)]
    B = [list(r) for r in cols]
    nc = len(B[0])
    for p in range(n):
        inv = 1 / A[p][p]
        for i in range(p + 1, n):
            m = A[i][p] * inv
            if m == 0:
                continue
            for j in range(p + 1, n):
                A[i][j] -= m * A[p][j]
            for j in range(nc):
                B[i][j] -= m * B[p][j]
    X = [[mp.mpf(0)] * nc for _ in range(n)]
    for i in range(n - 1, -1, -1):
        for j in range(nc):
            s = B[i][j]
            for q in range(i + 1, n):
                s -= A[i][q] * X[q][j]
            X[i][j] = s / A[i][i]
    return X


def exact_record(lc, f, n):
    """-> (S packed [NF (NF + 1) / 2], g [NF]) of the 50-digit elimination, rounded to double at the end"""
    import mpmath
    with mpmath.workdps(DPS):
        mp = mpmath.mp
        M = lc.shape[0]
        NF = M - n
        cols = [[mp.mpf(float(lc[i, n + c])) for c in range(NF)] + [mp.mpf(float(f[i]))] for i in range(n)]
        X = _solve_mp(lc, cols, n, mp)
        S = np.zeros(NF * (NF + 1) // 2)
        for j in range(NF):
            for i in range(j + 1):
                s = mp.mpf(float(lc[n + i, n + j]))
                for q in range(n):
                    s -= mp.mpf(float(lc[q, n + i])) * X[q][j]
                S[j * (j + 1) // 2 + i] = float(s)
        g = np.zeros(NF)
        for i in range(NF):
            s = mp.mpf(0)
            for q in range(n):
                s -= mp.mpf(float(lc[q, n + i])) * X[q][NF]
            g[i] = float(s)
    return S, g


def exact_recover(lc, f, uF, n):
    """-> u_T = A_TT^-1 (f - A_TF u_F) of the 50-digit substitution, rounded to double at the end"""
    import mpmath
    with mpmath.workdps(DPS):
        mp = mpmath.mp
        NF = lc.shape[0] - n
        cols = []
        for i in range(n):
            s = mp.mpf(float(f[i]))
            for c in range(NF):
                s -= mp.mpf(float(lc[i, n + c])) * mp.mpf(float(uF[c]))
            cols.append([s])
        X = _solve_mp(lc, cols, n, mp)
        return np.array([float(X[i][0]) for i in range(n)])


def record_error(S, g, S_ref, g_ref):
    """max |candidate - exact| over the record, relative to the record's largest entry"""
    scale = max(np.abs(S_ref).max(), np.abs(g_ref).max())
    return max(np.abs(S - S_ref).max(), np.abs(g - g_ref).max()) / scale


def worst_record_error(lcs, fs, S, g, n):
    """over the cells of lcs [ncut, M, M] / fs [ncut, n]: the largest record_error of the candidate records S / g"""
    worst = 0.0
    for c in range(len(lcs)):
        S_ref, g_ref = exact_record(lcs[c], fs[c], n)
        worst = max(worst, record_error(S[c], g[c], S_ref, g_ref))
    return worst


def worst_recover_error(lcs, fs, uFs, uT, n):
    worst = 0.0
    for c in range(len(lcs)):
        ref = exact_recover(lcs[c], fs[c], uFs[c], n)
        worst = max(worst, np.abs(uT[c] - ref).max() / np.abs(ref).max())
    return worst


def eliminate(lc, f, n, dtype):
    """the record by a Cholesky elimination carried out in `dtype` (numpy.float64: the plain-double route; numpy.longdouble: 11
    bits more), rounded to double at the end -> (S packed, g)"""
    M = lc.shape[0]
    NF = M - n
    A = lc[:n, :n].astype(dtype)
    B = np.concatenate([lc[:n, n:], np.asarray(f).reshape(n, 1)], axis=1).astype(dtype)
    L = np.zeros((n, n), dtype=dtype)
    for j in range(n):
        d = A[j, j] - np.dot(L[j, :j], L[j, :j])
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    W = np.zeros((n, NF + 1), dtype=dtype)
    for i in range(n):
        W[i] = (B[i] - L[i, :i] @ W[:i]) / L[i, i]
    Sfull = lc[n:, n:].astype(dtype) - W[:, :NF].T @ W[:, :NF]
    gv = -(W[:, :NF].T @ W[:, NF])
    S = np.zeros(NF * (NF + 1) // 2)
    for j in range(NF):
        for i in range(j + 1):
            S[j * (j + 1) // 2 + i] = float(Sfull[i, j])
    return S, np.array([float(v) for v in gv])
