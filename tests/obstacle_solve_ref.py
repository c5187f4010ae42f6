"""Host restatements for the tests of pa_obstacle_block_solve / pa_obstacle_solve: the block structure of obstacle_assembler's
system (hho.hpp:609-695, :688-693) in numpy, and the primal-dual active set loop of obstacle.cpp:117-197 on the CPU oracle with
scipy's sparse direct solve (the reference's SparseLU, obstacle.cpp:170-175)."""
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def row_map(A_ct, ncells, nrows, num_I):
    """CSR row of every row of the SPD block: one scatter of A_ct (inv[A_ct[c]] = c), the face rows shifted by num_A"""
    num_A = ncells - num_I
    nk = nrows - num_A
    rowmap = np.full(nk, -1, dtype=np.int64)
    cells = np.nonzero(np.asarray(A_ct) >= 0)[0]
    rowmap[np.asarray(A_ct)[cells]] = cells
    rowmap[num_I:] = np.arange(ncells, nrows)
    assert (rowmap >= 0).all()
    return rowmap


def extract_block(rowptr, colind, values, b, rowmap):
    """K (rowptr, colind, values) and its right-hand side: the rows rowmap names, entry for entry in their stored order"""
    nk = rowmap.shape[0]
    lens = rowptr[rowmap + 1] - rowptr[rowmap]
    krp = np.zeros(nk + 1, dtype=np.int64)
    np.cumsum(lens, out=krp[1:])
    idx = np.concatenate([np.arange(rowptr[r], rowptr[r + 1]) for r in rowmap]) if nk else np.zeros(0, dtype=np.int64)
    kci, kva = colind[idx], values[idx]
    assert nk == 0 or kci.max() < nk, "a kept row holds a multiplier column"
    return krp, kci.astype(np.int32), kva, b[rowmap]


def multipliers(rowptr, colind, values, b, in_A, B_ct, nk, y):
    """-> (columns, values, bounds): x[col] = b_i - sum_j A_ij y_j over the columns below nk of every active row i, summed as
    tests/cpp/obstacle_driver.cpp sums it, and 1e-14 (|b_i| + sum |A_ij y_j|), the rounding bound of a sum of 11 terms or fewer"""
    cols, vals, bounds = [], [], []
    for c in np.nonzero(in_A)[0]:
        s, mag = b[c], abs(b[c])
        for k in range(rowptr[c], rowptr[c + 1]):
            if colind[k] < nk:
                s -= values[k] * y[colind[k]]
                mag += abs(values[k] * y[colind[k]])
            else:
                assert colind[k] == nk + B_ct[c] and values[k] == 1.0
        cols.append(nk + B_ct[c]); vals.append(s); bounds.append(1e-14 * mag)
    return np.array(cols, dtype=np.int64), np.array(vals), np.array(bounds)


def solve_by_blocks(LHS, RHS, in_A, A_ct, B_ct, num_I, solve_K):
    """the solution of the whole system from a solve of the SPD block: the numpy statement of pa_obstacle_block_solve"""
    A = sp.csr_matrix(LHS)
    A.sort_indices()
    nrows, nc = A.shape[0], in_A.shape[0]
    rowmap = row_map(A_ct, nc, nrows, num_I)
    nk = rowmap.shape[0]
    krp, kci, kva, bk = extract_block(A.indptr.astype(np.int64), A.indices, A.data, RHS, rowmap)
    x = np.zeros(nrows)
    if nk:
        x[:nk] = solve_K(sp.csr_matrix((kva, kci, krp), shape=(nk, nk)), bk)
    cols, vals, _ = multipliers(A.indptr, A.indices, A.data, RHS, in_A, B_ct, nk, x[:nk])
    x[cols] = vals
    return x


def jacobi_cg(K, b, tol=1e-13):
    """scipy's conjugate gradient with the settings of the device solve: Jacobi, relative residual below tol, 20 n iterations"""
    n = K.shape[0]
    M = sp.diags(1.0 / K.diagonal())
    try:
        y, info = spla.cg(K, b, rtol=tol, atol=0.0, maxiter=20 * n, M=M)
    except TypeError:                                # scipy < 1.12
        y, info = spla.cg(K, b, tol=tol, atol=0.0, maxiter=20 * n, M=M)
    assert info == 0
    return y


@functools.lru_cache(maxsize=None)
def cpu_loop(N, degree, max_outer=50, c=1.0, outer_tol=1e-7):
    """obstacle.cpp:117-197 from obstacle_driver.ObstacleMesh, oracle_local_provider, oracle_lib.ObstacleAssembler and spsolve ->
    dict(alpha, beta, in_A (of the last system), num_A (per system), min_diff (smallest |beta + c (alpha - gamma)| met),
    dev_alpha / dev_beta (largest deviation of a Jacobi-CG at 1e-13 on the SPD block from spsolve on the same system, over the
    iterations), lc, msh)"""
    import obstacle_driver as od
    import oracle_lib as o
    msh = od.ObstacleMesh(N)
    di = o.degrees(0, degree)
    nc, nf, fbs = msh.ncells, msh.nfaces, degree + 1
    lc, rhs = od.oracle_local_provider(msh, degree)
    alpha, beta, gamma = np.zeros(nc + fbs * nf), np.ones(nc), np.zeros(nc)
    hist, min_diff, dev_alpha, dev_beta = [], np.inf, 0.0, 0.0
    converged = False
    in_A = None
    while len(hist) < max_outer:
        diff = beta + c * (alpha[:nc] - gamma)          # :133
        in_A = diff < 0
        min_diff = min(min_diff, np.abs(diff).min())
        asm = o.ObstacleAssembler(msh.mp, msh.points, msh.ptids, di, in_A, bf_id=4)
        rows, cols, vals = [], [], []
        RHS = np.zeros(asm.system_size)
        for cell in range(nc):                          # :148-156
            tr, tc, tv, rr, rv = asm.assemble_cell(cell, lc[cell], rhs[cell], gamma)
            rows.append(tr); cols.append(tc); vals.append(tv)
            ok = rr >= 0
            np.add.at(RHS, rr[ok], rv[ok])
        LHS = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(asm.system_size,) * 2)
        hist.append(int(in_A.sum()))
        sol = spla.spsolve(LHS, RHS)                    # :170-175
        sol_cg = solve_by_blocks(LHS, RHS, in_A, asm.A_ct, asm.B_ct, asm.num_I, jacobi_cg)
        alpha_prev = alpha
        alpha, beta = asm.expand_solution(sol, gamma)
        a_cg, b_cg = asm.expand_solution(sol_cg, gamma)
        dev_alpha, dev_beta = max(dev_alpha, np.abs(a_cg - alpha).max()), max(dev_beta, np.abs(b_cg - beta).max())
        if np.linalg.norm(alpha_prev - alpha) < outer_tol:   # :193
            converged = True
            break
    return dict(alpha=alpha, beta=beta, in_A=in_A, num_A=hist, min_diff=min_diff, dev_alpha=dev_alpha, dev_beta=dev_beta, lc=lc,
                msh=msh, converged=converged)
