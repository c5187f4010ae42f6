"""The interface problem condensed to its face unknowns on the device (pa_interface_condensed_*, interface_condensed.hip): the
records, the face-only system in CSR against the sorted path and against the Schur complement of the full system
(pa_interface_csr_*), the cut records against mpmath, the solve with recovery and the xlsx Interface table."""
import ctypes as C
import math

import numpy as np
import pytest

import interface_helpers as ih
from interface_helpers import condensed_sizes as sizes, real_ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def asm():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    from proton_amd.batch import BatchAssembler
    return BatchAssembler(0)


def sorted_path(asm, k, rec, g):
    """pa_interface_condensed_triplets_batch -> slots in cell order -> pa_csr_from_triplets"""
    return ih.sorted_path(asm, asm.interface_condensed_triplets(k, rec, g), sizes(k)[2], asm.ctx.interface_condensed_query(k).system_size)


def synthetic_records(asm, N, k, seed, **kw):
    """seeded random records and Dirichlet data (the interface operators stop at face degree 2)"""
    import torch
    asm.cut_preprocess(N, refsteps=4, **kw)
    qi = asm.ctx.interface_condensed_query(k)
    gen = torch.Generator(device=asm.device).manual_seed(seed)
    f64 = dict(dtype=torch.float64, device=asm.device)
    rec = {"cond": torch.rand(asm.ncells * qi.cond_doubles, generator=gen, **f64) - 0.5,
           "cond_cut": torch.rand(max(asm.ncut * qi.cond_cut_doubles, 1), generator=gen, **f64) - 0.5}
    g = torch.rand(2 * N * (N + 1) * (k + 1), generator=gen, **f64) - 0.5
    return rec, g


def check_bit_identical(asm, k, rec, g):
    return ih.check_bit_identical(asm, sorted_path(asm, k, rec, g), lambda: asm.interface_condensed_csr_pattern(k),
                                  lambda: asm.interface_condensed_csr_fill(k, rec, g))


def full_csr(asm, k, ops, g):
    import scipy.sparse as sp
    rp, ci = asm.interface_csr_pattern(k)
    va, RH = asm.interface_csr_fill(k, ops, g)
    asm.synchronize()
    n = RH.numel()
    return sp.csr_matrix((va.cpu().numpy(), ci.cpu().numpy(), rp.cpu().numpy()), shape=(n, n)), RH.cpu().numpy()


# ---- 1. the direct CSR against the sorted path ------------------------------------------------------------------------------
@pytest.mark.parametrize("N,k", [(10, 0), (10, 1), (20, 1), (20, 2)])
def test_condensed_csr_equals_sorted_path(asm, N, k):
    ops, g = real_ops(asm, N, k)
    assert asm.ncut > 0
    rec = asm.interface_condensed_ops(k, ops)
    check_bit_identical(asm, k, rec, g)


def test_condensed_csr_equals_sorted_path_at_bench_size(asm):
    """512 x 512, k = 2"""
    ops, g = real_ops(asm, 512, 2)
    rec = asm.interface_condensed_ops(2, ops)
    del ops
    check_bit_identical(asm, 2, rec, g)


def test_condensed_csr_face_degree_3_synthetic(asm):
    rec, g = synthetic_records(asm, 16, 3, seed=13)
    assert asm.ncut > 0
    check_bit_identical(asm, 3, rec, g)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_condensed_csr_line_level_set_drops_the_boundary_slots(asm, k):
    """a line level set: cut cells on the left and right boundaries, whose Dirichlet slots are dropped"""
    N = 12
    rec, g = synthetic_records(asm, N, k, seed=7 + k, line_y=0.43)
    cut_cells = np.nonzero(np.asarray(asm.cut_index) >= 0)[0]
    assert np.any(cut_cells % N == 0) and np.any(cut_cells % N == N - 1)
    check_bit_identical(asm, k, rec, g)


# ---- 2. the Schur complement of the full system ----------------------------------------------------------------------------
@pytest.mark.parametrize("N,k,kw", [(20, 2, {}), (10, 1, {}), (12, 1, {"line_y": 0.43})], ids=["circle-20-k2", "circle-10-k1", "line-12-k1"])
def test_condensed_pattern_is_the_face_block_of_the_full_pattern(asm, N, k, kw):
    """the face part of every face group's row (IfGroup::fu0, fpos) against the face-face block cut out of the full pattern on the
    host: the circle, and the line level set with Dirichlet faces on the cut cells' rows"""
    cbs, fbs, nf, NF = sizes(k)
    asm.cut_preprocess(N, refsteps=4, **kw)
    assert asm.ncut > 0
    info = asm.ctx.interface_info(k)
    rp, ci = asm.interface_csr_pattern(k)
    crp, cci = asm.interface_condensed_csr_pattern(k)
    asm.synchronize()
    rp, ci, crp, cci = rp.cpu().numpy(), ci.cpu().numpy(), crp.cpu().numpy(), cci.cpu().numpy()
    c0 = cbs * info.num_all_cells
    sub_rp, sub_ci = [0], []
    for r in range(c0, rp.size - 1):
        cols = ci[rp[r]:rp[r + 1]]
        cols = cols[cols >= c0] - c0
        sub_ci.append(cols)
        sub_rp.append(sub_rp[-1] + cols.size)
    assert np.array_equal(crp, np.asarray(sub_rp)) and np.array_equal(cci, np.concatenate(sub_ci))


def test_condensed_values_are_the_schur_complement(asm):
    """K_FF - K_FT K_TT^-1 K_TF of pa_interface_csr_fill's matrix (scipy, in double), 1e-9 of each row's largest entry"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    N, k = 20, 2
    cbs, fbs, nf, NF = sizes(k)
    ops, g = real_ops(asm, N, k)
    info = asm.ctx.interface_info(k)
    K, b = full_csr(asm, k, ops, g)
    rec = asm.interface_condensed_ops(k, ops)
    crp, cci = asm.interface_condensed_csr_pattern(k)
    cva, cRH = asm.interface_condensed_csr_fill(k, rec, g)
    asm.synchronize()
    c0 = cbs * info.num_all_cells
    K = K.tocsc()
    KTT, KTF, KFT, KFF = K[:c0, :c0], K[:c0, c0:], K[c0:, :c0], K[c0:, c0:]
    lu = spla.splu(KTT.tocsc())
    Y = lu.solve(KTF.toarray())
    S = KFF.toarray() - KFT @ Y
    bS = b[c0:] - KFT @ lu.solve(b[:c0])
    n = cRH.numel()
    A = sp.csr_matrix((cva.cpu().numpy(), cci.cpu().numpy(), crp.cpu().numpy()), shape=(n, n)).toarray()
    scale = np.abs(S).max(axis=1)
    assert np.all(np.abs(A - S).max(axis=1) <= 1e-9 * scale)
    assert np.abs(cRH.cpu().numpy() - bS).max() <= 1e-9 * np.abs(bS).max()


# ---- 3. the records -------------------------------------------------------------------------------------------------------
def mp_schur(lc, f, n, mp):
    """S (upper triangle, column-packed) and g of a symmetric local matrix at mp.dps digits: the lower triangle of A_TT, A_TF and
    the upper triangle of A_FF, the entries the kernel reads"""
    M = lc.shape[0]
    NF = M - n
    A = [[mp.mpf(float(lc[max(i, j), min(i, j)])) for j in range(n)] for i in range(n)]
    B = [[mp.mpf(float(lc[i, n + c])) for c in range(NF)] + [mp.mpf(float(f[i]))] for i in range(n)]
    # Gaussian elimination (A is SPD: no pivoting) on [A | B], then back substitution: X = A^-1 B
    for p in range(n):
        inv = 1 / A[p][p]
        for i in range(p + 1, n):
            m = A[i][p] * inv
            if m == 0:
                continue
            for j in range(p + 1, n):
                A[i][j] -= m * A[p][j]
            for j in range(NF + 1):
                B[i][j] -= m * B[p][j]
    X = [[mp.mpf(0)] * (NF + 1) for _ in range(n)]
    for i in range(n - 1, -1, -1):
        for j in range(NF + 1):
            s = B[i][j]
            for q in range(i + 1, n):
                s -= A[i][q] * X[q][j]
            X[i][j] = s / A[i][i]
    T = [[mp.mpf(float(lc[q, n + i])) for i in range(NF)] for q in range(n)]      # A_FT(i, q) = A_TF(q, i): the kernel reads A_TF
    S = np.zeros(NF * (NF + 1) // 2)
    for j in range(NF):
        for i in range(j + 1):
            s = mp.mpf(float(lc[n + i, n + j]))
            for q in range(n):
                s -= T[q][i] * X[q][j]
            S[j * (j + 1) // 2 + i] = float(s)
    gv = np.zeros(NF)
    for i in range(NF):
        s = mp.mpf(0)
        for q in range(n):
            s -= T[q][i] * X[q][NF]
        gv[i] = float(s)
    return S, gv


@pytest.mark.parametrize("N,k", [(20, 1), (20, 2), (64, 1), (64, 2)])
def test_cut_records_against_mpmath(asm, N, k):
    """every cut cell's S and g against a 50-digit elimination of the GPU's own lc_cut / rhs_cut: <= 1e-13 of the record's largest
    entry (plain double: 1e-12 .. 7e-11); the uncut records are pa_static_condensation_packed_batch's, bit for bit"""
    import torch
    import mpmath
    import proton_amd as pa
    from proton_amd.batch import to_rowcol
    cbs, fbs, nf, NF = sizes(k)
    ops, g = real_ops(asm, N, k)
    rec = asm.interface_condensed_ops(k, ops)
    ntri, NTRI = nf * (nf + 1) // 2, NF * (NF + 1) // 2
    n, ncut = asm.ncells, asm.ncut
    di, _ = pa.capi.degree_info(k + 1, k)
    Sp = torch.empty((n, ntri), dtype=torch.float64, device=asm.device)
    gp = torch.empty((n, nf), dtype=torch.float64, device=asm.device)
    asm.ctx.static_condensation_packed(di, n, ops["lc"].data_ptr(), ops["rhs"].data_ptr(), Sp.data_ptr(), gp.data_ptr(), None)
    asm.synchronize()
    assert torch.equal(rec["cond"][:n * ntri], Sp.reshape(-1)) and torch.equal(rec["cond"][n * ntri:], gp.reshape(-1))
    assert int(rec["info"].abs().sum()) == 0 and int(rec["info_cut"].abs().sum()) == 0
    lcc, rhsc = to_rowcol(ops["lc_cut"]), ops["rhs_cut"].cpu().numpy()
    cc = rec["cond_cut"].cpu().numpy()
    S_gpu, g_gpu = cc[:ncut * NTRI].reshape(ncut, NTRI), cc[ncut * NTRI:].reshape(ncut, NF)
    mpmath.mp.dps = 50
    worst = 0.0
    for c in range(ncut):
        S, gv = mp_schur(lcc[c], rhsc[c], 2 * cbs, mpmath.mp)
        scale = max(np.abs(S).max(), np.abs(gv).max())
        err = max(np.abs(S_gpu[c] - S).max(), np.abs(g_gpu[c] - gv).max()) / scale
        worst = max(worst, err)
    print("N %d k %d: %d cut cells, max record-relative error %.3e" % (N, k, ncut, worst))
    assert worst <= 1e-13


# ---- 4. / 5. solve and recovery ---------------------------------------------------------------------------------------------
def condensed_solve(asm, k, ops, g, tol):
    rec = asm.interface_condensed_ops(k, ops)
    rp, ci = asm.interface_condensed_csr_pattern(k)
    va, RH = asm.interface_condensed_csr_fill(k, rec, g)
    n = RH.numel()
    xF, reason, iters, relres = asm.conjugated_gradient(rp, ci, va, RH, tol=tol, max_iter=20 * n, precond=True)
    assert reason == 0, (reason, iters, relres)
    return asm.interface_condensed_recover(k, ops, xF, g)


def test_condensed_solve_matches_a_direct_solve_of_the_full_system(asm):
    import scipy.sparse.linalg as spla
    N, k = 20, 2
    ops, g = real_ops(asm, N, k)
    K, b = full_csr(asm, k, ops, g)
    ref = spla.spsolve(K.tocsc(), b)
    full = condensed_solve(asm, k, ops, g, 1e-13)
    asm.synchronize()
    assert np.abs(full.cpu().numpy() - ref).max() <= 1e-8 * np.abs(ref).max()


@pytest.mark.parametrize("k,N,ref", [(0, 10, 0.285023), (1, 20, 5.22389e-3), (2, 20, 1.38029e-4)])
def test_condensed_path_reproduces_xlsx(asm, oracle, k, N, ref):
    """the energy-norm error (:1762-1833) of the recovered full vector, CG threshold 1e-9 with Jacobi (:1737-1743)"""
    o = oracle
    ops, g = real_ops(asm, N, k)
    sol = condensed_solve(asm, k, ops, g, 1e-9).cpu().numpy()
    msh = o.CutMesh(N, refsteps=4)
    di = o.degrees(k + 1, k)
    ct, ft, num_all_cells, num_other = msh.interface_tables()
    assert sol.size == di.cbs * num_all_cells + di.fbs * num_other
    L = o.lib()
    cbs, rd = di.cbs, di.rec_deg
    H1 = 0.0
    gx, gy, bar = np.zeros(32), np.zeros(32), np.zeros(2)
    for c in range(msh.nc):
        pts = np.ascontiguousarray(msh.points[msh.ptids[c].astype(np.int64)].reshape(8))
        L.hho_cell_barycenter(o._dp(pts), o._dp(bar))
        h = L.hho_cell_diameter(o._dp(pts))
        sides = (o.CUT_NEG, o.CUT_POS) if msh.cell_loc[c] == o.CUT_ON_INTERFACE else (int(msh.cell_loc[c]),)
        for where in sides:
            o0 = L.cut_interface_cell_offset(msh.h, di, c, o._i64p(ct), where)
            dofs = sol[o0:o0 + cbs]
            qx, qy, qw = msh.cell_quadrature(c, 2 * di.cell_deg, where)
            for q in range(len(qw)):
                L.hho_cell_basis_grad(o._dp(bar), h, rd, qx[q], qy[q], o._dp(gx), o._dp(gy))
                g0 = float(np.dot(dofs[1:], gx[1:cbs]))
                g1 = float(np.dot(dofs[1:], gy[1:cbs]))
                s0 = math.pi * math.cos(math.pi * qx[q]) * math.sin(math.pi * qy[q])
                s1 = math.pi * math.sin(math.pi * qx[q]) * math.cos(math.pi * qy[q])
                H1 += qw[q] * ((s0 - g0) ** 2 + (s1 - g1) ** 2)
    err = math.sqrt(H1)
    assert abs(err - ref) / ref < 6e-6, err


# ---- 6. no cut cells ------------------------------------------------------------------------------------------------------
def test_condensed_without_cut_cells_is_the_plain_condensed_system(asm):
    """a circle outside the square, kappa_1 = kappa_2 = 1: the records of pa_static_condensation_packed_batch assembled by
    pa_condensed_csr_*, bit for bit"""
    import torch
    import proton_amd as pa
    N, k = 9, 1
    cbs, fbs, nf, NF = sizes(k)
    asm.level_set = pa.capi.LevelSet(0, 2.0, 0.5, 0.5, 0.0)
    asm.ctx.cut_preprocess(N, N, asm.level_set, 4)
    asm.ncut, asm.cell_loc, asm.cut_index = asm.ctx.cut_query()
    assert asm.ncut == 0
    ops = asm.interface_local_ops(k)
    g = asm.dirichlet_data(k, pa.capi.FN_SIN_SIN_SOL)
    rec = asm.interface_condensed_ops(k, ops)
    rp, ci = asm.interface_condensed_csr_pattern(k)
    va, RH = asm.interface_condensed_csr_fill(k, rec, g)
    n, ntri = asm.ncells, nf * (nf + 1) // 2
    di, _ = pa.capi.degree_info(k + 1, k)
    Sp = torch.empty((n, ntri), dtype=torch.float64, device=asm.device)
    gp = torch.empty((n, nf), dtype=torch.float64, device=asm.device)
    asm.ctx.static_condensation_packed(di, n, ops["lc"].data_ptr(), ops["rhs"].data_ptr(), Sp.data_ptr(), gp.data_ptr(), None)
    plain = torch.cat([Sp, gp], dim=1).contiguous()
    rp2, ci2 = asm.condensed_csr_pattern(k + 1, k)
    va2, RH2 = asm.condensed_csr_fill(k + 1, k, plain, g)
    asm.synchronize()
    assert torch.equal(rp, rp2) and torch.equal(ci, ci2) and torch.equal(va, va2) and torch.equal(RH, RH2)


# ---- 7. contexts and refusals ---------------------------------------------------------------------------------------------
def test_condensed_second_cut_of_the_same_context(asm):
    """pa_cut_preprocess again with another radius, another face degree in between: the output is a fresh context's"""
    import torch
    from proton_amd.batch import BatchAssembler
    N, k = 20, 2
    ops, g = real_ops(asm, N, k)
    rec = asm.interface_condensed_ops(k, ops)
    asm.interface_condensed_csr_pattern(k)
    asm.interface_condensed_csr_fill(k, rec, g)
    asm.interface_condensed_csr_pattern(1)
    ops, g = real_ops(asm, N, k, radius=0.3)
    rec = asm.interface_condensed_ops(k, ops)
    rp, ci = asm.interface_condensed_csr_pattern(k)
    va, RH = asm.interface_condensed_csr_fill(k, rec, g)
    fresh = BatchAssembler(0)
    ops2, g2 = real_ops(fresh, N, k, radius=0.3)
    rec2 = fresh.interface_condensed_ops(k, ops2)
    rp2, ci2 = fresh.interface_condensed_csr_pattern(k)
    va2, RH2 = fresh.interface_condensed_csr_fill(k, rec2, g2)
    asm.synchronize(); fresh.synchronize()
    assert torch.equal(rec["cond_cut"], rec2["cond_cut"]) and torch.equal(rec["cond"], rec2["cond"])
    assert torch.equal(rp, rp2) and torch.equal(ci, ci2) and torch.equal(va, va2) and torch.equal(RH, RH2)


def test_condensed_with_cut_overlap(asm):
    """pa_context_set_cut_overlap(1): a cut-cell kernel on the side stream writes the records' input; the entry points join the side
    stream first and give the same bits as with overlap off"""
    import torch
    import proton_amd as pa
    N, k = 20, 2
    ops, g = real_ops(asm, N, k)

    def run(overlap):
        asm.ctx.set_cut_overlap(overlap)
        try:
            lc_cut = ops["lc_cut"].clone()
            asm.ctx.cut_local_ops(k, asm.level_set, pa.capi.LOC_NEGATIVE, pa.capi.FN_SIN_SIN_RHS, pa.capi.FN_SIN_SIN_SOL,
                                  None, None, None, lc_cut.data_ptr(), None, None)
            rec = asm.interface_condensed_ops(k, dict(ops, lc_cut=lc_cut))
            va, RH = asm.interface_condensed_csr_fill(k, rec, g)
            asm.synchronize()
        finally:
            asm.ctx.set_cut_overlap(False)
        return rec["cond_cut"].clone(), va.clone(), RH.clone(), lc_cut

    c1, va, RH, lc_cut = run(False)
    c2, va2, RH2, lc_cut2 = run(True)
    assert not torch.equal(lc_cut, ops["lc_cut"]) and torch.equal(lc_cut, lc_cut2)
    # (the fictitious-domain lc written over the two-sided one is no SPD matrix: NaNs among the records, compared as bits)
    bits = lambda t: t.view(torch.int64)        # noqa: E731
    assert torch.equal(bits(c1), bits(c2)) and torch.equal(bits(va), bits(va2)) and torch.equal(bits(RH), bits(RH2))


def test_condensed_refusals(asm):
    """the refusals of pa_interface_csr_*, in its order"""
    import torch
    import proton_amd as pa
    from proton_amd.batch import BatchAssembler
    L = pa.capi.lib()
    out = pa.capi.InterfaceCondensedInfo()
    buf = torch.zeros(1 << 16, dtype=torch.float64, device=asm.device)
    p = buf.data_ptr()

    def calls(h, fd):
        return [L.pa_interface_condensed_query(h, fd, C.byref(out)),
                L.pa_interface_condensed_ops_batch(h, fd, p, None, p, None, p, p, None, None),
                L.pa_interface_condensed_triplets_batch(h, fd, p, p, None, *([p] * 10)),
                L.pa_interface_condensed_csr_pattern(h, fd, p, None),
                L.pa_interface_condensed_csr_fill(h, fd, p, p, None, p, None),
                L.pa_interface_condensed_recover(h, fd, p, None, p, None, None, p, p)]
    bare = BatchAssembler(0)
    assert calls(bare.ctx.h, 1) == [5] * 6                       # no mesh
    bare.generate_mesh(8, 8)
    assert calls(bare.ctx.h, 1) == [5] * 6                       # a plain mesh, no cut mesh
    asm.cut_preprocess(12, rows=(3, 8))
    assert calls(asm.ctx.h, 1) == [1] * 6                        # a slab
    assert "whole mesh" in L.pa_last_error(asm.ctx.h).decode()
    asm.cut_preprocess(12)
    assert asm.ncut > 0
    for fd in (-1, 4):
        assert calls(asm.ctx.h, fd) == [2] * 6                   # face degree
    # the cut-cell arrays with cut cells, NULL outputs
    assert L.pa_interface_condensed_ops_batch(asm.ctx.h, 1, p, None, None, None, p, p, None, None) == 1
    assert L.pa_interface_condensed_ops_batch(asm.ctx.h, 1, p, None, p, None, p, None, None, None) == 1
    assert L.pa_interface_condensed_triplets_batch(asm.ctx.h, 1, p, None, None, *([p] * 10)) == 1
    assert L.pa_interface_condensed_csr_fill(asm.ctx.h, 1, p, None, None, p, None) == 1
    assert L.pa_interface_condensed_recover(asm.ctx.h, 1, p, None, None, None, None, p, p) == 1
    assert L.pa_interface_condensed_query(asm.ctx.h, 1, None) == 1
    assert L.pa_interface_condensed_csr_pattern(asm.ctx.h, 1, None, None) == 1
    assert L.pa_interface_condensed_csr_fill(asm.ctx.h, 1, p, p, None, None, None) == 1
    # the same context still works; colind may be NULL
    assert L.pa_interface_condensed_query(asm.ctx.h, 1, C.byref(out)) == 0
    rp = torch.empty(out.system_size + 1, dtype=torch.int64, device=asm.device)
    assert L.pa_interface_condensed_csr_pattern(asm.ctx.h, 1, rp.data_ptr(), None) == 0
    asm.synchronize()
    assert int(rp[-1]) == out.nnz and out.nf == 8 and out.NF == 16
