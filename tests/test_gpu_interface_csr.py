"""interface_assembler's global system (cuthho_square.cpp:1091-1443) built directly in CSR (pa_interface_csr_*,
interface_csr.hip) against the sorted path: pa_csr_from_triplets of pa_interface_triplets_batch's slots taken in cell order."""
import ctypes as C

import numpy as np
import pytest

import interface_helpers as ih
from interface_helpers import full_sizes as sizes, real_ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def asm():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    from proton_amd.batch import BatchAssembler
    return BatchAssembler(0)


def sorted_path(asm, k, ops, g):
    """pa_interface_triplets_batch -> slots in cell order -> pa_csr_from_triplets"""
    return ih.sorted_path(asm, asm.interface_triplets(k, ops, g), sizes(k)[1], asm.ctx.interface_info(k).system_size)


def synthetic_ops(asm, N, k, seed, **kw):
    """seeded random local matrices and right-hand sides (the interface operators stop at face degree 2)"""
    import torch
    asm.cut_preprocess(N, refsteps=4, **kw)
    cbs, ms = sizes(k)
    gen = torch.Generator(device=asm.device).manual_seed(seed)
    f64 = dict(dtype=torch.float64, device=asm.device)
    nfaces = 2 * N * (N + 1)
    ops = {"lc": torch.rand((asm.ncells, ms, ms), generator=gen, **f64) - 0.5,
           "rhs": torch.rand((asm.ncells, cbs), generator=gen, **f64) - 0.5,
           "lc_cut": torch.rand((asm.ncut, 2 * ms, 2 * ms), generator=gen, **f64) - 0.5,
           "rhs_cut": torch.rand((asm.ncut, 2 * cbs), generator=gen, **f64) - 0.5}
    g = torch.rand(nfaces * (k + 1), generator=gen, **f64) - 0.5
    return ops, g


def check_bit_identical(asm, k, ops, g):
    return ih.check_bit_identical(asm, sorted_path(asm, k, ops, g), lambda: asm.interface_csr_pattern(k),
                                  lambda: asm.interface_csr_fill(k, ops, g))


@pytest.mark.parametrize("N,k", [(10, 0), (20, 1), (20, 2)])
def test_interface_csr_equals_sorted_path(asm, N, k):
    ops, g = real_ops(asm, N, k)
    assert asm.ncut > 0
    check_bit_identical(asm, k, ops, g)


def test_interface_csr_equals_sorted_path_at_bench_size(asm):
    """the bench's interface size: 512 x 512, k = 2"""
    ops, g = real_ops(asm, 512, 2)
    check_bit_identical(asm, 2, ops, g)


def test_interface_csr_face_degree_3_synthetic(asm):
    """k = 3: the index maps go to face degree 3 (the operators refuse it with PA_ERR_QUADRATURE), random local matrices"""
    import proton_amd as pa
    asm.cut_preprocess(16, refsteps=4)
    with pytest.raises(pa.capi.ProtonAmdError):
        asm.interface_local_ops(3)
    ops, g = synthetic_ops(asm, 16, 3, seed=11)
    assert asm.ncut > 0
    check_bit_identical(asm, 3, ops, g)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_interface_csr_line_level_set_drops_the_boundary_slots(asm, k):
    """a line level set: cut cells on the left and right boundaries.  The reference throws there (:1304-1305), the triplet kernel
    drops the Dirichlet slots, and so does the CSR"""
    ops, g = synthetic_ops(asm, 12, k, seed=5 + k, line_y=0.43)
    ci = np.asarray(asm.cut_index)
    N = 12
    cut_cells = np.nonzero(ci >= 0)[0]
    assert np.any(cut_cells % N == 0) and np.any(cut_cells % N == N - 1)
    check_bit_identical(asm, k, ops, g)


def test_interface_csr_without_cut_cells_is_the_plain_assembler(asm):
    """a circle outside the square: the system is assembler<Mesh>'s, and so is its direct CSR, bit for bit"""
    import torch
    import proton_amd as pa
    N, k = 9, 1
    asm.level_set = pa.capi.LevelSet(0, 2.0, 0.5, 0.5, 0.0)
    asm.ctx.cut_preprocess(N, N, asm.level_set, 4)
    asm.ncut, asm.cell_loc, asm.cut_index = asm.ctx.cut_query()
    assert asm.ncut == 0
    ops = asm.interface_local_ops(k)
    g = asm.dirichlet_data(k, pa.capi.FN_SIN_SIN_SOL)
    rp, ci = asm.interface_csr_pattern(k)
    va, RH = asm.interface_csr_fill(k, ops, g)
    rp2, ci2 = asm.assembler_csr_pattern(k + 1, k)
    va2, RH2 = asm.assembler_csr_fill(k + 1, k, ops["lc"], ops["rhs"], g)
    asm.synchronize()
    assert torch.equal(rp, rp2) and torch.equal(ci, ci2) and torch.equal(va, va2) and torch.equal(RH, RH2)


def test_interface_csr_structure(asm):
    """rows sorted and duplicate-free, symmetric pattern, nnz of the query"""
    import scipy.sparse as sp
    N, k = 20, 1
    real_ops(asm, N, k)
    info = asm.ctx.interface_csr_query(k)
    rp, ci = asm.interface_csr_pattern(k)
    asm.synchronize()
    rp, ci = rp.cpu().numpy(), ci.cpu().numpy()
    assert info.nrows == asm.ctx.interface_info(k).system_size and info.nnz == ci.size == rp[-1]
    assert np.all(np.diff(rp) > 0)
    d = np.diff(ci.astype(np.int64))
    first = np.zeros(ci.size, dtype=bool)
    first[rp[:-1]] = True
    assert np.all(d[~first[1:]] > 0)
    n = info.nrows
    A = sp.csr_matrix((np.ones(ci.size), ci, rp), shape=(n, n))
    assert (A != A.T).nnz == 0


def test_interface_csr_second_cut_of_the_same_context(asm):
    """pa_cut_preprocess again with another radius: the tables are rebuilt, the output is a fresh context's"""
    import torch
    from proton_amd.batch import BatchAssembler
    N, k = 20, 2
    ops, g = real_ops(asm, N, k)
    asm.interface_csr_pattern(k)
    asm.interface_csr_fill(k, ops, g)
    asm.interface_csr_pattern(1)                           # another face degree in between
    ops, g = real_ops(asm, N, k, radius=0.3)
    rp, ci = asm.interface_csr_pattern(k)
    va, RH = asm.interface_csr_fill(k, ops, g)
    fresh = BatchAssembler(0)
    ops2, g2 = real_ops(fresh, N, k, radius=0.3)
    rp2, ci2 = fresh.interface_csr_pattern(k)
    va2, RH2 = fresh.interface_csr_fill(k, ops2, g2)
    asm.synchronize(); fresh.synchronize()
    assert torch.equal(ops["lc_cut"], ops2["lc_cut"])
    assert torch.equal(rp, rp2) and torch.equal(ci, ci2) and torch.equal(va, va2) and torch.equal(RH, RH2)


def test_interface_csr_with_cut_overlap(asm):
    """pa_context_set_cut_overlap(1): a cut-cell kernel on the side stream writes part of the fill's input; the fill joins the side
    stream first and gives the same bits as with overlap off"""
    import torch
    import proton_amd as pa
    N, k = 20, 2
    cbs, ms = sizes(k)
    ops, g = real_ops(asm, N, k)

    def run(overlap):
        asm.ctx.set_cut_overlap(overlap)
        try:
            lc_cut = ops["lc_cut"].clone()
            asm.ctx.cut_local_ops(k, asm.level_set, pa.capi.LOC_NEGATIVE, pa.capi.FN_SIN_SIN_RHS, pa.capi.FN_SIN_SIN_SOL,
                                  None, None, None, lc_cut.data_ptr(), None, None)
            va, RH = asm.interface_csr_fill(k, dict(ops, lc_cut=lc_cut), g)
            asm.synchronize()
        finally:
            asm.ctx.set_cut_overlap(False)
        return va.clone(), RH.clone(), lc_cut

    va, RH, lc_cut = run(False)
    va2, RH2, lc_cut2 = run(True)
    assert not torch.equal(lc_cut, ops["lc_cut"]) and torch.equal(lc_cut, lc_cut2)
    assert torch.equal(va, va2) and torch.equal(RH, RH2)


def test_interface_csr_refusals(asm):
    """the refusals of pa_interface_triplets_batch"""
    import torch
    import proton_amd as pa
    from proton_amd.batch import BatchAssembler
    L = pa.capi.lib()
    out = pa.capi.AssemblerCsrInfo()
    dev = asm.device
    buf = torch.zeros(1 << 16, dtype=torch.float64, device=dev)
    p = buf.data_ptr()
    # no cut mesh: a context without any mesh, and one with a plain generated mesh
    bare = BatchAssembler(0)
    assert L.pa_interface_csr_query(bare.ctx.h, 1, C.byref(out)) == 5
    bare.generate_mesh(8, 8)
    assert L.pa_interface_csr_query(bare.ctx.h, 1, C.byref(out)) == 5
    assert L.pa_interface_csr_pattern(bare.ctx.h, 1, p, None) == 5
    assert L.pa_interface_csr_fill(bare.ctx.h, 1, p, None, None, p, None, p, None) == 5
    # a slab of pa_cut_preprocess_rows: the interface numbering covers the whole mesh
    asm.cut_preprocess(12, rows=(3, 8))
    assert L.pa_interface_csr_query(asm.ctx.h, 1, C.byref(out)) == 1
    assert "whole mesh" in L.pa_last_error(asm.ctx.h).decode()
    assert L.pa_interface_csr_pattern(asm.ctx.h, 1, p, None) == 1
    assert L.pa_interface_csr_fill(asm.ctx.h, 1, p, None, None, p, None, p, None) == 1
    # face degree outside 0..3
    asm.cut_preprocess(12)
    assert asm.ncut > 0
    for fd in (-1, 4):
        assert L.pa_interface_csr_query(asm.ctx.h, fd, C.byref(out)) == 2
        assert L.pa_interface_csr_pattern(asm.ctx.h, fd, p, None) == 2
        assert L.pa_interface_csr_fill(asm.ctx.h, fd, p, None, None, p, None, p, None) == 2
    # NULL arrays: out, rowptr, lc, values, and lc_cut with cut cells
    assert L.pa_interface_csr_query(asm.ctx.h, 1, None) == 1
    assert L.pa_interface_csr_query(None, 1, C.byref(out)) == 1
    assert L.pa_interface_csr_pattern(asm.ctx.h, 1, None, None) == 1
    assert L.pa_interface_csr_fill(asm.ctx.h, 1, None, None, None, p, None, p, None) == 1
    assert L.pa_interface_csr_fill(asm.ctx.h, 1, p, None, None, p, None, None, None) == 1
    assert L.pa_interface_csr_fill(asm.ctx.h, 1, p, None, None, None, None, p, None) == 1
    # the same context still works; colind may be NULL
    assert L.pa_interface_csr_query(asm.ctx.h, 1, C.byref(out)) == 0
    rp = torch.empty(out.nrows + 1, dtype=torch.int64, device=dev)
    assert L.pa_interface_csr_pattern(asm.ctx.h, 1, rp.data_ptr(), None) == 0
    asm.synchronize()
    assert int(rp[-1]) == out.nnz


def test_interface_csr_solve_matches_a_direct_solve(asm):
    """pa_conjugated_gradient on the direct CSR against scipy's sparse direct solve of the same matrix"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    N, k = 20, 2
    ops, g = real_ops(asm, N, k)
    rp, ci = asm.interface_csr_pattern(k)
    va, RH = asm.interface_csr_fill(k, ops, g)
    n = RH.numel()
    x, reason, iters, relres = asm.conjugated_gradient(rp, ci, va, RH, tol=1e-13, max_iter=20 * n, precond=True)
    asm.synchronize()
    A = sp.csr_matrix((va.cpu().numpy(), ci.cpu().numpy(), rp.cpu().numpy()), shape=(n, n))
    ref = spla.spsolve(A.tocsc(), RH.cpu().numpy())
    assert reason == 0, (reason, iters, relres)
    assert np.abs(x.cpu().numpy() - ref).max() <= 1e-8 * np.abs(ref).max()
