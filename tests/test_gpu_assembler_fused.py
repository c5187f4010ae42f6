"""pa_assembler_csr_assemble: the local-operator kernel writes the CSR values and right-hand side of assembler<Mesh>'s own
system (hho.hpp:344-406, 451-455) from its on-chip image of lc.  The reference of every comparison is the two-step path it
stands next to: pa_local_ops_batch, pa_assembler_csr_pattern, pa_assembler_csr_fill."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T, FAN, FANCY, NAIVE = 0, 1, 2, 1          # PA_QUAD_TENSOR / PA_QUAD_FAN, PA_STAB_FANCY / PA_STAB_NAIVE

# (cell degree, face degree, quadrature, stabilization)
PAIRS = [
    (1, 1, T, FANCY), (2, 1, T, FANCY), (3, 2, T, FANCY), (4, 3, T, FANCY),
    (2, 1, FAN, NAIVE), (3, 2, FAN, NAIVE),
    (0, 0, T, FANCY), (1, 0, T, FANCY), (0, 1, T, FANCY),      # the small pairs and the obstacle pair
    (2, 2, T, FANCY),                                           # equal order
]
# N = 2: every cell a corner; N = 5: corner, edge and interior cells, a last wavefront that is not full at 2 and at 4 cells per
# wavefront; N = 33: an odd count over several blocks
SIZES = [2, 5, 33]


@pytest.fixture(scope="module")
def asm():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    from proton_amd.batch import BatchAssembler
    return BatchAssembler(0)


def nerr_cells(a, b):
    """worst per-cell normwise error of [n, r, c] batches (tests/test_gpu_parity.py)"""
    num = np.abs(a - b).reshape(a.shape[0], -1).max(axis=1)
    den = np.abs(b).reshape(b.shape[0], -1).max(axis=1)
    return (num / np.maximum(den, 1e-300)).max()


def inputs(asm, cd, fd, quad):
    import torch
    import proton_amd as pa
    rhs = asm.cell_rhs(cd, pa.capi.FN_SIN_SIN_RHS, quad)
    # boundary data of a function that vanishes nowhere on the boundary and is no polynomial: every coefficient of g counts
    xyw = asm.face_quadrature_points(fd)
    fv = torch.cos(3.0 * xyw[:, :, 0] + 1.0) + xyw[:, :, 1] * xyw[:, :, 1] + 0.5
    g = asm.dirichlet_data(fd, pa.capi.FN_SAMPLED, fvals=fv.contiguous())
    return rhs, g


def check_bit_identity(asm, cd, fd, quad, stab):
    """the fused entry with lc requested; that lc through pa_assembler_csr_fill: the same bits.  -> (fused outputs, rhs, g)"""
    import torch
    rhs, g = inputs(asm, cd, fd, quad)
    out = asm.assembler_csr_assemble(cd, fd, quad, stab, rhs=rhs, g=g, want=("lc", "info"))
    va, RHS = asm.assembler_csr_fill(cd, fd, out["lc"], rhs, g)
    asm.synchronize()
    assert int(out["info"].abs().max()) == 0
    assert torch.equal(out["values"], va)
    assert torch.equal(out["RHS"], RHS)
    return out, rhs, g


_worst_lc = {}


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("cd,fd,quad,stab", PAIRS)
def test_scatter_is_bit_identical_to_the_gather_and_lc_is_the_local_matrix(asm, N, cd, fd, quad, stab):
    """Checks 1 and 2 on the same call.  (1) values and RHS equal, bit for bit, pa_assembler_csr_fill of the lc the call
    returned.  (2) that lc is pa_local_ops_batch's: per-cell normwise error below 1e-11, the bound tests/test_gpu_condensed.py
    holds this image's condensed output to against the two-kernel path."""
    from proton_amd.batch import to_rowcol
    asm.generate_mesh(N, N)
    out, _, _ = check_bit_identity(asm, cd, fd, quad, stab)
    ref = asm.local_ops(cd, fd, quad, stab, want=("lc",))
    asm.synchronize()
    err = nerr_cells(to_rowcol(out["lc"]), to_rowcol(ref["lc"]))
    key = (cd, fd, quad, stab)
    _worst_lc[key] = max(_worst_lc.get(key, 0.0), float(err))
    print("fused lc vs pa_local_ops_batch, pair %s N=%d: worst per-cell normwise error %.3e (so far %.3e)" % (key, N, err, _worst_lc[key]))
    assert err < 1e-11


@pytest.mark.parametrize("cd,fd", [(2, 1), (4, 3)])
def test_lc_output_and_stale_buffers_change_nothing(asm, cd, fd):
    """values and RHS do not depend on whether lc is written, nor on what the buffers held (only the accumulated entries are
    zeroed, every other one is overwritten); without cell right-hand side and boundary data they equal the gather's."""
    import torch
    asm.generate_mesh(5, 5)
    with_lc, rhs, g = check_bit_identity(asm, cd, fd, T, FANCY)
    plain = asm.assembler_csr_assemble(cd, fd, T, FANCY, rhs=rhs, g=g)
    asm.synchronize()
    assert set(plain) == {"values", "RHS"}
    assert torch.equal(plain["values"], with_lc["values"]) and torch.equal(plain["RHS"], with_lc["RHS"])
    # a second call into the same buffers, not re-zeroed
    again = asm.assembler_csr_assemble(cd, fd, T, FANCY, rhs=rhs, g=g, values=plain["values"], RHS=plain["RHS"])
    asm.synchronize()
    assert again["values"].data_ptr() == plain["values"].data_ptr()
    assert torch.equal(again["values"], with_lc["values"]) and torch.equal(again["RHS"], with_lc["RHS"])
    # ... and into buffers full of something else
    junk_v = torch.full_like(with_lc["values"], 7.5)
    junk_r = torch.full_like(with_lc["RHS"], -3.25)
    third = asm.assembler_csr_assemble(cd, fd, T, FANCY, rhs=rhs, g=g, values=junk_v, RHS=junk_r)
    asm.synchronize()
    assert torch.equal(third["values"], with_lc["values"]) and torch.equal(third["RHS"], with_lc["RHS"])
    # d_rhs = NULL, d_g = NULL
    a = asm.assembler_csr_assemble(cd, fd, T, FANCY)
    b = asm.assembler_csr_assemble(cd, fd, T, FANCY)
    va, RHS = asm.assembler_csr_fill(cd, fd, with_lc["lc"])
    asm.synchronize()
    assert torch.equal(a["values"], b["values"]) and torch.equal(a["RHS"], b["RHS"])
    assert torch.equal(a["values"], va) and torch.equal(a["RHS"], RHS)


@pytest.mark.parametrize("cd,fd", [(2, 1), (3, 2)])
def test_pieces_under_the_record_cap(asm, cd, fd):
    """96 x 96 = 9216 cells run in three pieces at the clamped minimum of 4096 cells per piece: the same bits as in one piece"""
    import torch
    asm.generate_mesh(96, 96)
    rhs, g = inputs(asm, cd, fd, T)
    whole = asm.assembler_csr_assemble(cd, fd, T, FANCY, rhs=rhs, g=g, want=("lc",))
    asm.synchronize()
    asm.ctx.set_record_cap(1 << 20)          # clamps to the minimum piece (4096 cells)
    try:
        pieces = asm.assembler_csr_assemble(cd, fd, T, FANCY, rhs=rhs, g=g, want=("lc",))
        asm.synchronize()
    finally:
        asm.ctx.set_record_cap(4 << 30)
    for k in ("values", "RHS", "lc"):
        assert torch.equal(whole[k], pieces[k]), k
    va, RHS = asm.assembler_csr_fill(cd, fd, whole["lc"], rhs, g)
    asm.synchronize()
    assert torch.equal(whole["values"], va) and torch.equal(whole["RHS"], RHS)


@pytest.mark.parametrize("open_left", [False, True])
def test_uploaded_general_quadrilateral_mesh(asm, oracle, open_left):
    """a perturbed 6 x 6 mesh of general quadrilaterals with explicit face tables (pa_mesh_upload + pa_mesh_set_faces); with
    the left boundary's faces not Dirichlet there are face rows with a single cell"""
    N = 6
    mp, points, ptids = oracle.make_mesh(N, N)
    rng = np.random.default_rng(5)
    ij = np.arange(points.shape[0])
    i, j = ij % (N + 1), ij // (N + 1)
    interior = (i > 0) & (i < N) & (j > 0) & (j < N)
    points[interior] += rng.uniform(-0.1 / N, 0.1 / N, size=points.shape)[interior]
    ref = oracle.Assembler(mp, points, ptids, oracle.degrees(2, 1))
    is_dir = ref.is_dir.copy()
    if open_left:
        left = (points[ref.faces[:, 0].astype(np.int64), 0] == 0.0) & (points[ref.faces[:, 1].astype(np.int64), 0] == 0.0)
        assert left.sum() == N and is_dir[left].all()
        is_dir[left] = 0
    asm.set_mesh(points, ptids)
    asm.set_faces(ref.cell_faces, ref.faces, is_dir)
    for cd, fd in [(2, 1), (3, 2)]:
        info = asm.assembler_info(cd, fd)
        assert info.num_other_faces == int((is_dir == 0).sum())
        check_bit_identity(asm, cd, fd, T, FANCY)


def test_refusals_touch_no_buffer(asm):
    """a slab is refused with pa_assembler_csr_fill's code, a pair beyond the tables with PA_ERR_QUADRATURE, a stabilization
    kind that does not exist with PA_ERR_INVALID_ARG -- before anything is written"""
    import torch
    import proton_amd as pa
    L = pa.capi.lib()
    f64 = dict(dtype=torch.float64, device=asm.device)
    values, RHS, lc = torch.full((4096,), 1.5, **f64), torch.full((4096,), 2.5, **f64), torch.full((4096,), 3.5, **f64)
    info = torch.full((4096,), 9, dtype=torch.int32, device=asm.device)

    def call(di, quad, stab):
        return L.pa_assembler_csr_assemble(asm.ctx.h, di, quad, stab, None, None, values.data_ptr(), RHS.data_ptr(), lc.data_ptr(),
                                           info.data_ptr())

    def untouched():
        asm.synchronize()
        return bool((values == 1.5).all()) and bool((RHS == 2.5).all()) and bool((lc == 3.5).all()) and bool((info == 9).all())

    di, _ = pa.capi.degree_info(2, 1)
    asm.generate_mesh(8, 8, rows=(2, 5))
    want = L.pa_assembler_csr_fill(asm.ctx.h, di, lc.data_ptr(), None, None, values.data_ptr(), RHS.data_ptr())
    assert want != 0
    assert call(di, T, FANCY) == want and untouched()
    asm.generate_mesh(8, 8)
    big, _ = pa.capi.degree_info(5, 4)
    assert call(big, T, FANCY) == 3 and untouched()             # PA_ERR_QUADRATURE
    assert call(di, T, 7) == 1 and untouched()                  # PA_ERR_INVALID_ARG
    assert call(di, T, -1) == 1 and untouched()


@pytest.mark.parametrize("cd,fd", [(2, 1), (3, 2)])
def test_end_to_end_solve(asm, cd, fd):
    """pa_conjugated_gradient on the fused system, then pa_take_local_data_batch: the local solutions of the two-step path's
    system solved the same way, to the tolerance both solves were given (the 1e-9 of test_config1_plumbing_poisson_solve)"""
    TOL = 1e-9
    N = 16
    asm.generate_mesh(N, N)
    rhs, g = inputs(asm, cd, fd, T)
    rowptr, colind = asm.assembler_csr_pattern(cd, fd)
    lc = asm.local_ops(cd, fd, T, FANCY, want=("lc",))["lc"]
    va_p, RHS_p = asm.assembler_csr_fill(cd, fd, lc, rhs, g)
    fused = asm.assembler_csr_assemble(cd, fd, T, FANCY, rhs=rhs, g=g)
    n = RHS_p.numel()
    loc = []
    for va, b in ((va_p, RHS_p), (fused["values"], fused["RHS"])):
        x, reason, iters, relres = asm.conjugated_gradient(rowptr, colind, va, b, tol=TOL, max_iter=3 * n, precond=True)
        assert reason == 0 and relres < TOL
        loc.append(asm.take_local_data(cd, fd, x, g))
    asm.synchronize()
    diff = float((loc[0] - loc[1]).abs().max())
    print("end to end (%d,%d): max |local solution difference| %.3e" % (cd, fd, diff))
    assert diff < TOL
