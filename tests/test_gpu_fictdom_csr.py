"""pa_fictdom_csr_assemble: the global system of the fictitious-domain problem (cuthho_square.cpp:881-905) in one pass on the cut
mesh -- the uncut cells from the local-operator kernel's on-chip image, the cut cells' operators through the same scatter.  The
reference of every comparison is the two-step path it stands next to: the uncut lc of pa_assembler_csr_assemble(FAN, NAIVE),
pa_cut_local_ops_batch + pa_cut_uncut_rhs_batch + pa_cut_merge, then pa_assembler_csr_fill of the merged arrays."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FAN, NAIVE = 1, 1          # PA_QUAD_FAN, PA_STAB_NAIVE
NEG, POS = 0, 1            # PA_LOC_NEGATIVE, PA_LOC_POSITIVE

# the smallest cut meshes the suite proves the preprocessing on (tests/test_gpu_cuthho.py): (N, k, cut_preprocess arguments).
# The line's cut cells touch the left and right Dirichlet boundary: cut cells with Dirichlet columns.
CIRCLES = [(10, 0, dict(refsteps=4)), (10, 1, dict(refsteps=4)), (20, 2, dict(refsteps=4))]
LINES = [(9, 0, dict(refsteps=3, line_y=0.5)), (10, 1, dict(refsteps=3, line_y=0.53)), (12, 2, dict(refsteps=3, line_y=0.47))]


def case_id(c):
    return "%s-%d-k%d" % ("line%g" % c[2]["line_y"] if "line_y" in c[2] else "circle", c[0], c[1])


@pytest.fixture(scope="module")
def asm():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    from proton_amd.batch import BatchAssembler
    return BatchAssembler(0)


def boundary_data(asm, k):
    """boundary data of a function that vanishes nowhere on the boundary and is no polynomial (inputs() of
    tests/test_gpu_assembler_fused.py): every coefficient of g counts"""
    import torch
    import proton_amd as pa
    xyw = asm.face_quadrature_points(k)
    fv = torch.cos(3.0 * xyw[:, :, 0] + 1.0) + xyw[:, :, 1] * xyw[:, :, 1] + 0.5
    return asm.dirichlet_data(k, pa.capi.FN_SAMPLED, fvals=fv.contiguous())


def uncut_rhs(asm, k, where=NEG):
    import torch
    import proton_amd as pa
    cd = k + 1
    rhs = torch.empty((asm.ncells, (cd + 1) * (cd + 2) // 2), dtype=torch.float64, device=asm.device)
    asm.ctx.cut_uncut_rhs(cd, where, pa.capi.FN_SIN_SIN_RHS, rhs.data_ptr())
    return rhs


def two_step(asm, k, where, rhs, g, cut_lc, cut_rhs):
    """-> (values, RHS, merged lc, merged rhs) of the path with lc in HBM.  A missing rhs / cut_rhs counts as zeros, which is what
    the new entry documents for its NULL pointers."""
    import torch
    cd = k + 1
    lc = asm.assembler_csr_assemble(cd, k, FAN, NAIVE, want=("lc",))["lc"]            # the uncut formulas on every cell
    r = torch.zeros((asm.ncells, (cd + 1) * (cd + 2) // 2), dtype=torch.float64, device=asm.device) if rhs is None else rhs.clone()
    if asm.ncut and cut_rhs is None:
        cut_rhs = torch.zeros((asm.ncut, r.shape[1]), dtype=torch.float64, device=asm.device)
    asm.ctx.cut_merge(k, where, None if cut_lc is None else cut_lc.data_ptr(), None if cut_rhs is None else cut_rhs.data_ptr(),
                      lc.data_ptr(), r.data_ptr())
    va, RHS = asm.assembler_csr_fill(cd, k, lc, r, g)
    asm.synchronize()
    return va, RHS, lc, r


def synthetic_cut(asm, k, seed):
    """random NON-symmetric cut matrices and right-hand sides: a transposed or misplaced block cannot cancel"""
    import torch
    cbs = (k + 3) * (k + 2) // 2
    ms = cbs + 4 * (k + 1)
    gen = torch.Generator(device="cpu").manual_seed(seed)
    lc = torch.rand((asm.ncut, ms, ms), generator=gen, dtype=torch.float64) - 0.5
    r = torch.rand((asm.ncut, cbs), generator=gen, dtype=torch.float64) - 0.5
    return lc.to(asm.device), r.to(asm.device)


def cut_rows(asm):
    import torch
    return torch.from_numpy(np.nonzero(asm.cell_loc == 2)[0]).to(asm.device)


# ---- 1. real operators, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,k,kw", CIRCLES + LINES, ids=[case_id(c) for c in CIRCLES + LINES])
def test_real_operators_bit_for_bit(asm, N, k, kw):
    import torch
    ncut = asm.cut_preprocess(N, **kw)
    assert ncut > 0
    g = boundary_data(asm, k)
    rhs = uncut_rhs(asm, k)
    cut = asm.cut_local_ops(k, NEG, want=("lc", "rhs"))
    va, RHS, lc, _ = two_step(asm, k, NEG, rhs, g, cut["lc"], cut["rhs"])
    out = asm.fictdom_csr_scatter(k, NEG, rhs, g, cut["lc"], cut["rhs"], want=("lc",))
    asm.synchronize()
    assert torch.equal(out["values"], va)
    assert torch.equal(out["RHS"], RHS)
    assert torch.equal(out["lc"], lc)
    assert torch.equal(out["lc"][cut_rows(asm)], cut["lc"])                    # the cut rows are a bit copy of d_cut_lc
    # the convenience method runs the same three calls
    conv = asm.fictdom_csr_assemble(k, NEG, g=g)
    asm.synchronize()
    assert torch.equal(conv["values"], va) and torch.equal(conv["RHS"], RHS)
    assert torch.equal(conv["rhs"], rhs) and torch.equal(conv["cut_lc"], cut["lc"]) and torch.equal(conv["cut_rhs"], cut["rhs"])


# ---- 2. synthetic cut operators ---------------------------------------------------------------------------------------------
SYNTH = [(12, 0, dict(refsteps=3, line_y=0.43)), (12, 1, dict(refsteps=3, line_y=0.43)), (12, 2, dict(refsteps=3, line_y=0.43)),
         (10, 1, dict(refsteps=4))]


@pytest.mark.parametrize("where", [NEG, POS])
@pytest.mark.parametrize("N,k,kw", SYNTH, ids=[case_id(c) for c in SYNTH])
def test_synthetic_cut_operators(asm, N, k, kw, where):
    import torch
    assert asm.cut_preprocess(N, **kw) > 0
    g = boundary_data(asm, k)
    # a right-hand side that is nonzero on EVERY cell: the zeroing outside `where` is the entry's, not the caller's
    gen = torch.Generator(device="cpu").manual_seed(100 + k)
    rhs = (torch.rand((asm.ncells, (k + 3) * (k + 2) // 2), generator=gen, dtype=torch.float64) + 0.5).to(asm.device)
    cut_lc, cut_rhs = synthetic_cut(asm, k, seed=11 + k)
    va, RHS, lc, r = two_step(asm, k, where, rhs, g, cut_lc, cut_rhs)
    out = asm.fictdom_csr_scatter(k, where, rhs, g, cut_lc, cut_rhs, want=("lc",))
    asm.synchronize()
    assert torch.equal(out["values"], va)
    assert torch.equal(out["RHS"], RHS)
    assert torch.equal(out["lc"], lc)
    # the reference did zero something and did keep something
    outside = torch.from_numpy((asm.cell_loc != 2) & (asm.cell_loc != where)).to(asm.device)
    assert bool(outside.any()) and bool((r[outside] == 0).all()) and bool((r[~outside] != 0).all())


# ---- 3. buffers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,k,kw", [(10, 1, dict(refsteps=4)), (12, 2, dict(refsteps=3, line_y=0.43))], ids=["circle-10-k1", "line0.43-12-k2"])
def test_lc_output_and_stale_buffers_change_nothing(asm, N, k, kw):
    import torch
    asm.cut_preprocess(N, **kw)
    g = boundary_data(asm, k)
    rhs = uncut_rhs(asm, k)
    cut_lc, cut_rhs = synthetic_cut(asm, k, seed=3)
    va, RHS, _, _ = two_step(asm, k, NEG, rhs, g, cut_lc, cut_rhs)
    plain = asm.fictdom_csr_scatter(k, NEG, rhs, g, cut_lc, cut_rhs)
    asm.synchronize()
    assert set(plain) == {"values", "RHS"}
    assert torch.equal(plain["values"], va) and torch.equal(plain["RHS"], RHS)
    # a second call into the same buffers, not re-zeroed
    again = asm.fictdom_csr_scatter(k, NEG, rhs, g, cut_lc, cut_rhs, values=plain["values"], RHS=plain["RHS"])
    asm.synchronize()
    assert again["values"].data_ptr() == plain["values"].data_ptr()
    assert torch.equal(again["values"], va) and torch.equal(again["RHS"], RHS)
    # buffers full of something else, with lc
    third = asm.fictdom_csr_scatter(k, NEG, rhs, g, cut_lc, cut_rhs, values=torch.full_like(va, 7.5), RHS=torch.full_like(RHS, -3.25),
                                    want=("lc", "info"))
    asm.synchronize()
    assert torch.equal(third["values"], va) and torch.equal(third["RHS"], RHS)
    # d_RHS = NULL: the same values
    v4 = torch.full_like(va, -1.0)
    asm.ctx.fictdom_csr_assemble(k, NEG, rhs.data_ptr(), g.data_ptr(), cut_lc.data_ptr(), cut_rhs.data_ptr(), v4.data_ptr(), None, None, None)
    asm.synchronize()
    assert torch.equal(v4, va)
    # d_rhs = d_g = d_cut_rhs = NULL: the fill with zeros
    va0, RHS0, _, _ = two_step(asm, k, NEG, None, None, cut_lc, None)
    a = asm.fictdom_csr_scatter(k, NEG, None, None, cut_lc, None)
    b = asm.fictdom_csr_scatter(k, NEG, None, None, cut_lc, None, values=torch.full_like(va, 2.0), RHS=torch.full_like(RHS, 2.0))
    asm.synchronize()
    assert torch.equal(a["values"], va0) and torch.equal(a["RHS"], RHS0)
    assert torch.equal(b["values"], va0) and torch.equal(b["RHS"], RHS0)


# ---- 4. no cut cell -----------------------------------------------------------------------------------------------------------
def test_without_cut_cells_it_is_the_fused_assembly(asm):
    import torch
    assert asm.cut_preprocess(9, radius=2.0, refsteps=4) == 0
    k = 1
    g = boundary_data(asm, k)
    rhs = uncut_rhs(asm, k)          # every cell lies inside: nothing is zeroed
    assert bool((asm.cell_loc == NEG).all())
    ref = asm.assembler_csr_assemble(k + 1, k, FAN, NAIVE, rhs=rhs, g=g, want=("lc",))
    out = asm.fictdom_csr_scatter(k, NEG, rhs, g, None, None, want=("lc",))
    asm.synchronize()
    for key in ("values", "RHS", "lc"):
        assert torch.equal(out[key], ref[key]), key


# ---- 5. the mask does not leak ------------------------------------------------------------------------------------------------
def test_the_mask_does_not_leak_into_the_plain_fused_entry(asm):
    import torch
    k = 1
    asm.cut_preprocess(10, refsteps=4)
    g = boundary_data(asm, k)
    rhs = uncut_rhs(asm, k)
    before = asm.assembler_csr_assemble(k + 1, k, FAN, NAIVE, rhs=rhs, g=g, want=("lc",))
    new = asm.fictdom_csr_assemble(k, NEG, g=g, want=("lc",))
    after = asm.assembler_csr_assemble(k + 1, k, FAN, NAIVE, rhs=rhs, g=g, want=("lc",))
    asm.synchronize()
    for key in ("values", "RHS", "lc"):
        assert torch.equal(before[key], after[key]), key
    # it keeps treating every cell with the uncut formulas: its cut rows are not the cut operators
    rows = cut_rows(asm)
    assert not torch.equal(after["lc"][rows], new["lc"][rows])
    uncut = torch.from_numpy(asm.cell_loc != 2).to(asm.device)
    assert torch.equal(after["lc"][uncut], new["lc"][uncut])
    assert not torch.equal(after["values"], new["values"])


# ---- 6. pieces ------------------------------------------------------------------------------------------------------------------
def test_pieces_under_the_record_cap(asm):
    """96 x 96 = 9216 cells run in three pieces at the clamped minimum of 4096 cells per piece: the same bits as in one piece"""
    import torch
    k = 1
    asm.cut_preprocess(96, refsteps=4)
    g = boundary_data(asm, k)
    whole = asm.fictdom_csr_assemble(k, NEG, g=g, want=("lc",))
    asm.synchronize()
    asm.ctx.set_record_cap(1 << 20)
    try:
        pieces = asm.fictdom_csr_scatter(k, NEG, whole["rhs"], g, whole["cut_lc"], whole["cut_rhs"], want=("lc",))
        asm.synchronize()
    finally:
        asm.ctx.set_record_cap(4 << 30)
    for key in ("values", "RHS", "lc"):
        assert torch.equal(whole[key], pieces[key]), key
    va, RHS, _, _ = two_step(asm, k, NEG, whole["rhs"], g, whole["cut_lc"], whole["cut_rhs"])
    assert torch.equal(whole["values"], va) and torch.equal(whole["RHS"], RHS)


# ---- 7. side stream ----------------------------------------------------------------------------------------------------------------
def test_cut_kernel_on_the_side_stream(asm):
    """the cut kernel under pa_context_set_cut_overlap(1), joined by the new entry itself"""
    import torch
    k = 1
    asm.cut_preprocess(40, refsteps=4)
    g = boundary_data(asm, k)
    one = asm.fictdom_csr_assemble(k, NEG, g=g, want=("lc",))
    asm.synchronize()
    for _ in range(2):
        two = asm.fictdom_csr_assemble(k, NEG, g=g, want=("lc",), overlap=True)
        asm.synchronize()
        for key in ("values", "RHS", "lc", "cut_lc", "cut_rhs"):
            assert torch.equal(one[key], two[key]), key


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_touch_no_buffer(asm):
    import torch
    import proton_amd as pa
    from proton_amd.batch import BatchAssembler
    L = pa.capi.lib()
    f64 = dict(dtype=torch.float64, device=asm.device)
    n = 1 << 16
    values, RHS, lc = torch.full((n,), 1.5, **f64), torch.full((n,), 2.5, **f64), torch.full((n,), 3.5, **f64)
    info = torch.full((n,), 9, dtype=torch.int32, device=asm.device)
    cut_lc = torch.zeros(n, **f64)

    def call(h, k=1, where=NEG, v=values, c=cut_lc):
        return L.pa_fictdom_csr_assemble(h, k, where, None, None, None if c is None else c.data_ptr(), None,
                                         None if v is None else v.data_ptr(), RHS.data_ptr(), lc.data_ptr(), info.data_ptr())

    def untouched():
        asm.synchronize()
        return bool((values == 1.5).all()) and bool((RHS == 2.5).all()) and bool((lc == 3.5).all()) and bool((info == 9).all())

    assert asm.cut_preprocess(8, refsteps=4) > 0
    assert call(None) == 1 and untouched()                       # NULL ctx: PA_ERR_INVALID_ARG
    assert call(asm.ctx.h, v=None) == 1 and untouched()          # NULL d_values
    assert call(asm.ctx.h, c=None) == 1 and untouched()          # cut cells without d_cut_lc
    assert call(asm.ctx.h, where=2) == 1 and untouched()         # `where` = PA_LOC_ON_INTERFACE
    assert call(asm.ctx.h, where=-1) == 1 and untouched()
    assert call(asm.ctx.h, k=3) == 3 and untouched()             # PA_ERR_QUADRATURE, as the cut entries
    # a slab: the code pa_assembler_csr_fill gives
    asm.cut_preprocess(8, refsteps=4, rows=(2, 5))
    di, _ = pa.capi.degree_info(2, 1)
    want = L.pa_assembler_csr_fill(asm.ctx.h, di, lc.data_ptr(), None, None, values.data_ptr(), RHS.data_ptr())
    assert want != 0
    assert call(asm.ctx.h) == want and untouched()
    # no cut preprocessing on the context: PA_ERR_NO_MESH
    plain = BatchAssembler(0)
    plain.generate_mesh(8, 8)
    assert call(plain.ctx.h) == 5 and untouched()
    asm.cut_preprocess(8, refsteps=4)                            # leave a whole-mesh cut context behind


# ---- 9. end to end ------------------------------------------------------------------------------------------------------------------------
# energy errors of apps/cuthho/cuthho.xlsx and the tolerance of test_fictitious_domain_end_to_end_matches_xlsx
XLSX = {(0, 10): 0.188501, (1, 20): 3.08508e-3, (2, 20): 9.30124e-5}
# relative residual asked of pa_conjugated_gradient: what tests/cpp/cuthho_driver.cpp -f asks of its solver on the same systems
# (the xlsx values come from a direct solve, so the iteration has to be run down to the floor of double precision)
CG_TOL = 1e-13


def energy_error(oracle, msh, k, sol):
    """the loop of tests/cuthho_driver.py:45-65 (cuthho_square.cpp:1030-1049) with the oracle's quadrature"""
    di = oracle.degrees(k + 1, k)
    L = oracle.lib()
    cbs, rd = di.cbs, di.rec_deg
    H1 = 0.0
    gx, gy, bar = np.zeros(32), np.zeros(32), np.zeros(2)
    for c in range(msh.nc):
        if msh.cell_loc[c] == oracle.CUT_POS:
            continue
        pts = np.ascontiguousarray(msh.points[msh.ptids[c].astype(np.int64)].reshape(8))
        L.hho_cell_barycenter(oracle._dp(pts), oracle._dp(bar))
        h = L.hho_cell_diameter(oracle._dp(pts))
        dofs = sol[c * cbs:(c + 1) * cbs]
        qx, qy, qw = msh.cell_quadrature(c, 2 * di.cell_deg, oracle.CUT_NEG)
        for q in range(len(qw)):
            L.hho_cell_basis_grad(oracle._dp(bar), h, rd, qx[q], qy[q], oracle._dp(gx), oracle._dp(gy))
            g0 = float(np.dot(dofs[1:], gx[1:cbs]))
            g1 = float(np.dot(dofs[1:], gy[1:cbs]))
            s0 = math.pi * math.cos(math.pi * qx[q]) * math.sin(math.pi * qy[q])
            s1 = math.pi * math.sin(math.pi * qx[q]) * math.cos(math.pi * qy[q])
            H1 += qw[q] * ((s0 - g0) ** 2 + (s1 - g1) ** 2)
    return math.sqrt(H1)


@pytest.mark.parametrize("N,k", [(10, 0), (20, 1), (20, 2)])
def test_end_to_end_matches_xlsx(asm, oracle, N, k):
    """preprocess, fictdom_csr_assemble and pa_conjugated_gradient where the system was assembled; only the solution goes to the
    host, for the energy error"""
    import proton_amd as pa
    cd = k + 1
    asm.cut_preprocess(N, refsteps=4)
    g = asm.dirichlet_data(k, pa.capi.FN_SIN_SIN_SOL)                      # bcs_fun = sol_fun
    rowptr, colind = asm.assembler_csr_pattern(cd, k)
    out = asm.fictdom_csr_assemble(k, NEG, g=g)
    n = out["RHS"].numel()
    x, reason, iters, relres = asm.conjugated_gradient(rowptr, colind, out["values"], out["RHS"], tol=CG_TOL, max_iter=4 * n, precond=True)
    assert reason == 0 and relres < CG_TOL
    sol = x.cpu().numpy()
    msh = oracle.CutMesh(N, refsteps=4)
    assert n == oracle.Assembler(oracle.MeshParams(N, N, 0.0, 1.0, 0.0, 1.0), msh.points, msh.ptids, oracle.degrees(cd, k), bf_id=2).system_size
    err = energy_error(oracle, msh, k, sol)
    print("fictdom N=%d k=%d: system %d, cg iterations %d, energy error %.10e (xlsx %.6e)" % (N, k, n, iters, err, XLSX[(k, N)]))
    assert abs(err - XLSX[(k, N)]) / XLSX[(k, N)] < 6e-6
    # the two-step system, solved the same way: the same matrix and right-hand side, so the same iterates
    va, RHS, _, _ = two_step(asm, k, NEG, out["rhs"], g, out["cut_lc"], out["cut_rhs"])
    x2, reason2, _, relres2 = asm.conjugated_gradient(rowptr, colind, va, RHS, tol=CG_TOL, max_iter=4 * n, precond=True)
    assert reason2 == 0 and relres2 < CG_TOL
    diff = float((x - x2).abs().max()) / float(x.abs().max())
    print("fictdom N=%d k=%d: max relative difference of the two solutions %.3e" % (N, k, diff))
    assert diff <= CG_TOL
