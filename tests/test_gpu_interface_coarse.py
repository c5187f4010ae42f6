"""The coarse table of the interface problem's face-only system (pa_interface_condensed_coarse, coarse_precond.hip) and the solve
through it on the device: both tables bit for bit against the twin of tests/interface_coarse_twin.py, against pa_condensed_coarse
where nothing is cut, through pa_coarse_precond_factor on the real system, interface_condensed_solve(patches="cell", coarse=H) end to
end against a direct solve, the iteration counts against the cell patches alone, the xlsx Interface table, the side stream, and the
refusals.  One run: profiles/interface_coarse_parity.txt
(INTERFACE_COARSE_PROFILE=that file python -m pytest tests/test_gpu_interface_coarse.py -m gpu -s)."""
import ctypes as C
import os

import numpy as np
import pytest

import interface_coarse_twin as IC
from interface_helpers import real_ops

pytestmark = pytest.mark.gpu

REPORT = []
PARTS = ("one", "side")


def say(line):
    print(line)
    REPORT.append(line)


@pytest.fixture(scope="module")
def asm():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    from proton_amd.batch import BatchAssembler
    return BatchAssembler(0)


def device_table(a, k, H, parts):
    ptr, cols, vals, ncoarse = a.interface_condensed_coarse(k, H, parts)
    a.synchronize()
    ptr, cols, vals = ptr.cpu().numpy(), cols.cpu().numpy(), vals.cpu().numpy()
    assert ptr.dtype == np.int64 and cols.dtype == np.int32 and vals.dtype == np.float64
    return ptr, cols, vals, ncoarse


def same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


# ---- 1. the tables against the twin -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,Hs,kw", [(16, (4, 3, 1), {}), (20, (4, 3, 1), {}), (12, (4, 3, 1), dict(line_y=0.47))],
                         ids=["circle16", "circle20", "line12"])
def test_tables_equal_the_twin(asm, oracle, N, Hs, kw):
    """k = 0 and 2, H = 4, 3 (does not divide 20) and 1, both parts: ptr, cols and vals bit for bit, the query's sizes the table's, a
    second call the same bits.  The line mesh has a cut face on either Dirichlet boundary: two unowned blocks with equal pointers"""
    from proton_amd import capi
    asm.cut_preprocess(N, **kw)
    assert asm.ncut > 0
    msh = oracle.CutMesh(N, refsteps=4, **kw)
    faces, _ = oracle.mesh_faces(oracle.MeshParams(N, N, 0.0, 1.0, 0.0, 1.0))
    holes = np.count_nonzero((msh.bnd != 0) & (msh.face_loc == 2))
    assert holes == (2 if kw else 0)
    for k in (0, 2):
        n = asm.ctx.interface_condensed_query(k).system_size
        for H in Hs:
            for parts in PARTS:
                want = IC.mesh_table(msh, faces, k, H, parts, device_numbering=True)
                got = device_table(asm, k, H, parts)
                assert got[0].size == n + 1 == want.ptr.size
                assert same_bits(got, want), (N, k, H, parts)
                assert asm.ctx.interface_condensed_coarse_query(k, H, {"one": capi.COARSE_ONE, "side": capi.COARSE_BY_SIDE}[parts]) == \
                    (want.ncoarse, want.cols.size)
                assert same_bits(device_table(asm, k, H, parts), got)
                say("table %-8s N %2d k %d H %d %-4s: %5d rows, %4d columns, %5d entries: equal to the twin"
                    % ("line" if kw else "circle", N, k, H, parts, n, want.ncoarse, want.cols.size))


# ---- 2. no cut cells --------------------------------------------------------------------------------------------------------------
def test_without_cut_cells_the_table_is_the_plain_one(asm):
    """the circle outside the square: both parts give pa_condensed_coarse(PA_COARSE_ONE)'s table of (k + 1, k), bit for bit"""
    import torch
    import proton_amd as pa
    N = 9
    asm.level_set = pa.capi.LevelSet(0, 2.0, 0.5, 0.5, 0.0)
    asm.ctx.cut_preprocess(N, N, asm.level_set, 4)
    asm.ncut, asm.cell_loc, asm.cut_index = asm.ctx.cut_query()
    assert asm.ncut == 0
    for k in (0, 2):
        for H in (3, 1):
            plain = asm.condensed_coarse(k + 1, k, H, "one")
            for parts in PARTS:
                got = asm.interface_condensed_coarse(k, H, parts)
                asm.synchronize()
                assert got[0].numel() > 1 and got[3] == plain[3] and all(torch.equal(x, y) for x, y in zip(got[:3], plain[:3])), (k, H, parts)


# ---- 3. through the coarse level on the real system ---------------------------------------------------------------------------------
def test_finest_table_by_side_fits_the_slots_on_the_real_system(asm):
    """(20, 2), H = 1 by side: pa_coarse_precond_factor takes the table (no row of A P beyond its 16 slots: that refusal would
    raise) and the coarse matrix is positive definite (pivot 0)"""
    N, k = 20, 2
    ops, g = real_ops(asm, N, k)
    rec = asm.interface_condensed_ops(k, ops)
    rp, ci = asm.interface_condensed_csr_pattern(k)
    va, _ = asm.interface_condensed_csr_fill(k, rec, g)
    tb = asm.interface_condensed_coarse(k, 1, "side")
    pre = asm.coarse_precond_factor(rp, ci, va, tb)
    asm.synchronize()
    assert pre["pivot"] == 0
    say("precond (%d, %d) H 1 side: %d columns, %d entries: factored, pivot 0, no row of A P beyond 16 columns" % (N, k, tb[3], tb[1].numel()))


# ---- 4. the solve end to end ------------------------------------------------------------------------------------------------------
def full_reference(asm, k, ops, g):
    """scipy's spsolve of the full system, and the same after two steps of iterative refinement (residuals in long double, the
    corrections through the LU factors).  spsolve alone is not good for a gate of 1e-8 at N = 64: measured on one MI355X run, it is
    5.930e-09 of max|ref| off its own refinement at (32, 2) and 1.652e-08 at (64, 2) -- and so is every device solve, the parent's
    Jacobi and cell-patch solves included, while all of them lie within 1.6e-11 of the refined vector.  The gate is taken against the
    refined vector; the distance to the raw one is printed beside it."""
    import scipy.sparse.linalg as spla

    import test_gpu_interface_condensed as T
    K, b = T.full_csr(asm, k, ops, g)
    K = K.tocsr()
    K.sort_indices()
    raw = spla.spsolve(K.tocsc(), b)
    lu = spla.splu(K.tocsc())
    data, starts, x = K.data.astype(np.longdouble), K.indptr[:-1], raw.copy()
    for _ in range(2):
        r = b.astype(np.longdouble) - np.add.reduceat(data * x.astype(np.longdouble)[K.indices], starts)
        x = x + lu.solve(np.asarray(r, dtype=np.float64))
    return raw, x


@pytest.mark.parametrize("N", [32, 64])
def test_interface_condensed_solve_with_the_coarse_level(asm, N):
    """interface_condensed_solve(k = 2, patches = "cell", coarse = 4) at 1e-13 with both tables: exit reason 0, the recovered vector
    within 1e-8 max|ref| of spsolve of the full system, refined (full_reference says why); coarse = None is the call without the
    keyword, bit for bit and iteration for iteration; at 64, 1.5 iterations(coarse) <= iterations(cell patches) for both tables (the CPU twin gives 3 x; the margin
    covers the device's tree-reduced dot products)"""
    import torch
    k = 2
    ops, g = real_ops(asm, N, k)
    raw, ref = full_reference(asm, k, ops, g)
    plain, it_cell, reason = asm.interface_condensed_solve(k, ops, g, tol=1e-13, patches="cell")
    none, it_none, reason_none = asm.interface_condensed_solve(k, ops, g, tol=1e-13, patches="cell", coarse=None)
    asm.synchronize()
    assert reason == 0 and reason_none == 0 and it_none == it_cell and torch.equal(plain, none)
    iters = {}
    for parts in PARTS:
        full, iters[parts], reason = asm.interface_condensed_solve(k, ops, g, tol=1e-13, patches="cell", coarse=4, coarse_parts=parts)
        asm.synchronize()
        err = np.abs(full.cpu().numpy() - ref).max() / np.abs(ref).max()
        say("interface (%d, %d) cell patches %4d iterations; + coarse H 4 %-4s: %4d iterations, against spsolve refined %.3e of max|ref| "
            "(raw spsolve %.3e; raw against refined %.3e)" % (N, k, it_cell, parts, iters[parts], err,
                                                             np.abs(full.cpu().numpy() - raw).max() / np.abs(ref).max(),
                                                             np.abs(raw - ref).max() / np.abs(ref).max()))
        assert reason == 0
        assert err <= 1e-8
    if N == 64:
        for parts in PARTS:
            assert 1.5 * iters[parts] <= it_cell, (parts, iters, it_cell)


def test_by_side_is_no_worse_with_a_jump_in_kappa(asm):
    """kappa = (1, 1e4) at (64, 2), H = 4, 1e-13: iterations(side) <= iterations(one) (the CPU twin: 243 against 296).  The divergence
    test is set far out, as the timing tools have it: with this jump the residual's 2-norm passes 100 times its start on the way
    (the default threshold ends the solve with exit reason 1), and the twin's count has no such test"""
    N, k, kappa = 64, 2, (1.0, 1e4)
    import proton_amd as pa
    asm.cut_preprocess(N, refsteps=4)
    ops = asm.interface_local_ops(k, kappa=kappa)
    g = asm.dirichlet_data(k, pa.capi.FN_SIN_SIN_SOL)
    iters = {}
    for parts in PARTS:
        _, iters[parts], reason = asm.interface_condensed_solve(k, ops, g, tol=1e-13, div=1e10, patches="cell", coarse=4, coarse_parts=parts)
        asm.synchronize()
        assert reason == 0
    _, it_cell, reason = asm.interface_condensed_solve(k, ops, g, tol=1e-13, div=1e10, patches="cell")
    asm.synchronize()
    assert reason == 0
    say("interface (%d, %d) kappa %s: cell patches %d iterations, + coarse H 4 one %d, side %d" % (N, k, kappa, it_cell, iters["one"], iters["side"]))
    assert iters["side"] <= iters["one"]


def test_coarse_needs_patches(asm):
    ops, g = real_ops(asm, 10, 1)
    with pytest.raises(ValueError):
        asm.interface_condensed_solve(1, ops, g, coarse=4)


# ---- 5. the xlsx Interface table --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,N,ref", [(1, 20, 5.22389e-3), (2, 20, 1.38029e-4)])
def test_coarse_solves_reproduce_xlsx(asm, oracle, k, N, ref):
    """the energy-norm error of the vector the coarse solves recover at the driver's threshold 1e-9 (:1737-1743), within 6e-6"""
    from test_gpu_interface_patch import energy_error
    ops, g = real_ops(asm, N, k)
    msh = oracle.CutMesh(N, refsteps=4)
    for parts in PARTS:
        full, iters, reason = asm.interface_condensed_solve(k, ops, g, tol=1e-9, patches="cell", coarse=4, coarse_parts=parts)
        asm.synchronize()
        assert reason == 0
        err = energy_error(oracle, msh, k, full.cpu().numpy())
        say("interface (%d, %d) cell + coarse H 4 %-4s at 1e-9: %4d iterations, energy error %.10e (xlsx %.6e)" % (N, k, parts, iters, err, ref))
        assert abs(err - ref) / ref < 6e-6, err


# ---- 6. the side stream -----------------------------------------------------------------------------------------------------------
def test_coarse_solve_with_cut_overlap(asm):
    """pa_context_set_cut_overlap(1) with a cut-cell kernel out on the side stream: the entry points join it first; table and solve
    have the bits of the run with overlap off"""
    import torch
    import proton_amd as pa
    N, k = 20, 2
    ops, g = real_ops(asm, N, k)

    def run(overlap):
        asm.ctx.set_cut_overlap(overlap)
        try:
            side = torch.empty((asm.ncut,) + tuple(ops["lc"].shape[1:]), dtype=torch.float64, device=asm.device)
            asm.ctx.cut_local_ops(k, asm.level_set, pa.capi.LOC_NEGATIVE, pa.capi.FN_SIN_SIN_RHS, pa.capi.FN_SIN_SIN_SOL,
                                  None, None, None, side.data_ptr(), None, None)
            tb = asm.interface_condensed_coarse(k, 4, "side")
            full, iters, reason = asm.interface_condensed_solve(k, ops, g, tol=1e-13, patches="cell", coarse=4)
            asm.synchronize()
        finally:
            asm.ctx.set_cut_overlap(False)
        assert reason == 0
        return [t.clone() for t in tb[:3]], full.clone(), iters

    t1, f1, i1 = run(False)
    t2, f2, i2 = run(True)
    assert i1 == i2 and all(torch.equal(x, y) for x, y in zip(t1, t2)) and torch.equal(f1, f2)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_touch_no_buffer(asm):
    """the refusals of pa_interface_csr_* in its order, then H, the parts and the NULL outputs, then the column count: each returns
    its code, and neither the table nor the query's sizes are written"""
    import torch
    import proton_amd as pa
    from proton_amd.batch import BatchAssembler
    capi = pa.capi
    L = capi.lib()
    ptr = torch.full((1 << 14,), -5, dtype=torch.int64, device=asm.device)
    cols = torch.full((1 << 16,), -7, dtype=torch.int32, device=asm.device)
    vals = torch.full((1 << 16,), -9.0, dtype=torch.float64, device=asm.device)
    a, b = C.c_size_t(7), C.c_size_t(9)

    def calls(h, fd, H=4, parts=capi.COARSE_BY_SIDE):
        return [L.pa_interface_condensed_coarse_query(h, fd, H, parts, C.byref(a), C.byref(b)),
                L.pa_interface_condensed_coarse(h, fd, H, parts, ptr.data_ptr(), cols.data_ptr(), vals.data_ptr())]

    def untouched():
        asm.synchronize()
        return (a.value, b.value) == (7, 9) and bool((ptr == -5).all()) and bool((cols == -7).all()) and bool((vals == -9.0).all())

    bare = BatchAssembler(0)
    assert calls(bare.ctx.h, 1) == [5, 5]                        # no mesh
    bare.generate_mesh(8, 8)
    assert calls(bare.ctx.h, 1) == [5, 5]                        # a plain mesh, no cut mesh
    bare.synchronize()
    asm.cut_preprocess(12, rows=(3, 8))
    assert calls(asm.ctx.h, 1) == [1, 1]                         # a slab
    assert "whole mesh" in L.pa_last_error(asm.ctx.h).decode()
    asm.cut_preprocess(12)
    assert asm.ncut > 0
    for fd in (-1, 4):
        assert calls(asm.ctx.h, fd) == [2, 2]                    # face degree
        assert calls(asm.ctx.h, fd, 0, 7) == [2, 2]              # ... before H and the parts
    for H in (0, -3):
        assert calls(asm.ctx.h, 1, H) == [1, 1]                  # H < 1
    for parts in (-1, 2):
        assert calls(asm.ctx.h, 1, 4, parts) == [1, 1]           # unknown parts
    h = asm.ctx.h
    assert L.pa_interface_condensed_coarse_query(h, 1, 4, capi.COARSE_ONE, None, C.byref(b)) == 1
    assert L.pa_interface_condensed_coarse_query(h, 1, 4, capi.COARSE_ONE, C.byref(a), None) == 1
    assert L.pa_interface_condensed_coarse(h, 1, 4, capi.COARSE_ONE, None, cols.data_ptr(), vals.data_ptr()) == 1
    assert L.pa_interface_condensed_coarse(h, 1, 4, capi.COARSE_ONE, ptr.data_ptr(), None, vals.data_ptr()) == 1
    assert L.pa_interface_condensed_coarse(h, 1, 4, capi.COARSE_ONE, ptr.data_ptr(), cols.data_ptr(), None) == 1
    assert calls(None, 1) == [1, 1]
    for H in (12, 13, 100):                                      # H >= N: no interior node
        for parts in (capi.COARSE_ONE, capi.COARSE_BY_SIDE):
            assert calls(h, 1, H, parts) == [1, 1]
            msg = L.pa_last_error(h).decode()
            assert "H = %d" % H in msg and " 0 coarse columns" in msg
    assert untouched()
    asm.cut_preprocess(66)
    h = asm.ctx.h
    assert calls(h, 0, 1, capi.COARSE_ONE) == [1, 1]             # 65 x 65 nodes
    msg = L.pa_last_error(h).decode()
    assert "H = 1" in msg and "4225" in msg
    assert calls(h, 0, 1, capi.COARSE_BY_SIDE) == [1, 1]         # ... and more by side
    assert untouched()
    # the same context still works, and writes what the query announced and no more
    assert calls(h, 0, 2, capi.COARSE_ONE) == [0, 0]
    asm.synchronize()
    ncoarse, entries = a.value, b.value
    n = asm.ctx.interface_condensed_query(0).system_size
    assert ncoarse == 32 * 32 and 0 < entries < (1 << 16) and n + 1 < (1 << 14)
    assert int(ptr[0]) == 0 and int(ptr[n]) == entries and bool((ptr[n + 1:] == -5).all())
    assert bool((cols[entries:] == -7).all()) and bool((vals[entries:] == -9.0).all())
    assert bool((cols[:entries] >= 0).all()) and bool((cols[:entries] < ncoarse).all()) and bool((vals[:entries] > 0).all())


# ---- 8. the report ----------------------------------------------------------------------------------------------------------------
def test_zz_report():
    """the lines of the run (with -s); written to the file INTERFACE_COARSE_PROFILE names, if it names one"""
    path = os.environ.get("INTERFACE_COARSE_PROFILE")
    if path and REPORT:
        with open(path, "w") as f:
            f.write("tests/test_gpu_interface_coarse.py on one MI355X: the tables of pa_interface_condensed_coarse against the numpy twin of\n"
                    "tests/interface_coarse_twin.py (bit for bit), through pa_coarse_precond_factor, and interface_condensed_solve with the cell\n"
                    "patches and the coarse level (H = 4, one part and by side) against spsolve of the full system, the cell patches alone and\n"
                    "the xlsx Interface table.\n")
            f.write("\n".join(REPORT) + "\n")
