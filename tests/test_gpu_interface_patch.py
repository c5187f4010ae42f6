"""The patch tables of the interface problem's face-only system (pa_interface_condensed_patches, interface_condensed.hip) and the
solve through them on the device: both tables bit for bit against the twin of tests/interface_patch_twin.py, against
pa_condensed_patches where nothing is cut, through pa_patch_precond_* on the real system, interface_condensed_solve end to end
against a direct solve and the xlsx Interface table, the side stream, and the refusals.  One run: profiles/interface_patch_parity.txt
(INTERFACE_PATCH_PROFILE=that file python -m pytest tests/test_gpu_interface_patch.py -m gpu -s)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import interface_patch_twin as I
from interface_helpers import real_ops

pytestmark = pytest.mark.gpu

REPORT = []
KINDS = ("face", "cell")


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


def device_tables(a, k):
    out = {}
    for kind in KINDS:
        ptr, rows = a.interface_condensed_patches(k, kind)
        a.synchronize()
        out[kind] = (ptr.cpu().numpy(), rows.cpu().numpy())
        assert out[kind][0].dtype == np.int64 and out[kind][1].dtype == np.int32
    return out


def check_against_twin(a, msh, label):
    from proton_amd import capi
    for k in range(4):
        # (pa_cut_preprocess's numbering: the oracle's interface_tables() unless a cut face lies on the boundary -- see the twin)
        face, cell, n = I.mesh_tables(msh, k, device_numbering=True)
        assert n == a.ctx.interface_condensed_query(k).system_size
        got = device_tables(a, k)
        for kind, want in (("face", face), ("cell", cell)):
            ptr, rows = got[kind]
            assert np.array_equal(ptr, want.ptr) and np.array_equal(rows, want.rows), (label, k, kind)
            assert a.ctx.interface_condensed_patches_query(k, {"face": capi.PATCH_FACE, "cell": capi.PATCH_CELL}[kind]) == (ptr.size - 1, rows.size)
        say("tables %-22s k %d: %5d rows, face %5d patches (largest %d), cell %5d patches (largest %2d): equal to the twin"
            % (label, k, n, face.ptr.size - 1, np.diff(face.ptr).max(), cell.ptr.size - 1, np.diff(cell.ptr).max()))


# ---- 1. the tables against the twin -----------------------------------------------------------------------------------------------
def test_tables_equal_the_twin_on_the_circle(asm, oracle):
    """k = 0..3 at N = 10; then pa_cut_preprocess of the same context with another radius: the twin's tables of that mesh, and a
    fresh context's"""
    from proton_amd.batch import BatchAssembler
    asm.cut_preprocess(10, refsteps=4)
    assert asm.ncut > 0
    check_against_twin(asm, oracle.CutMesh(10, refsteps=4), "circle N 10")
    asm.cut_preprocess(10, radius=0.3, refsteps=4)
    check_against_twin(asm, oracle.CutMesh(10, radius=0.3, refsteps=4), "circle N 10 r 0.3 (2nd)")
    fresh = BatchAssembler(0)
    fresh.cut_preprocess(10, radius=0.3, refsteps=4)
    for k in range(4):
        a, b = device_tables(asm, k), device_tables(fresh, k)
        for kind in KINDS:
            assert np.array_equal(a[kind][0], b[kind][0]) and np.array_equal(a[kind][1], b[kind][1])


def test_tables_equal_the_twin_on_the_line(asm, oracle):
    """the line level set at N = 12: cut cells on the Dirichlet boundary, whose slots are dropped"""
    N = 12
    asm.cut_preprocess(N, refsteps=4, line_y=0.43)
    cut_cells = np.nonzero(np.asarray(asm.cut_index) >= 0)[0]
    assert np.any(cut_cells % N == 0) and np.any(cut_cells % N == N - 1)
    msh = oracle.CutMesh(N, refsteps=4, line_y=0.43)
    check_against_twin(asm, msh, "line N 12 y 0.43")
    # the rows of the face patches are the non-empty rows of the device's own pattern, in order: the numbering counts the two cut
    # faces on the boundary, whose blocks nobody owns
    for k in range(4):
        rp, _ = asm.interface_condensed_csr_pattern(k)
        ptr, rows = asm.interface_condensed_patches(k, "face")
        asm.synchronize()
        rp = rp.cpu().numpy()
        nonempty = np.nonzero(np.diff(rp))[0]
        assert np.array_equal(rows.cpu().numpy(), nonempty) and nonempty.size == rp.size - 1 - 2 * (k + 1)


# ---- 2. no cut cells --------------------------------------------------------------------------------------------------------------
def test_without_cut_cells_the_tables_are_the_plain_ones(asm):
    """the circle outside the square: both tables are pa_condensed_patches(k + 1, k), bit for bit"""
    import torch
    import proton_amd as pa
    N = 9
    asm.level_set = pa.capi.LevelSet(0, 2.0, 0.5, 0.5, 0.0)
    asm.ctx.cut_preprocess(N, N, asm.level_set, 4)
    asm.ncut, asm.cell_loc, asm.cut_index = asm.ctx.cut_query()
    assert asm.ncut == 0
    for k in range(4):
        for kind in KINDS:
            ptr, rows = asm.interface_condensed_patches(k, kind)
            ptr2, rows2 = asm.condensed_patches(k + 1, k, kind)
            asm.synchronize()
            assert ptr.numel() > 1 and torch.equal(ptr, ptr2) and torch.equal(rows, rows2), (k, kind)


# ---- 3. through the preconditioner ------------------------------------------------------------------------------------------------
def condensed_system(a, k, ops, g):
    rec = a.interface_condensed_ops(k, ops)
    rp, ci = a.interface_condensed_csr_pattern(k)
    va, RH = a.interface_condensed_csr_fill(k, rec, g)
    return rp, ci, va, RH


def test_tables_pass_the_preconditioner_on_the_real_system(asm):
    """(20, 2): pa_patch_precond_query / _factor take both tables, no patch fails, the largest patch has 6 (face) and 12 (cell) rows,
    two applies give the same bits"""
    import torch
    N, k = 20, 2
    ops, g = real_ops(asm, N, k)
    rp, ci, va, RH = condensed_system(asm, k, ops, g)
    for kind, most in (("face", 6), ("cell", 12)):
        pre = asm.patch_precond_factor(rp, ci, va, asm.interface_condensed_patches(k, kind))
        assert pre["failed"] == 0 and int(pre["info"].abs().sum()) == 0
        assert pre["sizes"].max_patch_rows == most and pre["sizes"].lanes_per_patch == (8 if most <= 8 else 16)
        z = asm.patch_precond_apply(pre, RH)
        z2 = asm.patch_precond_apply(pre, RH, torch.full_like(RH, float("nan")))
        asm.synchronize()
        assert torch.equal(z, z2) and bool(torch.isfinite(z).all())
        say("precond (%d, %d) %-4s: %d patches, %d entries, max_patch_rows %d, lanes %d, factor %d doubles: no failed patch"
            % (N, k, kind, pre["patches"][0].numel() - 1, pre["sizes"].entries, most, pre["sizes"].lanes_per_patch, pre["sizes"].factor_doubles))


# ---- 4. the solve end to end ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,k,kappa,cell_ratio,face_ratio", [(20, 2, (1.0, 1.0), 4, 3), (32, 2, (1.0, 1.0), 3, 2), (20, 2, (1.0, 100.0), 4, None)],
                         ids=["20-k2", "32-k2", "20-k2-kappa-1-100"])
def test_interface_condensed_solve_with_patches(asm, N, k, kappa, cell_ratio, face_ratio):
    """interface_condensed_solve at 1e-13 with Jacobi, face and cell patches: exit reason 0, the recovered vector within 1e-8 max|ref|
    of spsolve of the full system, and the iteration conditions of tests/test_interface_patch_cpu.py against the Jacobi solve of the
    same call: 4 cell <= Jacobi and 3 face <= Jacobi at (20, 2), 3 cell <= Jacobi and 2 face <= Jacobi at (32, 2), 4 cell <= Jacobi
    with kappa = (1, 100); the Jacobi path gives the bits of the entry points called one by one"""
    import scipy.sparse.linalg as spla
    import torch

    import test_gpu_interface_condensed as IC
    asm.cut_preprocess(N, refsteps=4)
    import proton_amd as pa
    ops = asm.interface_local_ops(k, kappa=kappa)
    g = asm.dirichlet_data(k, pa.capi.FN_SIN_SIN_SOL)
    K, b = IC.full_csr(asm, k, ops, g)
    ref = spla.spsolve(K.tocsc(), b)
    iters = {}
    for patches in (None, "face", "cell"):
        full, iters[patches], reason = asm.interface_condensed_solve(k, ops, g, tol=1e-13, patches=patches)
        asm.synchronize()
        assert reason == 0
        err = np.abs(full.cpu().numpy() - ref).max() / np.abs(ref).max()
        say("interface (%d, %d) kappa %s patches %-5s: %4d iterations, against spsolve %.3e of max|ref|" % (N, k, kappa, patches, iters[patches], err))
        assert err <= 1e-8
        if patches is None:
            assert torch.equal(full, IC.condensed_solve(asm, k, ops, g, 1e-13))
    assert cell_ratio * iters["cell"] <= iters[None]
    if face_ratio:
        assert face_ratio * iters["face"] <= iters[None]


# ---- 5. the xlsx Interface table --------------------------------------------------------------------------------------------------
def energy_error(o, msh, k, sol):
    """the energy-norm error (:1762-1833) of a full solution vector, as tests/test_gpu_interface_condensed.py computes it"""
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
    return math.sqrt(H1)


@pytest.mark.parametrize("k,N,ref", [(1, 20, 5.22389e-3), (2, 20, 1.38029e-4)])
def test_patch_solves_reproduce_xlsx(asm, oracle, k, N, ref):
    """the energy-norm error of the vector the patch solves recover at the driver's threshold 1e-9 (:1737-1743), within 6e-6"""
    ops, g = real_ops(asm, N, k)
    msh = oracle.CutMesh(N, refsteps=4)
    for patches in KINDS:
        full, iters, reason = asm.interface_condensed_solve(k, ops, g, tol=1e-9, patches=patches)
        asm.synchronize()
        assert reason == 0
        err = energy_error(oracle, msh, k, full.cpu().numpy())
        say("interface (%d, %d) patches %-5s at 1e-9: %4d iterations, energy error %.10e (xlsx %.6e)" % (N, k, patches, iters, err, ref))
        assert abs(err - ref) / ref < 6e-6, err


# ---- 6. the side stream -----------------------------------------------------------------------------------------------------------
def test_cell_patch_solve_with_cut_overlap(asm):
    """pa_context_set_cut_overlap(1) with a cut-cell kernel out on the side stream: the entry points join it first; tables and solve
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
            ptr, rows = asm.interface_condensed_patches(k, "cell")
            full, iters, reason = asm.interface_condensed_solve(k, ops, g, tol=1e-13, patches="cell")
            asm.synchronize()
        finally:
            asm.ctx.set_cut_overlap(False)
        assert reason == 0
        return ptr.clone(), rows.clone(), full.clone(), iters

    p1, r1, f1, i1 = run(False)
    p2, r2, f2, i2 = run(True)
    assert i1 == i2 and torch.equal(p1, p2) and torch.equal(r1, r2) and torch.equal(f1, f2)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_touch_no_buffer(asm):
    """the refusals of pa_interface_csr_* in its order, then the kind and the NULL outputs: each returns its code, and neither the
    tables nor the query's sizes are written"""
    import torch
    import proton_amd as pa
    from proton_amd.batch import BatchAssembler
    capi = pa.capi
    L = capi.lib()
    ptr = torch.full((4096,), -5, dtype=torch.int64, device=asm.device)
    rows = torch.full((1 << 16,), -7, dtype=torch.int32, device=asm.device)
    a, b = C.c_size_t(7), C.c_size_t(9)

    def calls(h, fd, kind=capi.PATCH_CELL):
        return [L.pa_interface_condensed_patches_query(h, fd, kind, C.byref(a), C.byref(b)),
                L.pa_interface_condensed_patches(h, fd, kind, ptr.data_ptr(), rows.data_ptr())]

    def untouched():
        asm.synchronize()
        return (a.value, b.value) == (7, 9) and bool((ptr == -5).all()) and bool((rows == -7).all())

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
        assert calls(asm.ctx.h, fd, 2) == [2, 2]                 # ... before the kind
    for kind in (-1, 2):
        assert calls(asm.ctx.h, 1, kind) == [1, 1]               # an unknown kind
    assert L.pa_interface_condensed_patches_query(asm.ctx.h, 1, capi.PATCH_FACE, None, C.byref(b)) == 1
    assert L.pa_interface_condensed_patches_query(asm.ctx.h, 1, capi.PATCH_FACE, C.byref(a), None) == 1
    assert L.pa_interface_condensed_patches(asm.ctx.h, 1, capi.PATCH_FACE, None, rows.data_ptr()) == 1
    assert L.pa_interface_condensed_patches(asm.ctx.h, 1, capi.PATCH_FACE, ptr.data_ptr(), None) == 1
    assert calls(None, 1) == [1, 1]
    assert untouched()
    # the same context still works, and writes what the query announced and no more
    assert calls(asm.ctx.h, 1) == [0, 0]
    asm.synchronize()
    npatches, entries = a.value, b.value
    assert 0 < npatches < 4095 and 0 < entries < (1 << 16)
    assert int(ptr[npatches]) == entries and bool((ptr[npatches + 1:] == -5).all()) and bool((rows[entries:] == -7).all())
    assert bool((rows[:entries] >= 0).all())


# ---- 8. the report ----------------------------------------------------------------------------------------------------------------
def test_zz_report():
    """the lines of the run (with -s); written to the file INTERFACE_PATCH_PROFILE names, if it names one"""
    path = os.environ.get("INTERFACE_PATCH_PROFILE")
    if path and REPORT:
        with open(path, "w") as f:
            f.write("tests/test_gpu_interface_patch.py on one MI355X: the tables of pa_interface_condensed_patches against the numpy twin of\n"
                    "tests/interface_patch_twin.py (bit for bit), through pa_patch_precond_*, and interface_condensed_solve with Jacobi, face and\n"
                    "cell patches against spsolve of the full system and the xlsx Interface table.\n")
            f.write("\n".join(REPORT) + "\n")
