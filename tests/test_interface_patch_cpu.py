"""The patch tables of the interface problem's face-only system without a device: the boundary of the two new entry points (header
comment, declaration, binding, exported symbol, NULL context), the new C++ driver against the C ABI alone, and the judge of
tests/test_gpu_interface_patch.py (tests/interface_patch_twin.py) judged itself: its tables keep their promises, and on the Schur
complement of the oracle's `-i` system the patches save the iterations the issue measured."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import interface_patch_twin as I
import patch_pcg_twin as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pa_interface_condensed_patches_query", "pa_interface_condensed_patches"]


# ---- the boundary -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NEW)
def test_abi_trio(name):
    """the comment above the declaration cites solver_cg.hpp and the solve it serves; one declaration; the binding lists the name and
    the library exports it"""
    from proton_amd import capi
    h = open(os.path.join(ROOT, "include", "proton_amd.h")).read()
    decl = [m.start() for m in re.finditer(r"^int %s\(" % name, h, flags=re.M)]
    assert len(decl) == 1
    # (the two share the comment above pa_interface_condensed_patches_query)
    comment = h[:h.index("int pa_interface_condensed_patches_query(")].rsplit("/*", 1)[1]
    assert "solver_cg.hpp:63-144" in comment and re.search(r"cuthho_square\.cpp:1737-1743", comment), comment
    assert h.index("int pa_interface_condensed_recover(") < decl[0] < h.index("int pa_interface_rows_query(")
    assert "#define PA_ABI_VERSION 5" in h
    assert capi.EXPORTS.count(name) == 1
    assert getattr(capi.lib(), name).argtypes is not None
    so = os.path.join(ROOT, "proton_amd", "lib", "libproton_amd.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T %s$" % name, out, flags=re.M)


def test_null_context_is_refused():
    from proton_amd import capi
    L = capi.lib()
    a, b = C.c_size_t(7), C.c_size_t(7)
    assert L.pa_interface_condensed_patches_query(None, 2, capi.PATCH_CELL, C.byref(a), C.byref(b)) == 1
    assert L.pa_interface_condensed_patches(None, 2, capi.PATCH_CELL, None, None) == 1
    assert (a.value, b.value) == (7, 7)


def test_driver_compiles_against_the_c_abi():
    out_dir = os.path.join(ROOT, "tests", "cpp", "build")
    os.makedirs(out_dir, exist_ok=True)
    lib_dir = os.path.join(ROOT, "proton_amd", "lib")
    cmd = ["g++", "-O0", "-std=c++17", "-Wall", "-Werror", "-o", os.path.join(out_dir, "interface_patch_driver_cpu"),
           os.path.join(ROOT, "tests", "cpp", "interface_patch_driver.cpp"), "-L" + lib_dir, "-lproton_amd", "-Wl,-rpath," + lib_dir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    text = open(os.path.join(ROOT, "proton_amd", "host", "cuthho.hpp")).read()
    assert "int patches = -1" in text and "pa_interface_condensed_patches(" in text


# ---- the twin ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,k", [(10, 0), (10, 1), (10, 2), (10, 3), (20, 2)])
def test_tables_keep_their_promises(oracle, N, k):
    """every row in exactly one face patch and exactly two cell patches; sizes within 1..8 (face) and 1..16 (cell), at k = 2 up to 6
    and 12; no row twice in a patch; the face patches partition the rows in order; an uncut face of a cut cell in the patch of
    exactly one of its sides"""
    o = oracle
    msh = o.CutMesh(N, refsteps=4)
    assert np.count_nonzero(msh.cell_loc == o.CUT_ON_INTERFACE) > 0
    fbs = k + 1
    face, cell, n = I.mesh_tables(msh, k)
    ct, ft, num_all_cells, num_other = msh.interface_tables()
    assert n == fbs * num_other
    dft, dnum = I.device_face_table(msh.bnd, msh.face_loc)          # no cut face on the boundary: the device numbers as the oracle does
    assert np.array_equal(dft, ft) and dnum == num_other
    for pt, most, times in ((face, 8, 1), (cell, P.PMAX, 2)):
        sizes = np.diff(pt.ptr)
        assert pt.ptr[0] == 0 and pt.ptr[-1] == pt.rows.size and sizes.min() >= 1 and sizes.max() <= most
        assert np.array_equal(np.bincount(pt.rows, minlength=n), np.full(n, times))
        for p in range(sizes.size):
            r = pt.rows[pt.ptr[p]:pt.ptr[p + 1]]
            assert np.unique(r).size == r.size
    assert np.array_equal(face.rows, np.arange(n))
    assert np.array_equal(face.ptr, np.append(ft[ft >= 0], num_other) * fbs)
    assert np.diff(face.ptr).max() == 2 * fbs and np.diff(cell.ptr).max() == 4 * fbs
    sides = {}
    for c, s, bl in I.cell_side_blocks(ft, msh.cell_faces, msh.cell_loc, msh.face_loc):
        if s is not None:
            sides.setdefault(c, []).append(bl)
    seen = 0
    for c, (neg, pos) in sides.items():
        for f in msh.cell_faces[c]:
            f = int(f)
            if ft[f] < 0 or msh.face_loc[f] == o.CUT_ON_INTERFACE:
                continue
            assert (int(ft[f]) in neg) + (int(ft[f]) in pos) == 1
            assert (int(ft[f]) in neg) == (msh.face_loc[f] == o.CUT_NEG)
            seen += 1
    assert seen > 0


def test_line_level_set_skips_the_dirichlet_slots(oracle):
    """cut cells on the Dirichlet boundary: their dropped slots are in no patch and every row is still covered"""
    o = oracle
    N, k = 12, 1
    msh = o.CutMesh(N, refsteps=4, line_y=0.43)
    cut = np.nonzero(msh.cell_loc == o.CUT_ON_INTERFACE)[0]
    assert np.any(cut % N == 0) and np.any(cut % N == N - 1)
    face, cell, n = I.mesh_tables(msh, k)
    assert np.array_equal(np.bincount(face.rows, minlength=n), np.ones(n, dtype=np.int64))
    cnt = np.bincount(cell.rows, minlength=n)
    assert cnt.min() == 2 and cnt.max() == 2 and np.diff(cell.ptr).min() < 2 * (k + 1) + 1
    # the device's numbering counts the two cut faces on the boundary: one unowned block each, in no patch; the tables are the
    # oracle's with the rows behind each gap shifted by one block
    dface, dcell, dn = I.mesh_tables(msh, k, device_numbering=True)
    holes = np.nonzero(msh.bnd.astype(bool) & (msh.face_loc == o.CUT_ON_INTERFACE))[0]
    assert holes.size == 2 and dn == n + 2 * (k + 1)
    assert np.array_equal(dface.ptr, face.ptr) and np.array_equal(dcell.ptr, cell.ptr)
    dcnt = np.bincount(dface.rows, minlength=dn)
    assert np.count_nonzero(dcnt == 0) == 2 * (k + 1) and dcnt.max() == 1
    assert np.array_equal(np.bincount(dcell.rows, minlength=dn), 2 * dcnt)
    owned = np.nonzero(dcnt)[0]
    assert np.array_equal(owned[face.rows], dface.rows) and np.array_equal(owned[cell.rows], dcell.rows)


# ---- the oracle's condensed system --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,k,kappa,cell_ratio,face_ratio", [(20, 2, (1.0, 1.0), 4, 3), (32, 2, (1.0, 1.0), 3, 2), (20, 2, (1.0, 100.0), 4, None)],
                         ids=["20-k2", "32-k2", "20-k2-kappa-1-100"])
def test_patches_save_iterations_on_the_oracles_interface_system(oracle, N, k, kappa, cell_ratio, face_ratio):
    """Textbook PCG in double from x = 0 to 1e-13 on the Schur complement of the oracle's `-i` system.  Measured here:
        (20, 2), 2436 rows:                 Jacobi 484, face 108, cell 84    (5.8 x; face 4.5 x)
        (32, 2), 6228 rows:                 Jacobi 757, face 203, cell 153   (4.9 x; face 3.7 x)
        (20, 2), kappa = (1, 100):          Jacobi 528, face 131, cell 76    (6.9 x)
    Asserted: 4 cell <= Jacobi and 3 face <= Jacobi at (20, 2), 3 cell <= Jacobi and 2 face <= Jacobi at (32, 2), 4 cell <= Jacobi
    with kappa = (1, 100): margins of 1.44, 1.49, 1.65, 1.86 and 1.74 between the measured ratio and the condition (at least 1.3 is
    asserted too)."""
    sy = I.oracle_interface_condensed(N, k, kappa)
    jac, face, cell = (P.pcg_iterations(sy, t) for t in ("jacobi", sy.face, sy.cell))
    print("(%d, %d) kappa %s: %d rows, Jacobi %d, face patches %d, cell patches %d" % (N, k, kappa, sy.b.size, jac, face, cell))
    assert cell_ratio * cell <= jac and jac / cell >= 1.3 * cell_ratio
    if face_ratio:
        assert face_ratio * face <= jac and jac / face >= 1.3 * face_ratio
