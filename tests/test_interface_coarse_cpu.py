"""The coarse table of the interface problem's face-only system without a device: the boundary of the two new entry points (header
comment, declaration, binding, exported symbol, NULL context), the new C++ driver against the C ABI alone, and the judge of
tests/test_gpu_interface_coarse.py (tests/interface_coarse_twin.py) judged itself: its tables keep their promises, a row of A P fits
the 16 slots of the device, and on the Schur complement of the oracle's `-i` system the coarse level saves the iterations the issue
measured."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import coarse_twin as CT
import interface_coarse_twin as IC
import interface_patch_twin as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pa_interface_condensed_coarse_query", "pa_interface_condensed_coarse"]
EPS = np.finfo(float).eps


# ---- the boundary -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NEW)
def test_abi_trio(name):
    """the comment above the declaration cites solver_cg.hpp and the solve it serves; one declaration; the binding lists the name and
    the library exports it"""
    from proton_amd import capi
    h = open(os.path.join(ROOT, "include", "proton_amd.h")).read()
    decl = [m.start() for m in re.finditer(r"^int %s\(" % name, h, flags=re.M)]
    assert len(decl) == 1
    # (the two share the comment above pa_interface_condensed_coarse_query)
    comment = h[:h.index("int pa_interface_condensed_coarse_query(")].rsplit("/*", 1)[1]
    assert "solver_cg.hpp:63-144" in comment and re.search(r"cuthho_square\.cpp:1737-1743", comment), comment
    assert h.index("int pa_interface_condensed_patches(") < decl[0] < h.index("int pa_interface_rows_query(")
    assert "#define PA_ABI_VERSION 5" in h                               # an added export is compatible
    assert capi.EXPORTS.count(name) == 1
    assert getattr(capi.lib(), name).argtypes is not None
    so = os.path.join(ROOT, "proton_amd", "lib", "libproton_amd.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T %s$" % name, out, flags=re.M)


def test_null_context_is_refused():
    from proton_amd import capi
    L = capi.lib()
    a, b = C.c_size_t(7), C.c_size_t(7)
    assert L.pa_interface_condensed_coarse_query(None, 2, 4, capi.COARSE_BY_SIDE, C.byref(a), C.byref(b)) == 1
    assert L.pa_interface_condensed_coarse(None, 2, 4, capi.COARSE_BY_SIDE, None, None, None) == 1
    assert (a.value, b.value) == (7, 7)


def test_driver_compiles_against_the_c_abi():
    out_dir = os.path.join(ROOT, "tests", "cpp", "build")
    os.makedirs(out_dir, exist_ok=True)
    lib_dir = os.path.join(ROOT, "proton_amd", "lib")
    cmd = ["g++", "-O0", "-std=c++17", "-Wall", "-Werror", "-o", os.path.join(out_dir, "interface_coarse_driver_cpu"),
           os.path.join(ROOT, "tests", "cpp", "interface_coarse_driver.cpp"), "-L" + lib_dir, "-lproton_amd", "-Wl,-rpath," + lib_dir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    text = open(os.path.join(ROOT, "proton_amd", "host", "cuthho.hpp")).read()
    assert "int patches = -1, int coarse = 0,\n" in text and "int coarse_parts = PA_COARSE_BY_SIDE)" in text
    assert "pa_interface_condensed_coarse(" in text and "coarse needs patches" in text


# ---- the twin ---------------------------------------------------------------------------------------------------------------------
def _mesh(oracle, N, **kw):
    msh = oracle.CutMesh(N, refsteps=4, **kw)
    faces, bnd = oracle.mesh_faces(oracle.MeshParams(N, N, 0.0, 1.0, 0.0, 1.0))
    assert np.array_equal(faces, msh.faces) and np.array_equal(bnd != 0, msh.bnd != 0)
    return msh, faces


def _interior_blocks(pts, N, H):
    """the items whose two end points lie in no coarse cell that touches the boundary: between the second and the last-but-one line"""
    ln = CT.lines(N, H)
    if len(ln) < 4:
        return np.zeros(pts.shape[0], dtype=bool)
    x, y = pts % (N + 1), pts // (N + 1)
    return ((x >= ln[1]) & (x <= ln[-2]) & (y >= ln[1]) & (y <= ln[-2])).all(axis=1)


@pytest.mark.parametrize("N,H,kw", [(16, 4, {}), (20, 4, {}), (20, 3, {}), (20, 1, {}), (12, 4, dict(line_y=0.47)), (12, 1, dict(line_y=0.47))],
                         ids=["circle16-H4", "circle20-H4", "circle20-H3", "circle20-H1", "line12-H4", "line12-H1"])
@pytest.mark.parametrize("k", [0, 2])
def test_table_properties(oracle, N, H, kw, k):
    """pa_cut_preprocess's numbering (on the line mesh two blocks are unowned).  Rows of at most 4 ascending entries, the rows of modes
    above the second empty, both blocks of a cut face with the same values; no empty column; by side, a column is touched by blocks
    of one side only and the negative side's columns come first; for a block whose end points lie in no coarse cell touching the
    boundary the mode-0 row sums to 1 and the mode-1 row to 0, each within 4 ulp of 1 (at most 4 terms, each a correctly rounded
    product of two hats within [0, 1], halved exactly)"""
    fbs = k + 1
    msh, faces = _mesh(oracle, N, **kw)
    ft, num_other = I.device_face_table(msh.bnd, msh.face_loc)
    pts, blk, side = IC.block_items(ft, msh.face_loc, faces, num_other)
    order = np.argsort(blk)
    pts, side = pts[order], side[order]
    holes = num_other - np.count_nonzero(ft >= 0) - np.count_nonzero((ft >= 0) & (msh.face_loc == I.CUT))
    assert holes == (2 if kw else 0)
    inner = _interior_blocks(pts, N, H)
    assert inner.sum() > 10
    tabs = {}
    for parts in ("one", "side"):
        tb = tabs[parts] = IC.mesh_table(msh, faces, k, H, parts, device_numbering=True)
        assert tb.ptr.size == num_other * fbs + 1 and tb.ptr[0] == 0 and tb.ptr[-1] == tb.cols.size == tb.vals.size
        sizes = np.diff(tb.ptr)
        assert sizes.max() <= 4 and sizes.min() >= 0 and (sizes.reshape(-1, fbs)[:, 2:] == 0).all()
        for i in np.nonzero(sizes >= 2)[0]:
            assert (np.diff(tb.cols[tb.ptr[i]:tb.ptr[i + 1]]) > 0).all()
        assert np.array_equal(np.unique(tb.cols), np.arange(tb.ncoarse))             # no empty column, none out of range
        P = CT.dense(tb)
        assert np.abs(P[0::fbs][inner].sum(axis=1) - 1.0).max() <= 4 * EPS
        if fbs >= 2:
            assert np.abs(P[1::fbs][inner].sum(axis=1)).max() <= 4 * EPS
        # the blocks of a cut face: the same values row by row
        for f in np.nonzero((ft >= 0) & (msh.face_loc == I.CUT))[0]:
            r0, r1 = int(ft[f]) * fbs, (int(ft[f]) + 1) * fbs
            assert np.array_equal(tb.vals[tb.ptr[r0]:tb.ptr[r0 + fbs]], tb.vals[tb.ptr[r1]:tb.ptr[r1 + fbs]])
    one, two = tabs["one"], tabs["side"]
    assert np.array_equal(one.ptr, two.ptr) and np.array_equal(one.vals, two.vals) and two.ncoarse > one.ncoarse
    rowside = np.repeat(side, fbs)[np.repeat(np.arange(num_other * fbs), np.diff(two.ptr))]
    colside = np.full(two.ncoarse, -1)
    for c, s in zip(two.cols, rowside):
        assert colside[c] in (-1, s)
        colside[c] = s
    assert (np.diff(colside) >= 0).all() and set(colside) == {0, 1}


def test_by_side_without_cut_cells_is_the_one_part_table(oracle):
    """the circle outside the square: every face on the negative side, the two tables equal bit for bit, and equal to coarse_twin's of
    the plain numbering"""
    N, k, H = 9, 2, 3
    msh, faces = _mesh(oracle, N, radius=2.0)
    assert np.count_nonzero(msh.cell_loc == I.CUT) == 0
    one, two = (IC.mesh_table(msh, faces, k, H, p, device_numbering=True) for p in ("one", "side"))
    o = oracle.Assembler(oracle.MeshParams(N, N, 0.0, 1.0, 0.0, 1.0), msh.points, msh.ptids, oracle.degrees(k + 1, k))
    plain = CT.table(N, N, H, k + 1, o.compress, o.faces, o.num_other)
    for t in (two, plain):
        assert one.ncoarse == t.ncoarse and all(np.array_equal(a, b) for a, b in zip(one[:3], t[:3]))


def test_planted_defect_misses_the_bit_comparison(oracle):
    """one hat moved by a line: the values differ from the table's"""
    msh, faces = _mesh(oracle, 16)
    for parts in ("one", "side"):
        good = IC.mesh_table(msh, faces, 2, 4, parts)
        bad = IC.mesh_table(msh, faces, 2, 4, parts, shift=(4, 1))
        assert bad is not None and not (np.array_equal(good.cols, bad.cols) and np.array_equal(good.vals, bad.vals))


def test_refusals_of_the_twin(oracle):
    """no interior node (H >= N); more than 4096 columns"""
    msh, faces = _mesh(oracle, 12)
    assert IC.mesh_table(msh, faces, 1, 12, "one") is None and IC.mesh_table(msh, faces, 1, 6, "one").ncoarse == 1
    big, bfaces = _mesh(oracle, 66)
    assert IC.mesh_table(big, bfaces, 0, 1, "one") is None and 65 * 65 > CT.MAX_NODES
    assert IC.mesh_table(big, bfaces, 0, 2, "one").ncoarse == 32 * 32


# ---- the oracle's condensed system --------------------------------------------------------------------------------------------------
def _widest(sy, tb):
    import scipy.sparse as sp
    n = sy.b.size
    A = sp.csr_matrix((np.abs(sy.values), sy.colind, sy.rowptr), shape=(n, n))
    P = sp.csr_matrix((np.abs(tb.vals), tb.cols, tb.ptr), shape=(n, tb.ncoarse))
    W = (A @ P).tocsr()
    W.eliminate_zeros()
    return int(np.diff(W.indptr).max())


@pytest.mark.parametrize("N,k,H", [(20, 2, 1), (20, 2, 2), (32, 2, 4), (64, 2, 4), (21, 1, 3), (16, 0, 1)])
def test_a_row_of_a_p_fits_the_devices_slots(N, k, H):
    """a face row couples the seven faces of its two cells, whose six vertices meet at most six hats: at most 6 columns in one part
    and 12 by side -- the device keeps 16 (COARSE_W_SLOTS)"""
    sy = IC.oracle_interface_coarse(N, k, H)
    one, side = _widest(sy, sy.one), _widest(sy, sy.side)
    print("(%d, %d, H = %d): widest row of |A| |P|: one %d, side %d" % (N, k, H, one, side))
    assert one <= 12 and side <= 12


def test_the_coarse_level_saves_iterations_on_the_oracles_interface_system():
    """Textbook PCG in double from x = 0 to 1e-13 on the Schur complement of the oracle's `-i` system at (64, 2), H = 4.  The issue
    measured: cell patches 331, + coarse "one" 104, "side" 111 (3 x); with kappa = (1, 1e4): cell 359, "one" 296, "side" 243.
    Asserted: both tables take at most half of the cell patches' count; with the jump in kappa "side" takes at most what "one"
    takes."""
    sy = IC.oracle_interface_coarse(64, 2, 4)
    cell, one, side = (CT.two_level_iterations(sy, sy.cell, t) for t in (None, sy.one, sy.side))
    print("(64, 2) H = 4: %d rows, cell patches %d, + coarse one %d (%d columns), side %d (%d columns)"
          % (sy.b.size, cell, one, sy.one.ncoarse, side, sy.side.ncoarse))
    assert 2 * one <= cell and 2 * side <= cell
    sy = IC.oracle_interface_coarse(64, 2, 4, (1.0, 1e4))
    cell, one, side = (CT.two_level_iterations(sy, sy.cell, t) for t in (None, sy.one, sy.side))
    print("(64, 2) H = 4 kappa (1, 1e4): cell patches %d, + coarse one %d, side %d" % (cell, one, side))
    assert side <= one
