"""The two-level conjugate gradient on the row-partitioned system without a device: the boundary of the new entry points, the build
list, and the judge of tests/test_gpu_rows_pcg.py (tests/rows_pcg_twin.py) judged itself: it reaches the truth by two routes, the
double restatement passes its gates, the slab tables keep the properties the header states, and the two planted defects -- the ghost
rows of P left out of W, a cell patch that keeps a foreign row -- miss the gates."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import coarse_twin as CT
import patch_pcg_twin as PT
import rows_pcg_twin as RT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pa_conjugated_gradient_rows_patch_coarse", "pa_condensed_rows_patches_query", "pa_condensed_rows_patches",
       "pa_condensed_rows_coarse_query", "pa_condensed_rows_coarse"]


# ---- the boundary -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NEW)
def test_abi_trio(name):
    """one declaration under a comment that cites the reference; the binding lists the name and the library exports it"""
    from proton_amd import capi
    h = open(os.path.join(ROOT, "include", "proton_amd.h")).read()
    decl = [m.start() for m in re.finditer(r"^int %s\(" % name, h, flags=re.M)]
    assert len(decl) == 1
    comment = h[:decl[0]].rsplit("/*", 1)[1]
    assert re.search(r"(solver_cg\.hpp|hho\.hpp):\d+", comment), comment
    assert capi.EXPORTS.count(name) == 1
    so = os.path.join(ROOT, "proton_amd", "lib", "libproton_amd.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T %s$" % name, out, flags=re.M)


def test_null_context_is_refused_and_the_scope_is_stated():
    from proton_amd import capi
    L = capi.lib()
    a, b = C.c_size_t(0), C.c_size_t(0)
    di = capi.DegreeInfo(2, 1, 2)
    assert L.pa_conjugated_gradient_rows_patch_coarse(None, None, 0, 0, None, None, None, None, None, 0, None, None, 0, None, None, None, 1e-9,
                                                      100.0, 10, None, None, None, None) == 1
    assert L.pa_condensed_rows_patches_query(None, di, capi.PATCH_CELL, C.byref(a), C.byref(b)) == 1
    assert L.pa_condensed_rows_patches(None, di, capi.PATCH_CELL, None, None) == 1
    assert L.pa_condensed_rows_coarse_query(None, di, 4, capi.COARSE_ONE, C.byref(a), C.byref(b)) == 1
    assert L.pa_condensed_rows_coarse(None, di, 4, capi.COARSE_ONE, None, None, None) == 1
    h = open(os.path.join(ROOT, "include", "proton_amd.h")).read()
    comment = h[:h.index("int pa_condensed_rows_patches_query(")].rsplit("/*", 1)[1]
    for out_of_scope in ("PA_COARSE_BY_SIDE", "interface problem", "C++ headers"):
        assert out_of_scope in comment


def test_kernel_files_are_built_without_float_atomics():
    src = open(os.path.join(ROOT, "proton_amd", "_build.py")).read()
    assert re.search(r'for unit in \([^)]*"rows_precond"', src)
    text = open(os.path.join(ROOT, "proton_amd", "csrc", "rows_precond.hip")).read()
    assert "atomic" not in text.replace("floating-point atomics", "") and "__global__" not in text      # no kernel of its own
    patch = open(os.path.join(ROOT, "proton_amd", "csrc", "patch_precond.hip")).read()
    assert patch.count("void patch_factor_kernel(") == 1                # one statement of the Cholesky kernel: the table's row0


# ---- the generic case: two routes, the gates, the ghost rows --------------------------------------------------------------------------
def test_partitions_are_what_the_device_tests_need():
    sy = RT.generic_system()
    reach = int(np.abs(np.repeat(np.arange(sy.n), np.diff(sy.rowptr)) - sy.colind).max())
    assert [len(p) - 1 for p in RT.PARTITIONS] == [2, 3, 4]
    for parts in RT.PARTITIONS:
        slabs, pt, tb = RT.generic_tables(parts)
        assert parts[0] == 0 and parts[-1] == sy.n and all(b % 256 for b in parts[1:-1])
        for (r0, r1), t in zip(RT.generic_bounds(parts), slabs):
            assert r1 - r0 > reach                                          # a neighbour reads no further than this rank's rows
            assert t.rows.min() >= r0 and t.rows.max() < r1 and np.unique(t.rows).size == r1 - r0          # inside, and a cover
            assert 1 <= np.diff(t.ptr).min() and np.diff(t.ptr).max() <= PT.PMAX
        assert pt.rows.size == PT.patches(CT.base(RT.CASE)).rows.size      # cut, nothing lost


@pytest.mark.parametrize("parts", RT.PARTITIONS, ids=lambda p: "%dranks" % (len(p) - 1))
def test_two_routes_reach_the_truth_and_the_double_restatement_passes(parts):
    sy = RT.generic_system()
    tr, ranks = RT.truth(parts), RT.by_ranks(parts, "ld")
    assert len(tr.rr) == RT.M_MAX == 8
    agree = RT.errors(sy, ranks.x, tr.x)
    er = RT.e_ref(parts)
    print("%d ranks: routes agree within %s; e_ref %s" % (len(parts) - 1, " ".join("%.2e" % e for e in agree), " ".join("%.2e" % e for e in er)))
    assert max(agree) <= RT.ROUTES_AGREE
    assert max(er) <= RT.CAP                                                # every iterate is judged
    _, pt, tb = RT.generic_tables(parts)
    glob = RT.errors(sy, RT.pcg(sy, pt, tb, "f64").x, tr.x)                 # the same in double, summed globally: another order
    assert all(e <= RT.gate(r) for e, r in zip(glob, er))
    # patches only: the same judge
    assert max(RT.errors(sy, RT.by_ranks(parts, "ld", False).x, RT.truth(parts, False).x)) <= RT.ROUTES_AGREE
    assert max(RT.e_ref(parts, False)) <= RT.CAP


@pytest.mark.parametrize("parts", RT.PARTITIONS, ids=lambda p: "%dranks" % (len(p) - 1))
def test_partitioned_coarse_matrix_and_the_ghost_rows(parts):
    """A_c summed over the ranks is P^T A P; with the ghost rows of P left out of W it is not, and its iterates miss the gate"""
    sy = RT.generic_system()
    _, pt, tb = RT.generic_tables(parts)
    bnds = RT.generic_bounds(parts)
    ref = CT.matrix(RT.CASE, "ld")
    good_ld, good = RT.galerkin_rows(sy, tb, bnds, "ld"), RT.galerkin_rows(sy, tb, bnds, "f64")
    assert np.array_equal(good, good.T)
    g = CT.gate(CT.matrix_e_ref(RT.CASE))
    assert CT.matrix_error(RT.CASE, good_ld) <= g * 2.0 ** -11 and CT.matrix_error(RT.CASE, good) <= g
    bad = RT.galerkin_rows(sy, tb, bnds, "f64", drop_ghosts=True)
    assert CT.matrix_error(RT.CASE, bad) > 1e3 * g
    assert np.abs(bad - np.asarray(ref, dtype=np.float64)).max() > 0
    er, tr = RT.e_ref(parts), RT.truth(parts)
    errs = RT.errors(sy, RT.pcg(sy, pt, tb, "f64", bnds=bnds, Ac=bad).x, tr.x)
    assert any(e > RT.gate(r) for e, r in zip(errs, er)), errs


# ---- the tables of a slab on the mesh's numbering ---------------------------------------------------------------------------------------
MESHES = [(12, 1, 4, (0, 5, 12)), (9, 2, 3, (0, 2, 5, 9)), (4, 1, 2, (0, 1, 2, 3, 4))]


@pytest.mark.parametrize("N,k,H,parts", MESHES)
def test_slab_tables_and_the_foreign_row(oracle, N, k, H, parts):
    """the face tables of the slabs concatenate to the whole-mesh table, the cell tables to it with the foreign rows deleted: only the
    top faces of a slab's top cell row go; every slab's table covers its rows and stays inside them; the rows of P are P's.  A cell
    table that keeps the foreign rows breaks the rule the solver checks, and its iterates are another preconditioner's"""
    sy = CT.oracle_poisson(N, k, H)
    fbs = sy.fbs
    bnds = RT.bounds(N, N, parts, fbs)
    assert bnds[0][0] == 0 and bnds[-1][1] == sy.b.size and all(a[1] == b[0] for a, b in zip(bnds[:-1], bnds[1:]))
    face = RT.truncate_patches(sy.face, RT.row_owner(sy.face, bnds), bnds)
    assert np.array_equal(RT.concat(face).rows, sy.face.rows) and np.array_equal(RT.concat(face).ptr, sy.face.ptr)
    owner = RT.cell_owner(N, parts, sy.cell.ptr.size - 1)
    cell = RT.truncate_patches(sy.cell, owner, bnds)
    lost = sy.cell.rows.size - RT.concat(cell).rows.size
    assert lost == (len(parts) - 2) * N * fbs                              # the top faces of every slab but the last
    for (r0, r1), t in zip(bnds, cell):
        assert t.rows.min() >= r0 and t.rows.max() < r1 and np.unique(t.rows).size == r1 - r0
    for r0, r1 in bnds:
        t = RT.slab_coarse(sy.one, r0, r1)
        assert t.ptr[0] == 0 and np.array_equal(CT.dense(t), CT.dense(sy.one)[r0:r1])
    kept = RT.truncate_patches(sy.cell, owner, bnds, keep_foreign=True)
    assert any(t.rows.max() >= r1 for (r0, r1), t in zip(bnds[:-1], kept[:-1]))          # refused by the solver: PATCH_BAD_INDEX
    S = PT.T.System(sy.b.size, sy.rowptr, sy.colind, sy.values, sy.b, _diag(sy), None)
    good, bad = RT.concat(cell), RT.concat(kept)
    tr = RT.pcg(S, good, sy.one, "ld")
    er = [max(a, b) for a, b in zip(RT.errors(S, RT.pcg(S, good, sy.one, "f64", bnds=bnds).x, tr.x),
                                    RT.errors(S, RT.pcg(S, good, sy.one, "f64").x, tr.x))]
    assert max(RT.errors(S, RT.pcg(S, good, sy.one, "ld", bnds=bnds).x, tr.x)) <= RT.ROUTES_AGREE
    errs = RT.errors(S, RT.pcg(S, bad, sy.one, "f64", bnds=bnds).x, tr.x)
    assert all(e > RT.gate(r) for e, r in zip(errs[1:], er[1:])), (errs, er)


def _diag(sy):
    rows = np.repeat(np.arange(sy.b.size), np.diff(sy.rowptr))
    return sy.values[rows == sy.colind]


def test_the_mesh_of_the_device_solve_halves_jacobis_count(oracle):
    """the mesh on which tests/test_gpu_rows_pcg.py compares the count with the point Jacobi's is chosen here: textbook PCG to 1e-11
    with the slabs' cell patches and the coarse level against the point Jacobi.  Measured: (12, 1) H = 4 slabs (0, 5, 12): 42 against
    75, too small a mesh for the coarse level to pay; (24, 1) H = 4 slabs (0, 10, 24): 47 against 151 (the patches alone: 107)"""
    N, k, H, parts = RT.SOLVE_MESH
    sy = CT.oracle_poisson(N, k, H)
    bnds = RT.bounds(N, N, parts, sy.fbs)
    cell = RT.concat(RT.truncate_patches(sy.cell, RT.cell_owner(N, parts, sy.cell.ptr.size - 1), bnds))
    two = CT.two_level_iterations(sy, cell, sy.one, tol=1e-11)
    jac = PT.pcg_iterations(sy, "jacobi", tol=1e-11)
    print("(%d, %d) H = %d slabs %s: two-level %d iterations, Jacobi %d" % (N, k, H, parts, two, jac))
    assert 2 * two <= jac
