"""The patch preconditioner without a device: the boundary of the new entry points (header comment, declaration, binding, exported
symbol, NULL context), the build list, the new C++ driver against the C ABI alone, and the judge of tests/test_gpu_patch_pcg.py
(tests/patch_pcg_twin.py) judged itself: its two routes to the truth agree, its tables keep their promises, the planted defects
miss the gate, and on the oracle's condensed fictitious-domain system the patches save the iterations the issue measured."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import patch_pcg_twin as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pa_patch_precond_query", "pa_patch_precond_factor", "pa_patch_precond_apply", "pa_conjugated_gradient_patch",
       "pa_condensed_patches_query", "pa_condensed_patches"]


# ---- the boundary -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NEW)
def test_abi_trio(name):
    """the comment above the declaration cites solver_cg.hpp and the driver lines it serves; one declaration; the binding lists the
    name and the library exports it"""
    from proton_amd import capi
    h = open(os.path.join(ROOT, "include", "proton_amd.h")).read()
    decl = [m.start() for m in re.finditer(r"^int %s\(" % name, h, flags=re.M)]
    assert len(decl) == 1
    comment = h[:decl[0]].rsplit("/*", 1)[1]
    if name == "pa_condensed_patches":                   # shares the comment above pa_condensed_patches_query
        comment = h[:h.index("int pa_condensed_patches_query(")].rsplit("/*", 1)[1]
    assert "solver_cg.hpp:63-144" in comment and re.search(r"cuthho_square\.cpp:915-919", comment), comment
    assert capi.EXPORTS.count(name) == 1
    so = os.path.join(ROOT, "proton_amd", "lib", "libproton_amd.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T %s$" % name, out, flags=re.M)


def test_null_context_is_refused():
    from proton_amd import capi
    L = capi.lib()
    info = capi.PatchPrecondInfo()
    a, b = C.c_size_t(0), C.c_size_t(0)
    di = capi.DegreeInfo(3, 2, 3)
    assert L.pa_patch_precond_query(None, 0, 0, None, C.byref(info)) == 1
    assert L.pa_patch_precond_factor(None, 0, None, None, None, 0, None, None, None, None, None, None, None) == 1
    assert L.pa_patch_precond_apply(None, 0, 0, None, None, None, None, None, None, None) == 1
    assert L.pa_conjugated_gradient_patch(None, 0, None, None, None, None, None, 0, None, None, 1e-9, 100.0, 10, None, None, None) == 1
    assert L.pa_condensed_patches_query(None, di, capi.PATCH_CELL, C.byref(a), C.byref(b)) == 1
    assert L.pa_condensed_patches(None, di, capi.PATCH_CELL, None, None) == 1
    assert capi.PATCH_MAX_ROWS == 16 == P.PMAX
    assert "#define PA_PATCH_MAX_ROWS 16" in open(os.path.join(ROOT, "include", "proton_amd.h")).read()


def test_kernel_file_is_built():
    src = open(os.path.join(ROOT, "proton_amd", "_build.py")).read()
    assert re.search(r'for unit in \([^)]*"patch_precond"', src)
    assert os.path.exists(os.path.join(ROOT, "proton_amd", "csrc", "patch_precond.hip"))
    text = open(os.path.join(ROOT, "proton_amd", "csrc", "patch_precond.hip")).read()
    assert "atomicAdd(&z" not in text and "unsafeAtomicAdd" not in text          # the apply has no floating-point atomics


def test_driver_compiles_against_the_c_abi():
    out_dir = os.path.join(ROOT, "tests", "cpp", "build")
    os.makedirs(out_dir, exist_ok=True)
    lib_dir = os.path.join(ROOT, "proton_amd", "lib")
    cmd = ["g++", "-O0", "-std=c++17", "-Wall", "-Werror", "-o", os.path.join(out_dir, "fictdom_patch_driver_cpu"),
           os.path.join(ROOT, "tests", "cpp", "fictdom_patch_driver.cpp"), "-L" + lib_dir, "-lproton_amd", "-Wl,-rpath," + lib_dir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "int patches = -1" in open(os.path.join(ROOT, "proton_amd", "host", "hho.hpp")).read()


# ---- the twin ---------------------------------------------------------------------------------------------------------------------
def test_tables_keep_their_promises():
    """sizes within 1..maxm with both ends present, every row in 1 to 4 patches, no row twice in a patch, a patch across every
    multiple of 256 rows, and one table with a patch matrix of condition beyond 1e8"""
    for c in P.case_table():
        pt = P.patches(c)
        sizes = np.diff(pt.ptr)
        assert pt.ptr[0] == 0 and sizes.min() == 1 and sizes.max() == min(c.maxm, c.n)
        cnt = np.bincount(pt.rows, minlength=c.n)
        assert cnt.min() >= 1 and cnt.max() <= 4 and (c.n < 255 or cnt.max() == 4)
        for p in range(sizes.size):
            r = pt.rows[pt.ptr[p]:pt.ptr[p + 1]]
            assert np.unique(r).size == r.size
        for b in range(P.RB, c.n, P.RB):
            assert any(r.min() < b <= r.max() for r in (pt.rows[pt.ptr[p]:pt.ptr[p + 1]] for p in range(sizes.size)))
        perm, other = P.order_preserving_permutation(pt)
        assert c.n < 255 or np.count_nonzero(perm != np.arange(perm.size)) > perm.size // 4
    hard = [c for c in P.case_table() if c.hard]
    assert hard and P.max_patch_condition(hard[0]) >= 1e8
    assert {P.Case(257, 4), P.Case(257, 8)} <= set(P.case_table())


def test_truth_by_two_routes_agrees():
    """mpmath at 50 digits against longdouble wherever mpmath is the truth: z of both test vectors and every judged iterate within
    max(2^-58, 2^-5 e_ref), as tests/test_cg_twin_cpu.py asks of cg_twin (longdouble carries 11 bits more than double)"""
    worst = 0.0
    for c in P.case_table():
        if c.n > P.MP_ROWS:
            continue
        for w in (0, 1):
            e = P.scaled_error(c, P.apply_truth(c, w, "ld"), P.apply_truth(c, w, "mp"))
            assert e <= max(2.0 ** -58, 2.0 ** -5 * P.apply_e_ref(c)), (P.case_id(c), w, e)
            worst = max(worst, e)
        mp, ld, er = P.truth(c, "mp"), P.truth(c, "ld"), P.e_ref(c)
        assert len(mp.rr) == len(ld.rr) == len(er)
        for j in P.judged(c):
            e = P.T.scaled_error(ld.x[j - 1], mp.x[j - 1], P.system(c).diag)
            assert e <= max(2.0 ** -58, 2.0 ** -5 * er[j - 1]), (P.case_id(c), j, e)
            worst = max(worst, e)
    print("longdouble against mpmath: <= %.3e" % worst)


def test_double_restatement_passes_and_the_floor_holds():
    """every iterate of every case is judged (e_ref <= 1e-10) and e_ref stays below the floor 2^-45 of cg_twin; the double
    restatement in the device's order passes its own gate; one-row patches reproduce cg_twin's Jacobi truth"""
    lines = []
    for c in P.case_table():
        er = P.e_ref(c)
        assert P.judged(c) == list(range(1, len(er) + 1))
        assert max(er) <= P.FLOOR and P.apply_e_ref(c) <= P.FLOOR
        errs = P.errors(c, P.pcg(c, "f64", len(er), "dev").x)
        assert all(e <= P.gate(r) for e, r in zip(errs, er))
        lines.append("  %-16s apply e_ref %9.3e   pcg e_ref %s" % (P.case_id(c), P.apply_e_ref(c), " ".join("%9.3e" % e for e in er)))
    print("\n".join(lines))
    c = P.Case(257)
    jac = P.pcg(c, "mp", pt=P.jacobi_patches(c.n))
    ref = P.T.truth(P.T.Case(257, True, False))
    for a, b in zip(jac.x, ref.x):
        assert P.T.scaled_error(a, b, P.system(c).diag) <= 2.0 ** -58


def _fails(c, **defect):
    errs = P.errors(c, P.pcg(c, "f64", None, "dev", **defect).x)
    return any(errs[m - 1] > P.gate(P.e_ref(c)[m - 1]) for m in P.judged(c))


def test_planted_defects_miss_the_gate():
    """a shared row summed for its first patch only; L^T where L^-T belongs; r . r used for rho: each fails the gate on every case
    that can show it (the first needs a shared row: all cases have one), on z itself and on the iterates"""
    for c in P.case_table():
        for defect in (dict(first_slot_only=True), dict(lt_for_linvt=True)):
            z = P.apply_double(c, 0, **defect)
            assert P.scaled_error(c, z, P.apply_truth(c, 0)) > P.gate(P.apply_e_ref(c)), (P.case_id(c), defect)
            if c.n > 2:                                  # (with one or two rows CG ends whatever the preconditioner is)
                assert _fails(c, **defect), (P.case_id(c), defect)
        if c.n > 2:
            assert _fails(c, rho_rr=True), P.case_id(c)
        assert not _fails(c)


# ---- the oracle's condensed system --------------------------------------------------------------------------------------------------
def test_patches_save_iterations_on_the_oracles_condensed_system():
    """Textbook PCG in double from x = 0 to 1e-13 on the Schur complement of the oracle's `-f` system.  Measured here:
        (20, 2), 2280 rows: Jacobi 129, face blocks 63, cell patches 41   (3.1 x)
        (32, 2), 5952 rows: Jacobi 374, face blocks 113, cell patches 71  (5.3 x; face blocks 3.3 x)
    -- the issue's table has 131 / 63 / 43 and 401 / 113 / 76 (+-3 by how the Schur complement is formed; here it is symmetrised,
    which moves the Jacobi count at (32, 2) most): the ratios are the same.  Asserted: cell <= Jacobi / 2 at (20, 2), cell <= Jacobi / 3 and face <=
    Jacobi / 2 at (32, 2): margins of 1.57, 1.76 and 1.65 between the measured ratio and the condition (at least 1.3 is asserted too)."""
    for (N, k), cell_ratio, face_ratio in (((20, 2), 2, None), ((32, 2), 3, 2)):
        sy = P.oracle_condensed(N, k)
        jac, face, cell = (P.pcg_iterations(sy, t) for t in ("jacobi", sy.face, sy.cell))
        print("(%d, %d): %d rows, Jacobi %d, face blocks %d, cell patches %d" % (N, k, sy.b.size, jac, face, cell))
        assert cell_ratio * cell <= jac
        if face_ratio:
            assert face_ratio * face <= jac
        assert jac / cell >= 1.3 * cell_ratio and (face_ratio is None or jac / face >= 1.3 * face_ratio)
