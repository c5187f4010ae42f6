"""The device solve of the obstacle problem (pa_obstacle_block_solve, pa_obstacle_active_set_update, pa_obstacle_solve) without a
GPU: the header, the ctypes symbol list and the built library agree on the three exports, NULL contexts are refused, the host
header's solve_obstacle and its driver compile against the C ABI alone, and the block structure the device solve relies on -- row
map plus multiplier formula -- reproduces scipy's sparse direct solve on the oracle's system."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"pa_obstacle_block_solve": 18, "pa_obstacle_active_set_update": 12, "pa_obstacle_solve": 13}


@pytest.mark.parametrize("name", sorted(NAMES))
def test_header_binding_and_library_agree_on_the_new_exports(name):
    from proton_amd import capi
    h = open(os.path.join(ROOT, "include", "proton_amd.h")).read()
    assert len(re.findall(r"\b" + name + r"\s*\(", re.sub(r"/\*.*?\*/", "", h, flags=re.S))) == 1
    m = re.search(r"int " + name + r"\(([^;]*)\);", h, flags=re.S)
    assert m, "declaration"
    assert len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")) == NAMES[name]
    assert capi.EXPORTS.count(name) == 1
    assert len(getattr(capi.lib(), name).argtypes) == NAMES[name]
    so = os.path.join(ROOT, "proton_amd", "lib", "libproton_amd.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert len(re.findall(r" T " + name + r"$", out, flags=re.M)) == 1


def test_the_block_solve_comment_cites_the_reference_and_states_the_contract():
    h = open(os.path.join(ROOT, "include", "proton_amd.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int pa_obstacle_block_solve\(", h, flags=re.S)
    assert m
    comment = m.group(1)
    assert "hho.hpp:609-695" in comment and "688-693" in comment and "obstacle.cpp:170-175" in comment
    assert "BIT-IDENTICAL" in comment
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*typedef struct \{[^}]*\} pa_obstacle_solve_params;", h, flags=re.S)
    assert m and "obstacle.cpp:117-197" in m.group(1) and "does not converge" in m.group(1)


def test_the_abi_version_did_not_move():
    from proton_amd import capi
    assert capi.lib().pa_abi_version() == 5


def test_null_contexts_are_refused():
    from proton_amd import capi
    L = capi.lib()
    di, _ = capi.degree_info(0, 1)
    assert L.pa_obstacle_block_solve(None, di, None, None, None, None, None, None, None, 0, 1e-13, 100.0, 10, 1, None, None, None, None) == 1
    assert L.pa_obstacle_active_set_update(None, di, 1.0, None, None, None, None, None, None, None, None, None) == 1
    assert L.pa_obstacle_solve(None, di, None, None, None, None, None, None, None, None, None, None, None) == 1


def test_the_solve_parameters_default_to_the_reference():
    """obstacle.cpp:101 (c = 1), :119 (50 iterations), :193 (1e-7); the drivers' solver settings"""
    from proton_amd import capi
    p = capi.ObstacleSolveParams()
    assert (p.c, p.max_outer, p.outer_tol) == (1.0, 50, 1e-7)
    assert (p.cg_convergence_threshold, p.cg_divergence_threshold, p.cg_max_iter, p.apply_preconditioner) == (1e-13, 100.0, 0, 1)


def test_solve_obstacle_and_its_driver_compile_against_the_c_abi():
    """tests/cpp/obstacle_solve_driver.cpp needs nothing but proton_amd/host/hho.hpp, a C++17 compiler and the C ABI"""
    out_dir = os.path.join(ROOT, "tests", "cpp", "build")
    os.makedirs(out_dir, exist_ok=True)
    lib_dir = os.path.join(ROOT, "proton_amd", "lib")
    cmd = ["g++", "-O0", "-std=c++17", "-Wall", "-Werror", "-o", os.path.join(out_dir, "obstacle_solve_driver_cpu"),
           os.path.join(ROOT, "tests", "cpp", "obstacle_solve_driver.cpp"), "-L" + lib_dir, "-lproton_amd", "-Wl,-rpath," + lib_dir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.mark.parametrize("degree,p", [(0, 0.4), (1, 0.4), (1, 0.0), (1, 1.0)])
def test_row_map_and_multiplier_formula_reproduce_the_direct_solve(oracle, degree, p):
    """5 x 5, the oracle's obstacle system: the rows of the inactive cells (in A_ct order) and of the faces against the columns
    below nk are a symmetric positive definite block, every active row holds its multiplier with coefficient 1 and nothing else
    beyond nk, and solving the block then evaluating the multipliers gives what spsolve gives on the whole system"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    import obstacle_driver as od
    import obstacle_solve_ref as ref
    N = 5
    msh = od.ObstacleMesh(N)
    di = oracle.degrees(0, degree)
    lc, rhs = od.oracle_local_provider(msh, degree)
    rng = np.random.default_rng(11 + degree)
    in_A = rng.random(N * N) < p
    gamma = rng.standard_normal(N * N)
    asm = oracle.ObstacleAssembler(msh.mp, msh.points, msh.ptids, di, in_A, bf_id=4)
    rows, cols, vals = [], [], []
    RHS = np.zeros(asm.system_size)
    for c in range(N * N):
        tr, tc, tv, rr, rv = asm.assemble_cell(c, lc[c], rhs[c], gamma)
        rows.append(tr); cols.append(tc); vals.append(tv)
        ok = rr >= 0
        np.add.at(RHS, rr[ok], rv[ok])
    n = asm.system_size
    LHS = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    want = spla.spsolve(LHS, RHS)

    A = sp.csr_matrix(LHS)
    A.sort_indices()
    rowmap = ref.row_map(asm.A_ct, N * N, n, asm.num_I)
    nk = n - asm.num_A
    assert rowmap.shape == (nk,) and len(set(rowmap.tolist())) == nk
    assert not in_A[rowmap[:asm.num_I]].any() and (np.diff(rowmap[:asm.num_I]) > 0).all()
    krp, kci, kva, bk = ref.extract_block(A.indptr.astype(np.int64), A.indices, A.data, RHS, rowmap)
    K = sp.csr_matrix((kva, kci, krp), shape=(nk, nk)).toarray()
    assert np.abs(K - K.T).max() <= 1e-14 * np.abs(K).max()
    assert np.linalg.eigvalsh(0.5 * (K + K.T)).min() > 0
    # the rows set aside: one multiplier each, coefficient 1, and no multiplier anywhere else
    beyond = sp.csr_matrix(A[:, nk:])
    assert beyond.nnz == asm.num_A and (beyond.data == 1.0).all()
    assert sorted(sp.coo_matrix(beyond).row.tolist()) == np.nonzero(in_A)[0].tolist()

    got = ref.solve_by_blocks(LHS, RHS, in_A, asm.A_ct, asm.B_ct, asm.num_I, lambda Kb, b: np.linalg.solve(Kb.toarray(), b))
    assert np.abs(got - want).max() <= 1e-11 * max(1.0, np.abs(want).max())
    got_cg = ref.solve_by_blocks(LHS, RHS, in_A, asm.A_ct, asm.B_ct, asm.num_I, ref.jacobi_cg)
    assert np.abs(got_cg - want).max() <= 1e-10 * max(1.0, np.abs(want).max())
