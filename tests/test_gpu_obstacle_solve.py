"""The obstacle problem's active-set iteration on the device: pa_obstacle_block_solve (the solve of obstacle.cpp:170-175 in place
on the CSR arrays of pa_obstacle_csr_assemble), pa_obstacle_active_set_update (obstacle.cpp:133-142 and :193 in one pass) and
pa_obstacle_solve (the loop of obstacle.cpp:117-197).

References: for the block solve, pa_conjugated_gradient on the SPD block extracted with numpy from the downloaded CSR -- bit for
bit -- and the float64 host evaluation of the multipliers; for the update, numpy's unfused float64; for the loop, the CPU loop of
tests/obstacle_solve_ref.py (oracle operators, oracle obstacle_assembler, scipy's spsolve) and the energy errors the reference
commits in apps/obstacle/results/convergence.txt."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def asm():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    from proton_amd.batch import BatchAssembler
    return BatchAssembler(0)


def _dev(a, asm):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(asm.device)


def disc(N):
    """the cells of the N x N mesh on [-1,1]^2 whose barycentre lies in r < 0.7 (obstacle.cpp's contact region)"""
    x = -1.0 + (np.arange(N) + 0.5) * 2.0 / N
    X, Y = np.meshgrid(x, x)
    return (np.sqrt(X * X + Y * Y) < 0.7).reshape(-1)


# ---- block solve ---------------------------------------------------------------------------------------------------------
BLOCK_CASES = [(1, 1, "empty"), (1, 1, "full"), (2, 2, "empty"), (2, 2, "full"), (2, 2, "mixed"), (7, 5, 0.3), (48, 48, "disc")]


def active_set(Nx, Ny, kind):
    if kind == "empty":
        return np.zeros(Nx * Ny, dtype=bool)
    if kind == "full":
        return np.ones(Nx * Ny, dtype=bool)
    if kind == "mixed":
        return np.array([True, False, False, True])
    if kind == "disc":
        return disc(Nx)
    return np.random.default_rng(100 * Nx + Ny).random(Nx * Ny) < kind


@pytest.mark.parametrize("fd", [0, 1])
@pytest.mark.parametrize("Nx,Ny,kind", BLOCK_CASES)
def test_block_solve_equals_the_cg_on_the_extracted_block(asm, Nx, Ny, kind, fd):
    """one cell with every face Dirichlet (inactive: a 1 x 1 block; active: nk = 0), 2 x 2 with empty, full and mixed sets, 7 x 5
    with a random set, 48 x 48 with the disc (2304 cells, 11328 rows at fd = 1: beyond the 2048-entry scan tile, 708 blocks of
    the SpMV).  x[:nk], exit reason, iterations and relative residual equal pa_conjugated_gradient on K extracted on the host,
    bit for bit; every multiplier within 1e-14 (|b_i| + sum |A_ij y_j|) of its float64 host evaluation."""
    import torch
    import proton_amd as pa
    import obstacle_solve_ref as ref
    asm.generate_mesh(Nx, Ny, (-1.0, -1.0), (1.0, 1.0))
    nc = asm.ncells
    in_A_host = active_set(Nx, Ny, kind)
    lc = asm.local_ops(0, fd, pa.QUAD_TENSOR, pa.STAB_FANCY, want=("lc",))["lc"]
    rhs = asm.cell_rhs(0, pa.capi.FN_OBSTACLE_RHS, pa.QUAD_TENSOR, dinc=1)
    g = asm.dirichlet_data(fd, pa.capi.FN_OBSTACLE_SOL)
    gamma = _dev(0.1 * np.random.default_rng(Nx + fd).standard_normal(nc), asm)
    in_A = _dev(in_A_host.astype(np.uint8), asm)
    A_ct, B_ct, num_I, num_A = asm.obstacle_tables(in_A)
    rowptr, colind, values, RHS = asm.obstacle_csr_assemble(fd, lc, rhs, g, gamma, in_A, A_ct, B_ct, num_I)
    nrows = RHS.numel()
    nk = nrows - num_A
    if (Nx, Ny) == (48, 48):
        assert nk > 4096          # the kept block's SpMV partials (16 lanes a row, 256 a block) need a second trip of the one-block sum
    keep = [t.clone() for t in (rowptr, colind, values, RHS)]

    x, reason, iters, rr = asm.obstacle_block_solve(fd, rowptr, colind, values, RHS, in_A, A_ct, B_ct, num_I)
    asm.synchronize()
    assert x.shape == (nrows,)
    # in place means read in place: the system is as it was
    assert all(torch.equal(a, b) for a, b in zip(keep, (rowptr, colind, values, RHS)))

    rp, ci, va, b = (t.cpu().numpy() for t in (rowptr, colind, values, RHS))
    if nk == 0:
        assert kind == "full" and (Nx, Ny) == (1, 1)
        assert (reason, iters, rr) == (0, 0, 0.0)
    else:
        rowmap = ref.row_map(A_ct.cpu().numpy(), nc, nrows, num_I)
        krp, kci, kva, bk = ref.extract_block(rp, ci, va, b, rowmap)
        y, reason_k, iters_k, rr_k = asm.conjugated_gradient(_dev(krp, asm), _dev(kci, asm), _dev(kva, asm), _dev(bk, asm), tol=1e-13,
                                                             max_iter=20 * nk, precond=True)
        asm.synchronize()
        print("block solve %dx%d %s fd %d: nk %d of %d rows, %d iterations, relative residual %.3e" % (Nx, Ny, kind, fd, nk, nrows, iters, rr))
        assert reason_k == 0
        assert (reason, iters, rr) == (reason_k, iters_k, rr_k)
        assert torch.equal(x[:nk], y)
    xh = x.cpu().numpy()
    cols, vals, bounds = ref.multipliers(rp, ci, va, b, in_A_host, B_ct.cpu().numpy(), nk, xh[:nk])
    assert cols.shape == (num_A,) and sorted(cols.tolist()) == list(range(nk, nrows))
    if num_A:
        excess = np.abs(xh[cols] - vals) - bounds
        print("  multipliers: largest |device - host| %.3e, largest bound %.3e" % (np.abs(xh[cols] - vals).max(), bounds.max()))
        assert (excess <= 0).all()


# ---- active-set update -----------------------------------------------------------------------------------------------------
def test_active_set_update_rounds_as_the_reference_does(asm):
    """c = 0.37 on a 20 x 20 mesh, face degree 1 (400 cells, 2080 values of alpha: nine blocks, the last one partial).  Cells
    0..99 have beta = -fl(c d), d = fl(alpha - gamma): the unfused value is exactly zero (inactive) while the exact value
    beta + c d -- what a fused multiply-add rounds -- is negative for those picked here; cells 100..119 have alpha = gamma and
    beta = 0 (zero without any rounding); the rest are random.  Flags and counts equal numpy's unfused float64, the norm is
    within 1e-15 sqrt(n) relative of numpy's."""
    import torch
    fd, cpar = 1, 0.37
    asm.generate_mesh(20, 20, (-1.0, -1.0), (1.0, 1.0))
    nc = asm.ncells
    nf = asm.assembler_info(0, fd).nfaces_local
    n = nc + (fd + 1) * nf
    assert nc == 400 and n == 2080
    rng = np.random.default_rng(2024)
    gamma = rng.integers(-2 ** 20, 2 ** 20, nc) * 2.0 ** -20
    alpha = rng.standard_normal(n)
    beta = rng.standard_normal(nc)
    # d on a 2^-20 grid below 1, gamma on the same grid: alpha = gamma + d and alpha - gamma = d are exact
    picked = 0
    while picked < 100:
        d = float(rng.integers(1, 2 ** 20)) * 2.0 ** -20
        p = cpar * d
        if Fraction(cpar) * Fraction(d) < Fraction(p):           # the product was rounded up: the exact beta + c d is below zero
            alpha[picked] = gamma[picked] + d
            assert alpha[picked] - gamma[picked] == d
            beta[picked] = -p
            picked += 1
    alpha[100:120] = gamma[100:120]
    beta[100:120] = 0.0
    unfused = beta + cpar * (alpha[:nc] - gamma)
    assert (unfused[:120] == 0.0).all()
    exact = [Fraction(float(beta[i])) + Fraction(cpar) * (Fraction(float(alpha[i])) - Fraction(float(gamma[i]))) for i in range(100)]
    assert all(e < 0 for e in exact), "a fused evaluation would flag these cells"
    want = unfused < 0
    assert not want[:120].any() and 100 < want.sum() < 200

    alpha_prev = rng.standard_normal(n)
    prev = rng.random(nc) < 0.5
    d_alpha, d_beta, d_gamma, d_prev, d_flags = (_dev(a, asm) for a in (alpha, beta, gamma, alpha_prev, prev.astype(np.uint8)))
    in_A, num_A, changed, norm = asm.obstacle_active_set_update(fd, d_alpha, d_beta, d_gamma, c=cpar, alpha_prev=d_prev, in_A_prev=d_flags)
    asm.synchronize()
    got = in_A.cpu().numpy()
    assert set(np.unique(got).tolist()) <= {0, 1}
    assert np.array_equal(got.astype(bool), want)
    assert num_A == int(want.sum()) and changed == int((want != prev).sum())
    ref_norm = np.linalg.norm(alpha_prev - alpha)
    print("update: num_A %d changed %d norm %.17g (numpy %.17g)" % (num_A, changed, norm, ref_norm))
    assert abs(norm - ref_norm) <= 1e-15 * np.sqrt(n) * ref_norm
    # the first iteration: no previous alpha (zeros), no previous set (empty); and the flags updated in place
    in_A2, num_A2, changed2, norm2 = asm.obstacle_active_set_update(fd, d_alpha, d_beta, d_gamma, c=cpar)
    assert torch.equal(in_A2, in_A) and num_A2 == num_A and changed2 == num_A
    assert abs(norm2 - np.linalg.norm(alpha)) <= 1e-15 * np.sqrt(n) * np.linalg.norm(alpha)
    in_A3, num_A3, changed3, norm3 = asm.obstacle_active_set_update(fd, d_alpha, d_beta, d_gamma, c=cpar, alpha_prev=d_prev,
                                                                    in_A_prev=d_flags, in_A=d_flags)
    assert in_A3 is d_flags and torch.equal(d_flags, in_A) and (num_A3, changed3, norm3) == (num_A, changed, norm)


# ---- the whole loop ----------------------------------------------------------------------------------------------------------
LOOP_CASES = [(8, 0), (8, 1), (16, 1), (32, 1)]
HISTORY = {(8, 0): [0, 52, 52], (8, 1): [0, 44, 32, 32], (16, 1): [0, 172, 132, 120, 112, 112],
           (32, 1): [0, 716, 632, 560, 492, 436, 408, 400, 400]}
CONVERGENCE_TXT = {(8, 0): 2.26205, (8, 1): 0.197735, (16, 1): 0.0588187, (32, 1): 0.0171607}      # apps/obstacle/results/convergence.txt


def device_inputs(asm, N, k):
    import proton_amd as pa
    asm.generate_mesh(N, N, (-1.0, -1.0), (1.0, 1.0))                  # obstacle.cpp:234-238
    lc = asm.local_ops(0, k, pa.QUAD_TENSOR, pa.STAB_FANCY, want=("lc",))["lc"]
    rhs = asm.cell_rhs(0, pa.capi.FN_OBSTACLE_RHS, pa.QUAD_TENSOR, dinc=1)
    g = asm.dirichlet_data(k, pa.capi.FN_OBSTACLE_SOL)
    gamma = _dev(np.zeros(N * N), asm)                                 # obstacle_fun = 0 at the barycentres (:113)
    return lc, rhs, g, gamma


@pytest.mark.parametrize("N,k", LOOP_CASES)
def test_obstacle_solve_against_the_direct_solve_loop(asm, N, k):
    """obstacle -N N -k k in one call against the CPU loop with spsolve: the same active sets in every iteration (no decision is
    close: the smallest |diff| over all cells and iterations is 2.2e-2, 2.6e-2, 4.8e-3, 3.2e-4, nine orders above the solver
    error), the same final set, converged with a last step of exactly 0.0 (a repeated active set gives a repeated system and the
    solver is deterministic), alpha and beta within 100 x the deviation a Jacobi-CG at the same threshold shows from spsolve on
    the same systems (floor 1e-13 max|alpha|), and the energy error within 5e-6 of convergence.txt."""
    import proton_amd as pa
    import obstacle_solve_ref as ref
    cpu = ref.cpu_loop(N, k)
    assert cpu["converged"] and cpu["num_A"] == HISTORY[(N, k)]
    lc, rhs, g, gamma = device_inputs(asm, N, k)
    out = asm.obstacle_solve(k, lc, rhs, g, gamma)
    asm.synchronize()
    info = out["info"]
    alpha, beta = out["alpha"].cpu().numpy(), out["beta"].cpu().numpy()
    da, db = np.abs(alpha - cpu["alpha"]).max(), np.abs(beta - cpu["beta"]).max()
    floor = 1e-13 * np.abs(cpu["alpha"]).max()
    tol_a, tol_b = max(100 * cpu["dev_alpha"], floor), max(100 * cpu["dev_beta"], floor)
    local = asm.obstacle_take_local_data(0, k, out["alpha"])
    proj = asm.project_function(0, k, pa.capi.FN_OBSTACLE_SOL, dinc=1)
    err = float(np.sqrt(asm.energy_form(0, k, lc, local, proj).sum().item()))                 # obstacle.cpp:202-213
    print("obstacle_solve N %d k %d: num_A %s, cg iterations %s, last step %.3e; |alpha - direct| %.3e (tolerance %.3e, scipy CG %.3e), "
          "|beta - direct| %.3e (tolerance %.3e, scipy CG %.3e); error %.7g" %
          (N, k, out["num_A"], out["cg_iterations"], info.last_step_norm, da, tol_a, cpu["dev_alpha"], db, tol_b, cpu["dev_beta"], err))
    assert out["num_A"] == cpu["num_A"]
    assert np.array_equal(out["in_A"].cpu().numpy().astype(bool), cpu["in_A"])
    assert info.outer_iterations == len(cpu["num_A"]) and info.cg_iterations == sum(out["cg_iterations"])
    assert info.converged == 1 and info.cg_exit_reason == 0
    assert info.last_step_norm == 0.0
    assert da <= tol_a and db <= tol_b
    assert abs(err - CONVERGENCE_TXT[(N, k)]) / CONVERGENCE_TXT[(N, k)] < 5e-6


def test_a_cg_that_does_not_converge_ends_the_loop(asm):
    """one conjugate-gradient iteration allowed: PA_OK, converged = 0, exit reason 2 (max_iter), one system attempted, and alpha,
    beta of the last completed iteration -- the start, alpha = 0 and beta = 1 -- with the active set they give (empty)"""
    lc, rhs, g, gamma = device_inputs(asm, 8, 1)
    out = asm.obstacle_solve(1, lc, rhs, g, gamma, cg_max_iter=1)
    info = out["info"]
    assert (info.converged, info.cg_exit_reason, info.outer_iterations) == (0, 2, 1)
    assert out["num_A"] == [0] and out["cg_iterations"] == [info.cg_iterations]
    assert bool((out["alpha"] == 0.0).all()) and bool((out["beta"] == 1.0).all()) and not bool(out["in_A"].any())
    # and the iteration cap of the outer loop: two systems, not converged, the second system's active set
    out = asm.obstacle_solve(1, lc, rhs, g, gamma, max_outer=2)
    info = out["info"]
    assert (info.converged, info.cg_exit_reason, info.outer_iterations) == (0, 0, 2)
    assert out["num_A"] == HISTORY[(8, 1)][:2] and int(out["in_A"].sum()) == HISTORY[(8, 1)][1]
    assert info.last_step_norm > 1e-7


def test_refusals_touch_no_buffer(asm):
    """a slab, cell degree 1, NULL d_lc / d_alpha, max_outer = 0: status codes, and the poisoned outputs stay as they were"""
    import torch
    import proton_amd as pa
    L = pa.capi.lib()
    h = asm.ctx.h
    SA, SB, SF = 7.5, -3.25, 9
    alpha = torch.full((1024,), SA, dtype=torch.float64, device=asm.device)
    beta = torch.full((1024,), SB, dtype=torch.float64, device=asm.device)
    flags = torch.full((1024,), SF, dtype=torch.uint8, device=asm.device)
    zd = torch.zeros(64 * 81, dtype=torch.float64, device=asm.device)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    info = pa.capi.ObstacleSolveInfo(77, 77, 7.0, 7, 7)

    def call(di, lc=zd, out_alpha=alpha, max_outer=50):
        params = pa.capi.ObstacleSolveParams(max_outer=max_outer)
        return L.pa_obstacle_solve(h, di, p(lc), None, None, p(zd), C.byref(params), p(out_alpha), p(beta), p(flags), C.byref(info),
                                   None, None)

    def untouched():
        asm.synchronize()
        return bool((alpha == SA).all()) and bool((beta == SB).all()) and bool((flags == SF).all()) and \
            (info.outer_iterations, info.cg_iterations, info.last_step_norm, info.converged, info.cg_exit_reason) == (77, 77, 7.0, 7, 7)

    di, _ = pa.degree_info(0, 1)
    asm.generate_mesh(8, 8, rows=(2, 6))                        # a slab
    assert call(di) == 1 and b"whole mesh" in L.pa_last_error(h) and untouched()
    asm.generate_mesh(8, 8)
    d11, _ = pa.degree_info(1, 1)
    assert call(d11) == 2 and b"cbs = 1" in L.pa_last_error(h) and untouched()       # PA_ERR_INVALID_DEGREE
    assert call(pa.capi.DegreeInfo(7, 9, 10)) == 2 and untouched()
    assert call(di, lc=None) == 1 and untouched()               # PA_ERR_INVALID_ARG
    assert call(di, out_alpha=None) == 1 and untouched()
    assert call(di, max_outer=0) == 1 and b"max_outer" in L.pa_last_error(h) and untouched()
    # the block solve and the update refuse the same way
    x = torch.full((1024,), SA, dtype=torch.float64, device=asm.device)
    zi = torch.zeros(1024, dtype=torch.int32, device=asm.device)
    zl = torch.zeros(1024, dtype=torch.int64, device=asm.device)
    z8 = torch.zeros(1024, dtype=torch.uint8, device=asm.device)
    solve = lambda d, rowptr=zl: L.pa_obstacle_block_solve(h, d, p(rowptr), p(zi), p(zd), p(zd), p(z8), p(zi), p(zi), 64, 1e-13, 100.0, 10, 1,
                                                          p(x), None, None, None)
    update = lambda d, a=zd: L.pa_obstacle_active_set_update(h, d, 1.0, p(a), p(zd), p(zd), None, None, p(flags), None, None, None)
    assert solve(d11) == 2 and solve(di, rowptr=None) == 1 and update(d11) == 2 and update(di, a=None) == 1
    asm.generate_mesh(8, 8, rows=(2, 6))
    assert solve(di) == 1 and update(di) == 1
    asm.synchronize()
    assert bool((x == SA).all()) and untouched()
    # and the same call with nothing wrong goes through
    asm.generate_mesh(8, 8)
    assert call(di) == 0 and not untouched()
