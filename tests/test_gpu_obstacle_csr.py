"""pa_obstacle_csr_assemble: obstacle_assembler's system for cell degree 0 (hho.hpp:609-695, :746-750; the cell loop of
obstacle.cpp:147-158) built directly in CSR.  The reference of every comparison is the route the project already trusts:
pa_obstacle_triplets_batch + pa_csr_from_triplets and the scatter-add of the per-row right-hand-side sums in cell order -- bit
for bit.

hho_degree_info(0, fd) exists for fd <= 1 only (utils.hpp:75-95 reverts any other pair to equal order, and pa_local_ops_batch
has no instance of it), so for fd = 2 and 3 the degree triple (0, fd, fd + 1) is handed to both routes as it is and the local
matrices are random and NOT symmetric: the assembly reads lc as data, and a transposed read shows only on such matrices."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENT_I, SENT_V, SENT_R = -7, 7.5, -3.25          # what the output buffers hold before a call


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


def direct(asm, fd, lc, rhs, g, gamma, in_A, A_ct, B_ct, num_I):
    """the raw entry on buffers of pa_assembler_csr_query's sizes that hold sentinels -> (rowptr, colind, values, RHS, nnz)"""
    import torch
    import proton_amd as pa
    from proton_amd.batch import _ptr
    di = pa.capi.DegreeInfo(0, fd, fd + 1)
    info = asm.ctx.assembler_csr_query(di)
    rowptr = torch.full((info.nrows + 1,), SENT_I, dtype=torch.int64, device=asm.device)
    colind = torch.full((max(info.nnz, 1),), SENT_I, dtype=torch.int32, device=asm.device)
    values = torch.full((max(info.nnz, 1),), SENT_V, dtype=torch.float64, device=asm.device)
    RHS = torch.full((max(info.nrows, 1),), SENT_R, dtype=torch.float64, device=asm.device)
    nnz = asm.ctx.obstacle_csr_assemble(di, lc.data_ptr(), _ptr(rhs), _ptr(g), gamma.data_ptr(), in_A.data_ptr(), A_ct.data_ptr(),
                                        B_ct.data_ptr(), num_I, rowptr.data_ptr(), colind.data_ptr(), values.data_ptr(), RHS.data_ptr())
    return rowptr, colind, values, RHS[:info.nrows], nnz


def triplet_route(asm, fd, lc, rhs, g, gamma, in_A, A_ct, B_ct, num_I, nrows):
    """-> (rowptr, colind, values) of pa_csr_from_triplets(pa_obstacle_triplets_batch), RHS = np.add.at in cell order"""
    import torch
    import proton_amd as pa
    from proton_amd.batch import _ptr
    n, ms = lc.shape[0], lc.shape[1]
    i32, f64 = dict(dtype=torch.int32, device=asm.device), dict(dtype=torch.float64, device=asm.device)
    r, c, v = torch.empty((n, ms * ms + 1), **i32), torch.empty((n, ms * ms + 1), **i32), torch.empty((n, ms * ms + 1), **f64)
    rr, rv = torch.empty((n, ms), **i32), torch.empty((n, ms), **f64)
    asm.ctx.obstacle_triplets(pa.capi.DegreeInfo(0, fd, fd + 1), 0, n, lc.data_ptr(), _ptr(rhs), _ptr(g), gamma.data_ptr(),
                              in_A.data_ptr(), A_ct.data_ptr(), B_ct.data_ptr(), num_I, r.data_ptr(), c.data_ptr(), v.data_ptr(),
                              rr.data_ptr(), rv.data_ptr())
    rp, ci, va = asm.csr_from_triplets(r, c, v, nrows)
    asm.synchronize()
    rr, rv = rr.cpu().numpy().reshape(-1), rv.cpu().numpy().reshape(-1)          # cell-major: cell order
    RHS = np.zeros(nrows)
    ok = rr >= 0
    np.add.at(RHS, rr[ok], rv[ok])
    return rp, ci, va, RHS


def check_against_the_triplet_route(asm, fd, in_A_host, is_dir, cell_faces, seed):
    """every assertion of the issue for the mesh the context holds"""
    import torch
    import proton_amd as pa
    fbs = fd + 1
    nc = asm.ncells
    assert in_A_host.shape == (nc,)
    ms = 1 + 4 * fbs
    if fd <= 1:
        lc = asm.local_ops(0, fd, pa.QUAD_TENSOR, pa.STAB_FANCY, want=("lc",))["lc"]
        assert tuple(lc.shape) == (nc, ms, ms)
    else:
        lc = _dev(np.random.default_rng(seed + 77).standard_normal((nc, ms, ms)), asm)
    rhs = asm.cell_rhs(0, pa.capi.FN_OBSTACLE_RHS, pa.QUAD_TENSOR, dinc=1)
    g = asm.dirichlet_data(fd, pa.capi.FN_OBSTACLE_SOL)
    gamma = _dev(np.random.default_rng(seed).standard_normal(nc), asm)
    in_A = _dev(in_A_host.astype(np.uint8), asm)
    A_ct, B_ct, num_I, num_A = asm.obstacle_tables(in_A)
    info = asm.ctx.assembler_csr_query(pa.capi.DegreeInfo(0, fd, fd + 1))
    assert info.nrows == nc + fbs * int((is_dir == 0).sum())

    for use_rhs_g in (True, False):
        a_rhs, a_g = (rhs, g) if use_rhs_g else (None, None)
        rp, ci, va, RHS_ref = triplet_route(asm, fd, lc, a_rhs, a_g, gamma, in_A, A_ct, B_ct, num_I, info.nrows)
        rowptr, colind, values, RHS, nnz = direct(asm, fd, lc, a_rhs, a_g, gamma, in_A, A_ct, B_ct, num_I)
        asm.synchronize()
        # the stored count: the comparator's, and the plain system's minus fbs per (non-Dirichlet face, active adjacent cell)
        count = int((in_A_host.astype(bool)[:, None] & (is_dir[cell_faces.astype(np.int64)] == 0)).sum())
        assert nnz == ci.numel() == va.numel()
        assert nnz == info.nnz - fbs * count
        assert torch.equal(rowptr, rp)
        assert torch.equal(colind[:nnz], ci)
        assert torch.equal(values[:nnz], va)
        assert np.array_equal(RHS.cpu().numpy(), RHS_ref)
        # nothing at or beyond nnz is written
        assert bool((colind[nnz:] == SENT_I).all()) and bool((values[nnz:] == SENT_V).all())
        if use_rhs_g:
            # a second call, through the public method: identical arrays
            rowptr2, colind2, values2, RHS2 = asm.obstacle_csr_assemble(fd, lc, rhs, g, gamma, in_A, A_ct, B_ct, num_I)
            asm.synchronize()
            assert colind2.numel() == nnz and values2.numel() == nnz
            assert torch.equal(rowptr2, rowptr) and torch.equal(colind2, colind[:nnz]) and torch.equal(values2, values[:nnz])
            assert torch.equal(RHS2, RHS)


def disc(N):
    """the cells of the N x N mesh on [-1,1]^2 whose barycentre lies in r < 0.7 (obstacle.cpp's contact region)"""
    x = -1.0 + (np.arange(N) + 0.5) * 2.0 / N
    X, Y = np.meshgrid(x, x)
    return (np.sqrt(X * X + Y * Y) < 0.7).reshape(-1)


CASES = [(1, 1, 1, 0.0), (1, 1, 1, 1.0), (2, 2, 0, 0.5), (3, 2, 1, 0.5), (7, 7, 1, 0.4), (5, 5, 2, 0.3), (4, 4, 3, 0.5),
         (9, 9, 1, 0.0), (9, 9, 1, 1.0), (48, 48, 1, 0.3), (9, 9, 1, "disc")]


@pytest.mark.parametrize("Nx,Ny,fd,p", CASES)
def test_obstacle_csr_equals_the_triplet_route(asm, oracle, Nx, Ny, fd, p):
    """one cell with every face Dirichlet (one row, one entry), empty and full active sets, every face degree, 48 x 48 beyond the
    2048-entry scan tile in cells (2304) and rows (11328), and a contiguous active region (face rows with both cells active)"""
    asm.generate_mesh(Nx, Ny, (-1.0, -1.0), (1.0, 1.0))
    mp, points, ptids = oracle.make_mesh(Nx, Ny, (-1.0, -1.0), (1.0, 1.0))
    ref = oracle.Assembler(mp, points, ptids, oracle.degrees(0, fd))
    if p == "disc":
        in_A = disc(Nx)
        both = in_A[:-1] & in_A[1:]
        assert both.any()
    else:
        in_A = np.random.default_rng(1000 * Nx + 10 * fd + int(10 * p)).random(Nx * Ny) < p
    check_against_the_triplet_route(asm, fd, in_A, ref.is_dir, ref.cell_faces, seed=Nx + fd)


@pytest.mark.parametrize("open_left", [False, True])
def test_uploaded_general_quadrilateral_mesh(asm, oracle, open_left):
    """the perturbed 6 x 6 mesh of general quadrilaterals with explicit face tables of tests/test_gpu_assembler_fused.py; with the
    left boundary's faces not Dirichlet there are face rows with a single cell"""
    N, fd = 6, 1
    mp, points, ptids = oracle.make_mesh(N, N)
    rng = np.random.default_rng(5)
    ij = np.arange(points.shape[0])
    i, j = ij % (N + 1), ij // (N + 1)
    interior = (i > 0) & (i < N) & (j > 0) & (j < N)
    points[interior] += rng.uniform(-0.1 / N, 0.1 / N, size=points.shape)[interior]
    ref = oracle.Assembler(mp, points, ptids, oracle.degrees(0, fd))
    is_dir = ref.is_dir.copy()
    if open_left:
        left = (points[ref.faces[:, 0].astype(np.int64), 0] == 0.0) & (points[ref.faces[:, 1].astype(np.int64), 0] == 0.0)
        assert left.sum() == N and is_dir[left].all()
        is_dir[left] = 0
    asm.set_mesh(points, ptids)
    asm.set_faces(ref.cell_faces, ref.faces, is_dir)
    assert asm.assembler_info(0, fd).num_other_faces == int((is_dir == 0).sum())
    in_A = np.random.default_rng(17).random(N * N) < 0.4
    check_against_the_triplet_route(asm, fd, in_A, is_dir, ref.cell_faces, seed=3)


class DirectObstacleAssembler:
    """The shape tests/obstacle_driver.run_obstacle expects; assemble_all is the new entry, its CSR expanded to COO."""

    def __init__(self, asm, msh, di, in_A):
        self.asm, self.di = asm, di
        self.nf = msh.nfaces
        self.in_A = _dev(in_A.astype(np.uint8), asm)
        self.A_ct, self.B_ct, self.num_I, self.num_A = asm.obstacle_tables(self.in_A)
        self.system_size = asm.assembler_info(0, di.face_deg).system_size

    def assemble_all(self, lc_unused, rhs_unused, gamma):
        a = self.asm
        self.gamma = _dev(gamma, a)
        rowptr, colind, values, RHS = a.obstacle_csr_assemble(self.di.face_deg, a._lc, a._rhs, a._g, self.gamma, self.in_A, self.A_ct,
                                                              self.B_ct, self.num_I)
        a.synchronize()
        rp = rowptr.cpu().numpy()
        assert rp.shape == (self.system_size + 1,)
        rows = np.repeat(np.arange(self.system_size), np.diff(rp))
        return rows, colind.cpu().numpy(), values.cpu().numpy(), RHS.cpu().numpy()

    def expand_solution(self, sol, gamma):
        a = self.asm
        alpha, beta = a.obstacle_expand_solution(0, self.di.face_deg, _dev(sol, a), a._g, self.gamma, self.in_A, self.A_ct, self.B_ct,
                                                 self.num_I, self.nf)
        self._alpha, self._local = alpha, None
        return alpha.cpu().numpy(), beta.cpu().numpy()

    def take_local_data(self, c, alpha_host):
        if self._local is None:
            self._local = self.asm.obstacle_take_local_data(0, self.di.face_deg, self._alpha).cpu().numpy()
        return self._local[c]


def test_obstacle_end_to_end_with_the_direct_csr(asm):
    """obstacle -N 16 -k 1 (apps/obstacle/results/convergence.txt: 0.0588187) with the system of every active-set iteration from
    pa_obstacle_csr_assemble: the bounds of tests/test_gpu_obstacle.py's end-to-end test"""
    import obstacle_driver as od
    import proton_amd as pa
    from proton_amd.batch import to_rowcol

    def gpu_provider(msh, deg):
        asm.generate_mesh(msh.N, msh.N, (-1.0, -1.0), (1.0, 1.0))       # obstacle.cpp:234-238
        asm._lc = asm.local_ops(0, deg, pa.QUAD_TENSOR, pa.STAB_FANCY, want=("lc",))["lc"]
        asm._rhs = asm.cell_rhs(0, pa.capi.FN_OBSTACLE_RHS, pa.QUAD_TENSOR, dinc=1)
        asm._g = asm.dirichlet_data(deg, pa.capi.FN_OBSTACLE_SOL)
        asm.synchronize()
        return to_rowcol(asm._lc), asm._rhs.cpu().numpy()

    err, iters = od.run_obstacle(16, 1, local_provider=gpu_provider,
                                 assembler_factory=lambda msh, di, in_A: DirectObstacleAssembler(asm, msh, di, in_A))
    print("obstacle N 16 k 1 with the direct CSR: error %.7g after %d iterations" % (err, iters))
    assert iters < 50
    assert abs(err - 0.0588187) / 0.0588187 < 5e-6


def test_refusals_touch_no_buffer(asm):
    """a slab, cell degree 1, a degree triple outside the tables, NULL d_lc / d_in_A / nnz: status codes, before anything is
    written"""
    import torch
    import proton_amd as pa
    L = pa.capi.lib()
    h = asm.ctx.h
    M = 8192
    rowptr = torch.full((M,), SENT_I, dtype=torch.int64, device=asm.device)
    colind = torch.full((M,), SENT_I, dtype=torch.int32, device=asm.device)
    values = torch.full((M,), SENT_V, dtype=torch.float64, device=asm.device)
    RHS = torch.full((M,), SENT_R, dtype=torch.float64, device=asm.device)
    zd = torch.zeros(64 * 81, dtype=torch.float64, device=asm.device)
    z8 = torch.zeros(64, dtype=torch.uint8, device=asm.device)
    zi = torch.zeros(64, dtype=torch.int32, device=asm.device)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    nnz = C.c_size_t(12345)

    def call(di, lc=zd, in_A=z8, nnz_ref=C.byref(nnz)):
        return L.pa_obstacle_csr_assemble(h, di, p(lc), None, None, p(zd), p(in_A), p(zi), p(zi), 64, p(rowptr), p(colind), p(values),
                                          p(RHS), nnz_ref)

    def untouched():
        asm.synchronize()
        return bool((rowptr == SENT_I).all()) and bool((colind == SENT_I).all()) and bool((values == SENT_V).all()) and \
            bool((RHS == SENT_R).all()) and nnz.value == 12345

    di, _ = pa.degree_info(0, 1)
    asm.generate_mesh(8, 8, rows=(2, 6))                        # a slab
    assert call(di) == 1 and b"whole mesh" in L.pa_last_error(h) and untouched()
    asm.generate_mesh(8, 8)
    d11, _ = pa.degree_info(1, 1)
    assert call(d11) == 2 and b"cbs = 1" in L.pa_last_error(h) and untouched()       # PA_ERR_INVALID_DEGREE
    assert call(pa.capi.DegreeInfo(7, 9, 10)) == 2 and untouched()
    assert call(di, lc=None) == 1 and untouched()               # PA_ERR_INVALID_ARG
    assert call(di, in_A=None) == 1 and untouched()
    assert call(di, nnz_ref=None) == 1 and untouched()
    assert call(di) == 0 and not untouched()                    # and the same call with nothing wrong goes through
