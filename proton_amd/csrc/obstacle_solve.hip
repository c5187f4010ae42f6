// obstacle_solve.hip -- the linear solve and the active-set update of the primal-dual active set loop
// (apps/obstacle/obstacle.cpp:117-197) on the device.
//
// The system of obstacle_assembler (src/methods/hho_bits/hho.hpp:609-695) as obstacle_csr.hip builds it has rows that are not
// compacted -- cell rows at the cell index, the face rows behind them -- and compacted columns: inactive cells at [0, num_I), face
// unknowns up to nk = nrows - num_A, multipliers at [nk, nrows).  The multiplier of an active cell appears in that cell's row only,
// with coefficient 1 (hho.hpp:688-693).  So the rows of the inactive cells and of the faces against the columns below nk are the
// symmetric positive definite HHO matrix K with the active cells' values moved to the right-hand side, and every remaining row
// defines one multiplier.  The reference hands the whole system to Eigen::SparseLU (obstacle.cpp:170-175); here K goes to the
// reference's own conjugate gradient (solver.hip) and the multipliers follow from their rows.
//
// K is never formed.  Row r of K is CSR row rowmap[r]: the inverse of A_ct for r < num_I (one scatter), r + num_A for the face
// rows.  The map goes to solver.hip with the CSR arrays (CgCsr::rowmap): its two kernels that read the matrix -- inverse diagonal
// and SpMV -- are instantiated for the mapped row view (CgRowsMapped, cg.hpp), one body with the plain one, so the iterates are
// those of the solver on K extracted into arrays of its own, bit for bit.  A kept row holds no column at or beyond nk; the view's
// test keeps a system that is not obstacle_csr.hip's from reading past d.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_tmp.hpp"
#include "obstacle_solve.hpp"

namespace pa {

// rowmap[A_ct[c]] = c for the inactive cells, rowmap[r - num_A] = r for the face rows; one thread per row of the system.  A_ct is
// checked against num_I: tables that do not belong to num_I must not write outside the map.
__global__ __launch_bounds__(RB) void obstacle_rowmap_kernel(uint32_t ncells, uint64_t nrows, uint64_t num_I, const int32_t *A_ct,
                                                             int32_t *rowmap)
{
    const uint64_t t = (uint64_t)blockIdx.x * RB + threadIdx.x;
    if (t >= nrows) return;
    if (t < ncells) {
        const int32_t r = A_ct[t];
        if (r >= 0 && (uint64_t)r < num_I) rowmap[r] = (int32_t)t;
    } else {
        rowmap[t - ncells + num_I] = (int32_t)t;
    }
}

// bk[r] = RHS[rowmap[r]]: the right-hand side in K's numbering, what solver.hip's vector kernels read
__global__ __launch_bounds__(RB) void obstacle_gather_rhs_kernel(size_t n, const int32_t *rowmap, const double *RHS, double *bk)
{
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x;
    if (i < n) bk[i] = RHS[rowmap[i]];
}

// x[nk + B_ct[c]] = b_c - sum_j A_cj x_j over the columns below nk, for every active cell c: 16 lanes per cell row
__global__ __launch_bounds__(RB) void obstacle_multipliers_kernel(uint32_t ncells, uint64_t nk, uint64_t nrows, const uint8_t *in_A,
                                                                  const int32_t *B_ct, const int64_t *rowptr, const int32_t *colind,
                                                                  const double *values, const double *RHS, double *x)
{
    const uint64_t c = ((uint64_t)blockIdx.x * RB + threadIdx.x) / ROW_LANES;
    const int sub = threadIdx.x % ROW_LANES;
    const bool active = c < ncells && in_A[c] != 0;
    double s = 0.0;
    if (active)
        for (int64_t k = rowptr[c] + sub; k < rowptr[c + 1]; k += ROW_LANES) {
            const uint64_t col = (uint64_t)colind[k];
            if (col < nk) s += values[k] * x[col];
        }
#pragma unroll
    for (int o = ROW_LANES / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, ROW_LANES);
    if (active && sub == 0) {
        const int32_t m = B_ct[c];
        if (m >= 0 && nk + (uint64_t)m < nrows) x[nk + (uint64_t)m] = RHS[c] - s;
    }
}

// beta + c (alpha - gamma) with the difference, the product and the sum each rounded on its own.  Contraction is switched off
// for this expression: hipcc fuses the product and the sum into one fused multiply-add otherwise, through __dmul_rn / __dadd_rn
// as well (they are plain operators to it).
__device__ __forceinline__ double obstacle_diff(double beta, double c, double alpha, double gamma)
{
#pragma clang fp contract(off)
    const double d = alpha - gamma;
    const double p = c * d;
    return beta + p;
}

// obstacle.cpp:133-142 and the sum under the root of :193 in one pass over alpha.  Thread i < ncells forms the flag of cell i:
// the difference, the product and the sum each rounded on its own, as the reference's expression is evaluated -- a fused
// multiply-add can give the other sign where the exact value is a rounding error away from zero.
__global__ __launch_bounds__(RB) void obstacle_update_kernel(ObstacleUpdateArgs a, double *part_step, uint32_t *part_count)
{
    __shared__ double sh[RB / 64];
    const uint64_t i = (uint64_t)blockIdx.x * RB + threadIdx.x;
    double step = 0.0, active = 0.0, changed = 0.0;
    if (i < a.nalpha) {
        const double al = a.alpha[i];
        const double t = (a.alpha_prev != nullptr ? a.alpha_prev[i] : 0.0) - al;
        step = t * t;
        if (i < a.ncells) {
            const double diff = obstacle_diff(a.beta[i], a.c, al, a.gamma[i]);
            const uint8_t now = diff < 0 ? 1 : 0;
            const uint8_t before = a.in_A_prev != nullptr ? (uint8_t)(a.in_A_prev[i] != 0) : (uint8_t)0;
            a.in_A[i] = now;
            active = now;
            changed = now != before ? 1.0 : 0.0;
        }
    }
    // (the counts of a block are at most RB: exact as doubles)
    const double s0 = block_sum(step, sh), s1 = block_sum(active, sh), s2 = block_sum(changed, sh);
    if (threadIdx.x == 0) {
        part_step[blockIdx.x] = s0;
        part_count[2 * (size_t)blockIdx.x] = (uint32_t)s1;
        part_count[2 * (size_t)blockIdx.x + 1] = (uint32_t)s2;
    }
}

// one block: the partials of the update in a fixed order
__global__ __launch_bounds__(RB) void obstacle_update_reduce_kernel(size_t nparts, const double *part_step, const uint32_t *part_count,
                                                                    ObstacleUpdateResult *out)
{
    __shared__ double sh[RB / 64];
    __shared__ unsigned long long cnt[2];
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
    __syncthreads();
    double s = 0.0;
    unsigned long long na = 0, nc = 0;
    for (size_t i = threadIdx.x; i < nparts; i += RB) {
        s += part_step[i];
        na += part_count[2 * i];
        nc += part_count[2 * i + 1];
    }
    const double total = block_sum(s, sh);
    atomicAdd(&cnt[0], na);            // integers in LDS: the order does not show
    atomicAdd(&cnt[1], nc);
    __syncthreads();
    if (threadIdx.x == 0) { out->step2 = total; out->num_A = cnt[0]; out->changed = cnt[1]; }
}

__global__ __launch_bounds__(RB) void obstacle_fill_kernel(size_t n, double v, double *p)
{
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x;
    if (i < n) p[i] = v;
}

hipError_t obstacle_fill(hipStream_t stream, double *p, size_t n, double v)
{
    if (n) hipLaunchKernelGGL(obstacle_fill_kernel, dim3(blocks_for(n)), dim3(RB), 0, stream, n, v, p);
    return hipGetLastError();
}

static size_t update_blocks(size_t elements) { return elements ? (elements + RB - 1) / RB : 1; }

hipError_t obstacle_workspace_reserve(ObstacleSolveWorkspace *ws, size_t rows, size_t update_elements)
{
    obstacle_workspace_release(ws);
    const size_t nn = rows ? rows : 1, nb = update_blocks(update_elements);
    hipError_t e = cg_workspace_reserve(&ws->cg, nn, nn);
    if (e == hipSuccess) e = hipMalloc((void **)&ws->rowmap, nn * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&ws->bk, nn * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&ws->part_step, nb * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&ws->part_count, 2 * nb * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&ws->result, sizeof(ObstacleUpdateResult));
    if (e != hipSuccess) { obstacle_workspace_release(ws); return e; }
    ws->rows = nn; ws->blocks = nb;
    return hipSuccess;
}

void obstacle_workspace_release(ObstacleSolveWorkspace *ws)
{
    cg_workspace_release(&ws->cg);
    (void)hipFree(ws->rowmap); (void)hipFree(ws->bk); (void)hipFree(ws->part_step); (void)hipFree(ws->part_count);
    (void)hipFree(ws->result);
    *ws = ObstacleSolveWorkspace();
}

namespace {

// a workspace of the call's own where the caller brought none; gone with the scope, after the stream has drained
struct WorkspaceScope {
    hipStream_t stream;
    ObstacleSolveWorkspace own;
    ObstacleSolveWorkspace *ws;
    hipError_t error = hipSuccess;
    WorkspaceScope(hipStream_t s, ObstacleSolveWorkspace *given, size_t rows, size_t update_elements) : stream(s), ws(given)
    {
        if (ws == nullptr) {
            error = obstacle_workspace_reserve(&own, rows, update_elements);
            ws = &own;
        } else if (ws->rows < (rows ? rows : 1) || ws->blocks < update_blocks(update_elements)) {
            error = hipErrorInvalidValue;
        }
    }
    ~WorkspaceScope()
    {
        if (own.rows) { (void)hipStreamSynchronize(stream); obstacle_workspace_release(&own); }
    }
};

}  // namespace

hipError_t obstacle_block_solve(hipStream_t stream, const ObstacleBlockArgs &a, ObstacleSolveWorkspace *given,
                                double convergence_threshold, double divergence_threshold, size_t max_iter, int precond,
                                int *exit_reason, size_t *iterations, double *relative_residual)
{
    const uint64_t num_A = (uint64_t)a.ncells - a.num_I, nk = a.nrows - num_A;
    int reason = 0;
    size_t iters = 0;
    double rr = 0.0;
    if (nk > 0) {                                      // nk = 0: every cell active, every face Dirichlet -- nothing to solve
        WorkspaceScope scope(stream, given, (size_t)nk, 0);
        if (scope.error != hipSuccess) return scope.error;
        ObstacleSolveWorkspace *ws = scope.ws;
        hipError_t e = hipMemsetAsync(ws->rowmap, 0, (size_t)nk * sizeof(int32_t), stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(obstacle_rowmap_kernel, dim3(blocks_for((size_t)a.nrows)), dim3(RB), 0, stream, a.ncells, a.nrows, a.num_I,
                           a.A_ct, ws->rowmap);
        hipLaunchKernelGGL(obstacle_gather_rhs_kernel, dim3(blocks_for((size_t)nk)), dim3(RB), 0, stream, (size_t)nk, ws->rowmap, a.RHS,
                           ws->bk);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        e = conjugated_gradient_one_rank(stream, (size_t)nk, CgCsr{a.rowptr, a.colind, a.values, ws->rowmap}, nullptr, &ws->cg, ws->bk, a.x,
                                         convergence_threshold, divergence_threshold, max_iter, precond, &reason, &iters, &rr);
        if (e != hipSuccess) return e;
    }
    if (num_A > 0) {
        hipLaunchKernelGGL(obstacle_multipliers_kernel, dim3(blocks_for((size_t)a.ncells * ROW_LANES)), dim3(RB), 0, stream, a.ncells, nk,
                           a.nrows, a.in_A, a.B_ct, a.rowptr, a.colind, a.values, a.RHS, a.x);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const hipError_t e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return e;
    if (exit_reason) *exit_reason = reason;
    if (iterations) *iterations = iters;
    if (relative_residual) *relative_residual = rr;
    return hipSuccess;
}

hipError_t obstacle_active_set_update(hipStream_t stream, const ObstacleUpdateArgs &a, ObstacleSolveWorkspace *given,
                                      ObstacleUpdateResult *out)
{
    ObstacleUpdateResult h{0.0, 0, 0};
    if (a.nalpha > 0) {
        WorkspaceScope scope(stream, given, 0, (size_t)a.nalpha);
        if (scope.error != hipSuccess) return scope.error;
        ObstacleSolveWorkspace *ws = scope.ws;
        const size_t nb = update_blocks((size_t)a.nalpha);
        hipLaunchKernelGGL(obstacle_update_kernel, dim3((unsigned)nb), dim3(RB), 0, stream, a, ws->part_step, ws->part_count);
        hipLaunchKernelGGL(obstacle_update_reduce_kernel, dim3(1), dim3(RB), 0, stream, nb, ws->part_step, ws->part_count, ws->result);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&h, ws->result, sizeof(h), hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return e;
    }
    *out = h;
    return hipSuccess;
}

}  // namespace pa
