// cg.hpp -- what another translation unit needs to run solver.hip's conjugate gradient on a matrix it does not hold as a plain
// CSR: the two launches that read the matrix (inverse diagonal, product with the search direction) behind two callbacks, and
// the solver's device vectors as a workspace that outlives one solve.  Everything else -- the vector kernels, the reductions,
// the exit tests and their order (solver_cg.hpp:63-144) -- is solver.hip's and runs unchanged.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace pa {

constexpr int RB = 256;            // threads per block of the vector kernels
constexpr int ROW_LANES = 16;      // lanes that share a row in the SpMV (HHO rows hold 20-130 entries)

// sum of v over the block (RB threads), the same value in every thread; sh holds RB / 64 doubles
__device__ inline double block_sum(double v, double *sh)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < RB / 64; ++w) s += sh[w];
    __syncthreads();
    return s;
}

// The matrix of a solve.  inv_diag: iA[i] = 1 / A_ii, i < n, one thread per row.  spmv: y = A d and part_dy[blk] = the sum of
// d[row] y[row] over the rows of block blk, for the grid of cg_spmv_kernel -- (n ROW_LANES + RB - 1) / RB blocks of RB threads,
// ROW_LANES consecutive lanes per row, block_sum over the block -- so that the iterates do not depend on who formed the product.
struct CgMatrixOps {
    void *user;
    void (*inv_diag)(void *user, hipStream_t stream, size_t n, double *iA);
    void (*spmv)(void *user, hipStream_t stream, size_t n, const double *d, double *y, double *part_dy);
};

// The device vectors of a solve of up to `rows` unknowns.  cg_workspace_reserve leaves the workspace empty when it fails.
struct CgWorkspace {
    size_t rows = 0;
    double *r = nullptr, *d = nullptr, *y = nullptr, *iA = nullptr, *part_a = nullptr, *part_b = nullptr;
    void *scalars = nullptr;
};
hipError_t cg_workspace_reserve(CgWorkspace *ws, size_t rows);
void cg_workspace_release(CgWorkspace *ws);

// What a solver with an explicit preconditioned residual (patch_precond.hip) shares with this one: the device-resident scalars of
// the iteration, the one-block reduction of the per-block partials with the scalar algebra of the step (cg_reduce_kernel: mode 0
// after the first residual, 1 after the product, 2 after the update), and the plain CSR matrix behind CgMatrixOps (m must outlive
// the ops).
struct CgScalars { double rho, dy, nr2, rho_new, alpha, beta; };
void cg_launch_reduce(hipStream_t stream, int mode, size_t nparts, const double *part_a, const double *part_b, void *scalars);
struct CgCsr { const int64_t *rowptr; const int32_t *colind; const double *values; };
CgMatrixOps cg_csr_ops(const CgCsr *m);

// conjugated_gradient on the matrix `ops` describes.  ws: NULL = vectors of this call's own, gone on every path out; otherwise
// a workspace reserved for n rows at least, which the call leaves as it found it.
hipError_t conjugated_gradient_ops(hipStream_t stream, size_t n, const CgMatrixOps &ops, CgWorkspace *ws, const double *b, double *x,
                                   double convergence_threshold, double divergence_threshold, size_t max_iter, int precond,
                                   int *exit_reason, size_t *iterations, double *relative_residual);

// conjugated_gradient on a plain CSR matrix (solver_cg.hpp:63-144)
hipError_t conjugated_gradient(hipStream_t stream, size_t n, const int64_t *rowptr, const int32_t *colind, const double *values,
                               const double *b, double *x, double convergence_threshold, double divergence_threshold,
                               size_t max_iter, int precond, int *exit_reason, size_t *iterations, double *relative_residual);

// The transport of the row-partitioned solve (solver.hip): sums over the ranks, the two ends of the search direction's window
// from the neighbouring ranks, and what each neighbour needs of this rank's rows.
struct CgTransport {
    void *user;
    int (*allreduce_sum)(void *user, double *vals, int n);
    int (*halo)(void *user, const double *send_lo, size_t n_send_lo, const double *send_hi, size_t n_send_hi, double *recv_lo,
                size_t n_recv_lo, double *recv_hi, size_t n_recv_hi, void *stream);
    int (*neighbour_counts)(void *user, int64_t need_lo, int64_t need_hi, int64_t *give_lo, int64_t *give_hi);
};
hipError_t conjugated_gradient_rows(hipStream_t stream, const CgTransport *tp, int64_t row_begin, int64_t row_end, const int64_t *rowptr,
                                    const int32_t *colind, const double *values, const double *b, double *x,
                                    double convergence_threshold, double divergence_threshold, size_t max_iter, int precond,
                                    int *exit_reason, size_t *iterations, double *relative_residual, int *transport_status);

}  // namespace pa
