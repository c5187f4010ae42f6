// cg.hpp -- the conjugate gradient of solver.hip as its other translation units see it.  The six kernels of the iteration
// (inverse diagonal, product with the search direction, first residual, update, new direction, reduction of the block partials)
// are stated once, in solver.hip, as templates over the small device-side structs declared here: where a row of the matrix is
// stored and how a column finds its place in the vector (CgRows*), how the preconditioned residual is had (CgJacobi, CgStoredZ),
// and where the scalar of a step comes from (CgStep).  Two host loops launch them: the one-rank loop (conjugated_gradient_one_rank:
// one host read per iteration) and the row-partitioned loop (conjugated_gradient_rows: the sums go over the ranks).  The exit tests
// and their order are solver_cg.hpp:63-144's in both.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace pa {

constexpr int RB = 256;            // threads per block of the vector kernels
constexpr int ROW_LANES = 16;      // lanes that share a row in the SpMV (HHO rows hold 20-130 entries)

// the two grids of the solver: one thread per row, ROW_LANES lanes per row
inline unsigned cg_vector_grid(size_t n) { return (unsigned)((n + RB - 1) / RB); }
inline unsigned cg_row_grid(size_t n) { return (unsigned)((n * ROW_LANES + RB - 1) / RB); }

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

// ---- row views: the matrix kernels ask a view where row r of the system is stored, whether entry (r, c) is the diagonal's, whether
// column c is read at all, where it is in the vector, and where the row's own entry of the vector is.
// plain: the CSR arrays are the system
struct CgRowsPlain {
    __device__ int64_t storage(size_t r) const { return (int64_t)r; }
    __device__ bool diagonal(int32_t c, size_t r) const { return (size_t)c == r; }
    __device__ bool reads(int32_t, size_t) const { return true; }
    __device__ double at(const double *d, int32_t c) const { return d[c]; }
    __device__ double own(const double *d, size_t r) const { return d[r]; }
};
// window: rows [row_begin, row_begin + n) of a larger system with global column indices; the vector is a window that starts at
// column col0 and holds the rows' own entries from own0 on
struct CgRowsWindow {
    int64_t row_begin, col0;
    size_t own0;
    __device__ int64_t storage(size_t r) const { return (int64_t)r; }
    __device__ bool diagonal(int32_t c, size_t r) const { return (int64_t)c == row_begin + (int64_t)r; }
    __device__ bool reads(int32_t, size_t) const { return true; }
    __device__ double at(const double *d, int32_t c) const { return d[(int64_t)c - col0]; }
    __device__ double own(const double *d, size_t r) const { return d[own0 + r]; }
};
// mapped: row r is CSR row rowmap[r], and the columns at n and beyond are not the system's
struct CgRowsMapped {
    const int32_t *rowmap;
    __device__ int64_t storage(size_t r) const { return rowmap[r]; }
    __device__ bool diagonal(int32_t c, size_t r) const { return (size_t)c == r; }
    __device__ bool reads(int32_t c, size_t n) const { return (size_t)c < n; }
    __device__ double at(const double *d, int32_t c) const { return d[(size_t)c]; }
    __device__ double own(const double *d, size_t r) const { return d[r]; }
};

// ---- the preconditioned residual z = M^-1 r of the vector kernels
// Jacobi or none: z_i = iA_i r_i or r_i, formed where it is used
struct CgJacobi {
    static constexpr bool stored = false;
    const double *iA;
    int precond;
    __device__ double z(size_t i, double ri) const { return precond ? iA[i] * ri : ri; }
};
// a vector somebody else wrote, with the partials of r . z: the first residual and the update form no r . z and leave d alone;
// first: the direction is z itself
struct CgStoredZ {
    static constexpr bool stored = true;
    const double *zv;
    int first;
    __device__ double z(size_t i, double) const { return zv[i]; }
};

// the scalar of a step (alpha of the update, beta of the direction): on the device where the reduction left it, or by value
struct CgStep {
    const double *on_device;
    double value;
    __device__ double get() const { return on_device ? *on_device : value; }
};

// The matrix of a one-rank solve: CSR arrays, and rowmap = NULL (the arrays are the system) or the storage row of every row of
// the system (CgRowsMapped).
struct CgCsr { const int64_t *rowptr; const int32_t *colind; const double *values; const int32_t *rowmap; };

// The scalars of the iteration, resident on the device, and the modes of cg_reduce_kernel that fill them (solver.hip).
struct CgScalars { double rho, dy, nr2, rho_new, alpha, beta; };

// The device vectors of a solve of up to `rows` unknowns, with d_len >= rows entries for the search direction (the row-partitioned
// solve keeps a window there).  cg_workspace_reserve leaves the workspace empty when it fails.
struct CgWorkspace {
    size_t rows = 0;
    double *r = nullptr, *d = nullptr, *y = nullptr, *iA = nullptr, *part_a = nullptr, *part_b = nullptr;
    CgScalars *scalars = nullptr;
};
hipError_t cg_workspace_reserve(CgWorkspace *ws, size_t rows, size_t d_len);
void cg_workspace_release(CgWorkspace *ws);

// A preconditioner with an explicit z: apply writes z = M^-1 r and the block partials of r . z (cg_vector_grid(n) of them, in the
// blocks of the vector kernels) on the stream.  z holds n doubles and is the caller's.
struct CgPreconditioner {
    void *user;
    void (*apply)(void *user, hipStream_t stream, const double *r, double *z, double *part_rz);
    double *z;
};

// conjugated_gradient on one rank.  pre: NULL = Jacobi (precond != 0) or none, fused into the vector kernels; otherwise z comes from
// pre->apply and precond is not read.  ws: NULL = vectors of this call's own, gone on every path out; otherwise a workspace
// reserved for n rows at least, which the call leaves as it found it.
hipError_t conjugated_gradient_one_rank(hipStream_t stream, size_t n, const CgCsr &m, const CgPreconditioner *pre, CgWorkspace *ws,
                                        const double *b, double *x, double convergence_threshold, double divergence_threshold,
                                        size_t max_iter, int precond, int *exit_reason, size_t *iterations, double *relative_residual);

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

// ---- a preconditioner with an explicit z for the row-partitioned loop (rows_precond.hip states the one there is).
// What a rank knows once the counts have been exchanged: its rows, and the window of columns they read.
struct CgRowsSystem {
    const CgTransport *tp;                 // null: one rank
    int64_t row_begin, row_end, need_lo, need_hi, give_lo, give_hi;
    const int64_t *rowptr;
    const int32_t *colind;
    const double *values;
};
// This rank's status (those of conjugated_gradient_rows, and 5: a table of this rank was refused, 6: a patch of this rank or the
// coarse matrix is not positive definite), with the HIP error behind status 4.
struct CgRowsFail {
    int status = 0;
    hipError_t herr = hipSuccess;
    bool hip_ok(hipError_t e) { if (e != hipSuccess && !status) { status = 4; herr = e; } return e == hipSuccess; }
};
// prepare: the local part of the set-up (tables judged, patches factored), no collective inside; a failure goes to *fail.
// setup:   the collective part, entered by every rank after all of them have prepared; -> 0, or the status every rank leaves with.
// apply:   z = M^-1 r and the block partials of r . z; may sum over the ranks, the flag of *fail behind the sum; -> as setup.
// z: n doubles of the caller's.
struct CgRowsPreconditioner {
    void *user;
    void (*prepare)(void *user, hipStream_t stream, const CgRowsSystem &s, CgRowsFail *fail);
    int (*setup)(void *user, hipStream_t stream, const CgRowsSystem &s, CgRowsFail *fail);
    int (*apply)(void *user, hipStream_t stream, const CgRowsSystem &s, const double *r, double *z, double *part_rz, CgRowsFail *fail);
    double *z;
};
// The loop of conjugated_gradient_rows with z from pre: the recurrences, exit tests and exit order of the one-rank loop with a
// CgPreconditioner, three sums over the ranks per iteration (d . y, whatever pre->apply sums, (r . r, r . z)).  The iterate lives
// in the workspace and reaches x only with status 0: on every other exit x is untouched.
hipError_t conjugated_gradient_rows_stored(hipStream_t stream, const CgTransport *tp, int64_t row_begin, int64_t row_end,
                                           const int64_t *rowptr, const int32_t *colind, const double *values,
                                           const CgRowsPreconditioner *pre, const double *b, double *x, double convergence_threshold,
                                           double divergence_threshold, size_t max_iter, int *exit_reason, size_t *iterations,
                                           double *relative_residual, int *transport_status);

}  // namespace pa
