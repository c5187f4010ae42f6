// solver.hip -- the reference's Jacobi-preconditioned conjugate gradient
// (src/core/core_bits/solver_cg.hpp:63-144, used by run_cuthho_interface cuthho_square.cpp:1737-1743
// and offered by convergence_test) on the device, over the CSR matrix pa_csr_from_triplets builds.
// Same recurrences, exit tests and exit order as the reference; the dot products are block-tree
// reductions (deterministic run to run), not Eigen's sequential sums.
//
// Every kernel of the iteration is stated here, once, as a template over the structs of cg.hpp.  The plain matrix, the obstacle
// problem's matrix behind its row map, the rows of one rank of a partitioned matrix, the Jacobi residual formed in place and the
// patch preconditioner's stored one are instantiations of these bodies: the same statements in the same order, so that the
// iterates of two solvers on the same system are the same bits by construction.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cg.hpp"
#include "device_tmp.hpp"

namespace pa {

// iA = 1 / diag(A)   (solver_cg.hpp:77-80)
template <class Rows>
__global__ __launch_bounds__(RB) void cg_inv_diag_kernel(size_t n, Rows rows, const int64_t *rowptr, const int32_t *colind,
                                                         const double *values, double *iA)
{
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x;
    if (i >= n) return;
    const int64_t R = rows.storage(i);
    double d = 0.0;
    for (int64_t k = rowptr[R]; k < rowptr[R + 1]; ++k)
        if (rows.diagonal(colind[k], i)) d = values[k];
    iA[i] = 1.0 / d;
}

// y = A d and the per-block partial of d . y: ROW_LANES consecutive lanes per row, lane l taking entries l, l + ROW_LANES, ... of the
// row, a butterfly over the lanes of the row, block_sum over the rows of the block
template <class Rows>
__global__ __launch_bounds__(RB) void cg_spmv_kernel(size_t n, Rows rows, const int64_t *rowptr, const int32_t *colind,
                                                     const double *values, const double *d, double *y, double *part_dy)
{
    __shared__ double sh[RB / 64];
    const size_t row = ((size_t)blockIdx.x * RB + threadIdx.x) / ROW_LANES;
    const int sub = threadIdx.x % ROW_LANES;
    double s = 0.0;
    if (row < n) {
        const int64_t R = rows.storage(row);
        for (int64_t k = rowptr[R] + sub; k < rowptr[R + 1]; k += ROW_LANES) {
            const int32_t c = colind[k];
            if (rows.reads(c, n)) s += values[k] * rows.at(d, c);
        }
    }
#pragma unroll
    for (int o = ROW_LANES / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, ROW_LANES);
    double dyp = 0.0;
    if (row < n && sub == 0) { y[row] = s; dyp = rows.own(d, row) * s; }
    const double t = block_sum(dyp, sh);
    if (threadIdx.x == 0) part_dy[blockIdx.x] = t;
}

// r = b - y (first residual, x = 0 means y = 0 is never formed: r = b), partials of r.r; Jacobi: d = M^-1 r and partials of r.M^-1 r
template <class Pre>
__global__ __launch_bounds__(RB) void cg_init_kernel(size_t n, const double *b, Pre pre, double *x, double *r, double *d, double *part_a,
                                                     double *part_b)
{
    __shared__ double sh[RB / 64];
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x;
    double rr = 0.0, rz = 0.0;
    if (i < n) {
        const double ri = b[i];
        x[i] = 0.0; r[i] = ri;
        rr = ri * ri;
        if constexpr (!Pre::stored) {
            const double zi = pre.z(i, ri);
            d[i] = zi;
            rz = ri * zi;
        }
    }
    const double t0 = block_sum(rr, sh);
    if constexpr (!Pre::stored) {
        const double t1 = block_sum(rz, sh);
        if (threadIdx.x == 0) part_b[blockIdx.x] = t1;
    }
    if (threadIdx.x == 0) part_a[blockIdx.x] = t0;
}

// x += alpha d, r -= alpha y; partials of r.r; Jacobi: and of r.M^-1 r   (solver_cg.hpp:103-109, 126-127)
template <class Pre>
__global__ __launch_bounds__(RB) void cg_update_kernel(size_t n, CgStep step, Pre pre, const double *d, const double *y, double *x,
                                                       double *r, double *part_a, double *part_b)
{
    __shared__ double sh[RB / 64];
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x;
    const double alpha = step.get();
    double rr = 0.0, rz = 0.0;
    if (i < n) {
        x[i] += alpha * d[i];
        const double ri = r[i] - alpha * y[i];
        r[i] = ri;
        rr = ri * ri;
        if constexpr (!Pre::stored) rz = ri * pre.z(i, ri);
    }
    const double t0 = block_sum(rr, sh);
    if constexpr (!Pre::stored) {
        const double t1 = block_sum(rz, sh);
        if (threadIdx.x == 0) part_b[blockIdx.x] = t1;
    }
    if (threadIdx.x == 0) part_a[blockIdx.x] = t0;
}

// d = M^-1 r + beta d   (solver_cg.hpp:128)
template <class Pre>
__global__ __launch_bounds__(RB) void cg_direction_kernel(size_t n, CgStep step, Pre pre, const double *r, double *d)
{
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x;
    if (i >= n) return;
    if constexpr (Pre::stored) d[i] = pre.first ? pre.z(i, 0.0) : pre.z(i, 0.0) + step.get() * d[i];
    else d[i] = pre.z(i, r[i]) + step.get() * d[i];
}

// one block: sums up to two arrays of per-block partials, then the scalar algebra of the step
//   mode 0 (after init):   rho = sum(b) [r.M^-1 r], nr2 = sum(a)
//   mode 1 (after spmv):   dy = sum(a); alpha = rho / dy
//   mode 2 (after update): nr2 = sum(a), rho_new = sum(b); beta = rho_new / rho; rho = rho_new
//   mode 3 (the sums go over the ranks before anything is formed of them): the two sums of mode 2 -- nr2, rho_new -- and no algebra
enum { CG_SUMS_ONLY = 3 };
__global__ __launch_bounds__(RB) void cg_reduce_kernel(int mode, size_t nparts, const double *part_a, const double *part_b, CgScalars *sc)
{
    __shared__ double sh[RB / 64];
    double a = 0.0, b = 0.0;
    for (size_t i = threadIdx.x; i < nparts; i += RB) {
        a += part_a[i];
        if (part_b) b += part_b[i];
    }
    const double sa = block_sum(a, sh), sb = block_sum(b, sh);
    if (threadIdx.x == 0) {
        if (mode == 0) { sc->nr2 = sa; sc->rho = sb; }
        else if (mode == 1) { sc->dy = sa; sc->alpha = sc->rho / sa; }
        else {
            sc->nr2 = sa; sc->rho_new = sb;
            if (mode == 2) { sc->beta = sb / sc->rho; sc->rho = sb; }
        }
    }
}

namespace {

template <class Rows>
void launch_inv_diag(hipStream_t stream, size_t n, Rows rows, const int64_t *rowptr, const int32_t *colind, const double *values, double *iA)
{
    hipLaunchKernelGGL(cg_inv_diag_kernel<Rows>, dim3(cg_vector_grid(n)), dim3(RB), 0, stream, n, rows, rowptr, colind, values, iA);
}

template <class Rows>
void launch_spmv(hipStream_t stream, size_t n, Rows rows, const int64_t *rowptr, const int32_t *colind, const double *values, const double *d,
                 double *y, double *part_dy)
{
    hipLaunchKernelGGL(cg_spmv_kernel<Rows>, dim3(cg_row_grid(n)), dim3(RB), 0, stream, n, rows, rowptr, colind, values, d, y, part_dy);
}

void launch_reduce(hipStream_t stream, int mode, size_t nparts, const double *part_a, const double *part_b, CgScalars *sc)
{
    hipLaunchKernelGGL(cg_reduce_kernel, dim3(1), dim3(RB), 0, stream, mode, nparts, part_a, part_b, sc);
}

// the vector kernels of one solve: its grid, its vectors, and the preconditioned residual they are instantiated for
struct VectorKernels {
    hipStream_t stream;
    size_t n;
    unsigned gv;
    double *x, *r, *d, *y, *part_a, *part_b;
    template <class Pre> void init(const double *b, Pre pre) const
    {
        hipLaunchKernelGGL(cg_init_kernel<Pre>, dim3(gv), dim3(RB), 0, stream, n, b, pre, x, r, d, part_a, part_b);
    }
    template <class Pre> void update(CgStep alpha, Pre pre) const
    {
        hipLaunchKernelGGL(cg_update_kernel<Pre>, dim3(gv), dim3(RB), 0, stream, n, alpha, pre, (const double *)d, (const double *)y, x, r,
                           part_a, part_b);
    }
    template <class Pre> void direction(CgStep beta, Pre pre) const
    {
        hipLaunchKernelGGL(cg_direction_kernel<Pre>, dim3(gv), dim3(RB), 0, stream, n, beta, pre, (const double *)r, d);
    }
};

}  // namespace

hipError_t cg_workspace_reserve(CgWorkspace *ws, size_t rows, size_t d_len)
{
    cg_workspace_release(ws);
    const size_t nn = rows ? rows : 1;
    const size_t gv = cg_vector_grid(nn), gs = cg_row_grid(nn);
    const size_t nparts = gs > gv ? gs : gv;
    hipError_t e = hipMalloc((void **)&ws->r, nn * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&ws->d, (d_len > nn ? d_len : nn) * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&ws->y, nn * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&ws->iA, nn * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&ws->part_a, nparts * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&ws->part_b, nparts * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&ws->scalars, sizeof(CgScalars));
    if (e != hipSuccess) { cg_workspace_release(ws); return e; }
    ws->rows = nn;
    return hipSuccess;
}

void cg_workspace_release(CgWorkspace *ws)
{
    (void)hipFree(ws->r); (void)hipFree(ws->d); (void)hipFree(ws->y); (void)hipFree(ws->iA); (void)hipFree(ws->part_a);
    (void)hipFree(ws->part_b); (void)hipFree(ws->scalars);
    *ws = CgWorkspace();
}

// The one-rank loop on the vectors of ws.  Per iteration: product, reduction 1, update, [pre->apply,] reduction 2, one read of the
// scalars by the host, the exit tests, direction.  exit_reason: 0 converged, 1 diverged, 2 max_iter reached (cg_exit_reason,
// solver_cg.hpp:38-43)
static hipError_t cg_iterate(hipStream_t stream, size_t n, const CgCsr &m, const CgPreconditioner *pre, const CgWorkspace &ws, const double *b,
                             double *x, double convergence_threshold, double divergence_threshold, size_t max_iter, int precond,
                             int *exit_reason, size_t *iterations, double *relative_residual)
{
    const size_t gv = cg_vector_grid(n), gs = cg_row_grid(n);
    const VectorKernels k{stream, n, (unsigned)gv, x, ws.r, ws.d, ws.y, ws.part_a, ws.part_b};
    const CgJacobi jacobi{ws.iA, precond};
    CgScalars *sc = ws.scalars;
    const CgStep alpha{&sc->alpha, 0.0}, beta{&sc->beta, 0.0};
    CgScalars h{};
    auto read_scalars = [&]() -> hipError_t {
        const hipError_t e = hipMemcpyAsync(&h, sc, sizeof(h), hipMemcpyDeviceToHost, stream);
        return e != hipSuccess ? e : hipStreamSynchronize(stream);
    };
    hipError_t e = hipSuccess;
    size_t iter = 0;
    int reason = 2;
    double rr = 0.0;
    if (n) {
        if (pre) {
            k.init(b, CgStoredZ{pre->z, 0});                                                                               // :73-84
            pre->apply(pre->user, stream, ws.r, pre->z, ws.part_b);
            k.direction(beta, CgStoredZ{pre->z, 1});
        } else {
            if (m.rowmap) launch_inv_diag(stream, n, CgRowsMapped{m.rowmap}, m.rowptr, m.colind, m.values, ws.iA);
            else launch_inv_diag(stream, n, CgRowsPlain{}, m.rowptr, m.colind, m.values, ws.iA);
            k.init(b, jacobi);                                                                                             // :82-84
        }
        launch_reduce(stream, 0, gv, ws.part_a, ws.part_b, sc);
        if ((e = read_scalars()) != hipSuccess) return e;
        const double nr0 = sqrt(h.nr2);
        if (!(nr0 > 0.0)) { reason = 0; }                   // b = 0: x = 0 is the solution (the reference would divide by zero)
        else
            for (;;) {
                if (m.rowmap) launch_spmv(stream, n, CgRowsMapped{m.rowmap}, m.rowptr, m.colind, m.values, ws.d, ws.y, ws.part_a);
                else launch_spmv(stream, n, CgRowsPlain{}, m.rowptr, m.colind, m.values, ws.d, ws.y, ws.part_a);           // :99
                launch_reduce(stream, 1, gs, ws.part_a, nullptr, sc);                                                      // :101-102
                if (pre) {
                    k.update(alpha, CgStoredZ{pre->z, 0});                                                                 // :103-105
                    pre->apply(pre->user, stream, ws.r, pre->z, ws.part_b);
                } else k.update(alpha, jacobi);
                launch_reduce(stream, 2, gv, ws.part_a, ws.part_b, sc);
                if ((e = read_scalars()) != hipSuccess) return e;
                rr = sqrt(h.nr2) / nr0;
                if (rr < convergence_threshold) { reason = 0; break; }      // :107-110
                if (iter > max_iter) { reason = 2; break; }                  // :112-115
                if (rr > divergence_threshold) { reason = 1; break; }        // :117-120
                if (!(rr == rr)) { reason = 1; break; }                      // NaN: stop instead of spinning
                if (pre) k.direction(beta, CgStoredZ{pre->z, 0});                                                          // :126-128
                else k.direction(beta, jacobi);
                iter++;
            }
    } else reason = 0;
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (exit_reason) *exit_reason = reason;
    if (iterations) *iterations = iter;
    if (relative_residual) *relative_residual = rr;
    return hipSuccess;
}

hipError_t conjugated_gradient_one_rank(hipStream_t stream, size_t n, const CgCsr &m, const CgPreconditioner *pre, CgWorkspace *ws,
                                        const double *b, double *x, double convergence_threshold, double divergence_threshold,
                                        size_t max_iter, int precond, int *exit_reason, size_t *iterations, double *relative_residual)
{
    const size_t nn = n ? n : 1;
    CgWorkspace own;
    if (ws != nullptr && ws->rows < nn) return hipErrorInvalidValue;
    if (ws == nullptr) {
        const hipError_t e = cg_workspace_reserve(&own, nn, nn);
        if (e != hipSuccess) return e;
        ws = &own;
    }
    const hipError_t e = cg_iterate(stream, n, m, pre, *ws, b, x, convergence_threshold, divergence_threshold, max_iter, precond, exit_reason,
                                    iterations, relative_residual);
    cg_workspace_release(&own);
    return e;
}

hipError_t conjugated_gradient(hipStream_t stream, size_t n, const int64_t *rowptr, const int32_t *colind, const double *values,
                               const double *b, double *x, double convergence_threshold, double divergence_threshold,
                               size_t max_iter, int precond, int *exit_reason, size_t *iterations, double *relative_residual)
{
    return conjugated_gradient_one_rank(stream, n, CgCsr{rowptr, colind, values, nullptr}, nullptr, nullptr, b, x, convergence_threshold,
                                        divergence_threshold, max_iter, precond, exit_reason, iterations, relative_residual);
}

// ---- the same solver on a ROW-PARTITIONED system (several GPUs: the face-only condensed system is assembled by rows,
// pa_condensed_csr_fill; every rank solves where it assembled).  This rank holds rows [row_begin, row_end) of the global
// matrix in CSR with GLOBAL column indices.  The search direction lives in a window  [row_begin - need_lo, row_end + need_hi)
// -- the columns this rank's rows read; the matrix is symmetric and banded by the mesh's row structure, so they belong to the
// two neighbouring ranks -- whose two ends are refreshed from the neighbours once per iteration; the dot products are local
// partial sums added over the ranks.  The transport is three callbacks (RCCL: pa_comm_cg_transport; host-staged gloo in the
// tests: CgTransport, cg.hpp).  The kernels are the one-rank loop's with the window view (CgRowsWindow) and the scalars of a
// step by value; the loop is its own -- two host reads per iteration, because the sums go over the ranks before alpha and beta
// are formed of them, and a collective exit -- and without a transport it forms what the one-rank loop forms, in the same order.

// smallest and largest column index of the local rows (one block per 256 entries, atomics on two words)
__global__ __launch_bounds__(RB) void cg_col_range_kernel(size_t nnz, const int32_t *colind, int *minmax)
{
    const size_t k = (size_t)blockIdx.x * RB + threadIdx.x;
    if (k >= nnz) return;
    atomicMin(&minmax[0], colind[k]);
    atomicMax(&minmax[1], colind[k]);
}

// status: 0 ok; 1 a transport callback failed on THIS rank; 2 this rank's rows read a column no neighbour range covers (or, without a
// transport, beyond its own range); 3 another rank failed (its status says why); 4 a HIP error on this rank; 5, 6: what a
// preconditioner says of its tables (CgRowsFail, cg.hpp).
// EVERY exit is collective: a rank that fails locally -- a callback, a HIP call, the range check -- does not leave the others inside a
// reduction or a neighbour exchange.  Its failure is a flag that rides on the next all-reduce (an extra addend behind the dot products),
// every rank sees the sum and all of them leave together, at the same point.  (What cannot be covered: the all-reduce itself failing
// on one rank only -- then there is nothing left to tell the others with.)
// pre: null = Jacobi (precond != 0) or none, formed in the vector kernels; otherwise z comes from pre->apply, precond is not read, and
// the iterate lives in a vector of the call's own until the solve has ended well.
static hipError_t cg_rows_iterate(hipStream_t stream, const CgTransport *tp, int64_t row_begin, int64_t row_end, const int64_t *rowptr,
                                  const int32_t *colind, const double *values, const CgRowsPreconditioner *pre, const double *b, double *x,
                                  double convergence_threshold, double divergence_threshold, size_t max_iter, int precond,
                                  int *exit_reason, size_t *iterations, double *relative_residual, int *transport_status)
{
    const size_t n = (size_t)(row_end - row_begin);
    const size_t nn = n ? n : 1;
    const size_t gv = cg_vector_grid(nn), gs = cg_row_grid(nn);
    CgWorkspace ws;
    DeviceTmp tmp(stream);
    int *mm = nullptr;
    if (transport_status) *transport_status = 0;
    CgRowsFail failure;
    int &fail = failure.status;            // this rank's status (see above); 0 while everything went well
    hipError_t &herr = failure.herr;
    auto hip_ok = [&](hipError_t e) -> bool { return failure.hip_ok(e); };
    auto leave = [&](int status) -> hipError_t {
        if (transport_status) *transport_status = status;
        cg_workspace_release(&ws);
        return status == 4 ? herr : hipSuccess;
    };
    // all ranks agree on whether anybody failed: the flag summed over the ranks (one rank: the flag itself)
    auto agree = [&]() -> int {
        double f = fail ? 1.0 : 0.0;
        if (tp && tp->allreduce_sum(tp->user, &f, 1) != 0) return fail ? fail : 1;
        return f > 0.0 ? (fail ? fail : 3) : 0;
    };
    // the columns the local rows read
    int64_t need_lo = 0, need_hi = 0;
    {
        int64_t nnz = 0;
        if (n) {
            int64_t ends[2] = {0, 0};
            if (hip_ok(hipMemcpyAsync(&ends[0], rowptr, 8, hipMemcpyDeviceToHost, stream)) &&
                hip_ok(hipMemcpyAsync(&ends[1], rowptr + n, 8, hipMemcpyDeviceToHost, stream)) && hip_ok(hipStreamSynchronize(stream)))
                nnz = ends[1] - ends[0];
        }
        int h[2] = {0x7fffffff, -1};
        if (!fail && (tmp.alloc(&mm, 2) || hip_ok(tmp.error())) && hip_ok(hipMemcpyAsync(mm, h, 8, hipMemcpyHostToDevice, stream))) {
            if (nnz > 0) hipLaunchKernelGGL(cg_col_range_kernel, dim3((unsigned)((nnz + RB - 1) / RB)), dim3(RB), 0, stream, (size_t)nnz, colind, mm);
            if (hip_ok(hipMemcpyAsync(h, mm, 8, hipMemcpyDeviceToHost, stream)) && hip_ok(hipStreamSynchronize(stream)) && nnz > 0) {
                need_lo = h[0] < row_begin ? row_begin - h[0] : 0;
                need_hi = (int64_t)h[1] + 1 > row_end ? (int64_t)h[1] + 1 - row_end : 0;
            }
        }
    }
    int64_t give_lo = 0, give_hi = 0;      // what the neighbours below / above read of MY range (its first / last entries)
    if (tp) {
        // (a rank that already failed still answers its neighbours -- with what it needs, zero -- so that they are not left waiting)
        if (tp->neighbour_counts(tp->user, fail ? 0 : need_lo, fail ? 0 : need_hi, &give_lo, &give_hi) != 0 && !fail) fail = 1;
    } else if (need_lo || need_hi) fail = 2;
    if (!fail && (give_lo > (int64_t)n || give_hi > (int64_t)n)) fail = 2;
    const size_t nwin = n + (size_t)need_lo + (size_t)need_hi;
    if (!fail) (void)(hip_ok(cg_workspace_reserve(&ws, nn, nwin)) && hip_ok(hipMemsetAsync(ws.d, 0, (nwin ? nwin : 1) * 8, stream)));
    const CgRowsSystem sys{tp, row_begin, row_end, need_lo, need_hi, give_lo, give_hi, rowptr, colind, values};
    double *xw = x;                        // where the iterate lives
    if (pre) {
        if (!fail && !tmp.alloc(&xw, nn)) hip_ok(tmp.error());
        if (!fail) pre->prepare(pre->user, stream, sys, &failure);
    }
    {
        const int st = agree();            // nobody starts iterating unless everybody can
        if (st) return leave(st);
    }
    if (pre) {
        const int st = pre->setup(pre->user, stream, sys, &failure);
        if (st) return leave(st);
    }
    double *dwin = ws.d, *d = dwin + need_lo;            // the window, and its owned part
    const VectorKernels k{stream, n, (unsigned)gv, xw, ws.r, d, ws.y, ws.part_a, ws.part_b};
    const CgJacobi jacobi{ws.iA, precond};
    const CgRowsWindow rows{row_begin, row_begin - need_lo, (size_t)need_lo};
    double hs[3];
    // local sums -> host -> ranks, the failure flag behind them.  Returns 0, or the status all ranks leave with.
    auto reduce2 = [&](size_t np, const double *pb2, int nvals) -> int {
        hs[0] = hs[1] = 0.0;
        if (!fail) {
            launch_reduce(stream, CG_SUMS_ONLY, np, ws.part_a, pb2, ws.scalars);
            (void)(hip_ok(hipMemcpyAsync(hs, &ws.scalars->nr2, 16, hipMemcpyDeviceToHost, stream)) && hip_ok(hipStreamSynchronize(stream)));
        }
        hs[nvals] = fail ? 1.0 : 0.0;
        if (tp && tp->allreduce_sum(tp->user, hs, nvals + 1) != 0) return fail ? fail : 1;
        return hs[nvals] > 0.0 ? (fail ? fail : 3) : 0;
    };
    auto refresh = [&]() {                 // the two ends of the window from the neighbours, my ends to them
        if (!tp || fail) return;           // (a failed rank does not post: it tells the others at the reduction that follows the product)
        if (tp->halo(tp->user, d, (size_t)give_lo, d + (n - (size_t)give_hi), (size_t)give_hi, dwin, (size_t)need_lo, d + n, (size_t)need_hi,
                     (void *)stream) != 0)
            fail = 1;
    };
    size_t iter = 0;
    int reason = 2;
    double rr = 0.0;
    {
        int st = 0;
        if (pre) {
            k.init(b, CgStoredZ{pre->z, 0});                                                                         // :73-84
            st = pre->apply(pre->user, stream, sys, ws.r, pre->z, ws.part_b, &failure);
            if (st) return leave(st);
            k.direction(CgStep{nullptr, 0.0}, CgStoredZ{pre->z, 1});
        } else {
            if (n) launch_inv_diag(stream, n, rows, rowptr, colind, values, ws.iA);
            k.init(b, jacobi);             // r = b, d = M^-1 r (x = 0), partials of r.r and r.M^-1 r       solver_cg.hpp:73-84
        }
        st = reduce2(gv, ws.part_b, 2);
        if (st) return leave(st);
        const double nr0 = sqrt(hs[0]);
        double rho = hs[1];
        if (!(nr0 > 0.0)) { reason = 0; }
        else
            for (;;) {
                refresh();
                if (!fail) launch_spmv(stream, n, rows, rowptr, colind, values, dwin, ws.y, ws.part_a);              // :99
                st = reduce2(gs, nullptr, 1);
                if (st) return leave(st);
                const double alpha = rho / hs[0];                                                                    // :101-102
                if (pre) {
                    k.update(CgStep{nullptr, alpha}, CgStoredZ{pre->z, 0});                                          // :103-105
                    st = pre->apply(pre->user, stream, sys, ws.r, pre->z, ws.part_b, &failure);
                    if (st) return leave(st);
                } else k.update(CgStep{nullptr, alpha}, jacobi);
                st = reduce2(gv, ws.part_b, 2);
                if (st) return leave(st);
                rr = sqrt(hs[0]) / nr0;
                if (rr < convergence_threshold) { reason = 0; break; }      // :107-110
                if (iter > max_iter) { reason = 2; break; }                  // :112-115
                if (rr > divergence_threshold) { reason = 1; break; }        // :117-120
                if (!(rr == rr)) { reason = 1; break; }
                const double beta = hs[1] / rho;
                rho = hs[1];
                if (pre) k.direction(CgStep{nullptr, beta}, CgStoredZ{pre->z, 0});                                   // :126-128
                else k.direction(CgStep{nullptr, beta}, jacobi);
                iter++;
            }
    }
    (void)(hip_ok(hipGetLastError()) && hip_ok(hipStreamSynchronize(stream)));
    {
        const int st = agree();            // a rank whose last launches failed says so before anybody reports success
        if (st) return leave(st);
    }
    // (the solve has ended on every rank: a copy that fails here leaves nobody waiting)
    if (pre && n && !(hip_ok(hipMemcpyAsync(x, xw, n * 8, hipMemcpyDeviceToDevice, stream)) && hip_ok(hipStreamSynchronize(stream))))
        return leave(4);
    if (exit_reason) *exit_reason = reason;
    if (iterations) *iterations = iter;
    if (relative_residual) *relative_residual = rr;
    return leave(0);
}

hipError_t conjugated_gradient_rows(hipStream_t stream, const CgTransport *tp, int64_t row_begin, int64_t row_end, const int64_t *rowptr,
                                    const int32_t *colind, const double *values, const double *b, double *x,
                                    double convergence_threshold, double divergence_threshold, size_t max_iter, int precond,
                                    int *exit_reason, size_t *iterations, double *relative_residual, int *transport_status)
{
    return cg_rows_iterate(stream, tp, row_begin, row_end, rowptr, colind, values, nullptr, b, x, convergence_threshold, divergence_threshold,
                           max_iter, precond, exit_reason, iterations, relative_residual, transport_status);
}

hipError_t conjugated_gradient_rows_stored(hipStream_t stream, const CgTransport *tp, int64_t row_begin, int64_t row_end,
                                           const int64_t *rowptr, const int32_t *colind, const double *values,
                                           const CgRowsPreconditioner *pre, const double *b, double *x, double convergence_threshold,
                                           double divergence_threshold, size_t max_iter, int *exit_reason, size_t *iterations,
                                           double *relative_residual, int *transport_status)
{
    return cg_rows_iterate(stream, tp, row_begin, row_end, rowptr, colind, values, pre, b, x, convergence_threshold, divergence_threshold,
                           max_iter, 0, exit_reason, iterations, relative_residual, transport_status);
}

}  // namespace pa
