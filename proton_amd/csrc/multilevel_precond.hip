// multilevel_precond.hip -- a smoothed coarse level for the device conjugate gradient (solver_cg.hpp:63-144 with
//   z = sum_p R_p^T (R_p A R_p^T)^-1 R_p r + sum_l P_l diag(P_l^T A P_l)^-1 P_l^T r + P_c (P_c^T A P_c)^-1 P_c^T r
// where the reference multiplies by 1 / diag(A); the solve of cuthho_square.cpp:915-919 on the face-only system): the additive
// multilevel form on the nested hat spaces of coarse_precond.hip's table builders.  A smoothed level keeps P^T and one double per
// column: no dense matrix, no bound of 4096 columns, no triangular product.
//   set-up: the table is validated with coarse_precond.hip's kernels (one thread per row).  P^T: every entry q of P gets the key
//           (column << bits | q), the keys are sorted by rocPRIM's radix sort -- all different, so the order is the only one there
//           is: a column's entries by fine row ascending, in a time linear in the entries whatever the columns' lengths --, the
//           row pointer is the scan of the validation's counts.  d_j = sum_i P_ij (sum_k A_ik P_kj): the lanes of a column take its
//           entries, walk row i of A in its entry order and look column j up in row k of P (at most 4 entries).
//   apply:  u = D^-1 P^T r (a column per wavefront or per quarter wavefront), z += P u (a gather of at most 4 terms per row).
//   sums:   entry e of a column goes to slot e mod 64, a slot adds its entries in ascending order with fused multiply-adds, the 64
//           slots are added by the xor tree 32 .. 1.  A wavefront holds a slot per lane; a quarter wavefront holds the slots l, l + 16,
//           l + 32, l + 48 in lane l and takes the tree's steps 32 and 16 inside the lane -- the same additions, the same bits.  No
//           floating-point atomics anywhere.
//   fused:  multilevel_prolong_kernel adds the gathers of up to 9 tables onto the patch sum in one pass over z and leaves the block
//           partials of r . z; rows_precond.hip states the order of the calls.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <cmath>
#include <cstdint>

#include "cg.hpp"
#include "multilevel_precond.hpp"

namespace pa {

namespace {

constexpr int NFLAGS = 4, FLAG_COLUMN = 2;     // (flag 0: the validation's refusal, coarse_precond.hip)
constexpr uint32_t NO_COLUMN = 0xffffffffu;

inline size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }

inline unsigned bits_for(uint64_t count)       // bits that hold 0 .. count - 1, at least one
{
    unsigned b = 1;
    while (b < 63 && ((uint64_t)1 << b) < count) ++b;
    return b;
}

// the parts of the scratch buffer: the coarse vector of an apply in front
struct Scratch {
    double *vec;           // ncoarse: D^-1 P^T r
    int32_t *flags;        // NFLAGS
    uint32_t *counts;      // ncoarse + 2: entries per column
    double *dinv;          // ncoarse: 1 / d_j until every column has passed
    int32_t *erow;         // entries: the fine row of entry q
    uint64_t *keys;        // entries: (column << bits | q)
    uint64_t *sorted;      // entries
    char *work;            // the sort's and the scan's temporaries
};
inline Scratch scratch_parts(void *base, size_t nc, size_t entries, size_t work_bytes, size_t *bytes)
{
    char *p = (char *)base;
    Scratch s;
    s.vec = (double *)p; p += round256(nc * 8);
    s.flags = (int32_t *)p; p += round256(NFLAGS * 4);
    s.counts = (uint32_t *)p; p += round256((nc + 2) * 4);
    s.dinv = (double *)p; p += round256(nc * 8);
    s.erow = (int32_t *)p; p += round256(entries * 4);
    s.keys = (uint64_t *)p; p += round256(entries * 8);
    s.sorted = (uint64_t *)p; p += round256(entries * 8);
    s.work = p; p += round256(work_bytes);
    if (bytes) *bytes = (size_t)(p - (char *)base);
    return s;
}

// P^T in one buffer
struct Transpose { uint32_t *ptr; int32_t *rows; double *vals; };
inline Transpose pt_parts(const void *base, size_t nc, size_t entries, size_t *bytes)
{
    char *p = (char *)base;
    Transpose t;
    t.ptr = (uint32_t *)p; p += round256((nc + 1) * 4);
    t.rows = (int32_t *)p; p += round256(entries * 4);
    t.vals = (double *)p; p += round256(entries * 8);
    if (bytes) *bytes = (size_t)(p - (char *)base);
    return t;
}

// the temporaries of the two rocPRIM calls of a set-up (asked with a null buffer: nothing is launched)
hipError_t work_bytes(hipStream_t stream, size_t nc, size_t entries, size_t *bytes)
{
    size_t scan = 0, sort = 0;
    hipError_t e = rocprim::exclusive_scan(nullptr, scan, (const uint32_t *)nullptr, (uint32_t *)nullptr, 0u, nc + 1, rocprim::plus<uint32_t>(),
                                           stream);
    if (e == hipSuccess && entries)
        e = rocprim::radix_sort_keys(nullptr, sort, (const uint64_t *)nullptr, (uint64_t *)nullptr, entries, 0u,
                                     bits_for(entries) + bits_for(nc), stream);
    *bytes = scan > sort ? scan : sort;
    return e;
}

// ---- P^T ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RB) void smoothed_keys_kernel(size_t n, unsigned qbits, const int64_t *ptr, const int32_t *cols, int32_t *erow,
                                                           uint64_t *keys)
{
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x;
    if (i >= n) return;
    for (int64_t q = ptr[i]; q < ptr[i + 1]; ++q) {
        erow[q] = (int32_t)i;
        keys[q] = ((uint64_t)(uint32_t)cols[q] << qbits) | (uint64_t)q;
    }
}

__global__ __launch_bounds__(RB) void smoothed_gather_kernel(size_t entries, unsigned qbits, const uint64_t *sorted, const int32_t *erow,
                                                             const double *vals, int32_t *pt_rows, double *pt_vals)
{
    const size_t s = (size_t)blockIdx.x * RB + threadIdx.x;
    if (s >= entries) return;
    const uint64_t q = sorted[s] & (((uint64_t)1 << qbits) - 1);
    pt_rows[s] = erow[q];
    pt_vals[s] = vals[q];
}

// ---- a column's sum: S = 64 / G slots in every one of the G lanes that share the column ------------------------------------------------
template <int G>
__device__ __forceinline__ double column_tree(const double *a)
{
    double s;
    if constexpr (G == 64) {
        s = a[0];
        s += __shfl_xor(s, 32, 64);
        s += __shfl_xor(s, 16, 64);
    } else {
        static_assert(G == 16, "a wavefront or a quarter of one");
        s = (a[0] + a[2]) + (a[1] + a[3]);               // steps 32 and 16 of the tree: slots l | l + 32 and l + 16 | l + 48
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

// u_j = dinv_j * (row j of P^T) . r
template <int G>
__global__ __launch_bounds__(RB) void smoothed_restrict_kernel(uint32_t nc, const uint32_t *pt_ptr, const int32_t *pt_rows,
                                                               const double *pt_vals, const double *dinv, const double *r, double *u)
{
    constexpr int S = 64 / G;
    const uint32_t j = blockIdx.x * (RB / G) + threadIdx.x / G, l = threadIdx.x % G;
    double a[S];
#pragma unroll
    for (int k = 0; k < S; ++k) a[k] = 0.0;
    if (j < nc) {
        const uint32_t p1 = pt_ptr[j + 1];
        for (uint32_t base = pt_ptr[j]; base < p1; base += 64) {
#pragma unroll
            for (int k = 0; k < S; ++k) {
                const uint32_t e = base + k * G + l;
                if (e < p1) a[k] = fma(pt_vals[e], r[pt_rows[e]], a[k]);
            }
        }
    }
    const double tot = column_tree<G>(a);
    if (j < nc && l == 0) u[j] = dinv[j] * tot;
}

// d_j = sum over the entries (i, P_ij) of column j of P_ij * t, t = sum over row i of A in entry order of A_ik P_kj; dinv_j = 1 / d_j,
// and the smallest j + 1 whose d_j is no positive finite number goes to *bad
template <int G>
__global__ __launch_bounds__(RB) void smoothed_diagonal_kernel(size_t n, uint32_t nc, const int64_t *rowptr, const int32_t *colind,
                                                               const double *values, const int64_t *ptr, const int32_t *cols,
                                                               const double *vals, const uint32_t *pt_ptr, const int32_t *pt_rows,
                                                               const double *pt_vals, double *dinv, uint32_t *bad)
{
    constexpr int S = 64 / G;
    const uint32_t j = blockIdx.x * (RB / G) + threadIdx.x / G, l = threadIdx.x % G;
    double a[S];
#pragma unroll
    for (int k = 0; k < S; ++k) a[k] = 0.0;
    if (j < nc) {
        const uint32_t p1 = pt_ptr[j + 1];
        for (uint32_t base = pt_ptr[j]; base < p1; base += 64) {
#pragma unroll
            for (int k = 0; k < S; ++k) {
                const uint32_t e = base + k * G + l;
                if (e >= p1) continue;
                const size_t i = (size_t)pt_rows[e];
                double t = 0.0;
                for (int64_t m = rowptr[i]; m < rowptr[i + 1]; ++m) {
                    const int32_t c = colind[m];
                    if (c < 0 || (size_t)c >= n) continue;          // (not a column of the system: P has no row for it)
                    for (int64_t q = ptr[c]; q < ptr[c + 1]; ++q)
                        if ((uint32_t)cols[q] == j) t = fma(values[m], vals[q], t);
                }
                a[k] = fma(pt_vals[e], t, a[k]);
            }
        }
    }
    const double d = column_tree<G>(a);
    if (j < nc && l == 0) {
        const bool good = d > 0.0 && isfinite(d);
        dinv[j] = good ? 1.0 / d : 0.0;
        if (!good) atomicMin(bad, j + 1);
    }
}

// z_i = (accumulate ? z_i : 0) + the gathers of the tables in their order, every term onto the running sum; the block partials of r . z
__global__ __launch_bounds__(RB) void multilevel_prolong_kernel(size_t n, ProlongTables t, int accumulate, const double *r, double *z,
                                                                double *part_rz)
{
    __shared__ double sh[RB / 64];
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x;
    double rz = 0.0;
    if (i < n) {
        double s = accumulate ? z[i] : 0.0;
        for (int k = 0; k < t.count; ++k) {
            const int64_t q1 = t.ptr[k][i + 1];
            for (int64_t q = t.ptr[k][i]; q < q1; ++q) s = fma(t.vals[k][q], t.u[k][t.cols[k][q]], s);
        }
        z[i] = s;
        rz = r[i] * s;
    }
    const double tot = block_sum(rz, sh);
    if (part_rz != nullptr && threadIdx.x == 0) part_rz[blockIdx.x] = tot;
}

}  // namespace

// ---- host ---------------------------------------------------------------------------------------------------------------------------
hipError_t smoothed_query(hipStream_t stream, size_t n, size_t ncoarse, const int64_t *ptr, SmoothedSizes *out, int *refusal)
{
    *out = SmoothedSizes();
    uint64_t entries = 0;
    hipError_t e = coarse_check_ptr(stream, n, ncoarse, SMOOTHED_MAX_NODES, ptr, &entries, refusal);
    if (e != hipSuccess || *refusal) return e;
    size_t bytes = 0, work = 0;
    e = work_bytes(stream, ncoarse, (size_t)entries, &work);
    if (e != hipSuccess) return e;
    out->entries = entries;
    pt_parts(nullptr, ncoarse, (size_t)entries, &bytes);
    out->pt_bytes = bytes;
    out->dinv_doubles = ncoarse;
    out->work_bytes = work;
    scratch_parts(nullptr, ncoarse, (size_t)entries, work, &bytes);
    out->scratch_bytes = bytes;
    out->lanes = entries <= 32 * (uint64_t)ncoarse ? 16 : 64;           // a mean column of up to 32 entries: four columns a wavefront
    return hipSuccess;
}

hipError_t smoothed_validate(hipStream_t stream, const CoarseTable &t, const SmoothedSizes &sz, void *scratch, int *refusal)
{
    const Scratch s = scratch_parts(scratch, t.ncoarse, (size_t)sz.entries, (size_t)sz.work_bytes, nullptr);
    return coarse_check_rows(stream, t, s.counts, s.flags, refusal);
}

// (the counts of smoothed_validate are still in the scratch: the two are called back to back)
hipError_t smoothed_setup(hipStream_t stream, const int64_t *rowptr, const int32_t *colind, const double *values, const CoarseTable &t,
                          const SmoothedSizes &sz, void *pt, double *dinv, void *scratch, int32_t *column)
{
    *column = 0;
    const uint32_t nc = (uint32_t)t.ncoarse;
    const size_t entries = (size_t)sz.entries;
    const Scratch s = scratch_parts(scratch, nc, entries, (size_t)sz.work_bytes, nullptr);
    const Transpose tr = pt_parts(pt, nc, entries, nullptr);
    const unsigned qbits = bits_for(entries);
    size_t work = (size_t)sz.work_bytes;
    // P^T
    hipError_t e = rocprim::exclusive_scan(s.work, work, (const uint32_t *)s.counts, tr.ptr, 0u, (size_t)nc + 1, rocprim::plus<uint32_t>(), stream);
    if (e != hipSuccess) return e;
    if (entries) {
        hipLaunchKernelGGL(smoothed_keys_kernel, dim3(cg_vector_grid(t.n)), dim3(RB), 0, stream, t.n, qbits, t.ptr, t.cols, s.erow, s.keys);
        work = (size_t)sz.work_bytes;
        e = rocprim::radix_sort_keys(s.work, work, (const uint64_t *)s.keys, s.sorted, entries, 0u, qbits + bits_for(nc), stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(smoothed_gather_kernel, dim3(cg_vector_grid(entries)), dim3(RB), 0, stream, entries, qbits, s.sorted, s.erow, t.vals,
                           tr.rows, tr.vals);
    }
    // D
    uint32_t *bad = (uint32_t *)(s.flags + FLAG_COLUMN);
    e = hipMemsetAsync(bad, 0xff, 4, stream);
    if (e != hipSuccess) return e;
    if (sz.lanes == 16)
        hipLaunchKernelGGL((smoothed_diagonal_kernel<16>), dim3((nc + RB / 16 - 1) / (RB / 16)), dim3(RB), 0, stream, t.n, nc, rowptr, colind,
                           values, t.ptr, t.cols, t.vals, tr.ptr, tr.rows, tr.vals, s.dinv, bad);
    else
        hipLaunchKernelGGL((smoothed_diagonal_kernel<64>), dim3((nc + RB / 64 - 1) / (RB / 64)), dim3(RB), 0, stream, t.n, nc, rowptr, colind,
                           values, t.ptr, t.cols, t.vals, tr.ptr, tr.rows, tr.vals, s.dinv, bad);
    uint32_t h = NO_COLUMN;
    e = hipMemcpyAsync(&h, bad, 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (h != NO_COLUMN) { *column = (int32_t)h; return hipSuccess; }
    e = hipMemcpyAsync(dinv, s.dinv, (size_t)nc * 8, hipMemcpyDeviceToDevice, stream);
    return e == hipSuccess ? hipStreamSynchronize(stream) : e;
}

const double *smoothed_restrict(hipStream_t stream, const CoarseTable &t, const SmoothedSizes &sz, const void *pt, const double *dinv,
                                void *scratch, const double *r)
{
    const uint32_t nc = (uint32_t)t.ncoarse;
    const Scratch s = scratch_parts(scratch, nc, (size_t)sz.entries, (size_t)sz.work_bytes, nullptr);
    const Transpose tr = pt_parts(pt, nc, (size_t)sz.entries, nullptr);
    if (sz.lanes == 16)
        hipLaunchKernelGGL((smoothed_restrict_kernel<16>), dim3((nc + RB / 16 - 1) / (RB / 16)), dim3(RB), 0, stream, nc, tr.ptr, tr.rows, tr.vals,
                           dinv, r, s.vec);
    else
        hipLaunchKernelGGL((smoothed_restrict_kernel<64>), dim3((nc + RB / 64 - 1) / (RB / 64)), dim3(RB), 0, stream, nc, tr.ptr, tr.rows, tr.vals,
                           dinv, r, s.vec);
    return s.vec;
}

void smoothed_apply(hipStream_t stream, const CoarseTable &t, const SmoothedSizes &sz, const void *pt, const double *dinv, void *scratch,
                    int accumulate, const double *r, double *z, double *part_rz)
{
    if (t.n == 0) return;
    ProlongTables tb{};
    tb.count = 1;
    tb.ptr[0] = t.ptr; tb.cols[0] = t.cols; tb.vals[0] = t.vals;
    tb.u[0] = smoothed_restrict(stream, t, sz, pt, dinv, scratch, r);
    hipLaunchKernelGGL(multilevel_prolong_kernel, dim3(cg_vector_grid(t.n)), dim3(RB), 0, stream, t.n, tb, accumulate, r, z, part_rz);
}

void multilevel_prolong(hipStream_t stream, size_t n, const ProlongTables &tables, const double *r, double *z, double *part_rz)
{
    if (n) hipLaunchKernelGGL(multilevel_prolong_kernel, dim3(cg_vector_grid(n)), dim3(RB), 0, stream, n, tables, 1, r, z, part_rz);
}

}  // namespace pa
