// patch_precond.hip -- an additive Schwarz preconditioner over patches of rows for the device conjugate gradient
// (solver_cg.hpp:63-144 with  z = sum_p R_p^T (R_p A R_p^T)^-1 R_p r  where the reference multiplies by 1 / diag(A); the solve of
// cuthho_square.cpp:915-919 on the face-only system), and the patch tables of that system: one patch per face, or per cell; for the
// interface problem's system (the solve of cuthho_square.cpp:1737-1743) one per face with all its blocks, or per cell side.
//
// A patch holds 1..16 rows.  P = 4, 8 or 16 consecutive lanes share a patch (the smallest P that holds the table's largest patch),
// lane l owning row l: a 16-row patch fills a quarter of a wavefront, four patches a wavefront, and everything the lanes of a patch
// exchange goes through __shfl of width P -- no LDS, no barrier, no divergence (a patch of m < P rows is padded by identity rows).
//   factor: lane l gathers row l of A_p from the CSR arrays (binary search: columns are ascending), the group runs a right-looking
//           Cholesky on the rows in registers, then lane l forms column l of W = L^-1 by forward substitution and stores it into the
//           packed lower triangle of W (row i at i (i + 1) / 2).
//   apply:  t = W r_p (lane l reads row l of W), z_p = W^T t (lane l reads column l): two triangular products without a dependent
//           chain, symmetric by construction.  z_p goes to a patch-major buffer (slot = position in patch_rows); a second kernel
//           sums each row's slots in ascending order (= ascending patch order) and forms the block partials of r . z.  No
//           floating-point atomics: z is the same bits from call to call.
//   solve:  not here: rows_precond.hip calls patch_query, patch_factor and patch_apply in their order for every solver (TwoLevel).
//   tables: the closed-form ones (a patch per face; per cell of a loaded mesh from its cprefix), and one builder for the tables that
//           have to be counted first (item_patches: a count kernel, the scans of scan.hpp, a fill kernel), instantiated for the cells
//           of a slab of the generator mesh (SlabCellItems) and for the faces or cell sides of the interface problem, whole or by
//           slab (IfItems).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "cg.hpp"
#include "device_tmp.hpp"
#include "interface_csr.hpp"
#include "patch_precond.hpp"
#include "scan.hpp"
#include "structured_mesh.hpp"

namespace pa {

namespace {

constexpr int FLAG_REFUSAL = 0, FLAG_MAX_ROWS = 1, FLAG_FAILED = 2, NFLAGS = 4;

inline size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }

// the parts of the scratch buffer
struct Scratch {
    double *zbuf;          // entries: the patches' results, patch-major
    uint32_t *counts;      // n + 1: patches per row, then the fill cursor
    uint32_t *blk;         // row blocks + 1: their totals, scanned
    int32_t *flags;        // NFLAGS
};
inline uint32_t row_blocks(size_t n) { return (uint32_t)((n + SCAN_BLOCK - 1) / SCAN_BLOCK); }
inline size_t scratch_bytes(size_t n, size_t entries)
{
    return round256(entries * 8) + round256((n + 1) * 4) + round256(((size_t)row_blocks(n) + 2) * 4) + round256(NFLAGS * 4);
}
inline Scratch scratch_parts(void *base, size_t n, size_t entries)
{
    char *p = (char *)base;
    Scratch s;
    s.zbuf = (double *)p; p += round256(entries * 8);
    s.counts = (uint32_t *)p; p += round256((n + 1) * 4);
    s.blk = (uint32_t *)p; p += round256(((size_t)row_blocks(n) + 2) * 4);
    s.flags = (int32_t *)p;
    return s;
}

}  // namespace

const char *patch_refusal_text(int refusal)
{
    switch (refusal) {
    case PATCH_BAD_SIZE: return "patch table: patch_ptr must start at 0 and every patch must hold 1 to 16 rows";
    case PATCH_BAD_INDEX: return "patch table: a row index lies outside the system";
    case PATCH_REPEATED_ROW: return "patch table: a patch names a row twice";
    case PATCH_UNCOVERED_ROW: return "patch table: a row of the system lies in no patch";
    case PATCH_TOO_LARGE: return "patch table: 2^31 rows or entries and more";
    default: return "";
    }
}

// ---- validation -------------------------------------------------------------------------------------------------------------------
// ptr alone: ptr[0] = 0 and every difference within 1..16 (so ptr ascends and every offset is below ptr[npatches])
__global__ __launch_bounds__(RB) void patch_ptr_check_kernel(size_t npatches, const int64_t *ptr, int32_t *flags)
{
    const size_t p = (size_t)blockIdx.x * RB + threadIdx.x;
    if (p == 0 && ptr[0] != 0) atomicMax(&flags[FLAG_REFUSAL], (int32_t)PATCH_BAD_SIZE);
    if (p >= npatches) return;
    const int64_t m = ptr[p + 1] - ptr[p];
    if (m < 1 || m > PATCH_MAX_ROWS) atomicMax(&flags[FLAG_REFUSAL], (int32_t)PATCH_BAD_SIZE);
    else atomicMax(&flags[FLAG_MAX_ROWS], (int32_t)m);
}

// the rows of every patch (ptr has passed): in range, no repeats; counts[row] = patches that hold it
__global__ __launch_bounds__(RB) void patch_rows_check_kernel(size_t n, int64_t row0, size_t npatches, const int64_t *ptr,
                                                              const int32_t *rows, uint32_t *counts, int32_t *flags)
{
    const size_t p = (size_t)blockIdx.x * RB + threadIdx.x;
    if (p >= npatches) return;
    const int64_t p0 = ptr[p];
    const int m = (int)(ptr[p + 1] - p0);
    for (int l = 0; l < m; ++l) {
        const int64_t row = (int64_t)rows[p0 + l] - row0;
        if (row < 0 || (size_t)row >= n) { atomicMax(&flags[FLAG_REFUSAL], (int32_t)PATCH_BAD_INDEX); continue; }
        bool repeated = false;
        for (int q = 0; q < l; ++q) repeated |= rows[p0 + q] == rows[p0 + l];
        if (repeated) atomicMax(&flags[FLAG_REFUSAL], (int32_t)PATCH_REPEATED_ROW);
        atomicAdd(&counts[row], 1u);
    }
}

// every row is covered; the totals of the row blocks
__global__ __launch_bounds__(SCAN_BLOCK) void patch_cover_kernel(size_t n, const uint32_t *counts, uint32_t *blk, int32_t *flags)
{
    __shared__ uint32_t sh[SCAN_BLOCK / 64];
    const size_t i = (size_t)blockIdx.x * SCAN_BLOCK + threadIdx.x;
    const uint32_t c = i < n ? counts[i] : 0;
    if (i < n && c == 0) atomicMax(&flags[FLAG_REFUSAL], (int32_t)PATCH_UNCOVERED_ROW);
    uint32_t total;
    block_exclusive_scan(c, sh, total);
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

// ---- the row-to-slots table: slot_ptr (n + 1) and behind it slot_idx (entries) ------------------------------------------------------
__global__ __launch_bounds__(SCAN_BLOCK) void patch_slot_ptr_kernel(size_t n, uint32_t entries, uint32_t *counts, const uint32_t *blk,
                                                                    int32_t *slot_ptr)
{
    __shared__ uint32_t sh[SCAN_BLOCK / 64];
    const size_t i = (size_t)blockIdx.x * SCAN_BLOCK + threadIdx.x;
    const uint32_t c = i < n ? counts[i] : 0;
    uint32_t total;
    const uint32_t at = blk[blockIdx.x] + block_exclusive_scan(c, sh, total);
    if (i < n) { slot_ptr[i] = (int32_t)at; counts[i] = at; }
    if (i == 0) slot_ptr[n] = (int32_t)entries;
}

__global__ __launch_bounds__(RB) void patch_slot_fill_kernel(size_t npatches, int64_t row0, const int64_t *ptr, const int32_t *rows,
                                                             uint32_t *cursor, int32_t *slot_idx)
{
    const size_t p = (size_t)blockIdx.x * RB + threadIdx.x;
    if (p >= npatches) return;
    const int64_t p0 = ptr[p];
    const int m = (int)(ptr[p + 1] - p0);
    for (int l = 0; l < m; ++l) slot_idx[atomicAdd(&cursor[rows[p0 + l] - row0], 1u)] = (int32_t)(p0 + l);
}

// a row's slots ascending: the order of its patches, whatever order the fill reached them in
__global__ __launch_bounds__(RB) void patch_slot_sort_kernel(size_t n, const int32_t *slot_ptr, int32_t *slot_idx)
{
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x;
    if (i >= n) return;
    const int32_t s0 = slot_ptr[i], s1 = slot_ptr[i + 1];
    for (int32_t a = s0 + 1; a < s1; ++a) {
        const int32_t v = slot_idx[a];
        int32_t b = a;
        for (; b > s0 && slot_idx[b - 1] > v; --b) slot_idx[b] = slot_idx[b - 1];
        slot_idx[b] = v;
    }
}

// ---- factor -------------------------------------------------------------------------------------------------------------------------
// A(row, col) of a CSR matrix with ascending columns; an absent entry is zero.  row: the storage row (CgRowsWindow, cg.hpp: a rank's
// rows are stored from 0 on and keep global columns)
__device__ __forceinline__ double csr_entry(const int64_t *rowptr, const int32_t *colind, const double *values, int64_t row, int32_t col)
{
    const int64_t end = rowptr[row + 1];
    int64_t lo = rowptr[row], hi = end;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (colind[mid] < col) lo = mid + 1; else hi = mid;
    }
    return (lo < end && colind[lo] == col) ? values[lo] : 0.0;
}

template <int P>
__global__ __launch_bounds__(RB) void patch_factor_kernel(size_t npatches, int64_t row0, const int64_t *ptr, const int32_t *rows,
                                                          const int64_t *rowptr, const int32_t *colind, const double *values, int stride,
                                                          double *factors, int32_t *info, int32_t *flags)
{
    const size_t p = ((size_t)blockIdx.x * RB + threadIdx.x) / P;
    const int l = threadIdx.x % P;
    int64_t p0 = 0;
    int m = 0;
    if (p < npatches) { p0 = ptr[p]; m = (int)(ptr[p + 1] - p0); }
    const bool act = l < m;
    const int32_t gl = act ? rows[p0 + l] : -1;
    // row l of A_p; the rows beyond the patch are the identity's
    double a[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const int32_t gj = __shfl(gl, j, P);
        a[j] = (act && gj >= 0) ? csr_entry(rowptr, colind, values, (int64_t)gl - row0, gj) : (l == j ? 1.0 : 0.0);
    }
    // Cholesky, right-looking: after step j, a[j] of lane i >= j is L(i, j)
    int bad = 0;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const double djj = __shfl(a[j], j, P);
        if (!(djj > 0.0) && bad == 0) bad = j + 1;
        const double ljj = sqrt(djj);
        a[j] = l == j ? ljj : a[j] / ljj;
#pragma unroll
        for (int k = j + 1; k < P; ++k) {
            const double lkj = __shfl(a[j], k, P);
            a[k] -= a[j] * lkj;
        }
    }
    // column l of W = L^-1: W(i, l) = (delta_il - sum_{k < i} L(i, k) W(k, l)) / L(i, i)
    double w[P];
#pragma unroll
    for (int i = 0; i < P; ++i) {
        double s = i == l ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < i; ++k) s -= __shfl(a[k], i, P) * w[k];
        w[i] = s / __shfl(a[i], i, P);
    }
    if (p < npatches) {
        double *W = factors + p * (size_t)stride;
#pragma unroll
        for (int i = 0; i < P; ++i)
            if (act && i >= l && i < m) W[i * (i + 1) / 2 + l] = w[i];
        for (int q = m * (m + 1) / 2 + l; q < stride; q += P) W[q] = 0.0;      // a smaller patch leaves the rest of its stride zero
        if (l == 0) {
            info[p] = bad;
            if (bad) atomicAdd(&flags[FLAG_FAILED], 1);
        }
    }
}

// ---- apply --------------------------------------------------------------------------------------------------------------------------
template <int P>
__global__ __launch_bounds__(RB) void patch_apply_kernel(size_t npatches, int64_t row0, const int64_t *ptr, const int32_t *rows,
                                                         const double *factors, int stride, const double *r, double *zbuf)
{
    const size_t p = ((size_t)blockIdx.x * RB + threadIdx.x) / P;
    const int l = threadIdx.x % P;
    int64_t p0 = 0;
    int m = 0;
    if (p < npatches) { p0 = ptr[p]; m = (int)(ptr[p + 1] - p0); }
    const bool act = l < m;
    const double rl = act ? r[rows[p0 + l] - row0] : 0.0;
    const double *W = factors + (p < npatches ? p : 0) * (size_t)stride;
    double t = 0.0;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const double rj = __shfl(rl, j, P);
        if (act && j <= l) t += W[l * (l + 1) / 2 + j] * rj;
    }
    double z = 0.0;
#pragma unroll
    for (int i = 0; i < P; ++i) {
        const double ti = __shfl(t, i, P);
        if (act && i >= l && i < m) z += W[i * (i + 1) / 2 + l] * ti;
    }
    if (act) zbuf[p0 + l] = z;
}

// z_i = the sum of row i's slots in ascending order; the block partials of r . z
__global__ __launch_bounds__(RB) void patch_sum_kernel(size_t n, const int32_t *slot_ptr, const int32_t *slot_idx, const double *zbuf,
                                                       const double *r, double *z, double *part_rz)
{
    __shared__ double sh[RB / 64];
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x;
    double rz = 0.0;
    if (i < n) {
        double zi = 0.0;
        for (int32_t s = slot_ptr[i]; s < slot_ptr[i + 1]; ++s) zi += zbuf[slot_idx[s]];
        z[i] = zi;
        rz = r[i] * zi;
    }
    const double tot = block_sum(rz, sh);
    if (part_rz != nullptr && threadIdx.x == 0) part_rz[blockIdx.x] = tot;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
hipError_t patch_query(hipStream_t stream, size_t n, size_t npatches, const int64_t *ptr, PatchSizes *out, int *refusal)
{
    *out = PatchSizes();
    *refusal = PATCH_OK;
    if (n >= ((size_t)1 << 31) || npatches >= ((size_t)1 << 31)) { *refusal = PATCH_TOO_LARGE; return hipSuccess; }
    int32_t *d_flags = nullptr;
    hipError_t e = hipMalloc((void **)&d_flags, NFLAGS * 4);
    if (e != hipSuccess) return e;
    int32_t h[NFLAGS] = {0, 0, 0, 0};
    int64_t entries = 0;
    e = hipMemsetAsync(d_flags, 0, NFLAGS * 4, stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(patch_ptr_check_kernel, dim3((unsigned)((npatches + RB) / RB)), dim3(RB), 0, stream, npatches, ptr, d_flags);
        e = hipMemcpyAsync(h, d_flags, NFLAGS * 4, hipMemcpyDeviceToHost, stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&entries, ptr + npatches, 8, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    (void)hipFree(d_flags);
    if (e != hipSuccess) return e;
    if (h[FLAG_REFUSAL]) { *refusal = h[FLAG_REFUSAL]; return hipSuccess; }
    if (entries >= ((int64_t)1 << 31)) { *refusal = PATCH_TOO_LARGE; return hipSuccess; }
    out->entries = (uint64_t)entries;
    out->max_rows = h[FLAG_MAX_ROWS];
    out->lanes = out->max_rows <= 4 ? 4 : out->max_rows <= 8 ? 8 : 16;
    out->factor_doubles = (uint64_t)npatches * (uint64_t)(out->max_rows * (out->max_rows + 1) / 2);
    out->slot_ints = (uint64_t)n + 1 + out->entries;
    out->scratch_bytes = scratch_bytes(n, out->entries);
    return hipSuccess;
}

hipError_t patch_factor(hipStream_t stream, const int64_t *rowptr, const int32_t *colind, const double *values, const PatchTable &t,
                        const PatchSizes &sz, double *factors, int32_t *slots, void *scratch, int32_t *info, int *refusal, size_t *failed)
{
    *refusal = PATCH_OK;
    *failed = 0;
    if (t.n == 0 && t.npatches == 0) return hipSuccess;
    const Scratch s = scratch_parts(scratch, t.n, sz.entries);
    const uint32_t nb = row_blocks(t.n);
    const unsigned gp = (unsigned)((t.npatches + RB - 1) / RB), gr = (unsigned)((t.n + RB - 1) / RB);
    int32_t h[NFLAGS] = {0, 0, 0, 0};
    hipError_t e = hipMemsetAsync(s.counts, 0, (t.n + 1) * 4, stream);
    if (e == hipSuccess) e = hipMemsetAsync(s.flags, 0, NFLAGS * 4, stream);
    if (e != hipSuccess) return e;
    if (t.npatches) hipLaunchKernelGGL(patch_rows_check_kernel, dim3(gp), dim3(RB), 0, stream, t.n, t.row0, t.npatches, t.ptr, t.rows, s.counts, s.flags);
    if (t.n) hipLaunchKernelGGL(patch_cover_kernel, dim3(nb), dim3(SCAN_BLOCK), 0, stream, t.n, s.counts, s.blk, s.flags);
    e = hipMemcpyAsync(h, s.flags, NFLAGS * 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return e;
    if (h[FLAG_REFUSAL]) { *refusal = h[FLAG_REFUSAL]; return hipSuccess; }      // (a table with patches and no rows: a bad index)
    // the table holds: from here on it is indexed with
    int32_t *slot_ptr = slots, *slot_idx = slots + t.n + 1;
    hipLaunchKernelGGL(active_block_scan_kernel, dim3(1), dim3(SCAN_BLOCK), 0, stream, s.blk, nb);
    hipLaunchKernelGGL(patch_slot_ptr_kernel, dim3(nb), dim3(SCAN_BLOCK), 0, stream, t.n, (uint32_t)sz.entries, s.counts, s.blk, slot_ptr);
    hipLaunchKernelGGL(patch_slot_fill_kernel, dim3(gp), dim3(RB), 0, stream, t.npatches, t.row0, t.ptr, t.rows, s.counts, slot_idx);
    hipLaunchKernelGGL(patch_slot_sort_kernel, dim3(gr), dim3(RB), 0, stream, t.n, slot_ptr, slot_idx);
    const int stride = sz.max_rows * (sz.max_rows + 1) / 2;
    const unsigned gf = (unsigned)((t.npatches * (size_t)sz.lanes + RB - 1) / RB);
    if (sz.lanes == 4)
        hipLaunchKernelGGL(patch_factor_kernel<4>, dim3(gf), dim3(RB), 0, stream, t.npatches, t.row0, t.ptr, t.rows, rowptr, colind, values, stride, factors, info, s.flags);
    else if (sz.lanes == 8)
        hipLaunchKernelGGL(patch_factor_kernel<8>, dim3(gf), dim3(RB), 0, stream, t.npatches, t.row0, t.ptr, t.rows, rowptr, colind, values, stride, factors, info, s.flags);
    else
        hipLaunchKernelGGL(patch_factor_kernel<16>, dim3(gf), dim3(RB), 0, stream, t.npatches, t.row0, t.ptr, t.rows, rowptr, colind, values, stride, factors, info, s.flags);
    e = hipMemcpyAsync(h, s.flags, NFLAGS * 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return e;
    *failed = (size_t)h[FLAG_FAILED];
    return hipSuccess;
}

void patch_apply(hipStream_t stream, const PatchTable &t, const PatchSizes &sz, const double *factors, const int32_t *slots,
                 void *scratch, const double *r, double *z, double *part_rz)
{
    if (t.n == 0) return;
    const Scratch s = scratch_parts(scratch, t.n, sz.entries);
    const int stride = sz.max_rows * (sz.max_rows + 1) / 2;
    const unsigned ga = (unsigned)((t.npatches * (size_t)sz.lanes + RB - 1) / RB);
    if (sz.lanes == 4)
        hipLaunchKernelGGL(patch_apply_kernel<4>, dim3(ga), dim3(RB), 0, stream, t.npatches, t.row0, t.ptr, t.rows, factors, stride, r, s.zbuf);
    else if (sz.lanes == 8)
        hipLaunchKernelGGL(patch_apply_kernel<8>, dim3(ga), dim3(RB), 0, stream, t.npatches, t.row0, t.ptr, t.rows, factors, stride, r, s.zbuf);
    else
        hipLaunchKernelGGL(patch_apply_kernel<16>, dim3(ga), dim3(RB), 0, stream, t.npatches, t.row0, t.ptr, t.rows, factors, stride, r, s.zbuf);
    hipLaunchKernelGGL(patch_sum_kernel, dim3((unsigned)((t.n + RB - 1) / RB)), dim3(RB), 0, stream, t.n, slots, slots + t.n + 1, s.zbuf, r, z,
                       part_rz);
}

// ---- the patch tables of the face-only system ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(RB) void face_patches_kernel(uint32_t nfaces, int fbs, int32_t row0, int64_t *ptr, int32_t *rows)
{
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x;
    if (i <= nfaces) ptr[i] = (int64_t)i * fbs;
    if (i < (size_t)nfaces * fbs) rows[i] = row0 + (int32_t)i;
}

__global__ __launch_bounds__(RB) void cell_patch_flags_kernel(uint32_t ncells, const uint32_t *cprefix, uint8_t *flags)
{
    const size_t c = (size_t)blockIdx.x * RB + threadIdx.x;
    if (c < ncells) flags[c] = cprefix[c + 1] > cprefix[c] ? 1 : 0;
}

__global__ __launch_bounds__(RB) void cell_patches_kernel(uint32_t ncells, uint32_t npatches, const uint32_t *cell_faces,
                                                          const int32_t *face_compress, const uint32_t *cprefix, const int32_t *index, int fbs,
                                                          int64_t *ptr, int32_t *rows)
{
    const size_t c = (size_t)blockIdx.x * RB + threadIdx.x;
    if (c == 0) ptr[npatches] = (int64_t)cprefix[ncells] * fbs;
    if (c >= ncells) return;
    const int32_t p = index[c];
    if (p < 0) return;
    int64_t at = (int64_t)cprefix[c] * fbs;
    ptr[p] = at;
    for (int lf = 0; lf < 4; ++lf) {                     // bottom, right, top, left
        const int32_t comp = face_compress[cell_faces[4 * c + lf]];
        if (comp < 0) continue;
        for (int k = 0; k < fbs; ++k) rows[at++] = comp * fbs + k;
    }
}

void face_patches(hipStream_t stream, uint32_t nfaces, int fbs, int32_t row0, int64_t *ptr, int32_t *rows)
{
    const size_t total = (size_t)nfaces * fbs + 1;
    hipLaunchKernelGGL(face_patches_kernel, dim3((unsigned)((total + RB - 1) / RB)), dim3(RB), 0, stream, nfaces, fbs, row0, ptr, rows);
}

void cell_patch_flags(hipStream_t stream, uint32_t ncells, const uint32_t *cprefix, uint8_t *flags)
{
    if (ncells) hipLaunchKernelGGL(cell_patch_flags_kernel, dim3((ncells + RB - 1) / RB), dim3(RB), 0, stream, ncells, cprefix, flags);
}

void cell_patches(hipStream_t stream, uint32_t ncells, uint32_t npatches, const uint32_t *cell_faces, const int32_t *face_compress,
                  const uint32_t *cprefix, const int32_t *index, int fbs, int64_t *ptr, int32_t *rows)
{
    hipLaunchKernelGGL(cell_patches_kernel, dim3((ncells + RB) / RB), dim3(RB), 0, stream, ncells, npatches, cell_faces, face_compress, cprefix,
                       index, fbs, ptr, rows);
}


// ---- a patch table from items, counted and placed by the scans of scan.hpp.  An item is what may give a patch; an Items type says
//   int blocks(size_t i, int32_t *q) const      the face blocks item i gives, at most 4, in the patch's order (none: no patch)
//   int32_t first_row(int32_t q, int fbs) const  the first of the fbs rows of block q
// ------------------------------------------------------------------------------------------------------------------------------------
// per block of items: its patches (bp) and its face blocks (bb)
template <class Items>
__global__ __launch_bounds__(SCAN_BLOCK) void item_count_kernel(Items it, size_t nitems, uint32_t *bp, uint32_t *bb)
{
    __shared__ uint32_t sh[SCAN_BLOCK / 64];
    const size_t i = (size_t)blockIdx.x * SCAN_BLOCK + threadIdx.x;
    int32_t q[4];
    const uint32_t nb = i < nitems ? (uint32_t)it.blocks(i, q) : 0u;
    uint32_t tp, tb;
    block_exclusive_scan(nb ? 1u : 0u, sh, tp);
    block_exclusive_scan(nb, sh, tb);
    if (threadIdx.x == 0) { bp[blockIdx.x] = tp; bb[blockIdx.x] = tb; }
}

// bp, bb scanned (their totals at [nblk]): every item with blocks writes its patch
template <class Items>
__global__ __launch_bounds__(SCAN_BLOCK) void item_fill_kernel(Items it, size_t nitems, int fbs, const uint32_t *bp, const uint32_t *bb,
                                                               uint32_t nblk, int64_t *ptr, int32_t *rows)
{
    __shared__ uint32_t sh[SCAN_BLOCK / 64];
    const size_t i = (size_t)blockIdx.x * SCAN_BLOCK + threadIdx.x;
    int32_t q[4];
    const uint32_t nb = i < nitems ? (uint32_t)it.blocks(i, q) : 0u;
    uint32_t tp, tb;
    const uint32_t p = bp[blockIdx.x] + block_exclusive_scan(nb ? 1u : 0u, sh, tp);
    const uint32_t b0 = bb[blockIdx.x] + block_exclusive_scan(nb, sh, tb);
    if (i == 0) ptr[bp[nblk]] = (int64_t)bb[nblk] * fbs;
    if (nb == 0) return;
    int64_t at = (int64_t)b0 * fbs;
    ptr[p] = at;
    for (uint32_t j = 0; j < nb; ++j) {
        const int32_t row = it.first_row(q[j], fbs);
        for (int k = 0; k < fbs; ++k) rows[at++] = row + k;
    }
}

// the table of nitems items.  ptr = null, or 2^31 entries and more: the sizes only.  Waits for the stream.
template <class Items>
static hipError_t item_patches(hipStream_t stream, const Items &it, size_t nitems, int fbs, uint64_t *npatches, uint64_t *entries,
                               int64_t *ptr, int32_t *rows)
{
    const uint32_t nblk = (uint32_t)(nitems ? (nitems + SCAN_BLOCK - 1) / SCAN_BLOCK : 1);
    DeviceTmp tmp(stream);
    uint32_t *b[2] = {nullptr, nullptr}, tot[2] = {0, 0};
    if (!tmp.alloc(&b[0], (size_t)nblk + 1) || !tmp.alloc(&b[1], (size_t)nblk + 1)) return tmp.error();
    hipLaunchKernelGGL((item_count_kernel<Items>), dim3(nblk), dim3(SCAN_BLOCK), 0, stream, it, nitems, b[0], b[1]);
    if (!tmp.ok(scan_block_counts(stream, nblk, 2, b, tot))) return tmp.error();
    *npatches = tot[0];
    *entries = (uint64_t)tot[1] * fbs;
    if (ptr == nullptr || *entries >= ((uint64_t)1 << 31)) return hipSuccess;
    hipLaunchKernelGGL((item_fill_kernel<Items>), dim3(nblk), dim3(SCAN_BLOCK), 0, stream, it, nitems, fbs, b[0], b[1], nblk, ptr, rows);
    if (tmp.ok(hipGetLastError())) tmp.ok(hipStreamSynchronize(stream));       // the block offsets live until the kernel has read them
    return tmp.error();
}

// ---- the cell patches of a slab of the generator mesh (pa_condensed_rows_patches), from the closed forms of structured_mesh.hpp: the
// slab owns the compressed faces [p0, p1) -- of its top cell row's top faces none, unless it is the last slab --, and a patch names
// its rows by their global indices.  Item c: local cell c -> its owned non-Dirichlet faces in the cell's face order bottom, right,
// top, left; compressed face q owns the rows from q fbs on ------------------------------------------------------------------------
struct SlabCellItems {
    StructuredMesh sm;
    int32_t p0, p1;
    __device__ int blocks(size_t item, int32_t *q) const
    {
        const uint32_t c = (uint32_t)item, ci = c % sm.Nx, cj = sm.row0 + c / sm.Nx;
        const uint32_t f[4] = {sm_hface(sm, ci, cj), sm_vface(sm, ci + 1, cj), sm_hface(sm, ci, cj + 1), sm_vface(sm, ci, cj)};
        int n = 0;
        for (int lf = 0; lf < 4; ++lf) {
            uint32_t lo, hi;
            bool dirichlet;
            int32_t comp;
            sm_face_decode(sm, f[lf], lo, hi, dirichlet, comp);
            if (!dirichlet && comp >= p0 && comp < p1) q[n++] = comp;
        }
        return n;
    }
    __device__ int32_t first_row(int32_t q, int fbs) const { return q * fbs; }
};

hipError_t slab_cell_patches(hipStream_t stream, const StructuredMesh &sm, int32_t p0, int32_t p1, int fbs, uint64_t *npatches,
                             uint64_t *entries, int64_t *ptr, int32_t *rows)
{
    return item_patches(stream, SlabCellItems{sm, p0, p1}, (size_t)(sm.row1 - sm.row0) * sm.Nx, fbs, npatches, entries, ptr, rows);
}

// ---- the patch tables of the interface problem's face-only system (pa_interface_condensed_patches, pa_interface_rows_patches:
// interface_assembler's numbering, in which a cut face owns two blocks; the tables of IfCsrMesh alone -- the whole mesh's, or a slab's
// extended ones with the part of them that counts (IfPatchRange)).  Item r.item0 + i is a face (IF_PATCH_FACE), or side s of cell X
// as 2 X + s (IF_PATCH_CELL; an uncut cell is its item 2 X alone) -> its face blocks within the range; block q gives the rows of
// block r.shift + q, formed in 64 bits (the system has fewer than 2^31 rows, the extended numbering's blocks need not start at the
// system's) ------------------------------------------------------------------------------------------------------------------------
struct IfItems {
    IfCsrMesh m;
    IfPatchRange r;
    int kind;
    __device__ int blocks(size_t i, int32_t *blk) const
    {
        const size_t item = r.item0 + i;
        int n = 0;
        auto take = [&](int32_t q) { if (q >= r.q0 && q < r.q1) blk[n++] = q; };
        if (kind == IF_PATCH_FACE) {
            const int32_t b = m.face_table[item];
            if (b < 0) return 0;
            take(b);
            if (m.face_loc[item] == IF_LOC_CUT) take(b + 1);
            return n;
        }
        const size_t X = item >> 1;
        const int s = (int)(item & 1);
        const bool cut = m.cell_loc[X] == IF_LOC_CUT;
        if (!cut && s == 1) return 0;
        for (int lf = 0; lf < 4; ++lf) {                     // bottom, right, top, left
            const uint32_t f = m.cell_faces[4 * X + lf];
            const int32_t b = m.face_table[f];
            if (b < 0) continue;
            const int8_t fl = m.face_loc[f];
            if (cut && fl != IF_LOC_CUT && fl != s) continue;                                   // an uncut face: on its own side only
            take(b + ((cut && s == 1 && fl == IF_LOC_CUT) ? 1 : 0));                            // dup of if_global_index
        }
        return n;
    }
    __device__ int32_t first_row(int32_t q, int fbs) const { return (int32_t)((r.shift + q) * fbs); }
};

hipError_t ifcond_patches(hipStream_t stream, const IfCsrMesh &m, int face_deg, int kind, uint64_t *npatches, uint64_t *entries,
                          int64_t *ptr, int32_t *rows)
{
    const IfPatchRange whole{0, 0, INT32_MAX, 0};
    return item_patches(stream, IfItems{m, whole, kind}, kind == IF_PATCH_FACE ? (size_t)m.nfaces : 2 * (size_t)m.ncells,
                        if_dims(face_deg).fbs, npatches, entries, ptr, rows);
}

// a slab: every face of the extended tables may give a patch (its blocks are owned or not, both of a cut face together), of the
// cells the slab's own, which follow the halo_cells cells of the row below
hipError_t ifrows_patches(hipStream_t stream, const IfCsrMesh &m, uint32_t halo_cells, int32_t q0, int32_t q1, int64_t fb0, int face_deg,
                          int kind, uint64_t *npatches, uint64_t *entries, int64_t *ptr, int32_t *rows)
{
    const bool faces = kind == IF_PATCH_FACE;
    const IfPatchRange slab{faces ? (size_t)0 : 2 * (size_t)halo_cells, q0, q1, fb0};
    return item_patches(stream, IfItems{m, slab, kind}, faces ? (size_t)m.nfaces : 2 * (size_t)(m.ncells - halo_cells),
                        if_dims(face_deg).fbs, npatches, entries, ptr, rows);
}

}  // namespace pa
