// coarse_precond.hip -- a Galerkin coarse level for the device conjugate gradient (solver_cg.hpp:63-144 with
//   z = sum_p R_p^T (R_p A R_p^T)^-1 R_p r + P (P^T A P)^-1 P^T r
// where the reference multiplies by 1 / diag(A); the solve of cuthho_square.cpp:915-919 on the face-only system), and the coarse table
// of that system: bilinear hats on every H-th mesh line, interpolated to the face unknowns, whole or split by side of the interface.
//
// P (n x ncoarse, 0..4 entries per row, at most 4096 columns) is the caller's, in CSR.  One-level Schwarz has no global information;
// the coarse term carries it, and is small enough to be inverted exactly.
//   factor: the table is validated (one thread per row); P^T is built by a count per column, the block scan of scan.hpp, a fill and a
//           rank by fine row (a workgroup per coarse row), so that its rows ascend whatever order the fill ran in.  W = A P: one thread
//           per fine row, at most 16 (column, value) slots kept in column order, summed in the row's entry order.  A_c = P^T W: one
//           workgroup per coarse row j streams (P^T entry x W slot) in tiles through LDS, and the lane c mod 256 owns column c <= j
//           and adds its contributions in stream order; the lower triangle is mirrored.  Cholesky: one launch per column (left-looking,
//           a wavefront per row, lane-strided sums and the xor tree), then W = L^-1 from W L = I, a workgroup per row, into the packed
//           lower triangle (row i at i (i + 1) / 2).  Plain double throughout.
//   apply:  restrict (a workgroup per coarse row: lane-strided sums, block_sum's tree), t = W (P^T r) (a wavefront per row), u = W^T t
//           (64 columns x 4 row groups per workgroup), prolong (a gather of at most 4 terms per fine row, added to z or not, with the
//           block partials of r . z).  No dependent chain of length ncoarse, no floating-point atomics: the same bits on every call.
//   solve:  not here: rows_precond.hip calls coarse_query, coarse_validate, the factor and the apply in their order, after the patch
//           level's, for every solver (TwoLevel).
//   table:  the hats and the kernels that count, place and write them are stated once, for the numbering of pa_condensed_csr_pattern
//           (a non-Dirichlet face owns one block), for the rows of it that a slab of the generator mesh owns, and for
//           interface_assembler's (a cut face owns two: the solve of cuthho_square.cpp:1737-1743) and the rows of it that a slab of
//           the interface problem owns; a mesh type says what a face gives (face_blocks).
//   ranks:  for the row-partitioned solve (rows_precond.hip) the factor and the apply come in their stages: coarse_galerkin forms a
//           rank's addend P_r^T (A_r P_window) of A_c with P given for the window of columns the rank's rows read (its ends packed,
//           exchanged and unpacked here), the lower triangle travels packed, coarse_cholesky factors the sum; coarse_restrict and
//           coarse_correct are the two halves of an apply, the sum of the restrictions over the ranks between them.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "cg.hpp"
#include "coarse_precond.hpp"
#include "device_tmp.hpp"
#include "scan.hpp"

namespace pa {

namespace {

constexpr int FLAG_REFUSAL = 0, FLAG_PIVOT = 1, NFLAGS = 4;
constexpr int GAL_TILE = 64;               // P^T entries per tile of the Galerkin product: GAL_TILE * COARSE_W_SLOTS contributions

inline size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }

// the parts of the scratch buffer: the coarse vectors of an apply in front
struct Scratch {
    double *vec;           // 3 ncoarse: P^T r, t, u
    int32_t *flags;        // NFLAGS
    uint32_t *counts;      // ncoarse + 2: entries per column, scanned
    uint32_t *cursor;      // ncoarse + 2: the fill cursor
    double *ldiag;         // ncoarse: the diagonal of L
    int32_t *trow;         // entries: fine rows in fill order
    double *tval;          // entries
    int32_t *wcount;       // n: slots of a row of W = A P
    int32_t *wcols;        // n * COARSE_W_SLOTS
    double *wvals;         // n * COARSE_W_SLOTS
    double *G;             // ncoarse^2: A_c, then L below its diagonal and L^T above it
};
inline Scratch scratch_parts(void *base, size_t n, size_t nc, size_t entries, size_t *bytes)
{
    char *p = (char *)base;
    Scratch s;
    s.vec = (double *)p; p += round256(3 * nc * 8);
    s.flags = (int32_t *)p; p += round256(NFLAGS * 4);
    s.counts = (uint32_t *)p; p += round256((nc + 2) * 4);
    s.cursor = (uint32_t *)p; p += round256((nc + 2) * 4);
    s.ldiag = (double *)p; p += round256(nc * 8);
    s.trow = (int32_t *)p; p += round256(entries * 4);
    s.tval = (double *)p; p += round256(entries * 8);
    s.wcount = (int32_t *)p; p += round256(n * 4);
    s.wcols = (int32_t *)p; p += round256(n * COARSE_W_SLOTS * 4);
    s.wvals = (double *)p; p += round256(n * COARSE_W_SLOTS * 8);
    s.G = (double *)p; p += round256(nc * nc * 8);
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

}  // namespace

const char *coarse_refusal_text(int refusal)
{
    switch (refusal) {
    case COARSE_BAD_SIZE: return "coarse table: p_ptr must start at 0 and every row must hold 0 to 4 entries";
    case COARSE_BAD_VALUE: return "coarse table: a value is not finite";
    case COARSE_BAD_ORDER: return "coarse table: the columns of a row must ascend without repeats";
    case COARSE_BAD_INDEX: return "coarse table: a column index lies outside [0, ncoarse)";
    case COARSE_BAD_NODES: return "coarse table: ncoarse must lie within 1 to 4096";
    case COARSE_TOO_LARGE: return "coarse table: 2^29 rows and more";
    case COARSE_W_OVERFLOW: return "coarse table: a row of A P holds more than 16 columns";
    case COARSE_BAD_LEVEL_NODES: return "coarse table: ncoarse of a smoothed level must lie within 1 to 16777216";
    default: return "";
    }
}

// ---- validation -------------------------------------------------------------------------------------------------------------------
// ptr alone: ptr[0] = 0 and every difference within 0..4 (so ptr ascends and every offset is at most ptr[n])
__global__ __launch_bounds__(RB) void coarse_ptr_check_kernel(size_t n, const int64_t *ptr, int32_t *flags)
{
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x;
    if (i == 0 && ptr[0] != 0) atomicMax(&flags[FLAG_REFUSAL], (int32_t)COARSE_BAD_SIZE);
    if (i >= n) return;
    const int64_t m = ptr[i + 1] - ptr[i];
    if (m < 0 || m > COARSE_MAX_ROW_ENTRIES) atomicMax(&flags[FLAG_REFUSAL], (int32_t)COARSE_BAD_SIZE);
}

// the entries of every row (ptr has passed): in range, ascending, finite; counts[col] = rows that hold it
__global__ __launch_bounds__(RB) void coarse_rows_check_kernel(size_t n, uint32_t nc, const int64_t *ptr, const int32_t *cols,
                                                               const double *vals, uint32_t *counts, int32_t *flags)
{
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x;
    if (i >= n) return;
    const int64_t p0 = ptr[i];
    const int m = (int)(ptr[i + 1] - p0);
    int32_t prev = -1;
    for (int l = 0; l < m; ++l) {
        const int32_t c = cols[p0 + l];
        if (!isfinite(vals[p0 + l])) atomicMax(&flags[FLAG_REFUSAL], (int32_t)COARSE_BAD_VALUE);
        if (c < 0 || (uint32_t)c >= nc) { atomicMax(&flags[FLAG_REFUSAL], (int32_t)COARSE_BAD_INDEX); continue; }
        if (c <= prev) atomicMax(&flags[FLAG_REFUSAL], (int32_t)COARSE_BAD_ORDER);
        prev = c;
        atomicAdd(&counts[c], 1u);
    }
}

// ---- P^T ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RB) void coarse_pt_ptr_kernel(uint32_t nc, const uint32_t *counts, uint32_t *pt_ptr, uint32_t *cursor)
{
    const uint32_t j = blockIdx.x * RB + threadIdx.x;
    if (j <= nc) { pt_ptr[j] = counts[j]; cursor[j] = counts[j]; }
}

__global__ __launch_bounds__(RB) void coarse_pt_fill_kernel(size_t n, const int64_t *ptr, const int32_t *cols, const double *vals,
                                                            uint32_t *cursor, int32_t *trow, double *tval)
{
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x;
    if (i >= n) return;
    for (int64_t q = ptr[i]; q < ptr[i + 1]; ++q) {
        const uint32_t at = atomicAdd(&cursor[cols[q]], 1u);
        trow[at] = (int32_t)i;
        tval[at] = vals[q];
    }
}

// a workgroup per coarse row: every entry goes to its rank among the row's fine rows (all different: a row of P repeats no column)
__global__ __launch_bounds__(RB) void coarse_pt_rank_kernel(const uint32_t *pt_ptr, const int32_t *trow, const double *tval, int32_t *pt_rows,
                                                            double *pt_vals)
{
    constexpr uint32_t TILE = 1024;
    __shared__ int32_t tile[TILE];
    const uint32_t p0 = pt_ptr[blockIdx.x], p1 = pt_ptr[blockIdx.x + 1];
    for (uint32_t base = p0; base < p1; base += RB) {
        const uint32_t s = base + threadIdx.x;
        const bool act = s < p1;
        const int32_t mine = act ? trow[s] : 0;
        uint32_t rank = 0;
        for (uint32_t t0 = p0; t0 < p1; t0 += TILE) {
            const uint32_t cnt = p1 - t0 < TILE ? p1 - t0 : TILE;
            __syncthreads();
            for (uint32_t q = threadIdx.x; q < cnt; q += RB) tile[q] = trow[t0 + q];
            __syncthreads();
            for (uint32_t q = 0; q < cnt; ++q) rank += tile[q] < mine ? 1u : 0u;
        }
        if (act) { pt_rows[p0 + rank] = mine; pt_vals[p0 + rank] = tval[s]; }
    }
}

// ---- W = A P: one thread per fine row, the slots in column order, every slot summed in the row's entry order.  P is given for the
// np rows from col0 on (the system itself: col0 = 0, np = n; a rank's rows: the window of columns they read) ---------------------------
__global__ __launch_bounds__(RB) void coarse_w_kernel(size_t n, const int64_t *rowptr, const int32_t *colind, const double *values,
                                                      int64_t col0, size_t np, const int64_t *ptr, const int32_t *cols, const double *vals,
                                                      int32_t *wcount, int32_t *wcols, double *wvals, int32_t *flags)
{
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x;
    if (i >= n) return;
    int32_t wc[COARSE_W_SLOTS];
    double wv[COARSE_W_SLOTS];
    int cnt = 0;
    bool over = false;
    for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
        const int64_t c = (int64_t)colind[e] - col0;
        if (c < 0 || (size_t)c >= np) continue;          // (not a column of the system: P has no row for it)
        const double a = values[e];
        for (int64_t q = ptr[c]; q < ptr[c + 1]; ++q) {
            const int32_t j = cols[q];
            const double v = a * vals[q];
            int k = 0;
            while (k < cnt && wc[k] < j) ++k;
            if (k < cnt && wc[k] == j) { wv[k] += v; continue; }
            if (cnt == COARSE_W_SLOTS) { over = true; continue; }
            for (int s = cnt; s > k; --s) { wc[s] = wc[s - 1]; wv[s] = wv[s - 1]; }
            wc[k] = j; wv[k] = v;
            ++cnt;
        }
    }
    if (over) atomicMax(&flags[FLAG_REFUSAL], (int32_t)COARSE_W_OVERFLOW);
    wcount[i] = cnt;
    for (int k = 0; k < cnt; ++k) { wcols[i * COARSE_W_SLOTS + k] = wc[k]; wvals[i * COARSE_W_SLOTS + k] = wv[k]; }
}

// ---- A_c = P^T W: a workgroup per coarse row j; lane c mod RB owns column c <= j and adds its contributions in stream order (fine
// rows ascending); the lower triangle goes to both halves of G -----------------------------------------------------------------------
__global__ __launch_bounds__(RB) void coarse_galerkin_kernel(uint32_t nc, const uint32_t *pt_ptr, const int32_t *pt_rows, const double *pt_vals,
                                                             const int32_t *wcount, const int32_t *wcols, const double *wvals, double *G)
{
    __shared__ double acc[COARSE_MAX_NODES];
    __shared__ int32_t tcol[GAL_TILE * COARSE_W_SLOTS];
    __shared__ double tval[GAL_TILE * COARSE_W_SLOTS];
    const uint32_t j = blockIdx.x;
    for (uint32_t c = threadIdx.x; c <= j; c += RB) acc[c] = 0.0;
    const uint32_t p0 = pt_ptr[j], p1 = pt_ptr[j + 1];
    for (uint32_t t0 = p0; t0 < p1; t0 += GAL_TILE) {
        const uint32_t cnt = p1 - t0 < (uint32_t)GAL_TILE ? p1 - t0 : (uint32_t)GAL_TILE;
        __syncthreads();
        for (uint32_t s = threadIdx.x; s < cnt * COARSE_W_SLOTS; s += RB) {
            const uint32_t e = t0 + s / COARSE_W_SLOTS, k = s % COARSE_W_SLOTS;
            const size_t i = (size_t)pt_rows[e];
            const bool live = (int32_t)k < wcount[i];
            tcol[s] = live ? wcols[i * COARSE_W_SLOTS + k] : -1;
            tval[s] = live ? pt_vals[e] * wvals[i * COARSE_W_SLOTS + k] : 0.0;
        }
        __syncthreads();
        for (uint32_t s = 0; s < cnt * COARSE_W_SLOTS; ++s) {
            const int32_t c = tcol[s];
            if (c >= 0 && (uint32_t)c <= j && ((uint32_t)c & (RB - 1)) == threadIdx.x) acc[c] += tval[s];
        }
    }
    for (uint32_t c = threadIdx.x; c <= j; c += RB) {      // (every lane reads the columns it owns: no barrier needed)
        G[(size_t)j * nc + c] = acc[c];
        G[(size_t)c * nc + j] = acc[c];
    }
}

// ---- Cholesky, left-looking, one launch per column j, a wavefront per row i >= j:
//   L(i, j) = (A(i, j) - sum_{k < j} L(i, k) L(j, k)) / L(j, j),   L(j, j)^2 = A(j, j) - sum_{k < j} L(j, k)^2
// both sums lane-strided over k, then the xor tree.  G holds A (symmetric); L(i, k), i > k, replaces the lower triangle row by row
// (G[i nc + k]) and, transposed, the upper one (G[k nc + i]: what the inverse reads along a column); the diagonal of L goes to
// ldiag and that of A stays, every wavefront of the launch reads it -------------------------------------------------------------------
__global__ __launch_bounds__(RB) void coarse_chol_column_kernel(uint32_t nc, uint32_t j, double *G, double *ldiag, int32_t *flags)
{
    if (flags[FLAG_PIVOT] != 0) return;
    const uint32_t i = j + blockIdx.x * (RB / 64) + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (i >= nc) return;                                 // (a whole wavefront leaves: the shuffles below stay complete)
    const double *Li = G + (size_t)i * nc, *Lj = G + (size_t)j * nc;
    double si = 0.0, sj = 0.0;
    for (uint32_t k = lane; k < j; k += 64) {
        const double lj = Lj[k];
        si += Li[k] * lj;
        sj += lj * lj;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { si += __shfl_xor(si, o, 64); sj += __shfl_xor(sj, o, 64); }
    if (lane != 0) return;
    const double d = Lj[j] - sj;
    if (i == j) {
        if (!(d > 0.0)) { ldiag[j] = 1.0; atomicCAS(&flags[FLAG_PIVOT], 0, (int32_t)(j + 1)); }
        else ldiag[j] = sqrt(d);
    } else {
        const double l = (Li[j] - si) / sqrt(d);
        G[(size_t)i * nc + j] = l;
        G[(size_t)j * nc + i] = l;
    }
}

// ---- W = L^-1 from W L = I, a workgroup per row i, right to left: W(i, i) = 1 / L(i, i),
//   W(i, l) = -(sum_{l < k <= i} W(i, k) L(k, l)) / L(l, l)
// the row of W in LDS, column l of L read along the upper triangle of G, the sum lane-strided and then block_sum's tree; packed row
// by row (row i at i (i + 1) / 2) ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RB) void coarse_inverse_kernel(uint32_t nc, const double *G, const double *ldiag, const int32_t *flags, double *W)
{
    __shared__ double w[COARSE_MAX_NODES];
    __shared__ double sh[RB / 64];
    if (flags[FLAG_PIVOT] != 0) return;
    const uint32_t i = blockIdx.x;
    if (threadIdx.x == 0) w[i] = 1.0 / ldiag[i];
    __syncthreads();
    for (uint32_t l = i; l-- > 0;) {
        const double *Ll = G + (size_t)l * nc;
        double s = 0.0;
        for (uint32_t k = l + 1 + threadIdx.x; k <= i; k += RB) s += w[k] * Ll[k];
        const double tot = block_sum(s, sh);
        if (threadIdx.x == 0) w[l] = -tot / ldiag[l];
        __syncthreads();
    }
    double *Wi = W + (size_t)i * (i + 1) / 2;
    for (uint32_t l = threadIdx.x; l <= i; l += RB) Wi[l] = w[l];
}

// ---- apply --------------------------------------------------------------------------------------------------------------------------
// rc_j = sum over row j of P^T: lane-strided, then block_sum's tree
__global__ __launch_bounds__(RB) void coarse_restrict_kernel(const uint32_t *pt_ptr, const int32_t *pt_rows, const double *pt_vals,
                                                             const double *r, double *rc)
{
    __shared__ double sh[RB / 64];
    double s = 0.0;
    for (uint32_t e = pt_ptr[blockIdx.x] + threadIdx.x; e < pt_ptr[blockIdx.x + 1]; e += RB) s += pt_vals[e] * r[pt_rows[e]];
    const double tot = block_sum(s, sh);
    if (threadIdx.x == 0) rc[blockIdx.x] = tot;
}

// t_i = sum_{j <= i} W(i, j) rc_j: a wavefront per row, lane-strided, then the xor tree
__global__ __launch_bounds__(RB) void coarse_lower_kernel(uint32_t nc, const double *W, const double *rc, double *t)
{
    const uint32_t i = blockIdx.x * (RB / 64) + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    double s = 0.0;
    if (i < nc) {
        const double *Wi = W + (size_t)i * (i + 1) / 2;
        for (uint32_t j = lane; j <= i; j += 64) s += Wi[j] * rc[j];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (i < nc && lane == 0) t[i] = s;
}

// u_l = sum_{i >= l} W(i, l) t_i: 64 columns x 4 row groups (i = l + g, l + g + 4, ..), the groups added as (0 + 1) + (2 + 3)
__global__ __launch_bounds__(RB) void coarse_upper_kernel(uint32_t nc, const double *W, const double *t, double *u)
{
    __shared__ double sh[RB];
    const uint32_t c = threadIdx.x & 63, g = threadIdx.x >> 6;
    const uint32_t l = blockIdx.x * 64 + c;
    double s = 0.0;
    if (l < nc)
        for (uint32_t i = l + g; i < nc; i += RB / 64) s += W[(size_t)i * (i + 1) / 2 + l] * t[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    if (g == 0 && l < nc) u[l] = (sh[c] + sh[64 + c]) + (sh[128 + c] + sh[192 + c]);
}

// z_i = (accumulate ? z_i : 0) + sum of row i of P times u, in entry order; the block partials of r . z
__global__ __launch_bounds__(RB) void coarse_prolong_kernel(size_t n, const int64_t *ptr, const int32_t *cols, const double *vals,
                                                            const double *u, int accumulate, const double *r, double *z, double *part_rz)
{
    __shared__ double sh[RB / 64];
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x;
    double rz = 0.0;
    if (i < n) {
        double s = accumulate ? z[i] : 0.0;
        for (int64_t q = ptr[i]; q < ptr[i + 1]; ++q) s += vals[q] * u[cols[q]];
        z[i] = s;
        rz = r[i] * s;
    }
    const double tot = block_sum(rz, sh);
    if (part_rz != nullptr && threadIdx.x == 0) part_rz[blockIdx.x] = tot;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
hipError_t coarse_check_ptr(hipStream_t stream, size_t n, size_t ncoarse, size_t max_nodes, const int64_t *ptr, uint64_t *entries_out,
                            int *refusal)
{
    *entries_out = 0;
    *refusal = COARSE_OK;
    if (ncoarse < 1 || ncoarse > max_nodes) { *refusal = max_nodes == (size_t)COARSE_MAX_NODES ? COARSE_BAD_NODES : COARSE_BAD_LEVEL_NODES; return hipSuccess; }
    if (n >= ((size_t)1 << 29)) { *refusal = COARSE_TOO_LARGE; return hipSuccess; }          // 4 n entries stay below 2^31
    int32_t *d_flags = nullptr;
    hipError_t e = hipMalloc((void **)&d_flags, NFLAGS * 4);
    if (e != hipSuccess) return e;
    int32_t h[NFLAGS] = {0, 0, 0, 0};
    int64_t entries = 0;
    e = hipMemsetAsync(d_flags, 0, NFLAGS * 4, stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(coarse_ptr_check_kernel, dim3((unsigned)((n + RB) / RB)), dim3(RB), 0, stream, n, ptr, d_flags);
        e = hipMemcpyAsync(h, d_flags, NFLAGS * 4, hipMemcpyDeviceToHost, stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&entries, ptr + n, 8, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    (void)hipFree(d_flags);
    if (e != hipSuccess) return e;
    if (h[FLAG_REFUSAL]) { *refusal = h[FLAG_REFUSAL]; return hipSuccess; }
    *entries_out = (uint64_t)entries;
    return hipSuccess;
}

hipError_t coarse_query(hipStream_t stream, size_t n, size_t ncoarse, const int64_t *ptr, CoarseSizes *out, int *refusal)
{
    *out = CoarseSizes();
    uint64_t entries = 0;
    const hipError_t e = coarse_check_ptr(stream, n, ncoarse, (size_t)COARSE_MAX_NODES, ptr, &entries, refusal);
    if (e != hipSuccess || *refusal) return e;
    out->entries = entries;
    size_t bytes = 0;
    pt_parts(nullptr, ncoarse, (size_t)entries, &bytes);
    out->pt_bytes = bytes;
    out->factor_doubles = (uint64_t)ncoarse * (ncoarse + 1) / 2;
    scratch_parts(nullptr, n, ncoarse, (size_t)entries, &bytes);
    out->scratch_bytes = bytes;
    return hipSuccess;
}

hipError_t coarse_validate(hipStream_t stream, const CoarseTable &t, const CoarseSizes &sz, void *scratch, int *refusal)
{
    const Scratch s = scratch_parts(scratch, t.n, t.ncoarse, (size_t)sz.entries, nullptr);
    return coarse_check_rows(stream, t, s.counts, s.flags, refusal);
}

hipError_t coarse_check_rows(hipStream_t stream, const CoarseTable &t, uint32_t *counts, int32_t *flags, int *refusal)
{
    *refusal = COARSE_OK;
    int32_t h[NFLAGS] = {0, 0, 0, 0};
    hipError_t e = hipMemsetAsync(counts, 0, (t.ncoarse + 2) * 4, stream);
    if (e == hipSuccess) e = hipMemsetAsync(flags, 0, NFLAGS * 4, stream);
    if (e != hipSuccess) return e;
    if (t.n)
        hipLaunchKernelGGL(coarse_rows_check_kernel, dim3(cg_vector_grid(t.n)), dim3(RB), 0, stream, t.n, (uint32_t)t.ncoarse, t.ptr, t.cols,
                           t.vals, counts, flags);
    e = hipMemcpyAsync(h, flags, NFLAGS * 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return e;
    *refusal = h[FLAG_REFUSAL];
    return hipSuccess;
}

// (the counts of coarse_validate are still in the scratch: the two are called back to back)
hipError_t coarse_galerkin(hipStream_t stream, const int64_t *rowptr, const int32_t *colind, const double *values, const CoarseTable &t,
                           const CoarseSizes &sz, const CoarseWindow *win, void *pt, void *scratch, int *refusal)
{
    *refusal = COARSE_OK;
    const uint32_t nc = (uint32_t)t.ncoarse;
    const Scratch s = scratch_parts(scratch, t.n, nc, (size_t)sz.entries, nullptr);
    const Transpose tr = pt_parts(pt, nc, (size_t)sz.entries, nullptr);
    const unsigned gr = cg_vector_grid(t.n), gc = (nc + 1 + RB - 1) / RB;
    int32_t h[NFLAGS] = {0, 0, 0, 0};
    // P^T
    hipLaunchKernelGGL(active_block_scan_kernel, dim3(1), dim3(SCAN_BLOCK), 0, stream, s.counts, nc);
    hipLaunchKernelGGL(coarse_pt_ptr_kernel, dim3(gc), dim3(RB), 0, stream, nc, s.counts, tr.ptr, s.cursor);
    if (t.n) hipLaunchKernelGGL(coarse_pt_fill_kernel, dim3(gr), dim3(RB), 0, stream, t.n, t.ptr, t.cols, t.vals, s.cursor, s.trow, s.tval);
    hipLaunchKernelGGL(coarse_pt_rank_kernel, dim3(nc), dim3(RB), 0, stream, tr.ptr, s.trow, s.tval, tr.rows, tr.vals);
    // W = A P, A_c = P^T W
    if (t.n) {
        if (win != nullptr)
            hipLaunchKernelGGL(coarse_w_kernel, dim3(gr), dim3(RB), 0, stream, t.n, rowptr, colind, values, win->col0, win->rows, win->ptr,
                               win->cols, win->vals, s.wcount, s.wcols, s.wvals, s.flags);
        else
            hipLaunchKernelGGL(coarse_w_kernel, dim3(gr), dim3(RB), 0, stream, t.n, rowptr, colind, values, (int64_t)0, t.n, t.ptr, t.cols,
                               t.vals, s.wcount, s.wcols, s.wvals, s.flags);
    }
    hipError_t e = hipMemcpyAsync(h, s.flags, NFLAGS * 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (h[FLAG_REFUSAL]) { *refusal = h[FLAG_REFUSAL]; return hipSuccess; }
    hipLaunchKernelGGL(coarse_galerkin_kernel, dim3(nc), dim3(RB), 0, stream, nc, tr.ptr, tr.rows, tr.vals, s.wcount, s.wcols, s.wvals, s.G);
    return hipGetLastError();
}

hipError_t coarse_cholesky(hipStream_t stream, const CoarseTable &t, const CoarseSizes &sz, double *factor, void *scratch,
                           double *coarse_matrix, int32_t *pivot)
{
    *pivot = 0;
    const uint32_t nc = (uint32_t)t.ncoarse;
    const Scratch s = scratch_parts(scratch, t.n, nc, (size_t)sz.entries, nullptr);
    int32_t h[NFLAGS] = {0, 0, 0, 0};
    hipError_t e = hipSuccess;
    if (coarse_matrix != nullptr) {
        e = hipMemcpyAsync(coarse_matrix, s.G, (size_t)nc * nc * 8, hipMemcpyDeviceToDevice, stream);
        if (e != hipSuccess) return e;
    }
    // Cholesky and the packed L^-1
    for (uint32_t j = 0; j < nc; ++j)
        hipLaunchKernelGGL(coarse_chol_column_kernel, dim3((nc - j + RB / 64 - 1) / (RB / 64)), dim3(RB), 0, stream, nc, j, s.G, s.ldiag, s.flags);
    hipLaunchKernelGGL(coarse_inverse_kernel, dim3(nc), dim3(RB), 0, stream, nc, s.G, s.ldiag, s.flags, factor);
    e = hipMemcpyAsync(h, s.flags, NFLAGS * 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return e;
    *pivot = h[FLAG_PIVOT];
    return hipSuccess;
}

hipError_t coarse_factor(hipStream_t stream, const int64_t *rowptr, const int32_t *colind, const double *values, const CoarseTable &t,
                         const CoarseSizes &sz, void *pt, double *factor, void *scratch, double *coarse_matrix, int32_t *pivot,
                         int *refusal)
{
    *pivot = 0;
    const hipError_t e = coarse_galerkin(stream, rowptr, colind, values, t, sz, nullptr, pt, scratch, refusal);
    if (e != hipSuccess || *refusal) return e;
    return coarse_cholesky(stream, t, sz, factor, scratch, coarse_matrix, pivot);
}

// ---- the rows of P beyond a rank's own: what the window of columns its rows read takes from the two neighbouring ranks.  A row
// travels as 8 doubles, four (column as double, value) pairs, padded with column -1 --------------------------------------------------
__global__ __launch_bounds__(RB) void coarse_rows_pack_kernel(size_t first, size_t count, const int64_t *ptr, const int32_t *cols,
                                                              const double *vals, double *out)
{
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x;
    if (i >= count) return;
    const int64_t p0 = ptr[first + i];
    const int m = (int)(ptr[first + i + 1] - p0);
    for (int k = 0; k < COARSE_MAX_ROW_ENTRIES; ++k) {
        out[8 * i + 2 * k] = k < m ? (double)cols[p0 + k] : -1.0;
        out[8 * i + 2 * k + 1] = k < m ? vals[p0 + k] : 0.0;
    }
}

// the entries of a packed row: up to the first pair whose column is no column of the table (the padding; bytes nobody wrote)
__device__ __forceinline__ uint32_t packed_row_entries(const double *row, uint32_t nc)
{
    uint32_t m = 0;
    while (m < (uint32_t)COARSE_MAX_ROW_ENTRIES && row[2 * m] >= 0.0 && row[2 * m] < (double)nc) ++m;
    return m;
}

// one block: the pointers and entries of the ghost rows on both sides of the n own rows, whose `entries` entries lie between them
__global__ __launch_bounds__(SCAN_BLOCK) void coarse_window_ghosts_kernel(uint32_t nc, size_t n, uint32_t entries, size_t need_lo,
                                                                          size_t need_hi, const double *recv_lo, const double *recv_hi,
                                                                          int64_t *wptr, int32_t *wcols, double *wvals)
{
    __shared__ uint32_t sh[SCAN_BLOCK / 64];
    uint32_t carry = 0;
    for (int side = 0; side < 2; ++side) {
        const size_t count = side ? need_hi : need_lo, row0 = side ? need_lo + n : 0;
        const double *recv = side ? recv_hi : recv_lo;
        for (size_t b0 = 0; b0 < count; b0 += SCAN_BLOCK) {
            const size_t i = b0 + threadIdx.x;
            const uint32_t m = i < count ? packed_row_entries(recv + 8 * i, nc) : 0u;
            uint32_t total;
            const uint32_t at = carry + block_exclusive_scan(m, sh, total);
            if (i < count) {
                wptr[row0 + i] = at;
                for (uint32_t k = 0; k < m; ++k) { wcols[at + k] = (int32_t)recv[8 * i + 2 * k]; wvals[at + k] = recv[8 * i + 2 * k + 1]; }
            }
            carry += total;
        }
        if (threadIdx.x == 0) wptr[row0 + count] = carry;      // (below: where the own rows start; above: the end of the window)
        carry += side ? 0u : entries;
    }
}

// the own rows between the ghosts: pointers moved by the entries of the ghosts below, entries copied
__global__ __launch_bounds__(RB) void coarse_window_own_kernel(size_t n, uint32_t entries, size_t need_lo, const int64_t *ptr,
                                                               const int32_t *cols, const double *vals, int64_t *wptr, int32_t *wcols,
                                                               double *wvals)
{
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x;
    const int64_t base = wptr[need_lo];
    if (i >= 1 && i < n) wptr[need_lo + i] = base + ptr[i];
    if (i < entries) { wcols[base + i] = cols[i]; wvals[base + i] = vals[i]; }
}

void coarse_rows_pack(hipStream_t stream, const CoarseTable &t, size_t first, size_t count, double *out)
{
    if (count) hipLaunchKernelGGL(coarse_rows_pack_kernel, dim3(cg_vector_grid(count)), dim3(RB), 0, stream, first, count, t.ptr, t.cols, t.vals, out);
}

void coarse_window_build(hipStream_t stream, const CoarseTable &t, const CoarseSizes &sz, size_t need_lo, size_t need_hi,
                         const double *recv_lo, const double *recv_hi, int64_t *wptr, int32_t *wcols, double *wvals)
{
    const uint32_t entries = (uint32_t)sz.entries;
    hipLaunchKernelGGL(coarse_window_ghosts_kernel, dim3(1), dim3(SCAN_BLOCK), 0, stream, (uint32_t)t.ncoarse, t.n, entries, need_lo, need_hi,
                       recv_lo, recv_hi, wptr, wcols, wvals);
    const size_t items = t.n > (size_t)entries ? t.n : (size_t)entries;
    if (items)
        hipLaunchKernelGGL(coarse_window_own_kernel, dim3(cg_vector_grid(items)), dim3(RB), 0, stream, t.n, entries, need_lo, t.ptr, t.cols,
                           t.vals, wptr, wcols, wvals);
}

// ---- the lower triangle of A_c as the ranks add it: packed row by row (row i at i (i + 1) / 2), and back into both halves of G ------
__global__ __launch_bounds__(RB) void coarse_triangle_kernel(uint32_t nc, int unpack, double *G, double *tri)
{
    const size_t q = (size_t)blockIdx.x * RB + threadIdx.x;
    if (q >= (size_t)nc * nc) return;
    const uint32_t i = (uint32_t)(q / nc), j = (uint32_t)(q % nc);
    if (j > i) return;
    const size_t at = (size_t)i * (i + 1) / 2 + j;
    if (unpack) { const double v = tri[at]; G[(size_t)i * nc + j] = v; G[(size_t)j * nc + i] = v; }
    else tri[at] = G[q];
}

void coarse_matrix_triangle(hipStream_t stream, const CoarseTable &t, const CoarseSizes &sz, void *scratch, int unpack, double *tri)
{
    const uint32_t nc = (uint32_t)t.ncoarse;
    const Scratch s = scratch_parts(scratch, t.n, nc, (size_t)sz.entries, nullptr);
    hipLaunchKernelGGL(coarse_triangle_kernel, dim3(cg_vector_grid((size_t)nc * nc)), dim3(RB), 0, stream, nc, unpack, s.G, tri);
}

void coarse_apply(hipStream_t stream, const CoarseTable &t, const CoarseSizes &sz, const void *pt, const double *factor, void *scratch,
                  int accumulate, const double *r, double *z, double *part_rz)
{
    if (t.n == 0) return;
    coarse_restrict(stream, t, sz, pt, scratch, r);
    coarse_correct(stream, t, sz, factor, scratch, accumulate, r, z, part_rz);
}

double *coarse_restrict(hipStream_t stream, const CoarseTable &t, const CoarseSizes &sz, const void *pt, void *scratch, const double *r)
{
    const uint32_t nc = (uint32_t)t.ncoarse;
    const Scratch s = scratch_parts(scratch, t.n, nc, (size_t)sz.entries, nullptr);
    const Transpose tr = pt_parts(pt, nc, (size_t)sz.entries, nullptr);
    hipLaunchKernelGGL(coarse_restrict_kernel, dim3(nc), dim3(RB), 0, stream, tr.ptr, tr.rows, tr.vals, r, s.vec);
    return s.vec;
}

const double *coarse_solve(hipStream_t stream, const CoarseTable &t, const CoarseSizes &sz, const double *factor, void *scratch)
{
    const uint32_t nc = (uint32_t)t.ncoarse;
    const Scratch s = scratch_parts(scratch, t.n, nc, (size_t)sz.entries, nullptr);
    double *rc = s.vec, *tt = s.vec + nc, *u = s.vec + 2 * (size_t)nc;
    hipLaunchKernelGGL(coarse_lower_kernel, dim3((nc + RB / 64 - 1) / (RB / 64)), dim3(RB), 0, stream, nc, factor, rc, tt);
    hipLaunchKernelGGL(coarse_upper_kernel, dim3((nc + 63) / 64), dim3(RB), 0, stream, nc, factor, tt, u);
    return u;
}

void coarse_correct(hipStream_t stream, const CoarseTable &t, const CoarseSizes &sz, const double *factor, void *scratch, int accumulate,
                    const double *r, double *z, double *part_rz)
{
    const uint32_t nc = (uint32_t)t.ncoarse;
    const Scratch s = scratch_parts(scratch, t.n, nc, (size_t)sz.entries, nullptr);
    const double *u = coarse_solve(stream, t, sz, factor, scratch);
    hipLaunchKernelGGL(coarse_prolong_kernel, dim3(cg_vector_grid(t.n)), dim3(RB), 0, stream, t.n, t.ptr, t.cols, t.vals, u, accumulate, r, z,
                       part_rz);
}

// ---- the coarse table of the face-only system ---------------------------------------------------------------------------------------
// Coarse lines of a direction with N cells: the vertex indices 0, H, 2 H, .. below N, and N.  Hats live in index space; the values
// below are the table's definition and are formed without contraction: one division per 1-D hat, one product per 2-D hat.
#pragma clang fp contract(off)
namespace {

__device__ __forceinline__ int cl_lines(int N, int H) { return (N + H - 1) / H + 1; }
__device__ __forceinline__ int cl_pos(int j, int N, int H) { const long p = (long)j * H; return p < N ? (int)p : N; }
__device__ __forceinline__ double cl_hat(int j, int i, int N, int H)
{
    const int nl = cl_lines(N, H), lj = cl_pos(j, N, H);
    if (i == lj) return 1.0;
    if (j > 0) {
        const int lm = cl_pos(j - 1, N, H);
        if (i > lm && i < lj) return (double)(i - lm) / (double)(lj - lm);
    }
    if (j < nl - 1) {
        const int lp = cl_pos(j + 1, N, H);
        if (i > lj && i < lp) return (double)(lp - i) / (double)(lp - lj);
    }
    return 0.0;
}

struct FaceHats { int n = 0; int32_t node[4]; double v0[4], v1[4]; };

// the interior nodes whose hat does not vanish at both of the points pa, pb (a face's ends), in node order, with the values of the
// face's two lowest modes
__device__ __forceinline__ FaceHats point_hats(const StructuredMesh &sm, int H, uint32_t pa, uint32_t pb)
{
    FaceHats o;
    const int Nx = (int)sm.Nx, Ny = (int)sm.Ny, npr = Nx + 1;
    const int ax = (int)(pa % npr), ay = (int)(pa / npr), bx = (int)(pb % npr), by = (int)(pb / npr);
    const int nlx = cl_lines(Nx, H), nly = cl_lines(Ny, H), nix = nlx - 2;
    const int x0 = (ax < bx ? ax : bx) / H, x1 = (ax < bx ? bx : ax) / H + 1;
    const int y0 = (ay < by ? ay : by) / H, y1 = (ay < by ? by : ay) / H + 1;
    for (int jy = y0 < 1 ? 1 : y0; jy <= y1 && jy <= nly - 2; ++jy)
        for (int jx = x0 < 1 ? 1 : x0; jx <= x1 && jx <= nlx - 2; ++jx) {
            const double fa = cl_hat(jx, ax, Nx, H) * cl_hat(jy, ay, Ny, H);
            const double fb = cl_hat(jx, bx, Nx, H) * cl_hat(jy, by, Ny, H);
            if ((fa != 0.0 || fb != 0.0) && o.n < 4) {
                o.node[o.n] = (jy - 1) * nix + (jx - 1);
                o.v0[o.n] = 0.5 * (fa + fb);
                o.v1[o.n] = 0.5 * (fb - fa);
                ++o.n;
            }
        }
    return o;
}

// what face f gives: its hats, and the nb blocks that take them, each with its part; unowned: the block a face counted by the
// numbering leaves without an owner (-1: none), whose pointers are still due.  The default value is a face that gives nothing.
struct FaceBlocks { FaceHats h; int nb = 0; int32_t q[2]; int part[2]; int32_t unowned = -1; };

// the numbering of pa_condensed_csr_pattern: the one block of a non-Dirichlet face
__device__ __forceinline__ FaceBlocks face_blocks(const CoarseMesh &m, int H, uint32_t f)
{
    FaceBlocks o;
    const int32_t q = m.face_compress[f];
    if (q < 0) return o;
    o.nb = 1; o.q[0] = q; o.part[0] = 0;
    if (m.face_loc != nullptr) {
        const int loc = m.face_loc[f];
        o.part[0] = (loc != 2 && loc != m.where) ? 1 : 0;              // 2: PA_LOC_ON_INTERFACE
    }
    o.h = point_hats(m.sm, H, m.face_pts[2 * f], m.face_pts[2 * f + 1]);
    return o;
}

// interface_assembler's numbering: the two blocks of a cut face take the same values (the face basis of a cut face is the whole
// face's, cuthho_square.cpp:371, 471, 594), block b in part 0 and block b + 1 in part 1 by side; an uncut face's block is in the
// part of its side
__device__ __forceinline__ void if_owned_blocks(FaceBlocks &o, int32_t b, bool cut, int loc, bool by_side)
{
    o.nb = cut ? 2 : 1;
    o.q[0] = b; o.q[1] = b + 1;
    o.part[0] = (by_side && !cut && loc == 1) ? 1 : 0;                 // 1: PA_LOC_POSITIVE
    o.part[1] = by_side ? 1 : 0;
}

// A cut face on the Dirichlet boundary is counted and owns nothing: its block follows the blocks of the nearest owning face below
// it and the unowned blocks between the two.  -> that block; *found: there is an owning face below f (none: the unowned blocks
// below f alone were counted)
__device__ __forceinline__ int32_t if_unowned_block(const IfCsrMesh &im, uint32_t f, bool *found)
{
    int32_t at = 0;
    *found = false;
    for (uint32_t g = f; g-- > 0;) {
        const int32_t bg = im.face_table[g];
        const bool cg = im.face_loc[g] == IF_LOC_CUT;
        if (bg >= 0) { *found = true; return at + bg + (cg ? 2 : 1); }
        at += cg ? 1 : 0;
    }
    return at;
}

// the whole mesh of the interface problem: a face's end points from face_pts
__device__ __forceinline__ FaceBlocks face_blocks(const IfCoarseMesh &m, int H, uint32_t f)
{
    FaceBlocks o;
    const int32_t b = m.im.face_table[f];
    const bool cut = m.im.face_loc[f] == IF_LOC_CUT;
    if (b < 0) {
        bool found;
        if (cut) o.unowned = if_unowned_block(m.im, f, &found);
        return o;
    }
    if_owned_blocks(o, b, cut, m.im.face_loc[f], m.by_side != 0);
    o.h = point_hats(m.sm, H, m.face_pts[2 * f], m.face_pts[2 * f + 1]);
    return o;
}

// a slab of the generator mesh in closed form (structured_mesh.hpp): local face f is global face sm_face_base + f, and the slab owns
// the compressed faces [p0, p1), block q - p0 of its rows
__device__ __forceinline__ FaceBlocks face_blocks(const SlabCoarseMesh &m, int H, uint32_t f)
{
    FaceBlocks o;
    uint32_t lo, hi;
    bool dirichlet;
    int32_t q;
    sm_face_decode(m.sm, sm_face_base(m.sm) + f, lo, hi, dirichlet, q);
    if (dirichlet || q < m.p0 || q >= m.p1) return o;
    o.nb = 1; o.q[0] = q - m.p0; o.part[0] = 0;
    o.h = point_hats(m.sm, H, lo, hi);
    return o;
}

// a slab of the interface problem (interface_rows.hpp): im holds the extended tables -- the slab's faces and the halo row's below
// them --, extended face f is global face face0 + f, whose end points the closed form gives, and the slab owns the extended blocks
// [q0, q1), block q - q0 of its rows.  The halo row's faces give nothing.  An unowned block follows the nearest owning face below
// it as on the whole mesh; where there is none in the extended range it precedes the range's first owning face, whose block is 0.
__device__ __forceinline__ FaceBlocks face_blocks(const IfRowsCoarseMesh &m, int H, uint32_t f)
{
    FaceBlocks o;
    const int32_t b = m.im.face_table[f];
    const bool cut = m.im.face_loc[f] == IF_LOC_CUT;
    if (b < 0) {
        if (!cut) return o;
        bool found;
        int32_t at = if_unowned_block(m.im, f, &found);
        if (!found) {                                    // f and the unowned blocks up to the first owning face: below block 0
            at = 0;
            for (uint32_t g = f; g < m.im.nfaces && m.im.face_table[g] < 0; ++g) at -= m.im.face_loc[g] == IF_LOC_CUT ? 1 : 0;
        }
        if (at >= m.q0 && at < m.q1) o.unowned = at - m.q0;
        return o;
    }
    if (b < m.q0 || b >= m.q1) return o;                 // (both blocks of a cut face are owned together)
    if_owned_blocks(o, b - m.q0, cut, m.im.face_loc[f], m.by_side != 0);
    uint32_t lo, hi;
    bool dirichlet;
    int32_t comp;
    sm_face_decode(m.sm, m.face0 + f, lo, hi, dirichlet, comp);
    o.h = point_hats(m.sm, H, lo, hi);
    return o;
}

// the tags of the whole mesh, which every rank of a row partition holds: what face f gives to the parts by side -- the hats and
// parts of face_blocks(IfCoarseMesh), no blocks to write to
struct IfTagsMesh { StructuredMesh sm; const int8_t *face_loc; };
__device__ __forceinline__ FaceBlocks face_blocks(const IfTagsMesh &m, int H, uint32_t f)
{
    FaceBlocks o;
    uint32_t lo, hi;
    bool dirichlet;
    int32_t comp;
    sm_face_decode(m.sm, f, lo, hi, dirichlet, comp);
    if (dirichlet) return o;
    if_owned_blocks(o, 0, m.face_loc[f] == IF_LOC_CUT, m.face_loc[f], true);
    o.h = point_hats(m.sm, H, lo, hi);
    return o;
}

__device__ __forceinline__ uint32_t face_entries(const FaceBlocks &b, int fbs)
{
    uint32_t e = (uint32_t)b.h.n;
    if (fbs >= 2)
        for (int k = 0; k < b.h.n; ++k) e += b.h.v1[k] != 0.0 ? 1u : 0u;
    return e * (uint32_t)b.nb;
}

inline uint32_t coarse_faces(const CoarseMesh &m) { return m.nfaces; }
inline uint32_t coarse_faces(const IfCoarseMesh &m) { return m.im.nfaces; }
inline uint32_t coarse_faces(const SlabCoarseMesh &m) { return (m.sm.row1 - m.sm.row0) * sm_face_row(m.sm); }
inline uint64_t coarse_blocks(const CoarseMesh &m) { return sm_num_other_faces(m.sm); }
inline uint64_t coarse_blocks(const IfCoarseMesh &m) { return m.im.num_other_faces; }
inline uint64_t coarse_blocks(const SlabCoarseMesh &m) { return (uint64_t)(m.p1 - m.p0); }
inline bool coarse_by_side(const CoarseMesh &m) { return m.face_loc != nullptr; }
inline bool coarse_by_side(const IfCoarseMesh &m) { return m.by_side != 0; }
inline uint32_t coarse_faces(const IfRowsCoarseMesh &m) { return m.im.nfaces; }
inline uint64_t coarse_blocks(const IfRowsCoarseMesh &m) { return (uint64_t)(m.q1 - m.q0); }
inline bool coarse_by_side(const SlabCoarseMesh &) { return false; }
inline bool coarse_by_side(const IfRowsCoarseMesh &m) { return m.by_side != 0; }

// by side: used[part nnodes + node] = some block of the part meets the node's hat (every writer stores the same byte)
template <class Mesh>
__global__ __launch_bounds__(RB) void coarse_used_kernel(Mesh m, uint32_t nfaces, int H, uint32_t nnodes, uint8_t *used)
{
    const uint32_t f = blockIdx.x * RB + threadIdx.x;
    if (f >= nfaces) return;
    const FaceBlocks b = face_blocks(m, H, f);
    for (int s = 0; s < b.nb; ++s)
        for (int k = 0; k < b.h.n; ++k) used[(size_t)b.part[s] * nnodes + b.h.node[k]] = 1;
}

// the faces that decide which columns stay: the table's own, or -- a slab -- the whole mesh's by its tags
template <class Mesh>
void coarse_mark_used(hipStream_t stream, const Mesh &m, int H, uint32_t nnodes, uint8_t *used)
{
    const uint32_t nfaces = coarse_faces(m);
    hipLaunchKernelGGL((coarse_used_kernel<Mesh>), dim3((nfaces + RB - 1) / RB), dim3(RB), 0, stream, m, nfaces, H, nnodes, used);
}
void coarse_mark_used(hipStream_t stream, const IfRowsCoarseMesh &m, int H, uint32_t nnodes, uint8_t *used)
{
    const IfTagsMesh tags{m.sm, m.face_loc_all};
    hipLaunchKernelGGL((coarse_used_kernel<IfTagsMesh>), dim3((m.nfaces_all + RB - 1) / RB), dim3(RB), 0, stream, tags, m.nfaces_all, H, nnodes,
                       used);
}

// per block of faces: its entries
template <class Mesh>
__global__ __launch_bounds__(SCAN_BLOCK) void coarse_count_kernel(Mesh m, uint32_t nfaces, int H, int fbs, uint32_t *blk)
{
    __shared__ uint32_t sh[SCAN_BLOCK / 64];
    const uint32_t f = blockIdx.x * SCAN_BLOCK + threadIdx.x;
    uint32_t e = 0;
    if (f < nfaces) e = face_entries(face_blocks(m, H, f), fbs);
    uint32_t total;
    block_exclusive_scan(e, sh, total);
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

// blk scanned (the total at [nblk]): every face writes, for each of its blocks, the pointers of the fbs rows and the entries of the
// first two, and the pointers of a block it leaves unowned; column: the node's (index = null) or index[part nnodes + node]
template <class Mesh>
__global__ __launch_bounds__(SCAN_BLOCK) void coarse_fill_kernel(Mesh m, uint32_t nfaces, int H, int fbs, uint32_t nnodes,
                                                                 const int32_t *index, const uint32_t *blk, uint32_t nblk, uint64_t nrows,
                                                                 int64_t *ptr, int32_t *cols, double *vals)
{
    __shared__ uint32_t sh[SCAN_BLOCK / 64];
    const uint32_t f = blockIdx.x * SCAN_BLOCK + threadIdx.x;
    FaceBlocks b;
    if (f < nfaces) b = face_blocks(m, H, f);
    const uint32_t e = face_entries(b, fbs);
    uint32_t total;
    int64_t at = (int64_t)blk[blockIdx.x] + block_exclusive_scan(e, sh, total);
    if (f == 0) ptr[nrows] = (int64_t)blk[nblk];
    if (b.unowned >= 0)
        for (int k = 0; k < fbs; ++k) ptr[(int64_t)b.unowned * fbs + k] = at;
    for (int s = 0; s < b.nb; ++s) {
        const int64_t row0 = (int64_t)b.q[s] * fbs;
        const int32_t *col = index != nullptr ? index + (size_t)b.part[s] * nnodes : nullptr;
        ptr[row0] = at;
        for (int k = 0; k < b.h.n; ++k) {
            cols[at] = col != nullptr ? col[b.h.node[k]] : b.h.node[k];
            vals[at] = b.h.v0[k];
            ++at;
        }
        if (fbs >= 2) {
            ptr[row0 + 1] = at;
            for (int k = 0; k < b.h.n; ++k)
                if (b.h.v1[k] != 0.0) {
                    cols[at] = col != nullptr ? col[b.h.node[k]] : b.h.node[k];
                    vals[at] = b.h.v1[k];
                    ++at;
                }
        }
        for (int k = 2; k < fbs; ++k) ptr[row0 + k] = at;
    }
}

// the table of either numbering: the columns (by side: the used ones, scanned), the entries (counted, scanned), the fill
template <class Mesh>
hipError_t coarse_table(hipStream_t stream, const Mesh &m, int fbs, int H, uint64_t max_columns, uint64_t *ncoarse, uint64_t *entries,
                        int64_t *ptr, int32_t *cols, double *vals)
{
    *ncoarse = 0;
    *entries = 0;
    const uint32_t nfaces = coarse_faces(m);
    const uint64_t nix = (m.sm.Nx + (uint64_t)H - 1) / H, niy = (m.sm.Ny + (uint64_t)H - 1) / H;
    if (nix < 2 || niy < 2) return hipSuccess;                          // no interior line in some direction
    const uint64_t nn64 = (nix - 1) * (niy - 1);
    if (nn64 >= ((uint64_t)1 << 30)) { *ncoarse = nn64; return hipSuccess; }
    const uint32_t nnodes = (uint32_t)nn64;
    DeviceTmp tmp(stream);
    int32_t *index = nullptr;
    if (!coarse_by_side(m)) {
        *ncoarse = nnodes;
    } else {
        const uint32_t items = 2 * nnodes;
        uint8_t *used = nullptr;
        uint32_t *counts = nullptr, total = 0;
        int32_t *unused = nullptr;
        if (!tmp.alloc(&used, items) || !tmp.alloc(&counts, (size_t)scan_tiles(items) + 1) || !tmp.alloc(&unused, items) ||
            !tmp.alloc(&index, items))
            return tmp.error();
        if (!tmp.ok(hipMemsetAsync(used, 0, items, stream))) return tmp.error();
        coarse_mark_used(stream, m, H, nnodes, used);
        if (!tmp.ok(scan_flags(stream, used, items, counts, unused, index, &total))) return tmp.error();
        *ncoarse = total;
    }
    const uint32_t nblk = (nfaces + SCAN_BLOCK - 1) / SCAN_BLOCK;
    uint32_t *blk = nullptr, total = 0;
    if (!tmp.alloc(&blk, (size_t)nblk + 1)) return tmp.error();
    hipLaunchKernelGGL((coarse_count_kernel<Mesh>), dim3(nblk), dim3(SCAN_BLOCK), 0, stream, m, nfaces, H, fbs, blk);
    if (!tmp.ok(scan_block_counts(stream, nblk, blk, &total))) return tmp.error();
    *entries = total;
    if (ptr == nullptr || *ncoarse < 1 || *ncoarse > max_columns) return hipSuccess;
    const uint64_t nrows = coarse_blocks(m) * fbs;
    hipLaunchKernelGGL((coarse_fill_kernel<Mesh>), dim3(nblk), dim3(SCAN_BLOCK), 0, stream, m, nfaces, H, fbs, nnodes, index, blk, nblk, nrows, ptr,
                       cols, vals);
    if (tmp.ok(hipGetLastError())) tmp.ok(hipStreamSynchronize(stream));       // the temporaries live until the kernel has read them
    return tmp.error();
}

}  // namespace

hipError_t condensed_coarse(hipStream_t stream, const CoarseMesh &m, int fbs, int H, uint64_t max_columns, uint64_t *ncoarse,
                            uint64_t *entries, int64_t *ptr, int32_t *cols, double *vals)
{
    return coarse_table(stream, m, fbs, H, max_columns, ncoarse, entries, ptr, cols, vals);
}

hipError_t condensed_rows_coarse(hipStream_t stream, const SlabCoarseMesh &m, int fbs, int H, uint64_t *ncoarse, uint64_t *entries,
                                 int64_t *ptr, int32_t *cols, double *vals)
{
    return coarse_table(stream, m, fbs, H, (uint64_t)COARSE_MAX_NODES, ncoarse, entries, ptr, cols, vals);
}

hipError_t interface_condensed_coarse(hipStream_t stream, const IfCoarseMesh &m, int fbs, int H, uint64_t max_columns, uint64_t *ncoarse,
                                      uint64_t *entries, int64_t *ptr, int32_t *cols, double *vals)
{
    return coarse_table(stream, m, fbs, H, max_columns, ncoarse, entries, ptr, cols, vals);
}

hipError_t interface_rows_coarse(hipStream_t stream, const IfRowsCoarseMesh &m, int fbs, int H, uint64_t *ncoarse, uint64_t *entries,
                                 int64_t *ptr, int32_t *cols, double *vals)
{
    return coarse_table(stream, m, fbs, H, (uint64_t)COARSE_MAX_NODES, ncoarse, entries, ptr, cols, vals);
}

}  // namespace pa
