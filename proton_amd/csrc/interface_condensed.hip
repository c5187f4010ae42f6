// interface_condensed.hip -- the interface problem's global system (apps/cuthho/cuthho_square.cpp:1091-1443) condensed to its face
// unknowns on the device.
//
// Every cell block of interface_assembler's system couples only inside its cell, so the cell unknowns are eliminated cell by cell:
// S = A_FF - A_FT A_TT^-1 A_TF and g = -A_FT A_TT^-1 f_T of each cell's local matrix.  What is left is the same numbering without
// its cell blocks: unknown k of face block b at (face_table[F] + b) fbs + k.  Uncut cells are condensed in double by the plain
// mesh's static_condensation_kernel (hho_aux.hpp); a cut cell, whose [cell-, cell+] block A_TT has condition numbers to 1e8, in
// double-double (ifcond_cut_kernel): a Cholesky factorization of A_TT and the forward substitutions of the NF + 1 columns
// [A_TF | f_T], S = A_FF - W^T W and g = -W^T w_f with W = L^-1 A_TF, w_f = L^-1 f_T, rounded to double once.  The cut cell's local
// matrix is symmetric (cut_interface_lc_kernel stores both copies of data and of the stabilization), so A_FT = A_TF^T.
//
// The face-only CSR reuses the symbolic tables of interface_csr.hip: a face group's row is its cell units (a prefix of the sorted
// units: cell blocks come first in the numbering) followed by its face units; the condensed row keeps the face units.  The fill is
// the same gather (one wavefront per face group), reading the packed records instead of the local matrices; addends are summed in
// push order (cells ascending, local row, local column) from the first addend.  The right-hand side moves the Dirichlet columns of
// uncut cells to the right (g_i - sum_j S_ij u_D,j, as condensed_triplets_kernel); a cut cell's slots on a Dirichlet face are
// dropped, as pa_interface_triplets_batch drops them.  Bit-identical to pa_csr_from_triplets of ifcond_triplets_kernel's slots
// taken in cell order (tests/test_gpu_interface_condensed.py).
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include <cstdint>

#include "dd_arith.hpp"
#include "interface_csr.hpp"

namespace pa {

namespace {

constexpr int8_t IFD_LOC_CUT = 2;          // LOC_CUT of cut_host.hpp

inline unsigned blocks_for(size_t n) { return (unsigned)(n ? (n + 255) / 256 : 1); }

struct IfdDims {
    int cbs, fbs;
};
__host__ __device__ __forceinline__ IfdDims ifd_dims(int face_deg) { return {(face_deg + 3) * (face_deg + 2) / 2, face_deg + 1}; }

// entry (i, j) of a packed upper triangle
__device__ __forceinline__ double ifd_S(const double *S, int i, int j)
{
    const int a = i < j ? i : j, b = i < j ? j : i;
    return S[b * (b + 1) / 2 + a];
}

// the face part of a face group's row: first face unit, its position (= the cell units' width) and the condensed row length
__device__ __forceinline__ void ifd_face_units(const IfGroup &G, const IfUnit *units, int32_t cell_cols, int &u0, uint32_t &poff,
                                               uint32_t &Rc)
{
    u0 = G.nunits;
    for (int s = G.nunits - 1; s >= 0; --s)
        if (units[G.ustart + s].gcol >= cell_cols) u0 = s;
    poff = u0 < G.nunits ? units[G.ustart + u0].pos : G.R;
    Rc = G.R - poff;
}

// ---- symbolic: entries per face group, scanned --------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ifd_count_kernel(IfCsrMesh m, IfdDims d, const IfGroup *groups, const IfUnit *units,
                                                        uint64_t *gnnz)
{
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q > m.num_other_faces) return;
    if (q == m.num_other_faces) { gnnz[q] = 0; return; }
    const IfGroup G = groups[m.num_all_cells + q];
    int u0;
    uint32_t poff, Rc;
    ifd_face_units(G, units, (int32_t)m.num_all_cells * d.cbs, u0, poff, Rc);
    gnnz[q] = (uint64_t)Rc * (uint64_t)d.fbs;
}

// ---- pattern: one thread per row ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ifd_pattern_kernel(IfCsrMesh m, IfdDims d, uint64_t nrows, uint64_t nnz, const IfGroup *groups,
                                                          const IfUnit *units, const uint64_t *cvstart, int64_t *rowptr, int32_t *colind)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > nrows) return;
    if (r == nrows) { rowptr[r] = (int64_t)nnz; return; }
    const uint32_t q = (uint32_t)(r / d.fbs), i = (uint32_t)(r % d.fbs);
    const IfGroup G = groups[m.num_all_cells + q];
    const int32_t cell_cols = (int32_t)m.num_all_cells * d.cbs;
    int u0;
    uint32_t poff, Rc;
    ifd_face_units(G, units, cell_cols, u0, poff, Rc);
    const uint64_t start = cvstart[q] + (uint64_t)i * Rc;
    rowptr[r] = (int64_t)start;
    if (colind == nullptr) return;
    for (int s = u0; s < G.nunits; ++s) {
        const IfUnit U = units[G.ustart + s];
        for (int k = 0; k < U.width; ++k) colind[start + (U.pos - poff) + k] = U.gcol - cell_cols + k;
    }
}

// ---- numeric phase --------------------------------------------------------------------------------------------------------
struct IfdCell {
    const double *S, *g;        // the cell's packed S and its g
    int off;                    // local index of its first face unknown in the local matrix (cbs, or 2 cbs for a cut cell)
    bool cut;
};
__device__ __forceinline__ IfdCell ifd_cell(const IfCsrMesh &m, IfdDims d, const IfCondArgs &a, int32_t X)
{
    IfdCell c;
    c.cut = m.cell_loc[X] == IFD_LOC_CUT;
    if (c.cut) {
        const int NF = 8 * d.fbs, ntri = NF * (NF + 1) / 2;
        const size_t cc = (size_t)m.cut_index[X];
        c.S = a.cond_cut + cc * ntri; c.g = a.cond_cut + (size_t)a.ncut * ntri + cc * NF; c.off = 2 * d.cbs;
    } else {
        const int nf = 4 * d.fbs, ntri = nf * (nf + 1) / 2;
        c.S = a.cond + (size_t)X * ntri; c.g = a.cond + (size_t)m.ncells * ntri + (size_t)X * nf; c.off = d.cbs;
    }
    return c;
}

// right-hand-side contribution of record row `row` of cell X: g_row, less the Dirichlet columns times the boundary data for an
// uncut cell (accumulated in local column order, as cond_rhs_contrib of condensed.hip); a cut cell's Dirichlet slots are dropped
__device__ __forceinline__ double ifd_rhs_contrib(const IfCsrMesh &m, IfdDims d, const IfCondArgs &a, int32_t X, const IfdCell &c, int row)
{
    double s = c.g[row];
    if (c.cut) return s;
    for (int lf = 0; lf < 4; ++lf) {
        const uint32_t f = m.cell_faces[4 * (size_t)X + lf];
        if (m.face_table[f] >= 0) continue;
        for (int kp = 0; kp < d.fbs; ++kp) {
            const double dd_ = a.g != nullptr ? a.g[(size_t)f * d.fbs + kp] : 0.0;
            s -= ifd_S(c.S, row, lf * d.fbs + kp) * dd_;
        }
    }
    return s;
}

// one wavefront per face group, four groups per block
__global__ __launch_bounds__(256) void ifd_fill_kernel(IfCsrMesh m, IfdDims d, const IfGroup *__restrict__ groups,
                                                       const IfUnit *__restrict__ units, const uint64_t *__restrict__ cvstart,
                                                       IfCondArgs a, double *values, double *RHS)
{
    const uint32_t lane = threadIdx.x % 64u;
    const uint32_t q = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + threadIdx.x / 64u);
    if (q >= m.num_other_faces) return;
    const IfGroup G = groups[m.num_all_cells + q];
    int u0;
    uint32_t poff, Rc;
    ifd_face_units(G, units, (int32_t)m.num_all_cells * d.cbs, u0, poff, Rc);
    IfdCell C[2];
    uint32_t rc[2] = {0u, 0u};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int32_t X = G.cell[s];
        if (X < 0) { C[s] = IfdCell{a.cond, a.cond, 0, false}; continue; }
        C[s] = ifd_cell(m, d, a, X);
        rc[s] = (G.rcode >> (16 * s)) & 0xffffu;
    }
    const uint32_t total = (uint32_t)d.fbs * Rc;
    const IfUnit *U = units + G.ustart;
    const uint64_t vs = cvstart[q];
    for (uint32_t e = lane; e < total; e += 64u) {
        const uint32_t i = e / Rc, pos = e - i * Rc + poff;
        uint32_t upos = U[u0].pos, ucode = U[u0].ccode;
        for (int u = u0 + 1; u < G.nunits; ++u)
            if (pos >= U[u].pos) { upos = U[u].pos; ucode = U[u].ccode; }
        const uint32_t k = pos - upos;
        // all (at most 8) addends loaded first, then summed in push order: cell, local row, local column
        double v[2][2][2];
        bool on[2][2][2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const uint32_t cc = (ucode >> (16 * s)) & 0xffffu;
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    on[s][r][c] = r < ifc_count(rc[s]) && c < ifc_count(cc);
                    const int row = (r == 0 ? ifc_first(rc[s]) : ifc_second(rc[s])) + (int)i - C[s].off;
                    const int col = (c == 0 ? ifc_first(cc) : ifc_second(cc)) + (int)k - C[s].off;
                    v[s][r][c] = on[s][r][c] ? ifd_S(C[s].S, row, col) : 0.0;
                }
        }
        double acc = 0.0;
        bool first = true;
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int c = 0; c < 2; ++c)
                    if (on[s][r][c]) { acc = first ? v[s][r][c] : acc + v[s][r][c]; first = false; }
        values[vs + e] = acc;
    }
    if (RHS != nullptr && lane < (uint32_t)d.fbs) {
        double acc = 0.0;
        bool first = true;
        for (int s = 0; s < 2; ++s) {
            for (int r = 0; r < ifc_count(rc[s]); ++r) {
                const int row = (r == 0 ? ifc_first(rc[s]) : ifc_second(rc[s])) + (int)lane - C[s].off;
                const double w = ifd_rhs_contrib(m, d, a, G.cell[s], C[s], row);
                acc = first ? w : acc + w;
                first = false;
            }
        }
        RHS[(uint64_t)q * d.fbs + lane] = acc;
    }
}

// ---- triplets: the reference's push order, one slot per thread ------------------------------------------------------------
// global face-only index of local face unknown j of cell X (record numbering), -1 on a Dirichlet face
__device__ __forceinline__ int32_t ifd_index(const IfCsrMesh &m, IfdDims d, int32_t X, bool cut, int j)
{
    const int side = j / (4 * d.fbs), lf = (j / d.fbs) % 4, k = j % d.fbs;
    const uint32_t f = m.cell_faces[4 * (size_t)X + lf];
    const int32_t b = m.face_table[f];
    if (b < 0) return -1;
    const int32_t blk = b + ((cut && side == 1 && m.face_loc[f] == IFD_LOC_CUT) ? 1 : 0);      // faces+ of a cut face (:1319)
    return blk * d.fbs + k;
}

__global__ __launch_bounds__(256) void ifd_triplets_kernel(IfCsrMesh m, IfdDims d, IfCondArgs a, IfCondTriplets o)
{
    const int nf = 4 * d.fbs, NF = 8 * d.fbs;
    for (size_t X = blockIdx.x; X < m.ncells; X += gridDim.x) {
        const bool cut = m.cell_loc[X] == IFD_LOC_CUT;
        const IfdCell c = ifd_cell(m, d, a, (int32_t)X);
        const int n = cut ? NF : nf;
        int32_t *rows = cut ? o.rows_cut + (size_t)m.cut_index[X] * NF * NF : o.rows + X * nf * nf;
        int32_t *cols = cut ? o.cols_cut + (size_t)m.cut_index[X] * NF * NF : o.cols + X * nf * nf;
        double *vals = cut ? o.vals_cut + (size_t)m.cut_index[X] * NF * NF : o.vals + X * nf * nf;
        if (cut) {                                       // the uncut slots of a cut cell are empty
            for (int e = threadIdx.x; e < nf * nf; e += blockDim.x) {
                o.rows[X * nf * nf + e] = -1; o.cols[X * nf * nf + e] = -1; o.vals[X * nf * nf + e] = 0.0;
            }
            for (int e = threadIdx.x; e < nf; e += blockDim.x) { o.rhs_rows[X * nf + e] = -1; o.rhs_vals[X * nf + e] = 0.0; }
        }
        for (int e = threadIdx.x; e < n * n; e += blockDim.x) {
            const int i = e / n, j = e % n;
            const int32_t ri = ifd_index(m, d, (int32_t)X, cut, i), cj = ifd_index(m, d, (int32_t)X, cut, j);
            const bool keep = ri >= 0 && cj >= 0;
            rows[e] = keep ? ri : -1;
            cols[e] = keep ? cj : -1;
            vals[e] = ifd_S(c.S, i, j);
        }
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const int32_t ri = ifd_index(m, d, (int32_t)X, cut, i);
            int32_t *rr = cut ? o.rhs_rows_cut + (size_t)m.cut_index[X] * NF : o.rhs_rows + X * nf;
            double *rv = cut ? o.rhs_vals_cut + (size_t)m.cut_index[X] * NF : o.rhs_vals + X * nf;
            rr[i] = ri;
            rv[i] = ri >= 0 ? ifd_rhs_contrib(m, d, a, (int32_t)X, c, i) : 0.0;
        }
    }
}

// ---- dense kernels of one cell per wavefront: double (uncut) or double-double (cut) arithmetic ------------------------------
template <bool DD> struct IfdAr;
template <> struct IfdAr<true> {
    using T = dd;
    static __device__ __forceinline__ T from(double a) { return dd_from(a); }
    static __device__ __forceinline__ T add(T a, T b) { return dd_add(a, b); }
    static __device__ __forceinline__ T sub(T a, T b) { return dd_sub(a, b); }
    static __device__ __forceinline__ T mul(T a, T b) { return dd_mul(a, b); }
    static __device__ __forceinline__ T muld(T a, double b) { return dd_mul_d(a, b); }
    static __device__ __forceinline__ T rsqrt(T a) { return dd_rsqrt_1(a); }
    static __device__ __forceinline__ bool positive(T a) { return a.hi > 0.0; }
    static __device__ __forceinline__ double round(T a) { return dd_round(a); }
};
template <> struct IfdAr<false> {
    using T = double;
    static __device__ __forceinline__ T from(double a) { return a; }
    static __device__ __forceinline__ T add(T a, T b) { return a + b; }
    static __device__ __forceinline__ T sub(T a, T b) { return a - b; }
    static __device__ __forceinline__ T mul(T a, T b) { return a * b; }
    static __device__ __forceinline__ T muld(T a, double b) { return a * b; }
    static __device__ __forceinline__ T rsqrt(T a) { return 1.0 / sqrt(a); }
    static __device__ __forceinline__ bool positive(T a) { return a > 0.0; }
    static __device__ __forceinline__ double round(T a) { return a; }
};

// In-place Cholesky A = L L^T of an N x N row-major image in LDS (lower triangle read and written) by one wavefront of a 64-thread
// block: right-looking, lane i owns row i.  rinv[j] = 1 / L_jj.  Returns j + 1 of the first non-positive pivot, 0 if none.
template <int N, bool DD>
__device__ int ifd_cholesky(typename IfdAr<DD>::T *A, typename IfdAr<DD>::T *rinv, int lane)
{
    using Ar = IfdAr<DD>;
    using T = typename Ar::T;
    int bad = 0;
    for (int j = 0; j < N; ++j) {
        __syncthreads();
        const T dj = A[j * N + j];
        if (!Ar::positive(dj) && bad == 0) bad = j + 1;
        const T r = Ar::rsqrt(dj);
        if (lane == 0) rinv[j] = r;
        T lij = Ar::from(0.0);
        if (lane > j && lane < N) { lij = Ar::mul(A[lane * N + j], r); A[lane * N + j] = lij; }
        __syncthreads();
        if (lane > j && lane < N)
            for (int k = j + 1; k <= lane; ++k) A[lane * N + k] = Ar::sub(A[lane * N + k], Ar::mul(lij, A[k * N + j]));
    }
    __syncthreads();
    return bad;
}

// ---- the cut cells' records in double-double ------------------------------------------------------------------------------
template <int FD>
__global__ __launch_bounds__(64) void ifcond_cut_kernel(uint32_t ncut, const double *lc_cut, const double *rhs_cut, double *cond_cut,
                                                        int32_t *info)
{
    using Ar = IfdAr<true>;
    constexpr int CBS = (FD + 3) * (FD + 2) / 2, FBS = FD + 1, N = 2 * CBS, NF = 8 * FBS, M = N + NF, NTRI = NF * (NF + 1) / 2;
    constexpr int NC = NF + 1;                              // columns substituted: A_TF, then f_T
    __shared__ dd A[N * N], rinv[N], W[NC * N];             // W column-major by substituted column: W[c * N + i]
    const int lane = threadIdx.x;
    for (size_t cc = blockIdx.x; cc < ncut; cc += gridDim.x) {
        const double *L = lc_cut + cc * (size_t)M * M;       // column-major
        __syncthreads();
        for (int e = lane; e < N * N; e += 64) A[e] = dd_from(L[(e / N) + (size_t)(e % N) * M]);      // row e / N, column e % N
        const int bad = ifd_cholesky<N, true>(A, rinv, lane);
        for (int c = lane; c < NC; c += 64) {
            dd *w = W + c * N;
            for (int i = 0; i < N; ++i) {
                dd s = dd_from(c < NF ? L[i + (size_t)(N + c) * M] : (rhs_cut != nullptr ? rhs_cut[cc * N + i] : 0.0));
                for (int k = 0; k < i; ++k) s = Ar::sub(s, Ar::mul(A[i * N + k], w[k]));
                w[i] = Ar::mul(s, rinv[i]);
            }
        }
        __syncthreads();
        double *Sout = cond_cut + cc * NTRI, *gout = cond_cut + (size_t)ncut * NTRI + cc * NF;
        for (int e = lane; e < NTRI + NF; e += 64) {
            if (e < NTRI) {
                int j = 0;
                while ((j + 1) * (j + 2) / 2 <= e) ++j;
                const int i = e - j * (j + 1) / 2;
                dd s = dd_from(L[(N + i) + (size_t)(N + j) * M]);                          // A_FF(i, j), i <= j
                for (int k = 0; k < N; ++k) s = Ar::sub(s, Ar::mul(W[i * N + k], W[j * N + k]));
                Sout[e] = Ar::round(s);
            } else {
                const int i = e - NTRI;
                dd s = dd_from(0.0);
                for (int k = 0; k < N; ++k) s = Ar::sub(s, Ar::mul(W[i * N + k], W[NF * N + k]));
                gout[i] = Ar::round(s);
            }
        }
        if (info != nullptr && lane == 0) info[cc] = bad ? 200 + bad : 0;
    }
}

// ---- recovery: u_T = A_TT^-1 (f_T - A_TF u_F), one cell per wavefront ------------------------------------------------------
// CUT = false: the uncut cells (N = cbs, 4 fbs face unknowns, in double); CUT = true: the cut cells (N = 2 cbs, 8 fbs, in
// double-double).  u_F of a Dirichlet face: the boundary data for an uncut cell, zero for a cut cell (its slots were dropped).
template <int FD, bool CUT>
__global__ __launch_bounds__(64) void ifcond_recover_kernel(IfCsrMesh m, const uint32_t *cut_cells, uint32_t ncut, const double *lc,
                                                            const double *rhs, const double *g, const double *xF, double *full)
{
    using Ar = IfdAr<CUT>;
    using T = typename Ar::T;
    constexpr int CBS = (FD + 3) * (FD + 2) / 2, FBS = FD + 1, N = CUT ? 2 * CBS : CBS, NFL = CUT ? 8 * FBS : 4 * FBS, M = N + NFL;
    __shared__ T A[N * N], rinv[N], b[N];
    __shared__ double uF[NFL];
    const int lane = threadIdx.x;
    const size_t n = CUT ? ncut : m.ncells;
    for (size_t t = blockIdx.x; t < n; t += gridDim.x) {
        const int32_t X = CUT ? (int32_t)cut_cells[t] : (int32_t)t;
        if (!CUT && m.cell_loc[X] == IFD_LOC_CUT) continue;                                  // wave-uniform
        const double *L = lc + t * (size_t)M * M;
        __syncthreads();
        if (lane < NFL) {
            const int side = lane / (4 * FBS), lf = (lane / FBS) % 4, k = lane % FBS;
            const uint32_t f = m.cell_faces[4 * (size_t)X + lf];
            const int32_t blk = m.face_table[f];
            double u;
            if (blk < 0) u = (!CUT && g != nullptr) ? g[(size_t)f * FBS + k] : 0.0;
            else u = xF[(size_t)(blk + ((CUT && side == 1 && m.face_loc[f] == IFD_LOC_CUT) ? 1 : 0)) * FBS + k];
            uF[lane] = u;
        }
        for (int e = lane; e < N * N; e += 64) A[e] = Ar::from(L[(e / N) + (size_t)(e % N) * M]);
        __syncthreads();
        if (lane < N) {
            T s = Ar::from(rhs != nullptr ? rhs[t * N + lane] : 0.0);
            for (int j = 0; j < NFL; ++j) s = Ar::sub(s, Ar::muld(Ar::from(L[lane + (size_t)(N + j) * M]), uF[j]));
            b[lane] = s;
        }
        ifd_cholesky<N, CUT>(A, rinv, lane);
        // L y = b, then L^T x = y: lane i keeps its running entry, one pivot at a time
        T yi = lane < N ? b[lane] : Ar::from(0.0);
        for (int j = 0; j < N; ++j) {
            if (lane == j) b[j] = Ar::mul(yi, rinv[j]);
            __syncthreads();
            if (lane > j && lane < N) yi = Ar::sub(yi, Ar::mul(A[lane * N + j], b[j]));
        }
        __syncthreads();
        T xi = lane < N ? b[lane] : Ar::from(0.0);
        for (int j = N - 1; j >= 0; --j) {
            if (lane == j) b[j] = Ar::mul(xi, rinv[j]);
            __syncthreads();
            if (lane < j) xi = Ar::sub(xi, Ar::mul(A[j * N + lane], b[j]));
        }
        __syncthreads();
        if (lane < N) full[(size_t)m.cell_table[X] * CBS + lane] = Ar::round(b[lane]);
    }
}

// a failed pivot j of static_condensation_kernel (info j + 1) reported as pa_condensed_ops_batch reports it: 200 + j + 1
__global__ __launch_bounds__(256) void ifcond_info_kernel(size_t n, int32_t *info)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n && info[t] != 0) info[t] = 200 + info[t];
}

__global__ __launch_bounds__(256) void ifcond_copy_faces_kernel(size_t n, const double *xF, double *dst)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) dst[t] = xF[t];
}

}  // namespace

hipError_t ifcond_build(hipStream_t stream, const IfCsrMesh &m, IfCsrTables *t)
{
    if (t->cvstart != nullptr) return hipSuccess;
    const IfdDims d = ifd_dims(t->face_deg);
    const size_t nq = m.num_other_faces;
    uint64_t *gnnz = nullptr, *cv = nullptr;
    void *tmp = nullptr;
    hipError_t e = hipSuccess;
    auto cleanup = [&]() { (void)hipFree(gnnz); (void)hipFree(tmp); };
#define IFD_TRY(call) do { e = (call); if (e != hipSuccess) { (void)hipStreamSynchronize(stream); cleanup(); (void)hipFree(cv); return e; } } while (0)
    IFD_TRY(hipMalloc((void **)&gnnz, (nq + 1) * sizeof(uint64_t)));
    IFD_TRY(hipMalloc((void **)&cv, (nq + 1) * sizeof(uint64_t)));
    hipLaunchKernelGGL(ifd_count_kernel, dim3(blocks_for(nq + 1)), dim3(256), 0, stream, m, d, t->groups, t->units, gnnz);
    IFD_TRY(hipGetLastError());
    size_t bytes = 0;
    IFD_TRY(rocprim::exclusive_scan(nullptr, bytes, gnnz, cv, (uint64_t)0, nq + 1, rocprim::plus<uint64_t>(), stream));
    IFD_TRY(hipMalloc(&tmp, bytes ? bytes : 1));
    IFD_TRY(rocprim::exclusive_scan(tmp, bytes, gnnz, cv, (uint64_t)0, nq + 1, rocprim::plus<uint64_t>(), stream));
    uint64_t nnz = 0;
    IFD_TRY(hipMemcpyAsync(&nnz, cv + nq, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    IFD_TRY(hipStreamSynchronize(stream));
#undef IFD_TRY
    cleanup();
    t->cvstart = cv;
    t->cnnz = nnz;
    return hipSuccess;
}

hipError_t ifcond_pattern(hipStream_t stream, const IfCsrMesh &m, const IfCsrTables &t, int64_t *rowptr, int32_t *colind)
{
    const IfdDims d = ifd_dims(t.face_deg);
    const uint64_t nrows = (uint64_t)m.num_other_faces * d.fbs;
    hipLaunchKernelGGL(ifd_pattern_kernel, dim3(blocks_for(nrows + 1)), dim3(256), 0, stream, m, d, nrows, t.cnnz, t.groups, t.units,
                       t.cvstart, rowptr, colind);
    return hipGetLastError();
}

hipError_t ifcond_fill(hipStream_t stream, const IfCsrMesh &m, const IfCsrTables &t, const IfCondArgs &a, double *values, double *RHS)
{
    if (m.num_other_faces == 0) return hipSuccess;
    hipLaunchKernelGGL(ifd_fill_kernel, dim3((m.num_other_faces + 3) / 4), dim3(256), 0, stream, m, ifd_dims(t.face_deg), t.groups,
                       t.units, t.cvstart, a, values, RHS);
    return hipGetLastError();
}

hipError_t ifcond_cut_records(hipStream_t stream, int face_deg, int max_blocks, uint32_t ncut, const double *lc_cut,
                              const double *rhs_cut, double *cond_cut, int32_t *info)
{
    if (ncut == 0) return hipSuccess;
    const dim3 grid(ncut < (uint32_t)max_blocks ? ncut : (uint32_t)max_blocks);
    switch (face_deg) {
    case 0: hipLaunchKernelGGL((ifcond_cut_kernel<0>), grid, dim3(64), 0, stream, ncut, lc_cut, rhs_cut, cond_cut, info); break;
    case 1: hipLaunchKernelGGL((ifcond_cut_kernel<1>), grid, dim3(64), 0, stream, ncut, lc_cut, rhs_cut, cond_cut, info); break;
    case 2: hipLaunchKernelGGL((ifcond_cut_kernel<2>), grid, dim3(64), 0, stream, ncut, lc_cut, rhs_cut, cond_cut, info); break;
    default: hipLaunchKernelGGL((ifcond_cut_kernel<3>), grid, dim3(64), 0, stream, ncut, lc_cut, rhs_cut, cond_cut, info); break;
    }
    return hipGetLastError();
}

hipError_t ifcond_info_remap(hipStream_t stream, size_t n, int32_t *info)
{
    if (n == 0 || info == nullptr) return hipSuccess;
    hipLaunchKernelGGL(ifcond_info_kernel, dim3(blocks_for(n)), dim3(256), 0, stream, n, info);
    return hipGetLastError();
}

hipError_t ifcond_triplets(hipStream_t stream, const IfCsrMesh &m, int face_deg, int max_blocks, const IfCondArgs &a, const IfCondTriplets &o)
{
    if (m.ncells == 0) return hipSuccess;
    const dim3 grid(m.ncells < (uint32_t)max_blocks ? m.ncells : (uint32_t)max_blocks);
    hipLaunchKernelGGL(ifd_triplets_kernel, grid, dim3(256), 0, stream, m, ifd_dims(face_deg), a, o);
    return hipGetLastError();
}

hipError_t ifcond_recover(hipStream_t stream, const IfCsrMesh &m, int face_deg, int max_blocks, const IfCondArgs &a, const double *lc,
                          const double *rhs, const double *lc_cut, const double *rhs_cut, const double *xF, double *full)
{
    const IfdDims d = ifd_dims(face_deg);
    const size_t nF = (size_t)m.num_other_faces * d.fbs;
    if (nF) {
        hipLaunchKernelGGL(ifcond_copy_faces_kernel, dim3(blocks_for(nF)), dim3(256), 0, stream, nF, xF,
                           full + (size_t)m.num_all_cells * d.cbs);
    }
    const dim3 gu(m.ncells < (uint32_t)max_blocks ? (m.ncells ? m.ncells : 1) : (uint32_t)max_blocks);
    const dim3 gc(a.ncut < (uint32_t)max_blocks ? (a.ncut ? a.ncut : 1) : (uint32_t)max_blocks);
#define IFD_RECOVER(FD)                                                                                                                  \
    case FD:                                                                                                                             \
        if (m.ncells)                                                                                                                    \
            hipLaunchKernelGGL((ifcond_recover_kernel<FD, false>), gu, dim3(64), 0, stream, m, a.cut_cells, a.ncut, lc, rhs, a.g, xF, full); \
        if (a.ncut)                                                                                                                      \
            hipLaunchKernelGGL((ifcond_recover_kernel<FD, true>), gc, dim3(64), 0, stream, m, a.cut_cells, a.ncut, lc_cut, rhs_cut, a.g, xF, \
                               full);                                                                                                    \
        break;
    switch (face_deg) {
        IFD_RECOVER(0) IFD_RECOVER(1) IFD_RECOVER(2)
    default: IFD_RECOVER(3)
    }
#undef IFD_RECOVER
    return hipGetLastError();
}

}  // namespace pa
