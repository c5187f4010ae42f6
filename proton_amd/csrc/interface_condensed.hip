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
// This file holds the dense per-cell work: the cut cells' records, the recovery of the cell unknowns and the info remap.  The
// face-only CSR and its triplets are the gather of interface_csr.hip reading these records (IfCondSource).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dd_arith.hpp"
#include "device_tmp.hpp"
#include "ifd_dense.hpp"
#include "interface_csr.hpp"

namespace pa {

namespace {

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
        if (!CUT && m.cell_loc[X] == IF_LOC_CUT) continue;                                  // wave-uniform
        const double *L = lc + t * (size_t)M * M;
        __syncthreads();
        if (lane < NFL) {
            size_t bdof;
            const int32_t j = if_face_index(m, IfDims{CBS, FBS}, (size_t)X, CUT, lane, &bdof);
            uF[lane] = j >= 0 ? xF[j] : ((!CUT && g != nullptr) ? g[bdof] : 0.0);
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

hipError_t ifcond_recover(hipStream_t stream, const IfCsrMesh &m, int face_deg, int max_blocks, const IfCondArgs &a, const double *lc,
                          const double *rhs, const double *lc_cut, const double *rhs_cut, const double *xF, double *full)
{
    const IfDims d = if_dims(face_deg);
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
