// fictdom_condensed.hip -- the fictitious-domain problem's global system (apps/cuthho/cuthho_square.cpp:881-905) condensed to its
// face unknowns on the device: the dense work of the cut cells.
//
// The system is the plain assembler<Mesh>'s over all cells, so numbering, pattern, fill, halo and expansion are condensed.hip's.
// An uncut cell's record comes from the fused condensed pass; a cut cell's local matrix (make_hho_laplacian with the Nitsche terms
// plus make_hho_cut_stabilization, cuthho_square.cpp:893-895) has the plain cell's shape -- cbs cell unknowns, 4 fbs face
// unknowns -- and an A_TT whose condition number reaches 1e8 on sliver cells, so it is eliminated in double-double
// (fdcond_cut_kernel, the shape of ifcond_cut_kernel with N = cbs and NF = 4 fbs): a Cholesky factorization of A_TT, the forward
// substitutions of the NF + 1 columns [A_TF | f_T], S = A_FF - W^T W and g = -W^T w_f with W = L^-1 A_TF, w_f = L^-1 f_T, rounded
// to double once.  cut_local_ops_kernel stores both copies of the symmetric entries, so A_FT = A_TF^T exactly.
// fdcond_recover_kernel gives the cut cells' u_T = A_TT^-1 (f_T - A_TF u_F) (take_local_data's cell part, :959-962) the same way.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dd_arith.hpp"
#include "device_tmp.hpp"
#include "fictdom_condensed.hpp"
#include "ifd_dense.hpp"

namespace pa {

namespace {

constexpr int8_t FD_LOC_CUT = 2;                 // LOC_CUT of cut_host.hpp, PA_LOC_ON_INTERFACE

// ---- the cut cells' records in double-double, one cut cell per wavefront ---------------------------------------------------
template <int FD>
__global__ __launch_bounds__(64) void fdcond_cut_kernel(uint32_t ncut, const uint32_t *cut_cells, const double *cut_lc, const double *cut_rhs,
                                                        double *cond, int32_t *info_cut)
{
    using Ar = IfdAr<true>;
    constexpr int N = (FD + 3) * (FD + 2) / 2, FBS = FD + 1, NF = 4 * FBS, M = N + NF, NTRI = NF * (NF + 1) / 2;
    constexpr int NC = NF + 1;                              // columns substituted: A_TF, then f_T
    static_assert(N <= 64 && NC <= 64, "one lane per row of A_TT / per substituted column");
    __shared__ dd A[N * N], rinv[N], W[NC * N];             // W column-major by substituted column: W[c * N + i]
    const int lane = threadIdx.x;
    for (size_t cc = blockIdx.x; cc < ncut; cc += gridDim.x) {
        const double *L = cut_lc + cc * (size_t)M * M;       // column-major
        __syncthreads();
        for (int e = lane; e < N * N; e += 64) A[e] = dd_from(L[(e / N) + (size_t)(e % N) * M]);      // row e / N, column e % N
        const int bad = ifd_cholesky<N, true>(A, rinv, lane);
        for (int c = lane; c < NC; c += 64) {
            dd *w = W + c * N;
            for (int i = 0; i < N; ++i) {
                dd s = dd_from(c < NF ? L[i + (size_t)(N + c) * M] : (cut_rhs != nullptr ? cut_rhs[cc * N + i] : 0.0));
                for (int k = 0; k < i; ++k) s = Ar::sub(s, Ar::mul(A[i * N + k], w[k]));
                w[i] = Ar::mul(s, rinv[i]);
            }
        }
        __syncthreads();
        double *out = cond + (size_t)cut_cells[cc] * (NTRI + NF);      // [upper triangle of S, column-packed | g]
        for (int e = lane; e < NTRI + NF; e += 64) {
            if (e < NTRI) {
                int j = 0;
                while ((j + 1) * (j + 2) / 2 <= e) ++j;
                const int i = e - j * (j + 1) / 2;
                dd s = dd_from(L[(N + i) + (size_t)(N + j) * M]);                          // A_FF(i, j), i <= j
                for (int k = 0; k < N; ++k) s = Ar::sub(s, Ar::mul(W[i * N + k], W[j * N + k]));
                out[e] = Ar::round(s);
            } else {
                const int i = e - NTRI;
                dd s = dd_from(0.0);
                for (int k = 0; k < N; ++k) s = Ar::sub(s, Ar::mul(W[i * N + k], W[NF * N + k]));
                out[e] = Ar::round(s);
            }
        }
        if (info_cut != nullptr && lane == 0) info_cut[cc] = bad ? 200 + bad : 0;
    }
}

// ---- recovery of the cut cells: u_T = A_TT^-1 (f_T - A_TF u_F) in double-double, one cut cell per wavefront ------------------
// u_F of a Dirichlet face is the boundary data (the plain assembler's rule, hho.hpp:408-449): uF holds it already.
template <int FD>
__global__ __launch_bounds__(64) void fdcond_recover_kernel(uint32_t ncut, const uint32_t *cut_cells, const double *cut_lc, const double *cut_rhs,
                                                            const double *uF, double *uT)
{
    using Ar = IfdAr<true>;
    using T = typename Ar::T;
    constexpr int N = (FD + 3) * (FD + 2) / 2, FBS = FD + 1, NFL = 4 * FBS, M = N + NFL;
    static_assert(N <= 64 && NFL <= 64, "one lane per cell unknown / face unknown");
    __shared__ T A[N * N], rinv[N], b[N];
    __shared__ double uf[NFL];
    const int lane = threadIdx.x;
    for (size_t cc = blockIdx.x; cc < ncut; cc += gridDim.x) {
        const size_t X = cut_cells[cc];
        const double *L = cut_lc + cc * (size_t)M * M;
        __syncthreads();
        if (lane < NFL) uf[lane] = uF[X * NFL + lane];
        for (int e = lane; e < N * N; e += 64) A[e] = Ar::from(L[(e / N) + (size_t)(e % N) * M]);
        __syncthreads();
        if (lane < N) {
            T s = Ar::from(cut_rhs != nullptr ? cut_rhs[cc * N + lane] : 0.0);
            for (int j = 0; j < NFL; ++j) s = Ar::sub(s, Ar::muld(Ar::from(L[lane + (size_t)(N + j) * M]), uf[j]));
            b[lane] = s;
        }
        ifd_cholesky<N, true>(A, rinv, lane);
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
        if (lane < N) uT[X * N + lane] = Ar::round(b[lane]);
    }
}

// an uncut cell outside `where` takes a zero right-hand side (cuthho_square.cpp:659-664); a cut cell's comes from cut_rhs
__global__ __launch_bounds__(256) void fdcond_masked_rhs_kernel(size_t total, uint32_t cbs, const int8_t *cell_loc, int where, const double *src,
                                                                double *dst)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int loc = cell_loc[t / cbs];
    dst[t] = (src != nullptr && loc == where) ? src[t] : 0.0;
}

__global__ __launch_bounds__(256) void fdcond_copy_kernel(size_t n, const double *src, double *dst)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) dst[t] = src[t];
}

}  // namespace

hipError_t fdcond_cut_records(hipStream_t stream, int face_deg, int max_blocks, uint32_t ncut, const uint32_t *cut_cells, const double *cut_lc,
                              const double *cut_rhs, double *cond, int32_t *info_cut)
{
    if (ncut == 0) return hipSuccess;
    const dim3 grid(ncut < (uint32_t)max_blocks ? ncut : (uint32_t)max_blocks);
    switch (face_deg) {
    case 0: hipLaunchKernelGGL((fdcond_cut_kernel<0>), grid, dim3(64), 0, stream, ncut, cut_cells, cut_lc, cut_rhs, cond, info_cut); break;
    case 1: hipLaunchKernelGGL((fdcond_cut_kernel<1>), grid, dim3(64), 0, stream, ncut, cut_cells, cut_lc, cut_rhs, cond, info_cut); break;
    case 2: hipLaunchKernelGGL((fdcond_cut_kernel<2>), grid, dim3(64), 0, stream, ncut, cut_cells, cut_lc, cut_rhs, cond, info_cut); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t fdcond_cut_recover(hipStream_t stream, int face_deg, int max_blocks, uint32_t ncut, const uint32_t *cut_cells, const double *cut_lc,
                              const double *cut_rhs, const double *uF, double *uT)
{
    if (ncut == 0) return hipSuccess;
    const dim3 grid(ncut < (uint32_t)max_blocks ? ncut : (uint32_t)max_blocks);
    switch (face_deg) {
    case 0: hipLaunchKernelGGL((fdcond_recover_kernel<0>), grid, dim3(64), 0, stream, ncut, cut_cells, cut_lc, cut_rhs, uF, uT); break;
    case 1: hipLaunchKernelGGL((fdcond_recover_kernel<1>), grid, dim3(64), 0, stream, ncut, cut_cells, cut_lc, cut_rhs, uF, uT); break;
    case 2: hipLaunchKernelGGL((fdcond_recover_kernel<2>), grid, dim3(64), 0, stream, ncut, cut_cells, cut_lc, cut_rhs, uF, uT); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t fdcond_masked_rhs(hipStream_t stream, size_t ncells, int cbs, const int8_t *cell_loc, int where, const double *src, double *dst)
{
    const size_t total = ncells * (size_t)cbs;
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(fdcond_masked_rhs_kernel, dim3(blocks_for(total)), dim3(256), 0, stream, total, (uint32_t)cbs, cell_loc, where, src, dst);
    return hipGetLastError();
}

hipError_t fdcond_copy(hipStream_t stream, size_t n, const double *src, double *dst)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(fdcond_copy_kernel, dim3(blocks_for(n)), dim3(256), 0, stream, n, src, dst);
    return hipGetLastError();
}

}  // namespace pa
