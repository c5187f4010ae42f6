// ifd_dense.hpp -- the dense per-cell work the condensing units share (interface_condensed.hip, fictdom_condensed.hip), one cell
// per wavefront of a 64-thread block, each text stated once:
//   IfdAr<DD>            the arithmetic, double or double-double (dd_arith.hpp);
//   ifd_cholesky         the factorization of A_TT in LDS;
//   ifd_records_kernel   a cut cell's record: S = A_FF - A_FT A_TT^-1 A_TF and g = -A_FT A_TT^-1 f_T in double-double;
//   ifd_recover_cell     u_T = A_TT^-1 (f_T - A_TF u_F) of one cell, inside the recovery kernel of each unit;
//   ifd_copy_kernel      a bit copy of n doubles;
//   ifd_for_degree       the face degree as a compile-time constant.
// Everything sits in an unnamed namespace: internal to each unit that includes this, which instantiates the sizes it needs.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "dd_arith.hpp"

namespace pa {

namespace {

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

// ---- a cut cell's record in double-double ----------------------------------------------------------------------------------
// The local matrix of cut cell cc, M x M column-major with M = N + NF, at lc + cc M^2 and its f_T (or none: zero) at rhs + cc N:
// a Cholesky factorization of A_TT, the forward substitutions of the NF + 1 columns [A_TF | f_T], S = A_FF - W^T W and
// g = -W^T w_f with W = L^-1 A_TF, w_f = L^-1 f_T, rounded to double once.  The upper triangle of S, column-packed, goes to
// S + row * S_stride and g to g + row * g_stride, with row = rows[cc], or cc without rows.  info[cc] = 200 + j + 1 for a first
// failed pivot j, 0 for none.
template <int N, int NF>
__global__ __launch_bounds__(64) void ifd_records_kernel(uint32_t ncut, const uint32_t *rows, const double *lc, const double *rhs, double *S,
                                                         size_t S_stride, double *g, size_t g_stride, int32_t *info)
{
    using Ar = IfdAr<true>;
    constexpr int M = N + NF, NTRI = NF * (NF + 1) / 2;
    constexpr int NC = NF + 1;                              // columns substituted: A_TF, then f_T
    static_assert(N <= 64 && NC <= 64, "one lane per row of A_TT / per substituted column");
    __shared__ dd A[N * N], rinv[N], W[NC * N];             // W column-major by substituted column: W[c * N + i]
    const int lane = threadIdx.x;
    for (size_t cc = blockIdx.x; cc < ncut; cc += gridDim.x) {
        const double *L = lc + cc * (size_t)M * M;           // column-major
        __syncthreads();
        for (int e = lane; e < N * N; e += 64) A[e] = dd_from(L[(e / N) + (size_t)(e % N) * M]);      // row e / N, column e % N
        const int bad = ifd_cholesky<N, true>(A, rinv, lane);
        for (int c = lane; c < NC; c += 64) {
            dd *w = W + c * N;
            for (int i = 0; i < N; ++i) {
                dd s = dd_from(c < NF ? L[i + (size_t)(N + c) * M] : (rhs != nullptr ? rhs[cc * N + i] : 0.0));
                for (int k = 0; k < i; ++k) s = Ar::sub(s, Ar::mul(A[i * N + k], w[k]));
                w[i] = Ar::mul(s, rinv[i]);
            }
        }
        __syncthreads();
        const size_t row = rows != nullptr ? rows[cc] : cc;
        double *Sout = S + row * S_stride, *gout = g + row * g_stride;
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

// ---- recovery of one cell: x = A_TT^-1 (f_T - A_TF u_F) ---------------------------------------------------------------------
// Cell t of lc (the local matrices in HBM, M x M column-major with M = N + NFL: A_TT and the columns of A_TF are read) and of rhs
// (f_T, N per cell; null for zero); uF: the cell's NFL face values, in LDS, written by the calling kernel since the block's last
// barrier.  Called by every thread of the block, which is past a barrier since its last read of the returned image.  Returns x,
// in this function's LDS, behind a barrier.  Factorization and sweeps only: which u_F, and where u_T goes, is the caller's.
template <int N, int NFL, bool DD>
__device__ const typename IfdAr<DD>::T *ifd_recover_cell(const double *lc, const double *rhs, size_t t, const double *uF, int lane)
{
    using Ar = IfdAr<DD>;
    using T = typename Ar::T;
    constexpr int M = N + NFL;
    static_assert(N <= 64 && NFL <= 64, "one lane per cell unknown / face unknown");
    __shared__ T A[N * N], rinv[N], b[N];
    const double *L = lc + t * (size_t)M * M;
    for (int e = lane; e < N * N; e += 64) A[e] = Ar::from(L[(e / N) + (size_t)(e % N) * M]);
    __syncthreads();
    if (lane < N) {
        T s = Ar::from(rhs != nullptr ? rhs[t * N + lane] : 0.0);
        for (int j = 0; j < NFL; ++j) s = Ar::sub(s, Ar::muld(Ar::from(L[lane + (size_t)(N + j) * M]), uF[j]));
        b[lane] = s;
    }
    ifd_cholesky<N, DD>(A, rinv, lane);
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
    return b;
}

__global__ __launch_bounds__(256) void ifd_copy_kernel(size_t n, const double *src, double *dst)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) dst[t] = src[t];
}

// f(std::integral_constant<int, face_deg>{}) for a face degree 0..MAXFD (at most 3); false, and f not called, for any other
template <int MAXFD, class F>
bool ifd_for_degree(int face_deg, F &&f)
{
    static_assert(MAXFD >= 2 && MAXFD <= 3, "degrees 0..2 or 0..3");
    switch (face_deg) {
    case 0: f(std::integral_constant<int, 0>{}); return true;
    case 1: f(std::integral_constant<int, 1>{}); return true;
    case 2: f(std::integral_constant<int, 2>{}); return true;
    case 3:
        if constexpr (MAXFD >= 3) { f(std::integral_constant<int, 3>{}); return true; }
    }
    return false;
}

}  // namespace

}  // namespace pa
