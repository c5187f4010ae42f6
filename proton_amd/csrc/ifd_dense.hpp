// ifd_dense.hpp -- the dense per-cell arithmetic the condensing kernels share (interface_condensed.hip, fictdom_condensed.hip):
// one cell per wavefront of a 64-thread block, in double or in double-double (dd_arith.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "dd_arith.hpp"

namespace pa {

namespace {      // internal to each unit that includes this, as when interface_condensed.hip held the text itself

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

}  // namespace

}  // namespace pa
