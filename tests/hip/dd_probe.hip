// dd_probe.hip -- the double-double and cross-lane primitives of proton_amd/csrc/dd_arith.hpp, one at a time ON THE DEVICE, for
// tests/test_gpu_dd_primitives.py.  Built by proton_amd/_build.py's build_probe() with exactly the flags of the shipped library
// into proton_amd/lib/probe/libpa_dd_probe.so: what is tested is what those flags make of the header (contraction, approximate
// instructions, reassociation), so nothing here may do arithmetic of its own.  Every entry point takes device pointers, launches
// on the null stream, synchronizes and returns the hipError_t.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../proton_amd/csrc/dd_arith.hpp"

using namespace pa;

namespace {

// the numbering tests/dd_twin.py's OPS repeats
enum {
    OP_TWO_SUM = 0, OP_QUICK_TWO_SUM, OP_TWO_PROD, OP_DD_ADD, OP_DD_ADD_FAST, OP_DD_SUB, OP_DD_SUB_FAST, OP_DD_MUL, OP_DD_MUL_D,
    OP_DD_RSQRT, OP_DD_RSQRT_1, OP_DD_ROUND, OP_RSQ_SEED, OP_COUNT
};

// one op per kernel: no op's code is scheduled together with another's
template <int OP>
__global__ __launch_bounds__(256) void dd_kernel(int n, const double *ah, const double *al, const double *bh, const double *bl,
                                                 const double *d, double *out_hi, double *out_lo)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const dd a{ah[i], al[i]}, b{bh[i], bl[i]};
    dd r;
    if constexpr (OP == OP_TWO_SUM) r = two_sum(a.hi, b.hi);
    else if constexpr (OP == OP_QUICK_TWO_SUM) r = quick_two_sum(a.hi, b.hi);
    else if constexpr (OP == OP_TWO_PROD) r = two_prod(a.hi, b.hi);
    else if constexpr (OP == OP_DD_ADD) r = dd_add(a, b);
    else if constexpr (OP == OP_DD_ADD_FAST) r = dd_add_fast(a, b);
    else if constexpr (OP == OP_DD_SUB) r = dd_sub(a, b);
    else if constexpr (OP == OP_DD_SUB_FAST) r = dd_sub_fast(a, b);
    else if constexpr (OP == OP_DD_MUL) r = dd_mul(a, b);
    else if constexpr (OP == OP_DD_MUL_D) r = dd_mul_d(a, d[i]);
    else if constexpr (OP == OP_DD_RSQRT) r = dd_rsqrt(a);
    else if constexpr (OP == OP_DD_RSQRT_1) r = dd_rsqrt_1(a);
    else if constexpr (OP == OP_DD_ROUND) r = dd{dd_round(a), 0.0};
    else r = dd{__builtin_amdgcn_rsq(a.hi), 0.0};
    out_hi[i] = r.hi;
    out_lo[i] = r.lo;
}

// lanes_transpose_reduce<N, 32> as cut_device.hpp and cut_interface_device.hpp call it: the lane's N values, the two functor pairs
// of the kernels.  in: [thread][N] doubles, or [thread][N][2] (hi, lo).  Every lane writes what it was handed.
template <int N, bool DD>
__global__ __launch_bounds__(256) void transpose_reduce_kernel(int nwaves, const double *in, int32_t *out_index, int32_t *out_ok,
                                                               double *out_hi, double *out_lo)
{
    const int t = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    if (t / 64 >= nwaves) return;                                   // (wave-uniform)
    bool ok = true;
    if constexpr (DD) {
        dd v[N];
#pragma unroll
        for (int m = 0; m < N; ++m) v[m] = dd_load(in + ((size_t)t * N + m) * 2);
        dd tot;
        const int m = lanes_transpose_reduce<N, 32>(v, lane, dd_from(0.0), [](dd x, dd y) { return dd_add_fast(x, y); },
                                                    [](dd x, int off) { return dd_shfl_xor(x, off); }, tot, ok);
        out_index[t] = m; out_hi[t] = tot.hi; out_lo[t] = tot.lo;
    } else {
        double v[N];
#pragma unroll
        for (int m = 0; m < N; ++m) v[m] = in[(size_t)t * N + m];
        double tot;
        const int m = lanes_transpose_reduce<N, 32>(v, lane, 0.0, [](double x, double y) { return x + y; },
                                                    [](double x, int off) { return __shfl_xor(x, off); }, tot, ok);
        out_index[t] = m; out_hi[t] = tot; out_lo[t] = 0.0;
    }
    out_ok[t] = ok ? 1 : 0;
}

// dd_readlane(v, j) for a wave-uniform j and dd_shfl_xor(v, 1 << k): every lane writes what arrived.
//   j_arg >= 0: the lane index is the kernel argument; out_rl: [thread]
//   j_arg <  0: j = 0 .. 63 a uniform loop variable; out_rl: [wave][j][lane], and out_sx: [wave][k = 0 .. 5][lane]
__global__ __launch_bounds__(256) void lane_moves_kernel(int nwaves, int j_arg, const double *in_hi, const double *in_lo, double *rl_hi,
                                                         double *rl_lo, double *sx_hi, double *sx_lo)
{
    const int t = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63, wave = t / 64;
    if (wave >= nwaves) return;
    const dd v{in_hi[t], in_lo[t]};
    if (j_arg >= 0) {
        const dd r = dd_readlane(v, j_arg);
        rl_hi[t] = r.hi; rl_lo[t] = r.lo;
        return;
    }
    for (int j = 0; j < 64; ++j) {
        const dd r = dd_readlane(v, j);
        rl_hi[((size_t)wave * 64 + j) * 64 + lane] = r.hi; rl_lo[((size_t)wave * 64 + j) * 64 + lane] = r.lo;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const dd r = dd_shfl_xor(v, 1 << k);
        sx_hi[((size_t)wave * 6 + k) * 64 + lane] = r.hi; sx_lo[((size_t)wave * 6 + k) * 64 + lane] = r.lo;
    }
}

int finish()
{
    const hipError_t launch = hipGetLastError(), sync = hipDeviceSynchronize();
    return (int)(launch != hipSuccess ? launch : sync);
}

}  // namespace

extern "C" {

int pa_probe_dd(int op, int n, const double *ah, const double *al, const double *bh, const double *bl, const double *d, double *out_hi,
                double *out_lo)
{
    if (op < 0 || op >= OP_COUNT || n <= 0) return (int)hipErrorInvalidValue;
    const dim3 grid((n + 255) / 256), block(256);
    switch (op) {
#define PA_PROBE_OP(OP) case OP: hipLaunchKernelGGL((dd_kernel<OP>), grid, block, 0, 0, n, ah, al, bh, bl, d, out_hi, out_lo); break;
        PA_PROBE_OP(OP_TWO_SUM) PA_PROBE_OP(OP_QUICK_TWO_SUM) PA_PROBE_OP(OP_TWO_PROD) PA_PROBE_OP(OP_DD_ADD) PA_PROBE_OP(OP_DD_ADD_FAST)
        PA_PROBE_OP(OP_DD_SUB) PA_PROBE_OP(OP_DD_SUB_FAST) PA_PROBE_OP(OP_DD_MUL) PA_PROBE_OP(OP_DD_MUL_D) PA_PROBE_OP(OP_DD_RSQRT)
        PA_PROBE_OP(OP_DD_RSQRT_1) PA_PROBE_OP(OP_DD_ROUND) PA_PROBE_OP(OP_RSQ_SEED)
#undef PA_PROBE_OP
    }
    return finish();
}

// the counts the cut-cell kernels instantiate for k = 0, 1, 2 -- double-double: NMOM = 6, 15, 28 and the interface moments' passes
// 1, 5, 3 / 6, 9, 10 / 15, 13, 21; double: CBS = 3, 6, 10 -- and 2, 7, 33, 64 for the padding; each with both types
#define PA_PROBE_COUNTS(X) X(1) X(2) X(3) X(5) X(6) X(7) X(9) X(10) X(13) X(15) X(21) X(28) X(33) X(64)

int pa_probe_transpose_reduce(int N, int is_dd, int nwaves, const double *in, int32_t *out_index, int32_t *out_ok, double *out_hi,
                              double *out_lo)
{
    if (nwaves <= 0) return (int)hipErrorInvalidValue;
    const dim3 grid((nwaves + 3) / 4), block(256);
    switch (N) {
#define PA_PROBE_N(NN)                                                                                                                  \
    case NN:                                                                                                                            \
        if (is_dd) hipLaunchKernelGGL((transpose_reduce_kernel<NN, true>), grid, block, 0, 0, nwaves, in, out_index, out_ok, out_hi, out_lo); \
        else hipLaunchKernelGGL((transpose_reduce_kernel<NN, false>), grid, block, 0, 0, nwaves, in, out_index, out_ok, out_hi, out_lo);      \
        break;
        PA_PROBE_COUNTS(PA_PROBE_N)
#undef PA_PROBE_N
    default: return (int)hipErrorInvalidValue;
    }
    return finish();
}

int pa_probe_lane_moves(int nwaves, int j_arg, const double *in_hi, const double *in_lo, double *rl_hi, double *rl_lo, double *sx_hi,
                        double *sx_lo)
{
    if (nwaves <= 0 || j_arg >= 64) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(lane_moves_kernel, dim3((nwaves + 3) / 4), dim3(256), 0, 0, nwaves, j_arg, in_hi, in_lo, rl_hi, rl_lo, sx_hi, sx_lo);
    return finish();
}

}  // extern "C"
