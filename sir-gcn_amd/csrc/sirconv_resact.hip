// sirconv_resact.hip — the stack loop's residual + activation around a SIRConv layer, one pass per
// direction (the layer loops sirgcn.stacks restates; reference zinc/model.py:53-56 and
// ogbn-arxiv/model.py:65-73 without a norm):
//   order 0 (zinc) : out = act(y + r)            backward: g = act'(y + r) dout;  dy = g, dr = g
//   order 1 (arxiv): out = act(y) + r            backward: dy = act'(y) dout;     dr = dout (the caller's)
// y is the conv output in its storage type (fp32, or bf16 / fp16 under autocast), r and out fp32.
// Each value goes through the ops torch's add / relu / leaky_relu and their autograd apply, in the
// same order and types, so the result is bit-identical to the separate torch kernels they replace
// (two passes forward, two or three backward, plus the 16-bit cast of the gradient): under autocast
// an arxiv-order activation runs on the 16-bit y and rounds to it (torch's opmath), and the
// gradient of a 16-bit y is rounded once from fp32.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sirconv.h"
#include "sirconv_internal.h"
#include "sirconv_device.h"

namespace sir {
namespace {

// 4 consecutive elements per thread, rows of N (N % 4 == 0) — grid-stride over M * N / 4
template <int DT, int ACT, int ORDER>
__global__ void __launch_bounds__(256)
k_resact_fwd(const void* __restrict__ Y, int64_t ldy, const float* __restrict__ R, int64_t ldr, float* __restrict__ O,
             int64_t ldo, int64_t M, int N, float slope) {
    typedef typename Stor<DT>::T T;
    const int nq = N / 4;
    const int64_t total = M * nq;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
        const int64_t m = q / nq;
        const int n = (int)(q - m * nq) * 4;
        float yv[4], rv[4], o[4];
        vload<4>(rv, R + m * ldr + n);
        tload_p<DT, 4>(yv, static_cast<const T*>(Y) + m * ldy + n);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if constexpr (ORDER == 0) o[i] = sig<ACT>(yv[i] + rv[i], slope);                    // act(y + r)
            else o[i] = round_st<DT>(sig<ACT>(yv[i], slope)) + rv[i];                           // act(y) + r
        }
        vstore<4>(O + m * ldo + n, o);
    }
}

template <int DT, int ACT, int ORDER>
__global__ void __launch_bounds__(256)
k_resact_bwd(const float* __restrict__ D, int64_t ldd, const float* __restrict__ D2, int64_t ldd2,
             const void* __restrict__ Y, int64_t ldy,
             const float* __restrict__ R, int64_t ldr, void* __restrict__ DY, int64_t lddy, float* __restrict__ DR,
             int64_t lddr, int64_t M, int N, float slope) {
    typedef typename Stor<DT>::T T;
    const int nq = N / 4;
    const int64_t total = M * nq;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
        const int64_t m = q / nq;
        const int n = (int)(q - m * nq) * 4;
        float dv[4], yv[4], g[4];
        vload<4>(dv, D + m * ldd + n);
        if (D2 != nullptr) {           // a second gradient of the output: the sum autograd would form
            float d2[4];
            vload<4>(d2, D2 + m * ldd2 + n);
#pragma unroll
            for (int i = 0; i < 4; ++i) dv[i] += d2[i];
        }
        tload_p<DT, 4>(yv, static_cast<const T*>(Y) + m * ldy + n);
        if constexpr (ORDER == 0) {
            float rv[4];
            vload<4>(rv, R + m * ldr + n);
#pragma unroll
            for (int i = 0; i < 4; ++i) g[i] = dsig<ACT>(yv[i] + rv[i], dv[i], slope);
            if (DR != nullptr) vstore<4>(DR + m * lddr + n, g);
        } else {
            // the 16-bit activation's backward runs on the gradient rounded to its type (autograd
            // casts the add's fp32 gradient for the 16-bit operand), in opmath, rounded once more
#pragma unroll
            for (int i = 0; i < 4; ++i) g[i] = dsig<ACT>(yv[i], round_st<DT>(dv[i]), slope);
            // R's gradient is dout itself: written only when it is a sum formed here (D2)
            if (D2 != nullptr && DR != nullptr) vstore<4>(DR + m * lddr + n, dv);
        }
        tstore_p<DT, 4>(static_cast<T*>(DY) + m * lddy + n, g);
    }
}

}  // namespace

hipError_t run_resid_act_fwd(const void* Y, int64_t ldy, int dtype, const float* R, int64_t ldr, float* O, int64_t ldo,
                             int64_t M, int N, int act, float slope, int order, hipStream_t st) {
    if (M == 0 || N == 0) return hipSuccess;
    const dim3 grid(stream_grid(M, N));
    return by_dtype(dtype, [&](auto dt) {
        return by_act<ACTS_NORM>(act, [&](auto a) {
            if (order)
                hipLaunchKernelGGL((k_resact_fwd<dt(), a(), 1>), grid, dim3(256), 0, st, Y, ldy, R, ldr, O, ldo, M, N,
                                   slope);
            else
                hipLaunchKernelGGL((k_resact_fwd<dt(), a(), 0>), grid, dim3(256), 0, st, Y, ldy, R, ldr, O, ldo, M, N,
                                   slope);
            return hipGetLastError();
        });
    });
}

hipError_t run_resid_act_bwd(const float* D, int64_t ldd, const float* D2, int64_t ldd2, const void* Y, int64_t ldy,
                             int dtype, const float* R, int64_t ldr, void* DY, int64_t lddy, float* DR, int64_t lddr,
                             int64_t M, int N, int act, float slope, int order, hipStream_t st) {
    if (M == 0 || N == 0) return hipSuccess;
    const dim3 grid(stream_grid(M, N));
    return by_dtype(dtype, [&](auto dt) {
        return by_act<ACTS_NORM>(act, [&](auto a) {
            if (order)
                hipLaunchKernelGGL((k_resact_bwd<dt(), a(), 1>), grid, dim3(256), 0, st, D, ldd, D2, ldd2, Y, ldy, R, ldr,
                                   DY, lddy, DR, lddr, M, N, slope);
            else
                hipLaunchKernelGGL((k_resact_bwd<dt(), a(), 0>), grid, dim3(256), 0, st, D, ldd, D2, ldd2, Y, ldy, R, ldr,
                                   DY, lddy, DR, lddr, M, N, slope);
            return hipGetLastError();
        });
    });
}

}  // namespace sir

