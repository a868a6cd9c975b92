// sirconv_dropact.hip — the elementwise tail of the pre-norm residual block, one pass per direction
// (reference heterophilous-datasets/model.py:36-50: input_linear -> input_drop -> GELU; conv -> drop -> GELU;
// linears[i] -> drop -> + feats_resid): the dropout stands BEFORE the activation, which neither
// sirconv_resact.hip (no dropout, no GELU) nor the norm passes (dropout after the activation) express.
//   forward : out = act(d) + R,   d = keep(row, col) ? y * scale : +0      (R optional; drop off: d = y)
//   backward: dy  = keep ? act'(d) dout * scale : 0                        (dR is dout itself, the caller's)
// keep / scale / the seed are sirconv_dropout.h's at col0 = 0, the bits sir_dropout_apply writes for an
// [M, N] block; no mask is stored and the backward recomputes it (and d) from y.  A dropped element is a
// select, never a product: +0 whatever y held (NaN, Inf), and a zero gradient whatever dout held.
// y is fp32, bf16 or fp16 (the conv's and the Linear's output under autocast); R and out are fp32, or the
// 16-bit type of y.  A value is rounded to its storage type wherever torch's separate kernels would store
// it — after the dropout, after the activation, after the add; the gradient of a 16-bit y after the cast of
// dout, after act' and after the scale — with fp32 opmath in between, so Identity / ReLU / LeakyReLU are
// bit-identical to the composed torch ops and the GELUs differ from them only by erff / tanhf / expf.
// sigma and sigma' are sirconv_device.h's sig / dsig (the project's one GELU), the element access its
// tload_p / tstore_p and the roundings its round_st.
// A streaming kernel: no LDS, no atomics, 4 consecutive elements per thread in one vector access each.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sirconv.h"
#include "sirconv_internal.h"
#include "sirconv_dropout.h"
#include "sirconv_device.h"

namespace sir {
namespace {

// d = the dropout's output at (row hash rh, column n) as the fp32 value of its DT storage
template <int DT>
__device__ __forceinline__ float dropped(const Drop& drop, bool on, uint32_t rh, int n, float y, bool& keep) {
    keep = true;
    if (!on) return y;
    keep = drop_keep(drop, rh, n);
    return keep ? round_st<DT>(y * drop.scale) : 0.f;
}

// rows of N (N % 4 == 0), grid-stride over M * N / 4; DT: y (and dy), ODT: R and out (F32 or DT)
template <int DT, int ODT, int ACT>
__global__ void __launch_bounds__(256)
k_dropact_fwd(const void* __restrict__ Y, int64_t ldy, const void* __restrict__ R, int64_t ldr, void* __restrict__ O,
              int64_t ldo, int64_t M, int N, float slope, Drop drop) {
    typedef typename Stor<DT>::T T;
    typedef typename Stor<ODT>::T OT;
    drop = drop_resolve(drop);
    const bool on = drop.on();
    const int nq = N / 4;
    const int64_t total = M * nq;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
        const int64_t m = q / nq;
        const int n = (int)(q - m * nq) * 4;
        float yv[4], rv[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
        tload_p<DT, 4>(yv, static_cast<const T*>(Y) + m * ldy + n);
        if (R != nullptr) tload_p<ODT, 4>(rv, static_cast<const OT*>(R) + m * ldr + n);
        const uint32_t rh = on ? drop_row_hash(drop, m) : 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            bool keep;
            const float d = dropped<DT>(drop, on, rh, n + i, yv[i], keep);
            const float a = round_st<DT>(sig<ACT>(d, slope));
            o[i] = R != nullptr ? a + rv[i] : a;           // rounded to ODT by the store
        }
        tstore_p<ODT, 4>(static_cast<OT*>(O) + m * ldo + n, o);
    }
}

template <int DT, int ODT, int ACT>
__global__ void __launch_bounds__(256)
k_dropact_bwd(const void* __restrict__ D, int64_t ldd, const void* __restrict__ Y, int64_t ldy, void* __restrict__ DY,
              int64_t lddy, int64_t M, int N, float slope, Drop drop) {
    typedef typename Stor<DT>::T T;
    typedef typename Stor<ODT>::T OT;
    drop = drop_resolve(drop);
    const bool on = drop.on();
    const int nq = N / 4;
    const int64_t total = M * nq;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
        const int64_t m = q / nq;
        const int n = (int)(q - m * nq) * 4;
        float yv[4], dv[4], g[4];
        tload_p<DT, 4>(yv, static_cast<const T*>(Y) + m * ldy + n);
        tload_p<ODT, 4>(dv, static_cast<const OT*>(D) + m * ldd + n);
        const uint32_t rh = on ? drop_row_hash(drop, m) : 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            bool keep;
            const float d = dropped<DT>(drop, on, rh, n + i, yv[i], keep);
            // the activation's backward runs on dout cast to its type (autograd's cast of the add's fp32
            // gradient for a 16-bit operand), in opmath, rounded once; then the dropout's grad * scale
            const float ga = round_st<DT>(dsig<ACT>(d, round_st<DT>(dv[i]), slope));
            g[i] = !on ? ga : (keep ? ga * drop.scale : 0.f);   // rounded to DT by the store
        }
        tstore_p<DT, 4>(static_cast<T*>(DY) + m * lddy + n, g);
    }
}

}  // namespace

// dtype: y / dy; o_dtype: R, out and dout — SIR_DTYPE_F32 or dtype (checked by the ABI layer)
hipError_t run_drop_act_fwd(const void* Y, int64_t ldy, int dtype, const void* R, int64_t ldr, void* O, int64_t ldo,
                            int o_dtype, int64_t M, int N, int act, float slope, const Drop& drop, hipStream_t st) {
    if (M == 0 || N == 0) return hipSuccess;
    const dim3 grid(stream_grid(M, N));
    return by_dtype(dtype, [&](auto dt) {
        return by_act<ACTS_ALL>(act, [&](auto a) {
            if (o_dtype == ST_F32)
                hipLaunchKernelGGL((k_dropact_fwd<dt(), ST_F32, a()>), grid, dim3(256), 0, st, Y, ldy, R, ldr, O, ldo, M,
                                   N, slope, drop);
            else
                hipLaunchKernelGGL((k_dropact_fwd<dt(), dt(), a()>), grid, dim3(256), 0, st, Y, ldy, R, ldr, O, ldo, M,
                                   N, slope, drop);
            return hipGetLastError();
        });
    });
}

hipError_t run_drop_act_bwd(const void* D, int64_t ldd, int o_dtype, const void* Y, int64_t ldy, int dtype, void* DY,
                            int64_t lddy, int64_t M, int N, int act, float slope, const Drop& drop, hipStream_t st) {
    if (M == 0 || N == 0) return hipSuccess;
    const dim3 grid(stream_grid(M, N));
    return by_dtype(dtype, [&](auto dt) {
        return by_act<ACTS_ALL>(act, [&](auto a) {
            if (o_dtype == ST_F32)
                hipLaunchKernelGGL((k_dropact_bwd<dt(), ST_F32, a()>), grid, dim3(256), 0, st, D, ldd, Y, ldy, DY, lddy,
                                   M, N, slope, drop);
            else
                hipLaunchKernelGGL((k_dropact_bwd<dt(), dt(), a()>), grid, dim3(256), 0, st, D, ldd, Y, ldy, DY, lddy,
                                   M, N, slope, drop);
            return hipGetLastError();
        });
    });
}

}  // namespace sir
