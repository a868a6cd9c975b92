// sirconv_normdrop.h — the fused norm -> activation -> (dropout) -> + residual passes of GraphNorm
// (sirconv_graphnorm.hip), BatchNorm and LayerNorm (sirconv_nodenorm.hip): their launchers, the device helpers
// the kernels share and the host-side choice of a kernel instantiation.
//
// The layer dropout of the node-level models (ogbn-arxiv/model.py:49,70: norm -> act ->
// dropout -> + resid; zinc/model.py:24,56: norm -> act -> dropout) fused into the three norm passes:
//   forward : out = d + R,  d = keep(row, col) ? act(y) * scale : +0
//   backward: g = act'(y) g0,  g0 = keep(row, col) ? dY * scale : 0   (one fp32 rounding), wherever the
//             no-dropout kernels take act'(y) dY; R's gradient stays dY.
// keep / scale / the seed are sirconv_dropout.h's at col0 = 0 (row = the global node row), so the bits are
// those sir_dropout_apply writes for an [M, N] block: no mask is stored and the backward recomputes it.
// These are the op order of torch's autograd for act -> dropout -> add, so the fused pass is bit-identical
// to the composed one.  A Drop that is off (p <= 0) launches the no-dropout instantiation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "sirconv.h"
#include "sirconv_dropout.h"

namespace sir {

// One launcher per pass; `drop` off (Drop()): the pass without dropout.
hipError_t run_graph_norm_fwd(const int64_t* off, int64_t B, int F, const float* X, int64_t ldx, const float* w,
                              const float* bias, const float* ms, float eps, int act, float slope, const float* R,
                              int64_t ldr, float* Y, int64_t ldy, float* mean, float* sd, const Drop& drop,
                              hipStream_t st);
hipError_t run_graph_norm_bwd(const int64_t* off, int64_t B, int F, const float* X, int64_t ldx, const float* dY,
                              int64_t ldg, const float* w, const float* bias, const float* ms, const float* mean,
                              const float* sd, int act, float slope, float* dX, int64_t lddx, float* dw_part,
                              float* dms_part, float* db_part, const Drop& drop, hipStream_t st);
hipError_t run_batch_norm_act_fwd(const float* X, int64_t ldx, int64_t M, int N, const double* mean,
                                  const double* invstd, const float* gamma, const float* beta, int act, float slope,
                                  const float* R, int64_t ldr, float* Y, int64_t ldy, const Drop& drop,
                                  hipStream_t st);
hipError_t run_batch_norm_act_bwd(const float* X, int64_t ldx, const float* D, int64_t ldg, int64_t M, int N,
                                  const double* mean, const double* invstd, const float* gamma, const float* beta,
                                  int act, float slope, int training, float* dX, int64_t lddx, float* dgamma,
                                  float* dbeta, float* work, const Drop& drop, hipStream_t st);
hipError_t run_layer_norm_act_fwd(const float* X, int64_t ldx, int64_t M, int N, const float* gamma,
                                  const float* beta, float eps, int act, float slope, const float* R, int64_t ldr,
                                  float* Y, int64_t ldy, float* mean, float* rstd, const Drop& drop, hipStream_t st);
hipError_t run_layer_norm_act_bwd(const float* X, int64_t ldx, const float* D, int64_t ldg, int64_t M, int N,
                                  const float* gamma, const float* beta, const float* mean, const float* rstd,
                                  int act, float slope, float* dX, int64_t lddx, float* dw_part, float* db_part,
                                  int64_t ldp, const Drop& drop, hipStream_t st);

// VW floats at p: one 16-byte access (VW 4, p 16-B aligned) or one float
template <int VW>
__device__ __forceinline__ void vld(float (&d)[VW], const float* __restrict__ p) {
    if constexpr (VW == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        d[0] = t.x; d[1] = t.y; d[2] = t.z; d[3] = t.w;
    } else {
        d[0] = p[0];
    }
}

template <int VW>
__device__ __forceinline__ void vst(float* __restrict__ p, const float (&s)[VW]) {
    if constexpr (VW == 4) *reinterpret_cast<float4*>(p) = make_float4(s[0], s[1], s[2], s[3]);
    else p[0] = s[0];
}

// the stack's activation after the norm (ogbn-arxiv/model.py:65-73: h = act(norm(h)) + resid), the
// ops of torch's relu / leaky_relu and their backward (x > 0 ? g : 0 / g * slope)
template <int ACT>
__device__ __forceinline__ float norm_act(float y, float slope) {
    if constexpr (ACT == SIR_ACT_RELU) return y <= 0.f ? 0.f : y;         // ReLU(NaN) = NaN, as torch.relu
    else if constexpr (ACT == SIR_ACT_LEAKY_RELU) return y > 0.f ? y : y * slope;
    else return y;
}
template <int ACT>
__device__ __forceinline__ float norm_act_bwd(float y, float g, float slope) {
    if constexpr (ACT == SIR_ACT_RELU) return y > 0.f ? g : 0.f;
    else if constexpr (ACT == SIR_ACT_LEAKY_RELU) return y > 0.f ? g : g * slope;
    else return g;
}

// host: p may be read in 16-byte vectors (NULL: an operand that is not there)
inline bool al(const void* p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// host: the kernel instantiation of a pass, its template arguments handed to a generic lambda as
// std::integral_constants (k<vw(), act(), dropped()>).
// by_drop: f(DROP, d) with DROP = drop.on() and d = drop, or Drop() when drop is off; f's result.
template <typename Fn>
auto by_drop(const Drop& drop, Fn&& f) {
    if (!drop.on()) return f(std::false_type(), Drop());
    return f(std::true_type(), drop);
}
// by_act_vw: launch(ACT, VW) with the activation and the vector width (v4 ? 4 : 1), then hipGetLastError();
// hipErrorInvalidValue (nothing launched) for an activation the passes do not have.
template <typename Fn>
auto by_act_vw(int act, bool v4, Fn&& launch) {
    auto by_vw = [&](auto a) {
        if (v4) launch(a, std::integral_constant<int, 4>());
        else launch(a, std::integral_constant<int, 1>());
    };
    switch (act) {
    case SIR_ACT_IDENTITY: by_vw(std::integral_constant<int, SIR_ACT_IDENTITY>()); break;
    case SIR_ACT_RELU: by_vw(std::integral_constant<int, SIR_ACT_RELU>()); break;
    case SIR_ACT_LEAKY_RELU: by_vw(std::integral_constant<int, SIR_ACT_LEAKY_RELU>()); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
// both: launch(ACT, DROP, VW, d), for a pass that is one launch
template <typename Fn>
auto norm_dispatch(int act, const Drop& drop, bool v4, Fn&& launch) {
    return by_drop(drop, [&](auto dropped, const Drop& d) {
        return by_act_vw(act, v4, [&](auto a, auto vw) { launch(a, dropped, vw, d); });
    });
}

}  // namespace sir
