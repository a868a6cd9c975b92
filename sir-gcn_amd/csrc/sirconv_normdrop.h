// sirconv_normdrop.h — the fused norm -> activation -> (dropout) -> + residual passes of GraphNorm
// (sirconv_graphnorm.hip), BatchNorm and LayerNorm (sirconv_nodenorm.hip): their launchers and the host-side
// choice of a kernel instantiation.  The activation (sig / dsig) and the 1- or 4-float access (vload / vstore)
// of the kernels are sirconv_device.h's.
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
#include "sirconv_internal.h"
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
    return by_act<ACTS_NORM>(act, [&](auto a) {
        if (v4) launch(a, std::integral_constant<int, 4>());
        else launch(a, std::integral_constant<int, 1>());
        return hipGetLastError();
    });
}
// both: launch(ACT, DROP, VW, d), for a pass that is one launch
template <typename Fn>
auto norm_dispatch(int act, const Drop& drop, bool v4, Fn&& launch) {
    return by_drop(drop, [&](auto dropped, const Drop& d) {
        return by_act_vw(act, v4, [&](auto a, auto vw) { launch(a, dropped, vw, d); });
    });
}

}  // namespace sir
