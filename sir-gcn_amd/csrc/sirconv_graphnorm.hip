// sirconv_graphnorm.hip — fused GraphNorm (reference models/norm.py:7-29) for batched graphs.
//
// Nodes of graph b are rows [off[b], off[b+1]).  One wave per (graph, 64-lane column chunk); the
// graph's rows are walked sequentially, so every per-graph sum is taken in node order — the
// order of the reference's CPU scatter_add_ (norm.py:20,26) — and the forward reproduces it.
//   forward : mean = sum x / n;  d = x - mean * ms;  std = sqrt(sum d^2 / n + eps);
//             y = (w * d) / std + b                        (three passes over the graph's rows)
//   backward: A = sum gy*d, G = sum gy;  gd = w*gy/std - w*d*A/(n*std^3);  Bs = sum gd;
//             dx = gd - ms*Bs/n;  per-graph partials A/std, -mean*Bs, G for dw, dms, db
//             (reduced over graphs by the host with the deterministic column sum).
// The whole graph is re-read from L2 by each pass (molecule-sized graphs: a few KB), 32 (forward) / 16
// (backward, two arrays) rows' loads in flight at a time (walk_rows).  One wave per block (spread
// over the CUs), one column per lane by default (gn_wide below).
// Layer dropout (DROP instantiations; sirconv_normdrop.h): the forward stores keep(row, col) ? act(y) * scale : +0
// (+ R), the backward's gate takes act'(y) (keep ? dY * scale : 0); row = the row of X, not the row within its
// graph, hashed once per row (wave-uniform) and pass.  DROP = false: the kernels without it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sirconv.h"
#include "sirconv_internal.h"
#include "sirconv_device.h"
#include "sirconv_normdrop.h"

namespace sir {
namespace {

// Walk rows [r0, r1) in node order, RB rows' loads in flight at a time (a molecule has ~25 rows: the
// forward's passes take one memory latency each, the backward's two; a one-load-per-iteration loop
// paid one latency per row and pass, ~40 us per launch on cfg5);
// f(i, v) is applied in row order, so every per-graph sum keeps the reference's node order.
template <int VW, int RB = 32, typename Fn>
__device__ __forceinline__ void walk_rows(int64_t r0, int64_t r1, const float* __restrict__ base, int64_t ld, int c,
                                          Fn f) {
    int64_t i = r0;
    for (; i + RB <= r1; i += RB) {
        float v[RB][VW];
#pragma unroll
        for (int k = 0; k < RB; ++k) vload<VW>(v[k], base + (i + k) * ld + c * VW);
#pragma unroll
        for (int k = 0; k < RB; ++k) f(i + k, v[k]);
    }
    if (i < r1) {
        const int n = (int)(r1 - i);
        float v[RB][VW];
#pragma unroll
        for (int k = 0; k < RB; ++k) vload<VW>(v[k], base + (i + (k < n ? k : 0)) * ld + c * VW);
#pragma unroll
        for (int k = 0; k < RB; ++k)
            if (k < n) f(i + k, v[k]);
    }
}
// the same over two row-aligned arrays (X and dY)
template <int VW, int RB = 16, typename Fn>
__device__ __forceinline__ void walk_rows2(int64_t r0, int64_t r1, const float* __restrict__ a, int64_t lda,
                                           const float* __restrict__ b, int64_t ldb, int c, Fn f) {
    int64_t i = r0;
    for (; i + RB <= r1; i += RB) {
        float u[RB][VW], v[RB][VW];
#pragma unroll
        for (int k = 0; k < RB; ++k) {
            vload<VW>(u[k], a + (i + k) * lda + c * VW);
            vload<VW>(v[k], b + (i + k) * ldb + c * VW);
        }
#pragma unroll
        for (int k = 0; k < RB; ++k) f(i + k, u[k], v[k]);
    }
    if (i < r1) {
        const int n = (int)(r1 - i);
        float u[RB][VW], v[RB][VW];
#pragma unroll
        for (int k = 0; k < RB; ++k) {
            const int64_t q = i + (k < n ? k : 0);
            vload<VW>(u[k], a + q * lda + c * VW);
            vload<VW>(v[k], b + q * ldb + c * VW);
        }
#pragma unroll
        for (int k = 0; k < RB; ++k)
            if (k < n) f(i + k, u[k], v[k]);
    }
}

template <int VW, int ACT, bool DROP>
__global__ void __launch_bounds__(64)
k_gn_fwd(const int64_t* __restrict__ off, int64_t B, int F, int n_cc,
         const float* __restrict__ X, int64_t ldx, const float* __restrict__ w, const float* __restrict__ bias,
         const float* __restrict__ ms, float eps, float slope, const float* __restrict__ R, int64_t ldr,
         float* __restrict__ Y, int64_t ldy, float* __restrict__ mean_out, float* __restrict__ std_out, Drop drop) {
    if constexpr (DROP) drop = drop_resolve(drop);
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (wave >= B * n_cc) return;
    const int64_t b = wave / n_cc;
    const int cc = (int)(wave - b * n_cc);
    const int c = cc * 64 + (threadIdx.x & 63);          // in units of VW floats
    if (c * VW >= F) return;
    const int64_t r0 = off[b], r1 = off[b + 1];
    const float nf = (float)(r1 - r0);
    float s[VW], q[VW], t[VW], wv[VW], bv[VW], mv[VW];
#pragma unroll
    for (int x = 0; x < VW; ++x) { s[x] = 0.f; q[x] = 0.f; }
    walk_rows<VW>(r0, r1, X, ldx, c, [&](int64_t, const float (&v)[VW]) {   // norm.py:20 scatter_add_ (node order)
#pragma unroll
        for (int x = 0; x < VW; ++x) s[x] += v[x];
    });
    vload<VW>(wv, w + c * VW);
    if (bias) vload<VW>(bv, bias + c * VW);
    if (ms) vload<VW>(mv, ms + c * VW);
#pragma unroll
    for (int x = 0; x < VW; ++x) {
        s[x] = (r1 > r0) ? s[x] / nf : 0.f;               // norm.py:21 mean
        t[x] = ms ? s[x] * mv[x] : s[x];                  // norm.py:23 mean * mean_scale
    }
    walk_rows<VW>(r0, r1, X, ldx, c, [&](int64_t, const float (&v)[VW]) {   // norm.py:26 scatter_add_(demean^2)
#pragma unroll
        for (int x = 0; x < VW; ++x) {
            const float d = v[x] - t[x];
            q[x] += d * d;
        }
    });
    float sd[VW];
#pragma unroll
    for (int x = 0; x < VW; ++x) sd[x] = (r1 > r0) ? sqrtf(q[x] / nf + eps) : 0.f;   // norm.py:27
    auto norm_row = [&](int64_t i, const float (&v)[VW], float (&y)[VW]) {   // norm.py:29, then the activation
        uint32_t rh = 0;
        if constexpr (DROP) rh = drop_row_hash(drop, i);
#pragma unroll
        for (int x = 0; x < VW; ++x) {
            const float d = v[x] - t[x];
            y[x] = wv[x] * d / sd[x];
            if (bias) y[x] = y[x] + bv[x];
            y[x] = sig<ACT>(y[x], slope);
            if constexpr (DROP) y[x] = drop_keep(drop, rh, c * VW + x) ? y[x] * drop.scale : 0.f;
        }
    };
    if (R == nullptr) {
        walk_rows<VW>(r0, r1, X, ldx, c, [&](int64_t i, const float (&v)[VW]) {
            float y[VW];
            norm_row(i, v, y);
            vstore<VW>(Y + i * ldy + c * VW, y);
        });
    } else {                                              // + resid (model.py:73)
        walk_rows2<VW>(r0, r1, X, ldx, R, ldr, c, [&](int64_t i, const float (&v)[VW], const float (&r)[VW]) {
            float y[VW];
            norm_row(i, v, y);
#pragma unroll
            for (int x = 0; x < VW; ++x) y[x] = y[x] + r[x];
            vstore<VW>(Y + i * ldy + c * VW, y);
        });
    }
    vstore<VW>(mean_out + b * F + c * VW, s);
    vstore<VW>(std_out + b * F + c * VW, sd);
}

// ACT: dY is the gradient of act(y); the kernel takes g = act'(y) dY with y = the forward's norm output,
// recomputed by the forward's own ops (same bits, so the same side of 0)
template <int VW, int ACT, bool DROP>
__global__ void __launch_bounds__(64)
k_gn_bwd(const int64_t* __restrict__ off, int64_t B, int F, int n_cc,
         const float* __restrict__ X, int64_t ldx, const float* __restrict__ dY, int64_t ldg,
         const float* __restrict__ w, const float* __restrict__ bias, const float* __restrict__ ms,
         const float* __restrict__ mean, const float* __restrict__ sdv, float slope, float* __restrict__ dX,
         int64_t lddx, float* __restrict__ dw_part, float* __restrict__ dms_part, float* __restrict__ db_part,
         Drop drop) {
    if constexpr (DROP) drop = drop_resolve(drop);
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (wave >= B * n_cc) return;
    const int64_t b = wave / n_cc;
    const int cc = (int)(wave - b * n_cc);
    const int c = cc * 64 + (threadIdx.x & 63);
    if (c * VW >= F) return;
    const int64_t r0 = off[b], r1 = off[b + 1];
    const float nf = (float)(r1 - r0);
    float wv[VW], mv[VW], mu[VW], sd[VW], t[VW], A[VW], G[VW], Bs[VW], bv[VW];
    vload<VW>(wv, w + c * VW);
    if (ACT != SIR_ACT_IDENTITY && bias != nullptr) vload<VW>(bv, bias + c * VW);
    if (ms) vload<VW>(mv, ms + c * VW);
    else {
#pragma unroll
        for (int x = 0; x < VW; ++x) mv[x] = 1.f;
    }
    vload<VW>(mu, mean + b * F + c * VW);
    vload<VW>(sd, sdv + b * F + c * VW);
#pragma unroll
    for (int x = 0; x < VW; ++x) { t[x] = ms ? mu[x] * mv[x] : mu[x]; A[x] = 0.f; G[x] = 0.f; Bs[x] = 0.f; }
    // act'(y) dY for the row (y: the forward's norm output, same ops)
    auto gate = [&](int64_t i, const float (&v)[VW], const float (&gin)[VW], float (&g)[VW]) {
        uint32_t rh = 0;
        if constexpr (DROP) rh = drop_row_hash(drop, i);
#pragma unroll
        for (int x = 0; x < VW; ++x) {
            float g0 = gin[x];
            if constexpr (DROP) g0 = drop_keep(drop, rh, c * VW + x) ? g0 * drop.scale : 0.f;
            if constexpr (ACT == SIR_ACT_IDENTITY) {
                g[x] = g0;
            } else {
                float y = wv[x] * (v[x] - t[x]) / sd[x];
                if (bias) y = y + bv[x];
                g[x] = dsig<ACT>(y, g0, slope);
            }
        }
    };
    walk_rows2<VW>(r0, r1, X, ldx, dY, ldg, c, [&](int64_t i, const float (&v)[VW], const float (&g0)[VW]) {
        float g[VW];
        gate(i, v, g0, g);
#pragma unroll
        for (int x = 0; x < VW; ++x) { A[x] += g[x] * (v[x] - t[x]); G[x] += g[x]; }
    });
    float k1[VW], k2[VW];
#pragma unroll
    for (int x = 0; x < VW; ++x) {
        k1[x] = wv[x] / sd[x];                                       // w / s
        k2[x] = wv[x] * A[x] / (nf * sd[x] * sd[x] * sd[x]);          // w A / (n s^3)
    }
    walk_rows2<VW>(r0, r1, X, ldx, dY, ldg, c, [&](int64_t i, const float (&v)[VW], const float (&g0)[VW]) {
        float g[VW];
        gate(i, v, g0, g);
#pragma unroll
        for (int x = 0; x < VW; ++x) Bs[x] += k1[x] * g[x] - k2[x] * (v[x] - t[x]);
    });
    walk_rows2<VW>(r0, r1, X, ldx, dY, ldg, c, [&](int64_t i, const float (&v)[VW], const float (&g0)[VW]) {
        float g[VW];
        gate(i, v, g0, g);
        float o[VW];
#pragma unroll
        for (int x = 0; x < VW; ++x) o[x] = (k1[x] * g[x] - k2[x] * (v[x] - t[x])) - mv[x] * Bs[x] / nf;
        vstore<VW>(dX + i * lddx + c * VW, o);
    });
    float pw[VW], pm[VW];
#pragma unroll
    for (int x = 0; x < VW; ++x) {
        pw[x] = (r1 > r0) ? A[x] / sd[x] : 0.f;
        pm[x] = -(mu[x] * Bs[x]);
    }
    vstore<VW>(dw_part + b * F + c * VW, pw);
    if (dms_part) vstore<VW>(dms_part + b * F + c * VW, pm);
    vstore<VW>(db_part + b * F + c * VW, G);
}

// One column per lane (VW 1) by default: a wave walks its graph's rows in order three times, so
// its time is its instruction latency over the rows — 16-byte columns (VW 4) give each wave 4x the
// work and 4x fewer waves: config 5 (64 molecules, F = 300) 10.96 -> 6.48 us forward, 9.66 -> 6.63
// backward; 10,000 graphs at F = 128: 68.7 -> 54.5 forward, 108 vs 111 backward
// (profiles/r05_graphnorm.txt).  env SIR_GN_VW=4 takes the wide kernels.
bool gn_wide(int64_t, int) {
    const char* e = getenv("SIR_GN_VW");
    return e != nullptr && atoi(e) == 4;
}

}  // namespace

hipError_t run_graph_norm_fwd(const int64_t* off, int64_t B, int F, const float* X, int64_t ldx, const float* w,
                              const float* bias, const float* ms, float eps, int act, float slope, const float* R,
                              int64_t ldr, float* Y, int64_t ldy, float* mean, float* sd, const Drop& drop,
                              hipStream_t st) {
    if (B == 0) return hipSuccess;
    const bool v4 = F % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && (R == nullptr || ldr % 4 == 0) && aligned16(X) &&
                    aligned16(Y) && aligned16(R) && aligned16(w) && aligned16(bias) && aligned16(ms) &&
                    aligned16(mean) && aligned16(sd) && gn_wide(B, F);
    const int n_cc = (F / (v4 ? 4 : 1) + 63) / 64;
    const unsigned blocks = (unsigned)(B * n_cc);
    return norm_dispatch(act, drop, v4, [&](auto a, auto dropped, auto vw, const Drop& d) {
        hipLaunchKernelGGL((k_gn_fwd<vw(), a(), dropped()>), dim3(blocks), dim3(64), 0, st, off, B, F, n_cc, X, ldx, w,
                           bias, ms, eps, slope, R, ldr, Y, ldy, mean, sd, d);
    });
}

hipError_t run_graph_norm_bwd(const int64_t* off, int64_t B, int F, const float* X, int64_t ldx, const float* dY,
                              int64_t ldg, const float* w, const float* bias, const float* ms, const float* mean,
                              const float* sd, int act, float slope, float* dX, int64_t lddx, float* dw_part,
                              float* dms_part, float* db_part, const Drop& drop, hipStream_t st) {
    if (B == 0) return hipSuccess;
    const bool v4 = F % 4 == 0 && ldx % 4 == 0 && ldg % 4 == 0 && lddx % 4 == 0 && aligned16(X) && aligned16(dY) &&
                    aligned16(dX) && aligned16(w) && aligned16(bias) && aligned16(ms) && aligned16(mean) &&
                    aligned16(sd) && aligned16(dw_part) && aligned16(dms_part) && aligned16(db_part) && gn_wide(B, F);
    const int n_cc = (F / (v4 ? 4 : 1) + 63) / 64;
    const unsigned blocks = (unsigned)(B * n_cc);
    return norm_dispatch(act, drop, v4, [&](auto a, auto dropped, auto vw, const Drop& d) {
        hipLaunchKernelGGL((k_gn_bwd<vw(), a(), dropped()>), dim3(blocks), dim3(64), 0, st, off, B, F, n_cc, X, ldx, dY,
                           ldg, w, bias, ms, mean, sd, slope, dX, lddx, dw_part, dms_part, db_part, d);
    });
}

}  // namespace sir
