// sirconv_nodenorm.hip — BatchNorm1d and LayerNorm over node features [M, N] (reference models/norm.py:53-60,
// built by GetNorm, norm.py:68-82) with the stack's activation and residual fused: out = act(norm(x)) + R.
//
// fp32, row-major, explicit leading dimensions, any N >= 1: float4 columns (VW 4) when N % 4 == 0 and every
// row is 16-B aligned, scalar (VW 1) otherwise.  No atomics.  Every partition of the rows depends on (M, N)
// only — BatchNorm: slabs of SIR_BN_SLAB_ROWS rows; LayerNorm backward: ln_rows_per_part(M) rows per partial
// row — and partials are combined in slab order, so the bits do not depend on the device or the run.
//
// BatchNorm (nn.BatchNorm1d on 2-D input), a block per (slab, column chunk); thread (rsub, cv) walks the
// slab's rows rsub, rsub + RS, ... of its VW columns (RS rows x CWV column vectors = the block, RS * CWV <= 256):
//   k_bn_stats    per slab and column (mean, M2) in fp64: 8 rows in registers at a time -> their mean, then
//                 their centred squares, merged into the thread's running pair (Chan), the RS threads of a
//                 column merged in rsub order through LDS.  Never E[x^2] - mean^2.
//   k_bn_finish   merges the slabs' pairs per column: 64 slices of consecutive slabs, each in slab order,
//                 then the 64 slice results in slice order; mean, invstd = 1 / sqrt(M2 / M + eps) and the
//                 running buffers' update.  The same kernel sums the backward's per-slab pairs.
//   k_bn_apply    y = (x - mean) * (invstd * gamma) + beta with the [N] statistics in fp64, rounded once;
//                 out = act(y) + R.
//   k_bn_bwd_red  g = act'(y) D (y recomputed by k_bn_apply's own ops); per slab sum g, dotp = sum g (x - mean)
//                 (fp64); dbeta = sum g, dgamma = dotp * invstd.
//   k_bn_bwd_app  dX = ((g - dbeta / M) - (x - mean) * dotp * invstd^2 / M) * invstd * gamma (torch's CPU form;
//                 eval: g * invstd * gamma).
// LayerNorm (N <= 1024), one wave per row, the row in registers (NCH vectors per lane), RB rows in flight:
//   k_ln_fwd      mean, centred variance, rstd = 1 / sqrt(var + eps), y = (x - mean) * rstd * gamma + beta,
//                 out = act(y) + R in one pass; mean / rstd [M] kept.
//   k_ln_bwd      g = act'(y) D;  dX = rstd * (g gamma - mean_row(g gamma) - xhat * mean_row(g gamma xhat));
//                 the wave's rows' sum g * xhat, sum g as one partial row (summed by the deterministic
//                 column sum, run_colsum).
// Layer dropout (DROP instantiations; sirconv_normdrop.h): out = drop(act(y)) + R, drop(a) = keep(row, col) ? a * scale : +0
// with the bits of sirconv_dropout.h at col0 = 0 (the row hash once per row and thread, one fmix per element); every
// backward kernel takes g = act'(y) (keep ? D * scale : 0) wherever it took act'(y) D.  The DROP = false
// instantiations are the kernels without it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "sirconv.h"
#include "sirconv_internal.h"
#include "sirconv_device.h"
#include "sirconv_normdrop.h"

namespace sir {
namespace {

constexpr int SLAB = SIR_BN_SLAB_ROWS;
constexpr int BN_THREADS = 256;
constexpr int FIN_SLICES = 64;      // k_bn_finish: 64 slices x 16 columns per block
constexpr int FIN_COLS = 16;

// (na, mean, m2) <- merge with (nb, bm, bq) (Chan et al.); nb > 0.  The statistics are carried in fp64 (as
// torch's CPU BatchNorm accumulates them): mean and invstd come out correctly rounded, which is what keeps
// a two-row batch (1 - xhat^2 = eps * invstd^2: every ulp of the mean counts 1 / eps times) at torch's error.
__device__ __forceinline__ void chan(double& na, double& mean, double& m2, double nb, double bm, double bq) {
    const double nt = na + nb;
    const double w = nb / nt;
    const double d = bm - mean;
    mean = mean + d * w;
    m2 = m2 + (bq + d * d * (na * w));
    na = nt;
}

// the thread's place in a BatchNorm block: row slice rsub, column vector c (units of VW floats)
struct BnPos {
    int rsub, c;
    bool on;
};
__device__ __forceinline__ BnPos bn_pos(int cwv, int rs, int nv) {
    BnPos p;
    p.rsub = (int)threadIdx.x / cwv;
    const int cv = (int)threadIdx.x - p.rsub * cwv;
    p.c = (int)blockIdx.y * cwv + cv;
    p.on = p.rsub < rs && p.c < nv;
    return p;
}

template <int VW>
__global__ void __launch_bounds__(BN_THREADS)
k_bn_stats(const float* __restrict__ X, int64_t ldx, int64_t M, int N, int cwv, int rs,
           double* __restrict__ pmean, double* __restrict__ pm2) {
    __shared__ float s_n[BN_THREADS];
    __shared__ double s_mean[BN_THREADS][VW];
    __shared__ double s_m2[BN_THREADS][VW];
    const BnPos p = bn_pos(cwv, rs, N / VW);
    const int64_t r0 = (int64_t)blockIdx.x * SLAB;
    const int64_t r1 = r0 + SLAB < M ? r0 + SLAB : M;
    double na = 0.0, mean[VW], m2[VW];
#pragma unroll
    for (int x = 0; x < VW; ++x) { mean[x] = 0.0; m2[x] = 0.0; }
    if (p.on) {
        for (int64_t base = r0 + p.rsub; base < r1; base += (int64_t)rs * 8) {
            float v[8][VW];
            const int64_t left = (r1 - base + rs - 1) / rs;       // this thread's rows from `base` on
            const int nb = left < 8 ? (int)left : 8;
#pragma unroll
            for (int k = 0; k < 8; ++k) vload<VW>(v[k], X + (base + (int64_t)(k < nb ? k : 0) * rs) * ldx + (int64_t)p.c * VW);
            const double nbf = (double)nb;
            double n2 = na;
#pragma unroll
            for (int x = 0; x < VW; ++x) {
                double s = 0.0, q = 0.0;
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (k < nb) s += (double)v[k][x];
                const double bm = s / nbf;
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (k < nb) { const double d = (double)v[k][x] - bm; q += d * d; }
                n2 = na;
                chan(n2, mean[x], m2[x], nbf, bm, q);
            }
            na = n2;
        }
    }
    s_n[threadIdx.x] = (float)na;
#pragma unroll
    for (int x = 0; x < VW; ++x) { s_mean[threadIdx.x][x] = mean[x]; s_m2[threadIdx.x][x] = m2[x]; }
    __syncthreads();
    if (p.on && p.rsub == 0) {                                    // the column's RS threads, in rsub order
        for (int j = 1; j < rs; ++j) {
            const int t = j * cwv + (int)threadIdx.x;
            const double nb = (double)s_n[t];
            if (nb > 0.0) {
                double n2 = na;
#pragma unroll
                for (int x = 0; x < VW; ++x) {
                    n2 = na;
                    chan(n2, mean[x], m2[x], nb, s_mean[t][x], s_m2[t][x]);
                }
                na = n2;
            }
        }
#pragma unroll
        for (int x = 0; x < VW; ++x) {
            pmean[(int64_t)blockIdx.x * N + (int64_t)p.c * VW + x] = mean[x];
            pm2[(int64_t)blockIdx.x * N + (int64_t)p.c * VW + x] = m2[x];
        }
    }
}

// STATS: pa = the slabs' means, pb = their M2 -> stat_a = mean, stat_b = invstd (fp64; + running update).
// !STATS: pa = the slabs' sum g, pb = their sum g (x - mean) -> out_a = dbias, out_b = dweight = dotp * invstd,
//         and the apply pass's per-column constants stat_a[c] = sum g / M, stat_b[c] = dotp * invstd^2 / M.
template <bool STATS>
__global__ void __launch_bounds__(FIN_SLICES * FIN_COLS)
k_bn_finish(const double* __restrict__ pa, const double* __restrict__ pb, int64_t S, int64_t M, int N, float eps,
            float momentum, float* __restrict__ run_mean, float* __restrict__ run_var,
            const double* __restrict__ invstd, float* __restrict__ out_a, float* __restrict__ out_b,
            double* __restrict__ stat_a, double* __restrict__ stat_b) {
    __shared__ double s_n[FIN_SLICES][FIN_COLS];
    __shared__ double s_a[FIN_SLICES][FIN_COLS];
    __shared__ double s_b[FIN_SLICES][FIN_COLS];
    const int cl = (int)threadIdx.x % FIN_COLS, slice = (int)threadIdx.x / FIN_COLS;
    const int c = (int)blockIdx.x * FIN_COLS + cl;
    const int64_t per = (S + FIN_SLICES - 1) / FIN_SLICES;
    const int64_t s0 = slice * per;
    const int64_t s1 = s0 + per < S ? s0 + per : S;
    double na = 0.0, a = 0.0, b = 0.0;
    if (c < N) {
        for (int64_t s = s0; s < s1; s += 4) {
            double va[4], vb[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t q = s + k < s1 ? s + k : s;
                va[k] = pa[q * N + c];
                vb[k] = pb[q * N + c];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (s + k < s1) {
                    if constexpr (STATS) {
                        const int64_t left = M - (s + k) * SLAB;
                        chan(na, a, b, (double)(left < SLAB ? left : SLAB), va[k], vb[k]);
                    } else {
                        a += va[k];
                        b += vb[k];
                    }
                }
            }
        }
    }
    s_n[slice][cl] = na;
    s_a[slice][cl] = a;
    s_b[slice][cl] = b;
    __syncthreads();
    if (slice == 0 && c < N) {
        for (int j = 1; j < FIN_SLICES; ++j) {
            if constexpr (STATS) {
                if (s_n[j][cl] > 0.0) chan(na, a, b, s_n[j][cl], s_a[j][cl], s_b[j][cl]);
            } else {
                a += s_a[j][cl];
                b += s_b[j][cl];
            }
        }
        if constexpr (STATS) {
            const double var = b / (double)M;
            stat_a[c] = a;
            stat_b[c] = 1.0 / sqrt(var + (double)eps);
            if (run_mean != nullptr) {
                const double unb = b / (double)(M - 1), mo = (double)momentum;
                run_mean[c] = (float)((1.0 - mo) * (double)run_mean[c] + mo * a);
                run_var[c] = (float)((1.0 - mo) * (double)run_var[c] + mo * unb);
            }
        } else {
            const double is = invstd[c];
            out_a[c] = (float)a;
            out_b[c] = (float)(b * is);
            stat_a[c] = a / (double)M;
            stat_b[c] = b * is * is / (double)M;
        }
    }
}

// the columns' fp64 statistics: mu = mean, a = invstd * gamma, b = beta.  Per element c = x - mu and
// y = c * a + b are formed in fp64 and rounded once, so neither grows with |mean| / std.
template <int VW>
__device__ __forceinline__ void bn_cols(double (&mu)[VW], double (&a)[VW], double (&b)[VW], const double* __restrict__ mean,
                                        const double* __restrict__ invstd, const float* __restrict__ gamma,
                                        const float* __restrict__ beta, int64_t col) {
#pragma unroll
    for (int x = 0; x < VW; ++x) {
        mu[x] = mean[col + x];
        a[x] = invstd[col + x] * (double)gamma[col + x];
        b[x] = (double)beta[col + x];
    }
}

template <int VW, int ACT, bool DROP>
__global__ void __launch_bounds__(BN_THREADS)
k_bn_apply(const float* __restrict__ X, int64_t ldx, int64_t M, int N, int cwv, int rs,
           const double* __restrict__ mean, const double* __restrict__ invstd, const float* __restrict__ gamma,
           const float* __restrict__ beta, float slope, const float* __restrict__ R, int64_t ldr,
           float* __restrict__ Y, int64_t ldy, Drop drop) {
    if constexpr (DROP) drop = drop_resolve(drop);
    const BnPos p = bn_pos(cwv, rs, N / VW);
    if (!p.on) return;
    const int64_t r0 = (int64_t)blockIdx.x * SLAB;
    const int64_t r1 = r0 + SLAB < M ? r0 + SLAB : M;
    const int64_t col = (int64_t)p.c * VW;
    double mu[VW], a[VW], b[VW];
    bn_cols<VW>(mu, a, b, mean, invstd, gamma, beta, col);
    for (int64_t base = r0 + p.rsub; base < r1; base += (int64_t)rs * 4) {
        float v[4][VW], r[4][VW];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t row = base + (int64_t)k * rs < r1 ? base + (int64_t)k * rs : base;
            vload<VW>(v[k], X + row * ldx + col);
            if (R != nullptr) vload<VW>(r[k], R + row * ldr + col);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t row = base + (int64_t)k * rs;
            if (row < r1) {
                float o[VW];
                uint32_t rh = 0;
                if constexpr (DROP) rh = drop_row_hash(drop, row);
#pragma unroll
                for (int x = 0; x < VW; ++x) {
                    const float y = (float)(((double)v[k][x] - mu[x]) * a[x] + b[x]);
                    o[x] = sig<ACT>(y, slope);
                    if constexpr (DROP) o[x] = drop_keep(drop, rh, (int)col + x) ? o[x] * drop.scale : 0.f;
                    if (R != nullptr) o[x] = o[x] + r[k][x];
                }
                vstore<VW>(Y + row * ldy + col, o);
            }
        }
    }
}

// per slab: sum g and sum g (x - mean) (fp64), g = act'(y) D, y by k_bn_apply's own ops
template <int VW, int ACT, bool DROP>
__global__ void __launch_bounds__(BN_THREADS)
k_bn_bwd_red(const float* __restrict__ X, int64_t ldx, const float* __restrict__ D, int64_t ldg, int64_t M, int N,
             int cwv, int rs, const double* __restrict__ mean, const double* __restrict__ invstd,
             const float* __restrict__ gamma, const float* __restrict__ beta, float slope,
             double* __restrict__ pdb, double* __restrict__ pdg, Drop drop) {
    if constexpr (DROP) drop = drop_resolve(drop);
    __shared__ double s_b[BN_THREADS][VW];
    __shared__ double s_g[BN_THREADS][VW];
    const BnPos p = bn_pos(cwv, rs, N / VW);
    const int64_t r0 = (int64_t)blockIdx.x * SLAB;
    const int64_t r1 = r0 + SLAB < M ? r0 + SLAB : M;
    const int64_t col = (int64_t)p.c * VW;
    double sb[VW], sg[VW];
#pragma unroll
    for (int x = 0; x < VW; ++x) { sb[x] = 0.0; sg[x] = 0.0; }
    if (p.on) {
        double mu[VW], a[VW], b[VW];
        bn_cols<VW>(mu, a, b, mean, invstd, gamma, beta, col);
        for (int64_t base = r0 + p.rsub; base < r1; base += (int64_t)rs * 4) {
            float v[4][VW], d[4][VW];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t row = base + (int64_t)k * rs < r1 ? base + (int64_t)k * rs : base;
                vload<VW>(v[k], X + row * ldx + col);
                vload<VW>(d[k], D + row * ldg + col);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (base + (int64_t)k * rs < r1) {
                    uint32_t rh = 0;
                    if constexpr (DROP) rh = drop_row_hash(drop, base + (int64_t)k * rs);
#pragma unroll
                    for (int x = 0; x < VW; ++x) {
                        const double c = (double)v[k][x] - mu[x];
                        const float y = (float)(c * a[x] + b[x]);
                        float g0 = d[k][x];
                        if constexpr (DROP) g0 = drop_keep(drop, rh, (int)col + x) ? g0 * drop.scale : 0.f;
                        const float gg = dsig<ACT>(y, g0, slope);
                        sb[x] += (double)gg;
                        sg[x] += (double)gg * c;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int x = 0; x < VW; ++x) { s_b[threadIdx.x][x] = sb[x]; s_g[threadIdx.x][x] = sg[x]; }
    __syncthreads();
    if (p.on && p.rsub == 0) {
        for (int j = 1; j < rs; ++j) {
            const int t = j * cwv + (int)threadIdx.x;
#pragma unroll
            for (int x = 0; x < VW; ++x) { sb[x] += s_b[t][x]; sg[x] += s_g[t][x]; }
        }
#pragma unroll
        for (int x = 0; x < VW; ++x) {
            pdb[(int64_t)blockIdx.x * N + col + x] = sb[x];
            pdg[(int64_t)blockIdx.x * N + col + x] = sg[x];
        }
    }
}

// training: dX = ((g - gm) - (x - mean) k) invstd gamma, gm = sum g / M, k = dotp invstd^2 / M (fp64, rounded
// once); eval: dX = g invstd gamma
template <int VW, int ACT, bool DROP>
__global__ void __launch_bounds__(BN_THREADS)
k_bn_bwd_app(const float* __restrict__ X, int64_t ldx, const float* __restrict__ D, int64_t ldg, int64_t M, int N,
             int cwv, int rs, const double* __restrict__ mean, const double* __restrict__ invstd,
             const float* __restrict__ gamma, const float* __restrict__ beta, float slope,
             const double* __restrict__ gmean, const double* __restrict__ kdot, int training,
             float* __restrict__ dX, int64_t lddx, Drop drop) {
    if constexpr (DROP) drop = drop_resolve(drop);
    const BnPos p = bn_pos(cwv, rs, N / VW);
    if (!p.on) return;
    const int64_t r0 = (int64_t)blockIdx.x * SLAB;
    const int64_t r1 = r0 + SLAB < M ? r0 + SLAB : M;
    const int64_t col = (int64_t)p.c * VW;
    double mu[VW], a[VW], b[VW], gm[VW], kk[VW];
    bn_cols<VW>(mu, a, b, mean, invstd, gamma, beta, col);
#pragma unroll
    for (int x = 0; x < VW; ++x) {
        gm[x] = training ? gmean[col + x] : 0.0;
        kk[x] = training ? kdot[col + x] : 0.0;
    }
    for (int64_t base = r0 + p.rsub; base < r1; base += (int64_t)rs * 4) {
        float v[4][VW], d[4][VW];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t row = base + (int64_t)k * rs < r1 ? base + (int64_t)k * rs : base;
            vload<VW>(v[k], X + row * ldx + col);
            vload<VW>(d[k], D + row * ldg + col);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t row = base + (int64_t)k * rs;
            if (row < r1) {
                float o[VW];
                uint32_t rh = 0;
                if constexpr (DROP) rh = drop_row_hash(drop, row);
#pragma unroll
                for (int x = 0; x < VW; ++x) {
                    const double c = (double)v[k][x] - mu[x];
                    const float y = (float)(c * a[x] + b[x]);
                    float g0 = d[k][x];
                    if constexpr (DROP) g0 = drop_keep(drop, rh, (int)col + x) ? g0 * drop.scale : 0.f;
                    const float gg = dsig<ACT>(y, g0, slope);
                    o[x] = (float)((((double)gg - gm[x]) - c * kk[x]) * a[x]);
                }
                vstore<VW>(dX + row * lddx + col, o);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ LayerNorm
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// rows of one wave's iteration: up to 16 floats per lane and row in flight
constexpr int ln_rb(int vw, int nch, int cap) {
    const int r = cap / (vw * nch);
    return r < 1 ? 1 : (r > 4 ? 4 : r);
}

template <int VW, int NCH, int ACT, bool DROP>
__global__ void __launch_bounds__(64)
k_ln_fwd(const float* __restrict__ X, int64_t ldx, int64_t M, int N, int64_t rpw, const float* __restrict__ gamma,
         const float* __restrict__ beta, float eps, float slope, const float* __restrict__ R, int64_t ldr,
         float* __restrict__ Y, int64_t ldy, float* __restrict__ mean_out, float* __restrict__ rstd_out, Drop drop) {
    if constexpr (DROP) drop = drop_resolve(drop);
    constexpr int RB = ln_rb(VW, NCH, 16);
    const int lane = (int)threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * rpw;
    const int64_t r1 = r0 + rpw < M ? r0 + rpw : M;
    const float nf = (float)N;
    bool on[NCH];
    float g[NCH][VW], b[NCH][VW];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int c = (j * 64 + lane) * VW;
        on[j] = c < N;
#pragma unroll
        for (int x = 0; x < VW; ++x) { g[j][x] = 0.f; b[j][x] = 0.f; }
        if (on[j]) { vload<VW>(g[j], gamma + c); vload<VW>(b[j], beta + c); }
    }
    for (int64_t r = r0; r < r1; r += RB) {
        float v[RB][NCH][VW], rr[RB][NCH][VW];
#pragma unroll
        for (int k = 0; k < RB; ++k) {
            const int64_t row = r + k < r1 ? r + k : r;
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
#pragma unroll
                for (int x = 0; x < VW; ++x) { v[k][j][x] = 0.f; rr[k][j][x] = 0.f; }
                if (on[j]) {
                    vload<VW>(v[k][j], X + row * ldx + (j * 64 + lane) * VW);
                    if (R != nullptr) vload<VW>(rr[k][j], R + row * ldr + (j * 64 + lane) * VW);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < RB; ++k) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < NCH; ++j)
#pragma unroll
                for (int x = 0; x < VW; ++x) s += v[k][j][x];
            const float mu = wave_sum(s) / nf;
            float q = 0.f;
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                if (on[j]) {
#pragma unroll
                    for (int x = 0; x < VW; ++x) { const float d = v[k][j][x] - mu; q += d * d; }
                }
            }
            const float rstd = 1.0f / sqrtf(wave_sum(q) / nf + eps);
            if (r + k < r1) {
                uint32_t rh = 0;                                   // wave-uniform: the row is the wave's
                if constexpr (DROP) rh = drop_row_hash(drop, r + k);
#pragma unroll
                for (int j = 0; j < NCH; ++j) {
                    if (on[j]) {
                        float o[VW];
#pragma unroll
                        for (int x = 0; x < VW; ++x) {
                            const float y = (v[k][j][x] - mu) * rstd * g[j][x] + b[j][x];
                            o[x] = sig<ACT>(y, slope);
                            if constexpr (DROP)
                                o[x] = drop_keep(drop, rh, (j * 64 + lane) * VW + x) ? o[x] * drop.scale : 0.f;
                            if (R != nullptr) o[x] = o[x] + rr[k][j][x];
                        }
                        vstore<VW>(Y + (r + k) * ldy + (j * 64 + lane) * VW, o);
                    }
                }
                if (lane == 0) { mean_out[r + k] = mu; rstd_out[r + k] = rstd; }
            }
        }
    }
}

template <int VW, int NCH, int ACT, bool DROP>
__global__ void __launch_bounds__(64)
k_ln_bwd(const float* __restrict__ X, int64_t ldx, const float* __restrict__ D, int64_t ldg, int64_t M, int N,
         int64_t rpw, const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ mean,
         const float* __restrict__ rstd, float slope, float* __restrict__ dX, int64_t lddx,
         float* __restrict__ dw_part, float* __restrict__ db_part, int64_t ldp, Drop drop) {
    if constexpr (DROP) drop = drop_resolve(drop);
    constexpr int RB = ln_rb(VW, NCH, 8);
    const int lane = (int)threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * rpw;
    const int64_t r1 = r0 + rpw < M ? r0 + rpw : M;
    const float nf = (float)N;
    bool on[NCH];
    float g[NCH][VW], b[NCH][VW], dw[NCH][VW], db[NCH][VW];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int c = (j * 64 + lane) * VW;
        on[j] = c < N;
#pragma unroll
        for (int x = 0; x < VW; ++x) { g[j][x] = 0.f; b[j][x] = 0.f; dw[j][x] = 0.f; db[j][x] = 0.f; }
        if (on[j]) { vload<VW>(g[j], gamma + c); vload<VW>(b[j], beta + c); }
    }
    for (int64_t r = r0; r < r1; r += RB) {
        float v[RB][NCH][VW], d[RB][NCH][VW], mu[RB], rs[RB];
#pragma unroll
        for (int k = 0; k < RB; ++k) {
            const int64_t row = r + k < r1 ? r + k : r;
            mu[k] = mean[row];
            rs[k] = rstd[row];
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
#pragma unroll
                for (int x = 0; x < VW; ++x) { v[k][j][x] = 0.f; d[k][j][x] = 0.f; }
                if (on[j]) {
                    vload<VW>(v[k][j], X + row * ldx + (j * 64 + lane) * VW);
                    vload<VW>(d[k][j], D + row * ldg + (j * 64 + lane) * VW);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < RB; ++k) {
            if (r + k < r1) {                                      // wave-uniform
                float xh[NCH][VW], a[NCH][VW];
                float s1 = 0.f, s2 = 0.f;
                uint32_t rh = 0;
                if constexpr (DROP) rh = drop_row_hash(drop, r + k);
#pragma unroll
                for (int j = 0; j < NCH; ++j) {
#pragma unroll
                    for (int x = 0; x < VW; ++x) {
                        xh[j][x] = (v[k][j][x] - mu[k]) * rs[k];
                        const float y = xh[j][x] * g[j][x] + b[j][x];
                        float g0 = d[k][j][x];
                        if constexpr (DROP) g0 = drop_keep(drop, rh, (j * 64 + lane) * VW + x) ? g0 * drop.scale : 0.f;
                        const float gg = on[j] ? dsig<ACT>(y, g0, slope) : 0.f;
                        db[j][x] += gg;
                        dw[j][x] += gg * xh[j][x];
                        a[j][x] = gg * g[j][x];
                        s1 += a[j][x];
                        s2 += a[j][x] * xh[j][x];
                    }
                }
                const float m1 = wave_sum(s1) / nf;
                const float m2 = wave_sum(s2) / nf;
#pragma unroll
                for (int j = 0; j < NCH; ++j) {
                    if (on[j]) {
                        float o[VW];
#pragma unroll
                        for (int x = 0; x < VW; ++x) o[x] = rs[k] * ((a[j][x] - m1) - xh[j][x] * m2);
                        vstore<VW>(dX + (r + k) * lddx + (j * 64 + lane) * VW, o);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        if (on[j]) {
            vstore<VW>(dw_part + (int64_t)blockIdx.x * ldp + (j * 64 + lane) * VW, dw[j]);
            vstore<VW>(db_part + (int64_t)blockIdx.x * ldp + (j * 64 + lane) * VW, db[j]);
        }
    }
}

// block geometry of the BatchNorm kernels: column chunks of cwv vectors, rs row slices (rs * cwv <= 256)
struct BnGeom {
    int vw, cwv, rs;
    dim3 grid;
};
BnGeom bn_geom(int64_t M, int N, bool v4) {
    BnGeom g;
    g.vw = v4 ? 4 : 1;
    const int nv = N / g.vw;
    const int chunks = (nv + BN_THREADS - 1) / BN_THREADS;
    g.cwv = (nv + chunks - 1) / chunks;
    g.rs = BN_THREADS / g.cwv;
    if (g.rs > SLAB) g.rs = SLAB;
    g.grid = dim3((unsigned)((M + SLAB - 1) / SLAB), (unsigned)chunks);
    return g;
}

}  // namespace

int64_t batch_norm_slabs(int64_t M) { return (M + SLAB - 1) / SLAB; }

// workspace (floats): two [slabs, N] fp64 arrays of per-slab partials, then the backward's [2, N] fp64 constants
int64_t batch_norm_work_floats(int64_t M, int64_t N) { return M == 0 ? 0 : 4 * batch_norm_slabs(M) * N + 4 * N; }

hipError_t run_batch_norm_stats(const float* X, int64_t ldx, int64_t M, int N, float eps, float momentum,
                                float* run_mean, float* run_var, double* mean, double* invstd, float* work,
                                hipStream_t st) {
    if (M == 0) return hipSuccess;
    const int64_t S = batch_norm_slabs(M);
    double* pmean = reinterpret_cast<double*>(work);
    double* pm2 = pmean + S * N;
    const bool v4 = N % 4 == 0 && ldx % 4 == 0 && aligned16(X);
    const BnGeom g = bn_geom(M, N, v4);
    if (v4)
        hipLaunchKernelGGL((k_bn_stats<4>), g.grid, dim3(BN_THREADS), 0, st, X, ldx, M, N, g.cwv, g.rs, pmean, pm2);
    else
        hipLaunchKernelGGL((k_bn_stats<1>), g.grid, dim3(BN_THREADS), 0, st, X, ldx, M, N, g.cwv, g.rs, pmean, pm2);
    hipLaunchKernelGGL((k_bn_finish<true>), dim3((unsigned)((N + FIN_COLS - 1) / FIN_COLS)), dim3(FIN_SLICES * FIN_COLS),
                       0, st, pmean, pm2, S, M, N, eps, momentum, run_mean, run_var, nullptr, nullptr, nullptr, mean, invstd);
    return hipGetLastError();
}

hipError_t run_batch_norm_act_fwd(const float* X, int64_t ldx, int64_t M, int N, const double* mean,
                                  const double* invstd, const float* gamma, const float* beta, int act, float slope,
                                  const float* R, int64_t ldr, float* Y, int64_t ldy, const Drop& drop,
                                  hipStream_t st) {
    if (M == 0) return hipSuccess;
    const bool v4 = N % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && (R == nullptr || ldr % 4 == 0) && aligned16(X) &&
                    aligned16(Y) && aligned16(R);
    const BnGeom g = bn_geom(M, N, v4);
    return norm_dispatch(act, drop, v4, [&](auto a, auto dropped, auto vw, const Drop& d) {
        hipLaunchKernelGGL((k_bn_apply<vw(), a(), dropped()>), g.grid, dim3(BN_THREADS), 0, st, X, ldx, M, N, g.cwv,
                           g.rs, mean, invstd, gamma, beta, slope, R, ldr, Y, ldy, d);
    });
}

hipError_t run_batch_norm_act_bwd(const float* X, int64_t ldx, const float* D, int64_t ldg, int64_t M, int N,
                                  const double* mean, const double* invstd, const float* gamma, const float* beta,
                                  int act, float slope, int training, float* dX, int64_t lddx, float* dgamma,
                                  float* dbeta, float* work, const Drop& drop, hipStream_t st) {
    if (M == 0) return hipSuccess;
    const int64_t S = batch_norm_slabs(M);
    double* pdb = reinterpret_cast<double*>(work);
    double* pdg = pdb + S * N;
    double* gmean = pdg + S * N;
    double* kdot = gmean + N;
    const bool v4 = N % 4 == 0 && ldx % 4 == 0 && ldg % 4 == 0 && lddx % 4 == 0 && aligned16(X) && aligned16(D) &&
                    aligned16(dX);
    const BnGeom g = bn_geom(M, N, v4);
    return by_drop(drop, [&](auto dropped, const Drop& d) {
        const hipError_t err = by_act_vw(act, v4, [&](auto a, auto vw) {
            hipLaunchKernelGGL((k_bn_bwd_red<vw(), a(), dropped()>), g.grid, dim3(BN_THREADS), 0, st, X, ldx, D, ldg, M,
                               N, g.cwv, g.rs, mean, invstd, gamma, beta, slope, pdb, pdg, d);
        });
        if (err != hipSuccess) return err;
        hipLaunchKernelGGL((k_bn_finish<false>), dim3((unsigned)((N + FIN_COLS - 1) / FIN_COLS)),
                           dim3(FIN_SLICES * FIN_COLS), 0, st, pdb, pdg, S, M, N, 0.f, 0.f, nullptr, nullptr, invstd,
                           dbeta, dgamma, gmean, kdot);
        return by_act_vw(act, v4, [&](auto a, auto vw) {
            hipLaunchKernelGGL((k_bn_bwd_app<vw(), a(), dropped()>), g.grid, dim3(BN_THREADS), 0, st, X, ldx, D, ldg, M,
                               N, g.cwv, g.rs, mean, invstd, gamma, beta, slope, gmean, kdot, training, dX, lddx, d);
        });
    });
}

// rows per wave (= per partial row of the backward): a function of M alone
int64_t layer_norm_rows_per_part(int64_t M) {
    const int64_t r = (M + SIR_LN_MAX_PARTS - 1) / SIR_LN_MAX_PARTS;
    return r < 16 ? 16 : r;
}
int64_t layer_norm_parts(int64_t M) {
    const int64_t rpw = layer_norm_rows_per_part(M);
    return (M + rpw - 1) / rpw;
}

namespace {

// NCH: float4 rows 1, 2 or 4 vectors per lane (N <= 256, 512, 1024); scalar rows 1, 2, 4, 8 or 16.
// go(NCH) launches the kernel of width VW with that many vectors per lane.
template <int VW, typename Fn>
void ln_by_nch(int N, Fn&& go) {
    if constexpr (VW == 4) {
        if (N <= 256) go(std::integral_constant<int, 1>());
        else if (N <= 512) go(std::integral_constant<int, 2>());
        else go(std::integral_constant<int, 4>());
    } else {
        if (N <= 64) go(std::integral_constant<int, 1>());
        else if (N <= 128) go(std::integral_constant<int, 2>());
        else if (N <= 256) go(std::integral_constant<int, 4>());
        else if (N <= 512) go(std::integral_constant<int, 8>());
        else go(std::integral_constant<int, 16>());
    }
}

}  // namespace

hipError_t run_layer_norm_act_fwd(const float* X, int64_t ldx, int64_t M, int N, const float* gamma,
                                  const float* beta, float eps, int act, float slope, const float* R, int64_t ldr,
                                  float* Y, int64_t ldy, float* mean, float* rstd, const Drop& drop, hipStream_t st) {
    if (M == 0) return hipSuccess;
    const bool v4 = N % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && (R == nullptr || ldr % 4 == 0) && aligned16(X) &&
                    aligned16(Y) && aligned16(R) && aligned16(gamma) && aligned16(beta);
    const int64_t rpw = layer_norm_rows_per_part(M);
    const unsigned blocks = (unsigned)layer_norm_parts(M);
    return norm_dispatch(act, drop, v4, [&](auto a, auto dropped, auto vw, const Drop& d) {
        ln_by_nch<vw()>(N, [&](auto nch) {
            hipLaunchKernelGGL((k_ln_fwd<vw(), nch(), a(), dropped()>), dim3(blocks), dim3(64), 0, st, X, ldx, M, N, rpw,
                               gamma, beta, eps, slope, R, ldr, Y, ldy, mean, rstd, d);
        });
    });
}

hipError_t run_layer_norm_act_bwd(const float* X, int64_t ldx, const float* D, int64_t ldg, int64_t M, int N,
                                  const float* gamma, const float* beta, const float* mean, const float* rstd,
                                  int act, float slope, float* dX, int64_t lddx, float* dw_part, float* db_part,
                                  int64_t ldp, const Drop& drop, hipStream_t st) {
    if (M == 0) return hipSuccess;
    const bool v4 = N % 4 == 0 && ldx % 4 == 0 && ldg % 4 == 0 && lddx % 4 == 0 && ldp % 4 == 0 && aligned16(X) &&
                    aligned16(D) && aligned16(dX) && aligned16(gamma) && aligned16(beta) && aligned16(dw_part) &&
                    aligned16(db_part);
    const int64_t rpw = layer_norm_rows_per_part(M);
    const unsigned blocks = (unsigned)layer_norm_parts(M);
    return norm_dispatch(act, drop, v4, [&](auto a, auto dropped, auto vw, const Drop& d) {
        ln_by_nch<vw()>(N, [&](auto nch) {
            hipLaunchKernelGGL((k_ln_bwd<vw(), nch(), a(), dropped()>), dim3(blocks), dim3(64), 0, st, X, ldx, D, ldg, M,
                               N, rpw, gamma, beta, mean, rstd, slope, dX, lddx, dw_part, db_part, ldp, d);
        });
    });
}

}  // namespace sir

