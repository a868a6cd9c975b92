// sirconv_eedge.hip — gfx950 edge kernels of SIREConv (briangodwinlim/SIR-GCN models/conv.py:70-134):
// the edge-feature term W_E h_{u,v} inside sigma (conv.py:108), fused into the row-CSR edge pass.
//
//   forward  (k_eedge_fwd):   S[v] = sum_{p in row v} c_p * sigma((Q[v] + K[u_p]) + Eh[r(p)])
//   backward (k_eedge_bwd_e): dE[r(p)] = sigma'(z_p) * t_p,  t_p = g[v] (* c_p)
//
// p = the edge's destination-CSR position, r(p) = eidx ? eidx[p] : p (clamped into [0, n_erows)).
// Same work plan, lane shapes, summation order, split-row partials and combine kernel as
// k_edge<MODE_FWD> (sirconv_edge_impl.h); each edge gathers one K row and one Eh row.  The forward
// writes the sign of THIS z in the sir_mask_words layout, so dQ and dK come from the existing
// sign-mask backward passes (they never read Q or K); only the edge term's gradient is new.
// fp32 rows of float4 (H % 4 == 0, 16-B aligned rows), ReLU / LeakyReLU.
#include "sirconv_edge_impl.h"
#include "sirconv_eedge.h"

namespace sir {

// an edge-row id clamped into [0, n): a bad id reads (or writes) a wrong row, never out of bounds
__device__ __forceinline__ int clamp_erow(int r, int n) {
    r = r < n - 1 ? r : n - 1;
    return r > 0 ? r : 0;
}

// ------------------------------------------------------------------------------ forward batch
// UU consecutive edges [e, e+UU) of one row: indices first, then every K and Eh gather, then use.
template <int ACT, int AGG, int LPR, int NV, int UU, bool MASKW>
__device__ __forceinline__ void eedge_batch(int e, const int* __restrict__ col, const int* __restrict__ eidx,
                                            int n_erows, const float* __restrict__ K, int64_t ldk,
                                            const float* __restrict__ Eh, int64_t lde,
                                            const float* __restrict__ norm_col, float nr, float slope,
                                            int li, int HC, const float (&rv)[NV][4], float (&acc)[NV][4],
                                            uint64_t* __restrict__ mask, int lane) {
    static_assert(LPR == 64 || NV == 1, "sub-wave rows hold one float4 per lane");
    // the id load is unconditional (off col when there is no eidx, value unused): a load under the
    // eidx test compiled to one branch and one wait per edge; this form issues the batch's index loads
    // together (no measured change at H = 256, where the pass is bound by its row bytes)
    const bool has_idx = eidx != nullptr;
    const int* __restrict__ ip = has_idx ? eidx : col;
    int u[UU], r[UU];
#pragma unroll
    for (int i = 0; i < UU; ++i) {
        u[i] = col[e + i];
        const int q = ip[e + i];
        r[i] = clamp_erow(has_idx ? q : e + i, n_erows);
        if constexpr (LPR == 64) {      // e is wave-uniform: keep the row bases in SGPRs
            u[i] = __builtin_amdgcn_readfirstlane(u[i]);
            r[i] = __builtin_amdgcn_readfirstlane(r[i]);
        }
    }
    float kv[UU][NV][4], ev[UU][NV][4];
#pragma unroll
    for (int i = 0; i < UU; ++i) {
        const float* kp = K + (int64_t)u[i] * ldk;
        const float* ep = Eh + (int64_t)r[i] * lde;
        if constexpr (LPR == 64) {
            // 16-B buffer loads off the wave-uniform row bases; lanes past the row fail the range
            // check and read 0 (as the plain forward's K gather)
            const gemm::rsrc_t rk = gemm::mk_rsrc(kp, (uint32_t)(HC * 16));
            const gemm::rsrc_t re = gemm::mk_rsrc(ep, (uint32_t)(HC * 16));
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const sir_u4 a = __builtin_amdgcn_raw_buffer_load_b128(rk, (li + LPR * j) * 16, 0, 0);
                const sir_u4 b = __builtin_amdgcn_raw_buffer_load_b128(re, (li + LPR * j) * 16, 0, 0);
                kv[i][j][0] = __uint_as_float(a.x); kv[i][j][1] = __uint_as_float(a.y);
                kv[i][j][2] = __uint_as_float(a.z); kv[i][j][3] = __uint_as_float(a.w);
                ev[i][j][0] = __uint_as_float(b.x); ev[i][j][1] = __uint_as_float(b.y);
                ev[i][j][2] = __uint_as_float(b.z); ev[i][j][3] = __uint_as_float(b.w);
            }
        } else {
            // unconditional (see edge_batch): lanes past the row re-read column 0, values unused
            const int off = (li < HC ? li : 0) * 4;
            vload_gather<ST_F32, 4>(kv[i][0], kp + off);
            vload_gather<ST_F32, 4>(ev[i][0], ep + off);
        }
    }
    float cf[UU];
    if constexpr (AGG == AGG_SYM) {
#pragma unroll
        for (int i = 0; i < UU; ++i) cf[i] = norm_col[u[i]] * nr;       // out_norm[u] * in_norm[v]
    }
    float z[UU][NV][4];
#pragma unroll
    for (int i = 0; i < UU; ++i)
#pragma unroll
        for (int j = 0; j < NV; ++j)
#pragma unroll
            for (int w = 0; w < 4; ++w) z[i][j][w] = (rv[j][w] + kv[i][j][w]) + ev[i][j][w];   // conv.py:108
    if constexpr (MASKW && LPR < 64) {
        // sub-wave record (edge_batch's layout): bit (w * LPR + li) of the edge's MWS uint32 words
        constexpr int MWS = sub_mask_words<LPR, 4>();
        constexpr uint32_t FM = (LPR == 32) ? 0xffffffffu : ((1u << LPR) - 1u);
        const int sh = lane - li;
        uint32_t wd[UU][MWS];
#pragma unroll
        for (int i = 0; i < UU; ++i) {
#pragma unroll
            for (int k = 0; k < MWS; ++k) wd[i][k] = 0u;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const uint64_t b = __builtin_amdgcn_ballot_w64(li < HC && z[i][0][w] > 0.f);
                wd[i][(w * LPR) / 32] |= ((uint32_t)(b >> sh) & FM) << ((w * LPR) % 32);
            }
        }
        uint32_t* mrec = reinterpret_cast<uint32_t*>(mask) + (int64_t)e * MWS;
        constexpr int NWB = UU * MWS;
#pragma unroll
        for (int q0 = 0; q0 < (NWB + LPR - 1) / LPR; ++q0) {
            uint32_t mine = 0u;
#pragma unroll
            for (int i = 0; i < UU; ++i)
#pragma unroll
                for (int k = 0; k < MWS; ++k)
                    if ((i * MWS + k) / LPR == q0) mine = (li == (i * MWS + k) % LPR) ? wd[i][k] : mine;
            const int q = q0 * LPR + li;
            if (q < NWB) mrec[q] = mine;
        }
    } else if constexpr (MASKW) {
        // full-wave words (edge_batch's layout): word (j*4 + w) of edge e, bit lane = z[(lane + 64 j)*4 + w] > 0
        constexpr int NW = NV * 4;
        static_assert(UU * NW <= 64, "one mask store per batch");
        uint32_t mlo = 0, mhi = 0;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const uint64_t okm = __builtin_amdgcn_ballot_w64((li + LPR * j) < HC);
#pragma unroll
            for (int i = 0; i < UU; ++i) {
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const uint64_t b = __builtin_amdgcn_ballot_w64(z[i][j][w] > 0.f) & okm;
                    writelane(mlo, (uint32_t)b, i * NW + j * 4 + w);
                    writelane(mhi, (uint32_t)(b >> 32), i * NW + j * 4 + w);
                }
            }
        }
        const uint64_t mine = ((uint64_t)mhi << 32) | mlo;
        if (lane < UU * NW) mask[(int64_t)e * NW + lane] = mine;
    }
#pragma unroll
    for (int i = 0; i < UU; ++i) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            if (li + LPR * j < HC) {
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    float m = sig<ACT>(z[i][j][w], slope);
                    if constexpr (AGG == AGG_SYM) m = cf[i] * m;
                    acc[j][w] += m;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------ forward kernel
// One wave per item (LPR == 64) or 64 / LPR items per wave; Q[v] in registers; sums in edge order.
template <int ACT, int AGG, int LPR, int NV, int U, bool MASKW>
__global__ void __launch_bounds__(256)
k_eedge_fwd(const int* __restrict__ col, const int* __restrict__ eidx, int n_erows,
            const int4* __restrict__ items, int64_t n_items,
            const float* __restrict__ Q, int64_t ldq, const float* __restrict__ K, int64_t ldk,
            const float* __restrict__ Eh, int64_t lde,
            const float* __restrict__ norm_row, const float* __restrict__ norm_col, float slope, int H,
            float* __restrict__ S, int64_t lds, float* __restrict__ partial, uint64_t* __restrict__ mask) {
    constexpr int RPW = 64 / LPR;
    int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if constexpr (LPR == 64) wave = __builtin_amdgcn_readfirstlane((int)wave);
    const int lane = threadIdx.x & 63;
    const int sub = lane / LPR;
    const int li = lane - sub * LPR;
    const int64_t idx = wave * RPW + sub;
    if (idx >= n_items) return;
    int4 it = items[idx];
    if constexpr (LPR == 64) {
        it.x = __builtin_amdgcn_readfirstlane(it.x);
        it.y = __builtin_amdgcn_readfirstlane(it.y);
        it.z = __builtin_amdgcn_readfirstlane(it.z);
        it.w = __builtin_amdgcn_readfirstlane(it.w);
    }
    const int row = it.x, e0 = it.y, e1 = it.z, slot = it.w;
    const int HC = H / 4;

    float rv[NV][4], acc[NV][4];
    const float* qp = Q + (int64_t)row * ldq;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int c = li + LPR * j;
#pragma unroll
        for (int w = 0; w < 4; ++w) { acc[j][w] = 0.f; rv[j][w] = 0.f; }
        if (c < HC) vload_row<ST_F32, 4>(rv[j], qp + c * 4);
    }
    float nr = 1.f;
    if constexpr (AGG == AGG_SYM) nr = norm_row[row];

    int e = e0;
    for (; e + U <= e1; e += U)
        eedge_batch<ACT, AGG, LPR, NV, U, MASKW>(e, col, eidx, n_erows, K, ldk, Eh, lde, norm_col, nr, slope, li, HC,
                                                 rv, acc, mask, lane);
    if constexpr (U > 2) {
        if (e + 2 <= e1) {
            eedge_batch<ACT, AGG, LPR, NV, 2, MASKW>(e, col, eidx, n_erows, K, ldk, Eh, lde, norm_col, nr, slope, li, HC,
                                                     rv, acc, mask, lane);
            e += 2;
        }
    }
    if (e < e1)
        eedge_batch<ACT, AGG, LPR, NV, 1, MASKW>(e, col, eidx, n_erows, K, ldk, Eh, lde, norm_col, nr, slope, li, HC,
                                                 rv, acc, mask, lane);

    if (slot < 0) {
        if constexpr (AGG == AGG_MEAN) {
            const int d = e1 - e0;                      // unsplit: the whole row
            const float degf = (float)(d > 1 ? d : 1);
#pragma unroll
            for (int j = 0; j < NV; ++j)
#pragma unroll
                for (int w = 0; w < 4; ++w) acc[j][w] = acc[j][w] / degf;
        }
        float* op = S + (int64_t)row * lds;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = li + LPR * j;
            if (c < HC) vstore_row<ST_F32, 4>(op + c * 4, acc[j]);
        }
    } else {
        float* pp = partial + (int64_t)slot * H;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = li + LPR * j;
            if (c < HC) vstore<4>(pp + c * 4, acc[j]);
        }
    }
}

// ------------------------------------------------------------------------------ edge-term backward
// dE[r(p)] = bit_p ? t : (ReLU ? 0 : t * slope) for every edge position p of the item's row v, with
// t = g[v] (SUM) or g[v] * (norm_col[u] * norm_row[v]) (SYM); g[v] stays in registers.  Per-edge
// outputs: no partial rows, no combine.
template <int ACT, int AGG, int LPR, int NV>
__global__ void __launch_bounds__(256)
k_eedge_bwd_e(const int* __restrict__ col, const int* __restrict__ eidx, int n_erows,
              const int4* __restrict__ items, int64_t n_items, const uint64_t* __restrict__ mask,
              const float* __restrict__ G, int64_t ldg,
              const float* __restrict__ norm_row, const float* __restrict__ norm_col, float slope, int H,
              float* __restrict__ dE, int64_t ldde) {
    static_assert(LPR == 64 || NV == 1, "sub-wave rows hold one float4 per lane");
    constexpr int RPW = 64 / LPR;
    int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if constexpr (LPR == 64) wave = __builtin_amdgcn_readfirstlane((int)wave);
    const int lane = threadIdx.x & 63;
    const int sub = lane / LPR;
    const int li = lane - sub * LPR;
    const int64_t idx = wave * RPW + sub;
    if (idx >= n_items) return;
    int4 it = items[idx];
    if constexpr (LPR == 64) {
        it.x = __builtin_amdgcn_readfirstlane(it.x);
        it.y = __builtin_amdgcn_readfirstlane(it.y);
        it.z = __builtin_amdgcn_readfirstlane(it.z);
    }
    const int row = it.x, e0 = it.y, e1 = it.z;
    const int HC = H / 4;

    float gv[NV][4];
    const float* gp = G + (int64_t)row * ldg;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int c = li + LPR * j;
#pragma unroll
        for (int w = 0; w < 4; ++w) gv[j][w] = 0.f;
        if (c < HC) vload_row<ST_F32, 4>(gv[j], gp + c * 4);
    }
    float nr = 1.f;
    if constexpr (AGG == AGG_SYM) nr = norm_row[row];

    const bool has_idx = eidx != nullptr;
    const int* __restrict__ ip = has_idx ? eidx : col;      // unconditional id load (see eedge_batch)
    for (int p = e0; p < e1; ++p) {
        const int q = ip[p];
        int r = clamp_erow(has_idx ? q : p, n_erows);
        if constexpr (LPR == 64) r = __builtin_amdgcn_readfirstlane(r);
        float cf = 1.f;
        if constexpr (AGG == AGG_SYM) cf = norm_col[col[p]] * nr;
        float* op = dE + (int64_t)r * ldde;
        if constexpr (LPR == 64) {
            constexpr int NW = NV * 4;
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                float o[4];
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const uint64_t wd = uniform64(mask[(int64_t)p * NW + j * 4 + w]);
                    float t = gv[j][w];
                    if constexpr (AGG == AGG_SYM) t = t * cf;
                    o[w] = sel_mask<ACT>(wd, t, slope);
                }
                const int c = li + LPR * j;
                if (c < HC) vstore_row<ST_F32, 4>(op + c * 4, o);
            }
        } else {
            constexpr int MWS = sub_mask_words<LPR, 4>();
            static_assert(MWS == 2 || MWS == 4, "sub-wave records are 8 or 16 bytes");
            const uint32_t* rp = reinterpret_cast<const uint32_t*>(mask) + (int64_t)p * MWS;
            uint32_t mr[MWS];
            if constexpr (MWS == 4) {
                const sir_u4 t4 = *reinterpret_cast<const sir_u4*>(rp);
                mr[0] = t4.x; mr[1] = t4.y; mr[2] = t4.z; mr[3] = t4.w;
            } else {
                const sir_u2 t2 = *reinterpret_cast<const sir_u2*>(rp);
                mr[0] = t2.x; mr[1] = t2.y;
            }
            float o[4];
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                float t = gv[0][w];
                if constexpr (AGG == AGG_SYM) t = t * cf;
                const bool pos = (mr[(w * LPR) / 32] >> (((w * LPR) % 32) + li)) & 1u;
                o[w] = pos ? t : (ACT == ACT_RELU ? 0.f : t * slope);
            }
            if (li < HC) vstore_row<ST_F32, 4>(op + li * 4, o);
        }
    }
}

// ------------------------------------------------------------------------------ launch
namespace {

// lanes per row / float4 vectors per lane of an H % 4 == 0 row (the shapes pick_shape gives vw = 4 rows)
bool eshape(int H, int* lpr, int* nv) {
    if (H <= 0 || H % 4 != 0 || H > 1024) return false;
    const int hc = H / 4;
    *nv = 1;
    if (hc <= 4) *lpr = 4;
    else if (hc <= 8) *lpr = 8;
    else if (hc <= 16) *lpr = 16;
    else if (hc <= 32) *lpr = 32;
    else { *lpr = 64; *nv = (hc + 63) / 64; }
    return true;
}


template <int ACT, int AGG, int LPR, int NV>
hipError_t launch_fwd_t(const EEdgeArgs& a, hipStream_t st) {
    constexpr int U = (NV == 1) ? 4 : 2;            // two gathered rows per edge: half the plain forward's edges in flight
    constexpr int RPW = 64 / LPR;
    const int64_t waves = (a.n_items + RPW - 1) / RPW;
    const int64_t blocks = (waves + 3) / 4;
    if (blocks == 0) return hipSuccess;
#define SIR_EEDGE_FWD(MW)                                                                                          \
    hipLaunchKernelGGL((k_eedge_fwd<ACT, AGG, LPR, NV, U, MW>), dim3((unsigned)blocks), dim3(256), 0, st, a.col,   \
                       a.eidx, (int)a.n_erows, reinterpret_cast<const int4*>(a.items), a.n_items, a.Q, a.ldq, a.K, \
                       a.ldk, a.Eh, a.lde, a.norm_row, a.norm_col, a.slope, a.H, a.S, a.lds, a.partial, a.mask_out)
    if (a.mask_out != nullptr) SIR_EEDGE_FWD(true);
    else SIR_EEDGE_FWD(false);
#undef SIR_EEDGE_FWD
    return hipGetLastError();
}

template <int ACT, int AGG, int LPR, int NV>
hipError_t launch_bwd_t(const EEdgeArgs& a, hipStream_t st) {
    constexpr int RPW = 64 / LPR;
    const int64_t waves = (a.n_items + RPW - 1) / RPW;
    const int64_t blocks = (waves + 3) / 4;
    if (blocks == 0) return hipSuccess;
    static_assert(AGG != AGG_MEAN, "MEAN: the caller divides G and passes SUM");
    hipLaunchKernelGGL((k_eedge_bwd_e<ACT, AGG, LPR, NV>), dim3((unsigned)blocks), dim3(256), 0, st, a.col, a.eidx,
                       (int)a.n_erows, reinterpret_cast<const int4*>(a.items), a.n_items, a.mask_in, a.G, a.ldg,
                       a.norm_row, a.norm_col, a.slope, a.H, a.dE, a.ldde);
    return hipGetLastError();
}

template <bool FWD, int ACT, int AGG, int LPR, int NV>
hipError_t launch_t(const EEdgeArgs& a, hipStream_t st) {
    if constexpr (FWD) return launch_fwd_t<ACT, AGG, LPR, NV>(a, st);
    else return launch_bwd_t<ACT, AGG, LPR, NV>(a, st);
}

template <bool FWD, int ACT, int AGG>
hipError_t launch_shape(const EEdgeArgs& a, int lpr, int nv, hipStream_t st) {
    switch (lpr) {
        case 4: return launch_t<FWD, ACT, AGG, 4, 1>(a, st);
        case 8: return launch_t<FWD, ACT, AGG, 8, 1>(a, st);
        case 16: return launch_t<FWD, ACT, AGG, 16, 1>(a, st);
        case 32: return launch_t<FWD, ACT, AGG, 32, 1>(a, st);
        default: break;
    }
    switch (nv) {
        case 1: return launch_t<FWD, ACT, AGG, 64, 1>(a, st);
        case 2: return launch_t<FWD, ACT, AGG, 64, 2>(a, st);
        case 3: return launch_t<FWD, ACT, AGG, 64, 3>(a, st);
        default: return launch_t<FWD, ACT, AGG, 64, 4>(a, st);
    }
}

template <bool FWD, int ACT>
hipError_t launch_agg(const EEdgeArgs& a, int agg, int lpr, int nv, hipStream_t st) {
    switch (agg) {
        case AGG_SUM: return launch_shape<FWD, ACT, AGG_SUM>(a, lpr, nv, st);
        case AGG_SYM: return launch_shape<FWD, ACT, AGG_SYM>(a, lpr, nv, st);
        default:
            if constexpr (FWD) return launch_shape<FWD, ACT, AGG_MEAN>(a, lpr, nv, st);
            else return hipErrorInvalidValue;
    }
}

template <bool FWD>
hipError_t launch_act(const EEdgeArgs& a, int agg, int act, int lpr, int nv, hipStream_t st) {
    if (act == ACT_RELU) return launch_agg<FWD, ACT_RELU>(a, agg, lpr, nv, st);
    if (act == ACT_LEAKY) return launch_agg<FWD, ACT_LEAKY>(a, agg, lpr, nv, st);
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t run_eedge_fwd(const EEdgeArgs& a, int agg, int act, hipStream_t st, const char** why) {
    int lpr = 0, nv = 0;
    if (!eshape(a.H, &lpr, &nv)) {
        *why = "the edge-term forward needs H % 4 == 0 and 4 <= H <= 1024";
        return hipErrorInvalidValue;
    }
    if (!(aligned16(a.Q) && aligned16(a.K) && aligned16(a.Eh) && aligned16(a.S) && aligned16(a.partial) &&
          a.ldq % 4 == 0 && a.ldk % 4 == 0 && a.lde % 4 == 0 && a.lds % 4 == 0)) {
        *why = "the edge-term forward needs 16-B aligned rows (aligned pointers, leading dimensions multiples of 4)";
        return hipErrorInvalidValue;
    }
    hipError_t err = launch_act<true>(a, agg, act, lpr, nv, st);
    if (err == hipErrorInvalidValue) *why = "the edge-term forward covers SUM / MEAN / SYM with ReLU / LeakyReLU";
    if (err != hipSuccess || a.n_splits == 0) return err;
    // split rows: the partial rows are added in slot order by the plain forward's combine kernel
    const int4* sp = reinterpret_cast<const int4*>(a.splits);
    if (agg == AGG_MEAN)
        hipLaunchKernelGGL((k_combine<ST_F32, true, 4>), dim3((unsigned)a.n_splits), dim3(1024), 0, st, sp, a.partial,
                           a.H, a.S, a.lds, Drop(), 0);
    else
        hipLaunchKernelGGL((k_combine<ST_F32, false, 4>), dim3((unsigned)a.n_splits), dim3(1024), 0, st, sp, a.partial,
                           a.H, a.S, a.lds, Drop(), 0);
    return hipGetLastError();
}

hipError_t run_eedge_bwd_e(const EEdgeArgs& a, int agg, int act, hipStream_t st, const char** why) {
    int lpr = 0, nv = 0;
    if (!eshape(a.H, &lpr, &nv)) {
        *why = "the edge-term backward needs H % 4 == 0 and 4 <= H <= 1024";
        return hipErrorInvalidValue;
    }
    if (!(aligned16(a.G) && aligned16(a.dE) && a.ldg % 4 == 0 && a.ldde % 4 == 0)) {
        *why = "the edge-term backward needs 16-B aligned rows (aligned pointers, leading dimensions multiples of 4)";
        return hipErrorInvalidValue;
    }
    hipError_t err = launch_act<false>(a, agg, act, lpr, nv, st);
    if (err == hipErrorInvalidValue) *why = "the edge-term backward covers SUM / SYM with ReLU / LeakyReLU";
    return err;
}

}  // namespace sir
