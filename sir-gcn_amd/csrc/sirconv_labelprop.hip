// sirconv_labelprop.hip — one propagation step of Correct & Smooth's label spreading
// (ogbn-arxiv/correct_and_smooth.py:41-58: update_all(copy_u('y', 'm'), sum | mean) between two norm
// multiplies, the alpha / (1 - alpha) mix with y0 and the post step) in one launch.
//
// For destination row v, in-edges in CSR order (ascending edge id):
//   s[v]   = sum_e (SYM ? Y[u] * norm[u] : Y[u])            added one after another, starting from 0
//   p[v]   = SYM ? s[v] * norm[v] : MEAN ? s[v] / max(deg v, 1) : s[v]
//   out[v] = alpha * p[v] + beta * Y0[v]                    two rounded products, one add (no FMA: the
//                                                           library is built with -ffp-contract=off)
//   post   : NONE | CLAMP (torch.clamp: NaN stays) | FIX (fixed[v] ? Yfix[v] : out[v])
// A row of one work item (at most the plan's chunk of edges) is therefore the reference's CPU result bit
// for bit.  Longer rows leave one partial sum per item in `partial`; a second small launch adds them in
// slot order and runs the same epilogue.  A fixed row (FIX) is never gathered: its unsplit item copies
// Yfix, its split items return at once and the combine copies Yfix without reading the slots.
//
// Layout: the rows are narrow (40 classes on ogbn-arxiv), so a wave carries several: L lanes per work
// item, L the smallest of 4..64 that holds the row's columns (float4 columns when every row is 16-B
// aligned, single floats otherwise), 64 / L items per wave; rows wider than 64 lanes' worth are cut into
// column tiles (blockIdx.y).  Each lane owns its columns and walks the item's edges in order, LP_U edges'
// index and row loads in flight at a time; the adds stay in edge order.  No atomics, no cross-lane traffic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sirconv.h"
#include "sirconv_internal.h"

namespace sir {
namespace {

constexpr int LP_U = 8;           // edges in flight per lane

template <int VW>
__device__ __forceinline__ void lp_ld(float (&d)[VW], const float* __restrict__ p) {
    if constexpr (VW == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        d[0] = t.x; d[1] = t.y; d[2] = t.z; d[3] = t.w;
    } else {
        d[0] = p[0];
    }
}

template <int VW>
__device__ __forceinline__ void lp_st(float* __restrict__ p, const float (&s)[VW]) {
    if constexpr (VW == 4) *reinterpret_cast<float4*>(p) = make_float4(s[0], s[1], s[2], s[3]);
    else p[0] = s[0];
}

// the row-wise epilogue of one element: s the row's sum, y0 the element of Y0
__device__ __forceinline__ float lp_epilogue(float s, float y0, int agg, float nv, float degf, float alpha,
                                             float beta, int post, float lo, float hi) {
    float p = s;
    if (agg == SIR_AGG_SYM) p = s * nv;
    else if (agg == SIR_AGG_MEAN) p = s / degf;                 // IEEE division (fn.mean)
    const float a = alpha * p;
    const float b = beta * y0;
    float o = a + b;
    if (post == SIR_LP_POST_CLAMP) {                            // comparisons: a NaN passes through
        o = o < lo ? lo : o;
        o = o > hi ? hi : o;
    }
    return o;
}

// L lanes per work item, 256 / L items per block; blockIdx.y = column tile of L * VW columns
template <int L, int VW, bool SYM>
__global__ void __launch_bounds__(256)
k_label_prop(LabelPropArgs a) {
    const int64_t g = ((int64_t)blockIdx.x * 256 + threadIdx.x) / L;
    if (g >= a.n_items) return;
    const int c0 = ((int)blockIdx.y * L + (int)(threadIdx.x % L)) * VW;     // first column of this lane
    if (c0 >= a.F) return;
    const int4 it = reinterpret_cast<const int4*>(a.items)[g];
    const int row = it.x, e0 = it.y, e1 = it.z, slot = it.w;
    if (row < 0 || row >= a.V) return;                          // a malformed plan writes nothing
    if (a.post == SIR_LP_POST_FIX && a.fixed[row] != 0) {
        if (slot < 0) {
            float f[VW];
            lp_ld<VW>(f, a.Yfix + (int64_t)row * a.ldf + c0);
            lp_st<VW>(a.out + (int64_t)row * a.ldo + c0, f);
        }
        return;
    }
    const int* __restrict__ col = a.col;
    const float* __restrict__ Y = a.Y + c0;
    const float* __restrict__ norm = a.norm;
    float acc[VW];
#pragma unroll
    for (int x = 0; x < VW; ++x) acc[x] = 0.f;
    int e = e0;
    for (; e + LP_U <= e1; e += LP_U) {
        int u[LP_U];
        float v[LP_U][VW], nu[LP_U];
#pragma unroll
        for (int k = 0; k < LP_U; ++k) u[k] = col[e + k];
#pragma unroll
        for (int k = 0; k < LP_U; ++k) {
            lp_ld<VW>(v[k], Y + (int64_t)u[k] * a.ldy);
            nu[k] = SYM ? norm[u[k]] : 1.f;
        }
#pragma unroll
        for (int k = 0; k < LP_U; ++k)
#pragma unroll
            for (int x = 0; x < VW; ++x) acc[x] += SYM ? v[k][x] * nu[k] : v[k][x];
    }
    if (e < e1) {
        const int n = e1 - e;
        int u[LP_U];
        float v[LP_U][VW], nu[LP_U];
#pragma unroll
        for (int k = 0; k < LP_U; ++k) u[k] = col[e + (k < n ? k : 0)];
#pragma unroll
        for (int k = 0; k < LP_U; ++k) {
            lp_ld<VW>(v[k], Y + (int64_t)u[k] * a.ldy);
            nu[k] = SYM ? norm[u[k]] : 1.f;
        }
#pragma unroll
        for (int k = 0; k < LP_U; ++k)
            if (k < n) {
#pragma unroll
                for (int x = 0; x < VW; ++x) acc[x] += SYM ? v[k][x] * nu[k] : v[k][x];
            }
    }
    if (slot >= 0) {                                            // a split row: the combine finishes it
        lp_st<VW>(a.partial + (int64_t)slot * a.F + c0, acc);
        return;
    }
    const int d = e1 - e0;
    const float degf = (float)(d > 1 ? d : 1);
    const float nv = SYM ? norm[row] : 1.f;
    float y0[VW], o[VW];
    lp_ld<VW>(y0, a.Y0 + (int64_t)row * a.ldy0 + c0);
#pragma unroll
    for (int x = 0; x < VW; ++x)
        o[x] = lp_epilogue(acc[x], y0[x], a.agg, nv, degf, a.alpha, a.beta, a.post, a.lo, a.hi);
    lp_st<VW>(a.out + (int64_t)row * a.ldo + c0, o);
}

// split rows: the slot partials in slot order, then the epilogue; one block per split row
__global__ void __launch_bounds__(256)
k_label_prop_combine(LabelPropArgs a) {
    const int4 sp = reinterpret_cast<const int4*>(a.splits)[blockIdx.x];
    const int row = sp.x;
    if (row < 0 || row >= a.V) return;
    const bool fix = a.post == SIR_LP_POST_FIX && a.fixed[row] != 0;
    const float degf = (float)(sp.w > 1 ? sp.w : 1);
    const float nv = a.agg == SIR_AGG_SYM ? a.norm[row] : 1.f;
    for (int c = threadIdx.x; c < a.F; c += 256) {
        float o;
        if (fix) {
            o = a.Yfix[(int64_t)row * a.ldf + c];
        } else {
            float acc = 0.f;
            for (int k = 0; k < sp.z; ++k) acc += a.partial[(int64_t)(sp.y + k) * a.F + c];
            o = lp_epilogue(acc, a.Y0[(int64_t)row * a.ldy0 + c], a.agg, nv, degf, a.alpha, a.beta, a.post, a.lo,
                            a.hi);
        }
        a.out[(int64_t)row * a.ldo + c] = o;
    }
}


template <int L, int VW>
void lp_launch(const LabelPropArgs& a, dim3 grid, hipStream_t st) {
    if (a.agg == SIR_AGG_SYM) hipLaunchKernelGGL((k_label_prop<L, VW, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_label_prop<L, VW, false>), grid, dim3(256), 0, st, a);
}

template <int VW>
hipError_t lp_dispatch(const LabelPropArgs& a, hipStream_t st) {
    const int cols = a.F / VW;                                  // VW == 4 only when F % 4 == 0
    int L = 4;
    while (L < 64 && L < cols) L *= 2;
    const int tiles = (cols + L - 1) / L;                       // > 1 only at L = 64
    const int64_t per_block = 256 / L;
    const int64_t blocks = (a.n_items + per_block - 1) / per_block;
    if (blocks > 0x7fffffffLL || tiles > 65535) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks, (unsigned)tiles);
    switch (L) {
        case 4: lp_launch<4, VW>(a, grid, st); break;
        case 8: lp_launch<8, VW>(a, grid, st); break;
        case 16: lp_launch<16, VW>(a, grid, st); break;
        case 32: lp_launch<32, VW>(a, grid, st); break;
        default: lp_launch<64, VW>(a, grid, st); break;
    }
    return hipGetLastError();
}

}  // namespace

hipError_t run_label_prop(const LabelPropArgs& a, hipStream_t st) {
    if (a.V == 0 || a.n_items == 0) return hipSuccess;
    const bool v4 = a.F % 4 == 0 && a.ldy % 4 == 0 && a.ldy0 % 4 == 0 && a.ldo % 4 == 0 &&
                    (a.post != SIR_LP_POST_FIX || a.ldf % 4 == 0) && aligned16(a.Y) && aligned16(a.Y0) &&
                    aligned16(a.out) && aligned16(a.partial) && (a.post != SIR_LP_POST_FIX || aligned16(a.Yfix));
    hipError_t err = v4 ? lp_dispatch<4>(a, st) : lp_dispatch<1>(a, st);
    if (err != hipSuccess || a.n_splits == 0) return err;
    hipLaunchKernelGGL(k_label_prop_combine, dim3((unsigned)a.n_splits), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace sir
