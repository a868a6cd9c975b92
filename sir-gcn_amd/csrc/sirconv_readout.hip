// sirconv_readout.hip — graph readout on a batched graph: dgl.nn.SumPooling / AvgPooling / MaxPooling
// (ogbg-molhiv/model.py:69,85, zinc/model.py:41, super-pixel/model.py:28, hetero-edge-count/model.py:23,33)
// and dgl.broadcast_nodes, their backward.
//
// Nodes of graph b are rows [off[b], off[b+1]) (off = int64 [B+1], as for GraphNorm).
//   forward : P[b, c] = reduce over the graph's rows of X[v, c], reduce = sum / mean / max
//   backward: dX[v, c] = dP[b(v), c]  (sum),  dP[b(v), c] / n_b  (mean),
//             arg[b, c] == v - off[b] ? dP[b, c] : 0  (max)
// Sums are fp32 in node order; the maximum takes a later row only on a strict >, so the lowest node id wins
// a tie; an empty graph gives 0 (and arg -1).  No atomics.
//
// Work partition (both directions): slab slots.  A graph is cut into POOL_R-row slabs counted from its own
// first row; graph b owns the slots [b + off[b] / R, b + 1 + off[b+1] / R) — at least 1 + n_b / R of them, so
// enough for its ceil(n_b / R) slabs (an empty graph keeps one slot, which writes its zeros), B + V / R in
// all; the surplus slots idle.  One wave per (slot, 64-lane column chunk): it finds its graph by a 64-ary
// search over `off` (one load round for B <= 64), so the host never reads `off`.  A one-slab graph (the
// workload: molecules, super-pixels) is reduced and written by its wave; a longer graph's waves leave
// their slab partial (value and, for max, arg) in `work`, and a second launch combines them in slab
// order.  The partition is a function of (off, F) alone: results are bit-identical run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sirconv.h"
#include "sirconv_internal.h"
#include "sirconv_device.h"

namespace sir {
namespace {

constexpr int POOL_R = SIR_POOL_SLAB_ROWS;

template <int VW>
__device__ __forceinline__ void pst_i(int* __restrict__ p, const int (&s)[VW]) {
    if constexpr (VW == 4) *reinterpret_cast<int4*>(p) = make_int4(s[0], s[1], s[2], s[3]);
    else p[0] = s[0];
}

// Rows [r0, r1) in node order, RB rows' loads in flight at a time (sirconv_graphnorm.hip walk_rows, for
// any storage type); f(i, v) is applied in row order.
template <int DT, int VW, int RB = 32, typename Fn>
__device__ __forceinline__ void pool_walk(int64_t r0, int64_t r1, const typename Stor<DT>::T* __restrict__ base,
                                          int64_t ld, int c, Fn f) {
    int64_t i = r0;
    for (; i + RB <= r1; i += RB) {
        float v[RB][VW];
#pragma unroll
        for (int k = 0; k < RB; ++k) tload_p<DT, VW>(v[k], base + (i + k) * ld + c * VW);
#pragma unroll
        for (int k = 0; k < RB; ++k) f(i + k, v[k]);
    }
    if (i < r1) {
        const int n = (int)(r1 - i);
        float v[RB][VW];
#pragma unroll
        for (int k = 0; k < RB; ++k) tload_p<DT, VW>(v[k], base + (i + (k < n ? k : 0)) * ld + c * VW);
#pragma unroll
        for (int k = 0; k < RB; ++k)
            if (k < n) f(i + k, v[k]);
    }
}

// The graph of slab slot t: the largest b in [0, B) with b + off[b] / R <= t (the slot bases are strictly
// increasing in b).  64-ary search, every lane of the wave active: lane l probes lo + (l + 1) step.
__device__ __forceinline__ int64_t slot_graph(const int64_t* __restrict__ off, int64_t B, int64_t t) {
    const int lane = threadIdx.x & 63;
    int64_t lo = 0, hi = B;
    while (hi - lo > 1) {
        const int64_t step = (hi - lo + 63) / 64;
        const int64_t cand = lo + (lane + 1) * step;
        const bool ok = cand < hi && cand + off[cand] / POOL_R <= t;
        const int cnt = __popcll(__ballot(ok));
        lo += cnt * step;
        hi = (lo + step < hi) ? lo + step : hi;
    }
    return lo;
}

struct Slab {
    int64_t b, g0, r0, r1, n;     // graph, its first row, the slab's rows [r0, r1), the graph's row count
    int64_t j, nslab;             // slab index, slabs of the graph (an empty graph: 1)
};

// rows clamped to [0, V]: a malformed `off` cannot send an access out of the feature matrix
__device__ __forceinline__ Slab find_slab(const int64_t* __restrict__ off, int64_t B, int64_t V, int64_t t) {
    Slab s;
    s.b = slot_graph(off, B, t);
    int64_t a = off[s.b], e = off[s.b + 1];
    a = a < 0 ? 0 : (a > V ? V : a);
    e = e < a ? a : (e > V ? V : e);
    s.g0 = a;
    s.n = e - a;
    s.nslab = s.n > 0 ? (s.n + POOL_R - 1) / POOL_R : 1;
    s.j = t - (s.b + a / POOL_R);
    s.r0 = a + s.j * POOL_R;
    s.r1 = s.r0 + POOL_R < e ? s.r0 + POOL_R : e;
    return s;
}

// one wave per (slab slot, column chunk); work: [slots, F] fp32 partial values, then [slots, F] int32 args (max)
template <int DT, int VW, int OP>
__global__ void __launch_bounds__(64)
k_pool_fwd(const int64_t* __restrict__ off, int64_t B, int64_t V, int F, int n_cc, int64_t slots,
           const void* __restrict__ Xv, int64_t ldx, void* __restrict__ Pv, int64_t ldp, int* __restrict__ arg,
           float* __restrict__ work) {
    typedef typename Stor<DT>::T T;
    const T* __restrict__ X = static_cast<const T*>(Xv);
    T* __restrict__ P = static_cast<T*>(Pv);
    const int64_t t = (int64_t)blockIdx.x / n_cc;
    const int cc = (int)((int64_t)blockIdx.x - t * n_cc);
    if (t >= slots) return;
    const Slab s = find_slab(off, B, V, t);
    if (s.j >= s.nslab) return;                           // a surplus slot
    const int c = cc * 64 + (threadIdx.x & 63);           // in units of VW elements
    if (c * VW >= F) return;
    float acc[VW];
    int am[VW];
#pragma unroll
    for (int x = 0; x < VW; ++x) { acc[x] = 0.f; am[x] = -1; }
    if constexpr (OP == SIR_POOL_MAX) {
        // the slab's first row seeds (value, arg) whatever it holds — no "nothing seen yet" test in the walk —
        // and a later row replaces it in the maximum's order (max_beats: strict, so the first wins)
        if (s.r0 < s.r1) {
            tload_p<DT, VW>(acc, X + s.r0 * ldx + c * VW);
#pragma unroll
            for (int x = 0; x < VW; ++x) am[x] = (int)(s.r0 - s.g0);
        }
        pool_walk<DT, VW>(s.r0 + 1, s.r1, X, ldx, c, [&](int64_t i, const float (&v)[VW]) {
#pragma unroll
            for (int x = 0; x < VW; ++x)
                if (max_beats(v[x], acc[x])) { acc[x] = v[x]; am[x] = (int)(i - s.g0); }
        });
    } else {
        pool_walk<DT, VW>(s.r0, s.r1, X, ldx, c, [&](int64_t, const float (&v)[VW]) {
#pragma unroll
            for (int x = 0; x < VW; ++x) acc[x] += v[x];
        });
    }
    if (s.nslab == 1) {
        if constexpr (OP == SIR_POOL_MEAN) {
            const float nf = (float)(s.n > 1 ? s.n : 1);
#pragma unroll
            for (int x = 0; x < VW; ++x) acc[x] = acc[x] / nf;
        }
        tstore_p<DT, VW>(P + s.b * ldp + c * VW, acc);
        if constexpr (OP == SIR_POOL_MAX) pst_i<VW>(arg + s.b * F + c * VW, am);
    } else {
#pragma unroll
        for (int x = 0; x < VW; ++x) work[t * F + c * VW + x] = acc[x];
        if constexpr (OP == SIR_POOL_MAX) {
            int* __restrict__ warg = reinterpret_cast<int*>(work + slots * F);
#pragma unroll
            for (int x = 0; x < VW; ++x) warg[t * F + c * VW + x] = am[x];
        }
    }
}

// graphs of more than one slab: the slab partials in slab order, one thread per (graph, column)
template <int DT, int OP>
__global__ void __launch_bounds__(256)
k_pool_combine(const int64_t* __restrict__ off, int64_t B, int64_t V, int F, int64_t slots,
               const float* __restrict__ work, void* __restrict__ Pv, int64_t ldp, int* __restrict__ arg) {
    typedef typename Stor<DT>::T T;
    T* __restrict__ P = static_cast<T*>(Pv);
    const int* __restrict__ warg = reinterpret_cast<const int*>(work + slots * F);
    const int64_t total = B * F;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
        const int64_t b = q / F;
        const int c = (int)(q - b * F);
        int64_t a = off[b], e = off[b + 1];
        a = a < 0 ? 0 : (a > V ? V : a);
        e = e < a ? a : (e > V ? V : e);
        const int64_t n = e - a;
        if (n <= POOL_R) continue;                        // written by its forward wave
        const int64_t nslab = (n + POOL_R - 1) / POOL_R;
        const int64_t t0 = b + a / POOL_R;
        float acc = work[t0 * F + c];
        int am = 0;
        if constexpr (OP == SIR_POOL_MAX) am = warg[t0 * F + c];
        for (int64_t j = 1; j < nslab; ++j) {
            const float v = work[(t0 + j) * F + c];
            if constexpr (OP == SIR_POOL_MAX) {
                if (max_beats(v, acc)) { acc = v; am = warg[(t0 + j) * F + c]; }
            } else {
                acc += v;
            }
        }
        if constexpr (OP == SIR_POOL_MEAN) acc = acc / (float)n;
        P[b * ldp + c] = (T)acc;
        if constexpr (OP == SIR_POOL_MAX) arg[b * F + c] = am;
    }
}

// one wave per (slab slot, column chunk): the slab's rows of dX
template <int DT, int VW, int OP>
__global__ void __launch_bounds__(64)
k_pool_bwd(const int64_t* __restrict__ off, int64_t B, int64_t V, int F, int n_cc, int64_t slots,
           const void* __restrict__ dPv, int64_t ldg, const int* __restrict__ arg, void* __restrict__ dXv,
           int64_t lddx) {
    typedef typename Stor<DT>::T T;
    const T* __restrict__ dP = static_cast<const T*>(dPv);
    T* __restrict__ dX = static_cast<T*>(dXv);
    const int64_t t = (int64_t)blockIdx.x / n_cc;
    const int cc = (int)((int64_t)blockIdx.x - t * n_cc);
    if (t >= slots) return;
    const Slab s = find_slab(off, B, V, t);
    if (s.r0 >= s.r1) return;                             // a surplus slot, or an empty graph
    const int c = cc * 64 + (threadIdx.x & 63);
    if (c * VW >= F) return;
    float g[VW];
    tload_p<DT, VW>(g, dP + s.b * ldg + c * VW);
    if constexpr (OP == SIR_POOL_MAX) {
        int am[VW];
        if constexpr (VW == 4) {
            const int4 q = *reinterpret_cast<const int4*>(arg + s.b * F + c * VW);
            am[0] = q.x; am[1] = q.y; am[2] = q.z; am[3] = q.w;
        } else {
            am[0] = arg[s.b * F + c];
        }
        for (int64_t i = s.r0; i < s.r1; ++i) {
            const int rel = (int)(i - s.g0);
            float o[VW];
#pragma unroll
            for (int x = 0; x < VW; ++x) o[x] = am[x] == rel ? g[x] : 0.f;
            tstore_p<DT, VW>(dX + i * lddx + c * VW, o);
        }
    } else {
        if constexpr (OP == SIR_POOL_MEAN) {
            const float nf = (float)s.n;
#pragma unroll
            for (int x = 0; x < VW; ++x) g[x] = g[x] / nf;
        }
        for (int64_t i = s.r0; i < s.r1; ++i) tstore_p<DT, VW>(dX + i * lddx + c * VW, g);
    }
}

template <int DT, int VW>
void launch_fwd(int op, unsigned blocks, hipStream_t st, const int64_t* off, int64_t B, int64_t V, int F, int n_cc,
                int64_t slots, const void* X, int64_t ldx, void* P, int64_t ldp, int* arg, float* work) {
    if (op == SIR_POOL_SUM)
        hipLaunchKernelGGL((k_pool_fwd<DT, VW, SIR_POOL_SUM>), dim3(blocks), dim3(64), 0, st, off, B, V, F, n_cc, slots,
                           X, ldx, P, ldp, arg, work);
    else if (op == SIR_POOL_MEAN)
        hipLaunchKernelGGL((k_pool_fwd<DT, VW, SIR_POOL_MEAN>), dim3(blocks), dim3(64), 0, st, off, B, V, F, n_cc, slots,
                           X, ldx, P, ldp, arg, work);
    else
        hipLaunchKernelGGL((k_pool_fwd<DT, VW, SIR_POOL_MAX>), dim3(blocks), dim3(64), 0, st, off, B, V, F, n_cc, slots,
                           X, ldx, P, ldp, arg, work);
}

template <int DT>
void launch_combine(int op, unsigned blocks, hipStream_t st, const int64_t* off, int64_t B, int64_t V, int F,
                    int64_t slots, const float* work, void* P, int64_t ldp, int* arg) {
    if (op == SIR_POOL_SUM)
        hipLaunchKernelGGL((k_pool_combine<DT, SIR_POOL_SUM>), dim3(blocks), dim3(256), 0, st, off, B, V, F, slots, work,
                           P, ldp, arg);
    else if (op == SIR_POOL_MEAN)
        hipLaunchKernelGGL((k_pool_combine<DT, SIR_POOL_MEAN>), dim3(blocks), dim3(256), 0, st, off, B, V, F, slots, work,
                           P, ldp, arg);
    else
        hipLaunchKernelGGL((k_pool_combine<DT, SIR_POOL_MAX>), dim3(blocks), dim3(256), 0, st, off, B, V, F, slots, work,
                           P, ldp, arg);
}

template <int DT, int VW>
void launch_bwd(int op, unsigned blocks, hipStream_t st, const int64_t* off, int64_t B, int64_t V, int F, int n_cc,
                int64_t slots, const void* dP, int64_t ldg, const int* arg, void* dX, int64_t lddx) {
    if (op == SIR_POOL_SUM)
        hipLaunchKernelGGL((k_pool_bwd<DT, VW, SIR_POOL_SUM>), dim3(blocks), dim3(64), 0, st, off, B, V, F, n_cc, slots,
                           dP, ldg, arg, dX, lddx);
    else if (op == SIR_POOL_MEAN)
        hipLaunchKernelGGL((k_pool_bwd<DT, VW, SIR_POOL_MEAN>), dim3(blocks), dim3(64), 0, st, off, B, V, F, n_cc, slots,
                           dP, ldg, arg, dX, lddx);
    else
        hipLaunchKernelGGL((k_pool_bwd<DT, VW, SIR_POOL_MAX>), dim3(blocks), dim3(64), 0, st, off, B, V, F, n_cc, slots,
                           dP, ldg, arg, dX, lddx);
}

}  // namespace

int64_t graph_pool_slots(int64_t V, int64_t B) { return B + V / POOL_R; }

// partials exist only when a graph can be longer than one slab (V > R)
int64_t graph_pool_work_floats(int64_t V, int64_t B, int64_t F, int op) {
    if (B == 0 || V <= POOL_R) return 0;
    return graph_pool_slots(V, B) * F * (op == SIR_POOL_MAX ? 2 : 1);
}

hipError_t run_graph_pool_fwd(const int64_t* off, int64_t B, int64_t V, int F, int op, int dtype, const void* X,
                              int64_t ldx, void* P, int64_t ldp, int* arg, float* work, hipStream_t st) {
    if (B == 0) return hipSuccess;
    const uintptr_t vb = dtype == SIR_DTYPE_F32 ? 16 : 8;         // bytes of 4 elements
    const bool v4 = F % 4 == 0 && ldx % 4 == 0 && ldp % 4 == 0 && aligned_to(X, vb) && aligned_to(P, vb) &&
                    aligned16(arg);
    const int vw = v4 ? 4 : 1;
    const int n_cc = (F / vw + 63) / 64;
    const int64_t slots = graph_pool_slots(V, B);
    if (slots * n_cc > 0x7fffffffLL) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)(slots * n_cc);
    hipError_t err = by_dtype(dtype, [&](auto dt) {
        if (v4) launch_fwd<dt(), 4>(op, blocks, st, off, B, V, F, n_cc, slots, X, ldx, P, ldp, arg, work);
        else launch_fwd<dt(), 1>(op, blocks, st, off, B, V, F, n_cc, slots, X, ldx, P, ldp, arg, work);
        return hipGetLastError();
    });
    if (err != hipSuccess || V <= POOL_R) return err;
    int64_t cb = (B * F + 255) / 256;
    const unsigned cblocks = (unsigned)(cb < 2048 ? cb : 2048);
    return by_dtype(dtype, [&](auto dt) {
        launch_combine<dt()>(op, cblocks, st, off, B, V, F, slots, work, P, ldp, arg);
        return hipGetLastError();
    });
}

hipError_t run_graph_pool_bwd(const int64_t* off, int64_t B, int64_t V, int F, int op, int dtype, const void* dP,
                              int64_t ldg, const int* arg, void* dX, int64_t lddx, hipStream_t st) {
    if (B == 0 || V == 0) return hipSuccess;
    const uintptr_t vb = dtype == SIR_DTYPE_F32 ? 16 : 8;
    const bool v4 = F % 4 == 0 && ldg % 4 == 0 && lddx % 4 == 0 && aligned_to(dP, vb) && aligned_to(dX, vb) &&
                    aligned16(arg);
    const int vw = v4 ? 4 : 1;
    const int n_cc = (F / vw + 63) / 64;
    const int64_t slots = graph_pool_slots(V, B);
    if (slots * n_cc > 0x7fffffffLL) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)(slots * n_cc);
    return by_dtype(dtype, [&](auto dt) {
        if (v4) launch_bwd<dt(), 4>(op, blocks, st, off, B, V, F, n_cc, slots, dP, ldg, arg, dX, lddx);
        else launch_bwd<dt(), 1>(op, blocks, st, off, B, V, F, n_cc, slots, dP, ldg, arg, dX, lddx);
        return hipGetLastError();
    });
}

}  // namespace sir
