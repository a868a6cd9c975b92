// sirconv_paramnorm.hip — the L1 / L2 parameter penalty of the reference's training loops,
//     regularizer(model, args) = (l1 * sum_p sum|p| + l2 * sum_p sum p^2) * int(model.training)
// (benchmark-datasets/*/train.py, e.g. zinc/train.py:49-52), as one multi-tensor pass per direction over
// the fp32 parameters:
//   forward : L1 = sum_t sum_i |p_t[i]|,  L2 = sum_t sum_i p_t[i]^2
//   backward: dP_t[i] = fl(g1 * sgn(p_t[i])) + fl(g2 * fl(2 * p_t[i])),  sgn(+-0) = 0
//
// Multi-tensor: the device pointers and element counts of up to TM = SIR_PARAM_NORMS_MAX_TENSORS tensors
// travel in the kernel arguments (no device-side pointer table that could go stale); a longer list takes
// further launches of the same kernel.  A tensor is cut into chunks of CH = SIR_PARAM_NORMS_CHUNK elements
// counted from its own first element, so a chunk never spans tensors; block b of a launch finds its
// (tensor, chunk) by a binary search over the prefix of chunk counts in the arguments.  Tensors without
// elements (and, in the backward, without a gradient slot) are left out on the host: never read.
//
// Forward: one block of 256 threads per chunk; the chunk's sums go as one fp32 pair to work[2 q], work[2 q + 1],
// q the chunk's index in list order.  One last single-block launch adds all pairs in chunk order and writes
// out2 = {L1, L2}.  No atomics: both results are a function of the list alone (order and sizes, and each
// pointer's offset from a 16-B boundary), not of the grid, the CU count or the stream.
//
// Alignment: a parameter may be a view whose address is only 4-B aligned.  A chunk is its scalar head (the
// 0..3 elements before the first 16-B boundary), its body of whole 16-B vectors and its scalar tail (0..3);
// only the body is read with 16-B loads, head and tail with 4-B loads, and nothing outside the chunk is
// touched.  The gradient slots are 16-B aligned (checked by the ABI), so the backward stores whole vectors
// at aligned addresses and single floats at a tensor's last 0..3 elements; it reads a misaligned parameter
// with 4-B loads.
//
// Chain of roundings (fp32; the longest sequence of dependent rounded operations behind a result):
//   the square (L2 only)                                                         1
//   a vector's 4 terms, (x0 + x1) + (x2 + x3)                                    2
//   the thread's 4 vectors, (v0 + v1) + (v2 + v3)                                2
//   the thread's head / tail element, if it has one                              1
//   the wave's 64 lanes, xor-shuffle tree                                        6
//   the block's 4 waves through LDS, (w0 + w1) + (w2 + w3)                       2     chunk: 14 (L1: 13)
//   combine: thread i adds the pairs i, i + 256, ... in order                    ceil(C / 256) - 1
//   combine: the 256 partial sums, wave tree and LDS step                        6 + 2
// with C the list's chunks, C <= N / CH + T for N elements in T non-empty tensors.  N = 2^24 in one tensor:
// C = 4096, 14 + 15 + 8 = 37.  The chain stays <= 64 while C <= 43 * 256 = 11008, i.e. for every list of up
// to 2^24 elements in up to 6912 tensors.  No thread ever adds a whole chunk serially.
//
// Non-finite values: every term is non-negative, so the sums are NaN when a parameter is NaN and +Inf when
// one is +-Inf (never Inf - Inf); lanes and vector slots past a chunk's end contribute a selected +0, never
// a product.  The backward evaluates its expression as written (the library is built with
// -ffp-contract=off): g2 = 0 and p = Inf give NaN, as in torch; an absent g1 or g2 drops its term by
// selection (a template instance), it is never multiplied by zero.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sirconv.h"
#include "sirconv_internal.h"

namespace sir {
namespace {

constexpr int PN_CH = SIR_PARAM_NORMS_CHUNK;
constexpr int PN_TM = SIR_PARAM_NORMS_MAX_TENSORS;
constexpr int PN_THREADS = 256;
constexpr int PN_VPT = 4;                                  // 16-B vectors per thread
static_assert(PN_CH == PN_THREADS * PN_VPT * 4, "a chunk is 4 vectors of 4 floats per thread");
static_assert(SIR_PARAM_NORMS_COMBINE_THREADS == PN_THREADS, "the combine is one block of 256 threads");
// a launch's chunks fit a grid dimension; one tensor (at most 2^40 elements, checked by the ABI) always fits
constexpr int64_t PN_MAX_GRID = (int64_t)1 << 30;

struct PnFwd {
    const float* p[PN_TM];
    int64_t n[PN_TM];
    int cstart[PN_TM + 1];        // prefix of chunk counts: tensor t owns the blocks [cstart[t], cstart[t + 1])
    int nt;
};

struct PnBwd {
    const float* p[PN_TM];
    float* d[PN_TM];
    int64_t n[PN_TM];
    int cstart[PN_TM + 1];
    int nt;
};

// the tensor of block b: cstart[t] <= b < cstart[t + 1] (b is uniform, so is the search)
template <typename A>
__device__ __forceinline__ int pn_find(const A& a, int b) {
    int lo = 0, hi = a.nt;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.cstart[mid] <= b) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the sum over the block's 256 threads by a fixed tree; the result is valid in thread 0
__device__ __forceinline__ float pn_block_sum(float v, float* lds) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) lds[w] = v;
    __syncthreads();
    return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

__global__ void __launch_bounds__(PN_THREADS)
k_pn_fwd(const PnFwd a, float* __restrict__ work) {
    __shared__ float lds[8];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const int t = pn_find(a, b);
    const int64_t e0 = (int64_t)(b - a.cstart[t]) * PN_CH;
    const int64_t left = a.n[t] - e0;
    const int m = left < PN_CH ? (int)left : PN_CH;        // elements of this chunk, 1 .. CH
    const float* __restrict__ p = a.p[t] + e0;
    const int h0 = (int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(p) >> 2) & 3u)) & 3u);
    const int h = h0 < m ? h0 : m;                         // scalar head
    const int nb = (m - h) >> 2;                           // whole 16-B vectors of the body
    const int r = m - h - 4 * nb;                          // scalar tail
    float x[PN_VPT][4];
#pragma unroll
    for (int k = 0; k < PN_VPT; ++k) x[k][0] = x[k][1] = x[k][2] = x[k][3] = 0.f;
    if (nb > 0) {
        const float4* __restrict__ pv = reinterpret_cast<const float4*>(p + h);
        // every load is issued (the index is clamped into the body); a slot past the body keeps its +0
#pragma unroll
        for (int k = 0; k < PN_VPT; ++k) {
            const int j = k * PN_THREADS + tid;
            const float4 v = pv[j < nb ? j : nb - 1];
            if (j < nb) { x[k][0] = v.x; x[k][1] = v.y; x[k][2] = v.z; x[k][3] = v.w; }
        }
    }
    // head element i sits in thread i, tail element i in thread 4 + i
    float e = 0.f;
    if (tid < h) e = p[tid];
    else if (tid >= 4 && tid - 4 < r) e = p[h + 4 * nb + (tid - 4)];
    float s1[PN_VPT], s2[PN_VPT];
#pragma unroll
    for (int k = 0; k < PN_VPT; ++k) {
        s1[k] = (fabsf(x[k][0]) + fabsf(x[k][1])) + (fabsf(x[k][2]) + fabsf(x[k][3]));
        s2[k] = (x[k][0] * x[k][0] + x[k][1] * x[k][1]) + (x[k][2] * x[k][2] + x[k][3] * x[k][3]);
    }
    float a1 = (s1[0] + s1[1]) + (s1[2] + s1[3]);
    float a2 = (s2[0] + s2[1]) + (s2[2] + s2[3]);
    a1 = a1 + fabsf(e);
    a2 = a2 + e * e;
    a1 = pn_block_sum(a1, lds);
    a2 = pn_block_sum(a2, lds + 4);
    if (tid == 0) {
        work[2 * (int64_t)b] = a1;
        work[2 * (int64_t)b + 1] = a2;
    }
}

// all pairs in chunk order: thread i adds the pairs i, i + 256, ... then the fixed tree over the threads
__global__ void __launch_bounds__(PN_THREADS)
k_pn_combine(const float* __restrict__ work, int64_t n_chunks, float* __restrict__ out2) {
    __shared__ float lds[8];
    const float2* __restrict__ w = reinterpret_cast<const float2*>(work);
    float a1 = 0.f, a2 = 0.f;
    int64_t q = threadIdx.x;
    if (q < n_chunks) {
        const float2 v = w[q];
        a1 = v.x;
        a2 = v.y;
    }
#pragma unroll 4
    for (q += PN_THREADS; q < n_chunks; q += PN_THREADS) {
        const float2 v = w[q];
        a1 = a1 + v.x;
        a2 = a2 + v.y;
    }
    a1 = pn_block_sum(a1, lds);
    a2 = pn_block_sum(a2, lds + 4);
    if (threadIdx.x == 0) {
        out2[0] = a1;
        out2[1] = a2;
    }
}

// TERMS: 1 = the L1 term only, 2 = the L2 term only, 3 = both
template <int TERMS>
__device__ __forceinline__ float pn_grad(float p, float g1, float g2) {
    const float s = (float)((0.f < p) - (p < 0.f));
    if constexpr (TERMS == 1) return g1 * s;
    else if constexpr (TERMS == 2) return g2 * (2.f * p);
    else return g1 * s + g2 * (2.f * p);
}

template <int TERMS>
__global__ void __launch_bounds__(PN_THREADS)
k_pn_bwd(const PnBwd a, const float* __restrict__ g1p, const float* __restrict__ g2p) {
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const int t = pn_find(a, b);
    const int64_t e0 = (int64_t)(b - a.cstart[t]) * PN_CH;
    const int64_t left = a.n[t] - e0;
    const int m = left < PN_CH ? (int)left : PN_CH;
    const float* __restrict__ p = a.p[t] + e0;
    float* __restrict__ d = a.d[t] + e0;                   // 16-B aligned: the slot is, and e0 % 4 == 0
    float g1 = 0.f, g2 = 0.f;
    if constexpr ((TERMS & 1) != 0) g1 = *g1p;
    if constexpr ((TERMS & 2) != 0) g2 = *g2p;
    const bool p16 = (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
    if (m == PN_CH && p16) {                               // a whole chunk of an aligned parameter
        const float4* __restrict__ pv = reinterpret_cast<const float4*>(p);
        float4 v[PN_VPT];
#pragma unroll
        for (int k = 0; k < PN_VPT; ++k) v[k] = pv[k * PN_THREADS + tid];
#pragma unroll
        for (int k = 0; k < PN_VPT; ++k) {
            float4 o;
            o.x = pn_grad<TERMS>(v[k].x, g1, g2);
            o.y = pn_grad<TERMS>(v[k].y, g1, g2);
            o.z = pn_grad<TERMS>(v[k].z, g1, g2);
            o.w = pn_grad<TERMS>(v[k].w, g1, g2);
            reinterpret_cast<float4*>(d)[k * PN_THREADS + tid] = o;
        }
        return;
    }
    for (int k = 0; k < PN_VPT; ++k) {
        const int i0 = 4 * (k * PN_THREADS + tid);
        if (i0 + 4 <= m) {
            float4 v;
            if (p16) {
                v = *reinterpret_cast<const float4*>(p + i0);
            } else {
                v.x = p[i0]; v.y = p[i0 + 1]; v.z = p[i0 + 2]; v.w = p[i0 + 3];
            }
            float4 o;
            o.x = pn_grad<TERMS>(v.x, g1, g2);
            o.y = pn_grad<TERMS>(v.y, g1, g2);
            o.z = pn_grad<TERMS>(v.z, g1, g2);
            o.w = pn_grad<TERMS>(v.w, g1, g2);
            *reinterpret_cast<float4*>(d + i0) = o;
        } else {
            for (int i = i0; i < m; ++i) d[i] = pn_grad<TERMS>(p[i], g1, g2);
        }
    }
}

// adds tensor (p, n) to the batch; false when the batch has no room for it (flush first)
template <typename A>
bool pn_room(const A& a, int64_t chunks) {
    return a.nt < PN_TM && (int64_t)a.cstart[a.nt] + chunks <= PN_MAX_GRID;
}

}  // namespace

int64_t param_norms_chunks(int64_t numel) { return numel <= 0 ? 0 : (numel + PN_CH - 1) / PN_CH; }

hipError_t run_param_norms_fwd(const float* const* params, const int64_t* numel, int64_t T, float* work, float* out2,
                               hipStream_t st) {
    PnFwd a;
    a.nt = 0;
    a.cstart[0] = 0;
    int64_t done = 0;                                      // chunks of the launches issued so far
    auto flush = [&]() -> hipError_t {
        if (a.nt == 0) return hipSuccess;
        const int blocks = a.cstart[a.nt];
        hipLaunchKernelGGL(k_pn_fwd, dim3((unsigned)blocks), dim3(PN_THREADS), 0, st, a, work + 2 * done);
        done += blocks;
        a.nt = 0;
        return hipGetLastError();
    };
    for (int64_t t = 0; t < T; ++t) {
        const int64_t chunks = param_norms_chunks(numel[t]);
        if (chunks == 0) continue;
        if (chunks > PN_MAX_GRID) return hipErrorInvalidValue;
        if (!pn_room(a, chunks)) {
            hipError_t err = flush();
            if (err != hipSuccess) return err;
        }
        a.p[a.nt] = params[t];
        a.n[a.nt] = numel[t];
        a.cstart[a.nt + 1] = a.cstart[a.nt] + (int)chunks;
        ++a.nt;
    }
    hipError_t err = flush();
    if (err != hipSuccess || done == 0) return err;
    hipLaunchKernelGGL(k_pn_combine, dim3(1), dim3(PN_THREADS), 0, st, work, done, out2);
    return hipGetLastError();
}

hipError_t run_param_norms_bwd(const float* const* params, const int64_t* numel, float* const* grads, int64_t T,
                               const float* g1, const float* g2, hipStream_t st) {
    PnBwd a;
    a.nt = 0;
    a.cstart[0] = 0;
    const int terms = (g1 != nullptr ? 1 : 0) | (g2 != nullptr ? 2 : 0);
    auto flush = [&]() -> hipError_t {
        if (a.nt == 0) return hipSuccess;
        const dim3 grid((unsigned)a.cstart[a.nt]), block(PN_THREADS);
        if (terms == 1) hipLaunchKernelGGL(k_pn_bwd<1>, grid, block, 0, st, a, g1, g2);
        else if (terms == 2) hipLaunchKernelGGL(k_pn_bwd<2>, grid, block, 0, st, a, g1, g2);
        else hipLaunchKernelGGL(k_pn_bwd<3>, grid, block, 0, st, a, g1, g2);
        a.nt = 0;
        return hipGetLastError();
    };
    for (int64_t t = 0; t < T; ++t) {
        const int64_t chunks = param_norms_chunks(numel[t]);
        if (chunks == 0 || grads[t] == nullptr) continue;
        if (chunks > PN_MAX_GRID) return hipErrorInvalidValue;
        if (!pn_room(a, chunks)) {
            hipError_t err = flush();
            if (err != hipSuccess) return err;
        }
        a.p[a.nt] = params[t];
        a.d[a.nt] = grads[t];
        a.n[a.nt] = numel[t];
        a.cstart[a.nt + 1] = a.cstart[a.nt] + (int)chunks;
        ++a.nt;
    }
    return flush();
}

}  // namespace sir
