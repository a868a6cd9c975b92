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
// sigma and sigma' are sirconv_edge_impl.h's sig / dsig: the project's one GELU.
// A streaming kernel: no LDS, no atomics, 4 consecutive elements per thread in one vector access each.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sirconv.h"
#include "sirconv_internal.h"
#include "sirconv_dropout.h"
#include "sirconv_edge_impl.h"

namespace sir {
namespace {

template <int DT>
struct Elt;
template <>
struct Elt<SIR_DTYPE_F32> {
    typedef float T;
    static __device__ __forceinline__ float up(float x) { return x; }
    static __device__ __forceinline__ float down(float x) { return x; }
};
template <>
struct Elt<SIR_DTYPE_BF16> {
    typedef __bf16 T;
    static __device__ __forceinline__ float up(__bf16 x) { return (float)x; }
    static __device__ __forceinline__ __bf16 down(float x) { return (__bf16)x; }
};
template <>
struct Elt<SIR_DTYPE_F16> {
    typedef _Float16 T;
    static __device__ __forceinline__ float up(_Float16 x) { return (float)x; }
    static __device__ __forceinline__ _Float16 down(float x) { return (_Float16)x; }
};

// fp32 value after a store to DT and a reload
template <int DT>
__device__ __forceinline__ float rnd(float x) { return Elt<DT>::up(Elt<DT>::down(x)); }

// 4 consecutive elements of a DT row, widened to fp32 (one 16-byte or one 8-byte access)
template <int DT>
__device__ __forceinline__ void ld4(float (&v)[4], const void* __restrict__ base, int64_t off) {
    typedef typename Elt<DT>::T T;
    typedef T T4 __attribute__((ext_vector_type(4)));
    const T4 t = *reinterpret_cast<const T4*>(static_cast<const T*>(base) + off);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = Elt<DT>::up(t[i]);
}
template <int DT>
__device__ __forceinline__ void st4(void* __restrict__ base, int64_t off, const float (&v)[4]) {
    typedef typename Elt<DT>::T T;
    typedef T T4 __attribute__((ext_vector_type(4)));
    T4 t;
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] = Elt<DT>::down(v[i]);
    *reinterpret_cast<T4*>(static_cast<T*>(base) + off) = t;
}

// d = the dropout's output at (row hash rh, column n) as the fp32 value of its DT storage
template <int DT>
__device__ __forceinline__ float dropped(const Drop& drop, bool on, uint32_t rh, int n, float y, bool& keep) {
    keep = true;
    if (!on) return y;
    keep = drop_keep(drop, rh, n);
    return keep ? rnd<DT>(y * drop.scale) : 0.f;
}

// rows of N (N % 4 == 0), grid-stride over M * N / 4; DT: y (and dy), ODT: R and out (F32 or DT)
template <int DT, int ODT, int ACT>
__global__ void __launch_bounds__(256)
k_dropact_fwd(const void* __restrict__ Y, int64_t ldy, const void* __restrict__ R, int64_t ldr, void* __restrict__ O,
              int64_t ldo, int64_t M, int N, float slope, Drop drop) {
    drop = drop_resolve(drop);
    const bool on = drop.on();
    const int nq = N / 4;
    const int64_t total = M * nq;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
        const int64_t m = q / nq;
        const int n = (int)(q - m * nq) * 4;
        float yv[4], rv[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
        ld4<DT>(yv, Y, m * ldy + n);
        if (R != nullptr) ld4<ODT>(rv, R, m * ldr + n);
        const uint32_t rh = on ? drop_row_hash(drop, m) : 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            bool keep;
            const float d = dropped<DT>(drop, on, rh, n + i, yv[i], keep);
            const float a = rnd<DT>(sig<ACT>(d, slope));
            o[i] = R != nullptr ? a + rv[i] : a;           // rounded to ODT by the store
        }
        st4<ODT>(O, m * ldo + n, o);
    }
}

template <int DT, int ODT, int ACT>
__global__ void __launch_bounds__(256)
k_dropact_bwd(const void* __restrict__ D, int64_t ldd, const void* __restrict__ Y, int64_t ldy, void* __restrict__ DY,
              int64_t lddy, int64_t M, int N, float slope, Drop drop) {
    drop = drop_resolve(drop);
    const bool on = drop.on();
    const int nq = N / 4;
    const int64_t total = M * nq;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
        const int64_t m = q / nq;
        const int n = (int)(q - m * nq) * 4;
        float yv[4], dv[4], g[4];
        ld4<DT>(yv, Y, m * ldy + n);
        ld4<ODT>(dv, D, m * ldd + n);
        const uint32_t rh = on ? drop_row_hash(drop, m) : 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            bool keep;
            const float d = dropped<DT>(drop, on, rh, n + i, yv[i], keep);
            // the activation's backward runs on dout cast to its type (autograd's cast of the add's fp32
            // gradient for a 16-bit operand), in opmath, rounded once; then the dropout's grad * scale
            const float ga = rnd<DT>(dsig<ACT>(d, rnd<DT>(dv[i]), slope));
            g[i] = !on ? ga : (keep ? ga * drop.scale : 0.f);   // rounded to DT by the store
        }
        st4<DT>(DY, m * lddy + n, g);
    }
}

unsigned dropact_grid(int64_t M, int N) {
    const int64_t q = M * (N / 4);
    const int64_t b = (q + 255) / 256;
    const int64_t cap = 8 * (int64_t)device_cu_count();
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

template <int DT, int ODT>
hipError_t fwd_t(int act, const void* Y, int64_t ldy, const void* R, int64_t ldr, void* O, int64_t ldo, int64_t M, int N,
                 float slope, const Drop& drop, hipStream_t st) {
    const dim3 grid(dropact_grid(M, N));
#define SIR_DROPACT_FWD(A) \
    hipLaunchKernelGGL((k_dropact_fwd<DT, ODT, A>), grid, dim3(256), 0, st, Y, ldy, R, ldr, O, ldo, M, N, slope, drop)
    switch (act) {
    case SIR_ACT_IDENTITY: SIR_DROPACT_FWD(ACT_IDENTITY); break;
    case SIR_ACT_RELU: SIR_DROPACT_FWD(ACT_RELU); break;
    case SIR_ACT_LEAKY_RELU: SIR_DROPACT_FWD(ACT_LEAKY); break;
    case SIR_ACT_GELU: SIR_DROPACT_FWD(ACT_GELU); break;
    case SIR_ACT_GELU_TANH: SIR_DROPACT_FWD(ACT_GELU_TANH); break;
    default: return hipErrorInvalidValue;
    }
#undef SIR_DROPACT_FWD
    return hipGetLastError();
}

template <int DT, int ODT>
hipError_t bwd_t(int act, const void* D, int64_t ldd, const void* Y, int64_t ldy, void* DY, int64_t lddy, int64_t M,
                 int N, float slope, const Drop& drop, hipStream_t st) {
    const dim3 grid(dropact_grid(M, N));
#define SIR_DROPACT_BWD(A) \
    hipLaunchKernelGGL((k_dropact_bwd<DT, ODT, A>), grid, dim3(256), 0, st, D, ldd, Y, ldy, DY, lddy, M, N, slope, drop)
    switch (act) {
    case SIR_ACT_IDENTITY: SIR_DROPACT_BWD(ACT_IDENTITY); break;
    case SIR_ACT_RELU: SIR_DROPACT_BWD(ACT_RELU); break;
    case SIR_ACT_LEAKY_RELU: SIR_DROPACT_BWD(ACT_LEAKY); break;
    case SIR_ACT_GELU: SIR_DROPACT_BWD(ACT_GELU); break;
    case SIR_ACT_GELU_TANH: SIR_DROPACT_BWD(ACT_GELU_TANH); break;
    default: return hipErrorInvalidValue;
    }
#undef SIR_DROPACT_BWD
    return hipGetLastError();
}

}  // namespace

// dtype: y / dy; o_dtype: R, out and dout — SIR_DTYPE_F32 or dtype (checked by the ABI layer)
hipError_t run_drop_act_fwd(const void* Y, int64_t ldy, int dtype, const void* R, int64_t ldr, void* O, int64_t ldo,
                            int o_dtype, int64_t M, int N, int act, float slope, const Drop& drop, hipStream_t st) {
    if (M == 0 || N == 0) return hipSuccess;
    const bool o32 = o_dtype == SIR_DTYPE_F32;
#define SIR_DROPACT(DTV) \
    (o32 ? fwd_t<DTV, SIR_DTYPE_F32>(act, Y, ldy, R, ldr, O, ldo, M, N, slope, drop, st) \
         : fwd_t<DTV, DTV>(act, Y, ldy, R, ldr, O, ldo, M, N, slope, drop, st))
    if (dtype == SIR_DTYPE_F32) return fwd_t<SIR_DTYPE_F32, SIR_DTYPE_F32>(act, Y, ldy, R, ldr, O, ldo, M, N, slope, drop, st);
    if (dtype == SIR_DTYPE_BF16) return SIR_DROPACT(SIR_DTYPE_BF16);
    return SIR_DROPACT(SIR_DTYPE_F16);
#undef SIR_DROPACT
}

hipError_t run_drop_act_bwd(const void* D, int64_t ldd, int o_dtype, const void* Y, int64_t ldy, int dtype, void* DY,
                            int64_t lddy, int64_t M, int N, int act, float slope, const Drop& drop, hipStream_t st) {
    if (M == 0 || N == 0) return hipSuccess;
    const bool o32 = o_dtype == SIR_DTYPE_F32;
#define SIR_DROPACT(DTV) \
    (o32 ? bwd_t<DTV, SIR_DTYPE_F32>(act, D, ldd, Y, ldy, DY, lddy, M, N, slope, drop, st) \
         : bwd_t<DTV, DTV>(act, D, ldd, Y, ldy, DY, lddy, M, N, slope, drop, st))
    if (dtype == SIR_DTYPE_F32) return bwd_t<SIR_DTYPE_F32, SIR_DTYPE_F32>(act, D, ldd, Y, ldy, DY, lddy, M, N, slope, drop, st);
    if (dtype == SIR_DTYPE_BF16) return SIR_DROPACT(SIR_DTYPE_BF16);
    return SIR_DROPACT(SIR_DTYPE_F16);
#undef SIR_DROPACT
}

}  // namespace sir
