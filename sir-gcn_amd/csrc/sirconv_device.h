// sirconv_device.h — the device helpers every kernel file shares, each defined once: the activations
// (sigma, sigma'), the storage dtype (element type, widen, round once, the value after a store and a reload)
// and the typed 1- and 4-element loads and stores.  Nothing about any one pass lives here.
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma once
#include "sirconv.h"
#include "sirconv_internal.h"

namespace sir {

// The internal codes (sirconv_internal.h) are the ABI's (include/sirconv.h): either name may stand for the other.
static_assert(ACT_IDENTITY == SIR_ACT_IDENTITY && ACT_RELU == SIR_ACT_RELU && ACT_LEAKY == SIR_ACT_LEAKY_RELU &&
              ACT_GELU == SIR_ACT_GELU && ACT_GELU_TANH == SIR_ACT_GELU_TANH, "ACT_* must equal SIR_ACT_*");
static_assert(ST_F32 == SIR_DTYPE_F32 && ST_BF16 == SIR_DTYPE_BF16 && ST_F16 == SIR_DTYPE_F16,
              "ST_* must equal SIR_DTYPE_*");
static_assert(AGG_SUM == SIR_AGG_SUM && AGG_MEAN == SIR_AGG_MEAN && AGG_SYM == SIR_AGG_SYM,
              "AGG_* must equal SIR_AGG_*");

// ------------------------------------------------------------------------------ sigma
// Formulas follow torch's CPU/GPU kernels (aten Activation.cpp) operation for operation.
template <int ACT>
__device__ __forceinline__ float sig(float z, float slope) {
    if constexpr (ACT == ACT_IDENTITY) {
        return z;
    } else if constexpr (ACT == ACT_RELU) {
        return z <= 0.f ? 0.f : z;       // not z > 0 ? z : 0: ReLU(NaN) is NaN (torch.relu), never 0
    } else if constexpr (ACT == ACT_LEAKY) {
        return z > 0.f ? z : z * slope;
    } else if constexpr (ACT == ACT_GELU) {
        const float kAlpha = 0.70710678118654752440f;  // M_SQRT1_2
        return z * 0.5f * (1.0f + erff(z * kAlpha));
    } else {  // GELU tanh
        const float kBeta = 0.79788456080286535588f;   // M_SQRT2 * M_2_SQRTPI * 0.5
        const float kKappa = 0.044715f;
        const float inner = kBeta * (z + kKappa * z * z * z);
        return 0.5f * z * (1.0f + tanhf(inner));
    }
}

// sigma'(z) applied to an incoming gradient t (torch backward formulas).
template <int ACT>
__device__ __forceinline__ float dsig(float z, float t, float slope) {
    if constexpr (ACT == ACT_IDENTITY) {
        return t;
    } else if constexpr (ACT == ACT_RELU) {
        return z > 0.f ? t : 0.f;        // threshold_backward: result <= 0 -> 0
    } else if constexpr (ACT == ACT_LEAKY) {
        return z > 0.f ? t : t * slope;  // leaky_relu_backward
    } else if constexpr (ACT == ACT_GELU) {
        const float kAlpha = 0.70710678118654752440f;
        const float kBeta = 0.39894228040143267794f;   // M_2_SQRTPI * M_SQRT1_2 * 0.5
        const float cdf = 0.5f * (1.0f + erff(z * kAlpha));
        const float pdf = kBeta * expf(z * z * -0.5f);
        return t * (cdf + z * pdf);
    } else {
        const float kBeta = 0.79788456080286535588f;
        const float kKappa = 0.044715f;
        const float x_sq = z * z;
        const float x_cube = x_sq * z;
        const float inner = kBeta * (z + kKappa * x_cube);
        const float tanh_inner = tanhf(inner);
        const float left = 0.5f * z;
        const float right = 1.0f + tanh_inner;
        const float left_derivative = 0.5f * right;
        const float tanh_derivative = 1.0f - tanh_inner * tanh_inner;
        const float inner_derivative = kBeta * (1.0f + 3.0f * kKappa * x_sq);
        const float right_derivative = left * tanh_derivative * inner_derivative;
        return t * (left_derivative + right_derivative);
    }
}

// ------------------------------------------------------------------------------ storage dtype
// Feature rows (Q, K, G, S, dQ, dK, Gm) are stored as fp32, bf16 or fp16 (SIR_DTYPE_*; the AMP
// path of the reference, heterophilous-datasets/train.py:75, runs the layer under autocast).  Every
// value is converted to fp32 on load; sigma, sigma', the norm product and the accumulation run in
// fp32 (the reference accumulates its promoted fp32 messages), and results are
// rounded once (RNE) on store.  Partial rows of split items stay fp32.
template <int ST> struct Stor { typedef float T; };
template <> struct Stor<ST_BF16> { typedef __bf16 T; };
template <> struct Stor<ST_F16> { typedef _Float16 T; };

typedef unsigned int sir_u2 __attribute__((ext_vector_type(2)));
typedef unsigned int sir_u4 __attribute__((ext_vector_type(4)));

template <int ST>
__device__ __forceinline__ float h2f(uint32_t bits16) {
    if constexpr (ST == ST_BF16) return __uint_as_float(bits16 << 16);
    else return (float)__builtin_bit_cast(_Float16, (uint16_t)bits16);
}
template <int ST>
__device__ __forceinline__ uint32_t f2h(float x) {
    if constexpr (ST == ST_BF16) return (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)x);
    else return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)x);
}
// fp32 value rounded to the storage precision (what a store + reload yields)
template <int ST>
__device__ __forceinline__ float round_st(float x) {
    if constexpr (ST == ST_F32) return x;
    else return h2f<ST>(f2h<ST>(x));
}

// ------------------------------------------------------------------------------ vectors
template <int VW>
__device__ __forceinline__ void vload(float (&d)[VW], const float* __restrict__ p) {
    if constexpr (VW == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        d[0] = t.x; d[1] = t.y; d[2] = t.z; d[3] = t.w;
    } else {
#pragma unroll
        for (int w = 0; w < VW; ++w) d[w] = p[w];
    }
}

template <int VW>
__device__ __forceinline__ void vstore(float* __restrict__ p, const float (&s)[VW]) {
    if constexpr (VW == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(s[0], s[1], s[2], s[3]);
    } else {
#pragma unroll
        for (int w = 0; w < VW; ++w) p[w] = s[w];
    }
}

// typed loads / stores: fp32 as above; 16-bit storage as one 8-B access per 4 values
template <int ST, int VW>
__device__ __forceinline__ void tload_p(float (&d)[VW], const typename Stor<ST>::T* __restrict__ p) {
    if constexpr (ST == ST_F32) {
        vload<VW>(d, p);
    } else if constexpr (VW == 4) {
        const sir_u2* q = reinterpret_cast<const sir_u2*>(p);
        const sir_u2 t = *q;
        d[0] = h2f<ST>(t.x & 0xffffu); d[1] = h2f<ST>(t.x >> 16);
        d[2] = h2f<ST>(t.y & 0xffffu); d[3] = h2f<ST>(t.y >> 16);
    } else {
        const uint16_t* q = reinterpret_cast<const uint16_t*>(p);
#pragma unroll
        for (int w = 0; w < VW; ++w) d[w] = h2f<ST>(q[w]);
    }
}

template <int ST, int VW>
__device__ __forceinline__ void tstore_p(typename Stor<ST>::T* __restrict__ p, const float (&s)[VW]) {
    if constexpr (ST == ST_F32) {
        vstore<VW>(p, s);
    } else if constexpr (VW == 4) {
        sir_u2 t;
        t.x = f2h<ST>(s[0]) | (f2h<ST>(s[1]) << 16);
        t.y = f2h<ST>(s[2]) | (f2h<ST>(s[3]) << 16);
        *reinterpret_cast<sir_u2*>(p) = t;
    } else {
        uint16_t* q = reinterpret_cast<uint16_t*>(p);
#pragma unroll
        for (int w = 0; w < VW; ++w) q[w] = (uint16_t)f2h<ST>(s[w]);
    }
}

}  // namespace sir
