// sirconv_gemm_nt.h — what the split-fp16 projection GEMM kernels of sirconv_gemm.hip and
// sirconv_gemm_nt2.hip share: the running row scale, the hi/lo split, the dropout epilogue step and
// the launcher of the two-block persistent NT kernel.  (Numerics: the head of sirconv_gemm.hip.)
#pragma once
#include "sirconv_internal.h"
#include "sirconv_gemm_util.h"
#include "sirconv_dropout.h"

namespace sir {
namespace gemm {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f16v __attribute__((ext_vector_type(16)));
typedef unsigned int u4v __attribute__((ext_vector_type(4)));

constexpr int KC = 32;          // contraction elements per LDS stage (two k16 MFMA steps)

#ifndef SIR_HR
#define SIR_HR 8                // headroom bits of a reset running scale (see next_se)
#endif

// Smallest e with |m| < 2^e for normal m (e = -126 for 0 and subnormals, 129 for inf/nan).
__device__ inline int bexp(float m) { return (int)((__float_as_uint(m) >> 23) & 255u) - 126; }
// scale exponent for a running binade e: |x| * 2^(15 - e) < 2^15, clamped to a normal float
__device__ inline int scale_exp(int e) { int s = 15 - e; return s > 126 ? 126 : s; }
// Running scale of a data row / column with hysteresis: a chunk whose binade e_c still fits
// (|x| * 2^se < 2^15) keeps the current scale; otherwise the scale is reset with SIR_HR bits of
// headroom, so a row's scale changes (and its accumulators are rescaled) only when a chunk
// exceeds the row's earlier maximum by more than 2^SIR_HR — once per row in practice, at its
// first chunk.  Scaled values stay in [2^-14, 2^15) over >= 20 binades below the maximum, where
// the fp16 hi/lo pair is exact to ~22 bits; the split is scale-invariant there, so the result
// does not depend on which power-of-two scale was in force.
constexpr int SE_INIT = 127;    // no chunk seen yet
__device__ inline int next_se(int se_old, int e_c) {
    if (e_c + se_old <= 15) return se_old;
    const int s = 15 - SIR_HR - e_c;
    return s > 126 ? 126 : s;
}
__device__ inline float pow2(int e) { e = e < -126 ? -126 : (e > 127 ? 127 : e); return __uint_as_float((uint32_t)(e + 127) << 23); }
// feature dropout of QK (sirconv_dropout.h) on 4 consecutive output columns n .. n+3 of one row
__device__ inline void drop4(const Drop& d, int64_t row, int n, float4& o) {
    const uint32_t rh = drop_row_hash(d, row);
    const int c = d.col0 + n;
    o.x = drop_keep(d, rh, c + 0) ? o.x * d.scale : 0.f;
    o.y = drop_keep(d, rh, c + 1) ? o.y * d.scale : 0.f;
    o.z = drop_keep(d, rh, c + 2) ? o.z * d.scale : 0.f;
    o.w = drop_keep(d, rh, c + 3) ? o.w * d.scale : 0.f;
}

// hi/lo fp16 split of 8 floats scaled by s (exact power of two)
// hi = fp16(x s), lo = fp16(x s - hi), one v_fma_mix each, written into the halves of the fragment
// registers (x s is exact, and x s - hi is exact in the fused op: the same bits as rounding y = x s
// and y - hi separately, sirconv_gemm_w.hip).  s_nop 1: the VALU-write -> MFMA-read wait states
// (the hazard recognizer does not look inside inline asm).
__device__ inline void split8_mix(float4 a, float4 b, float s, h8& hi, h8& lo) {
    uint32_t h0, h1, h2, h3, l0, l1, l2, l3;
    asm volatile(
        "v_fma_mixlo_f16 %0, %8, %16, 0\n\tv_fma_mixhi_f16 %0, %9, %16, 0\n\t"
        "v_fma_mixlo_f16 %1, %10, %16, 0\n\tv_fma_mixhi_f16 %1, %11, %16, 0\n\t"
        "v_fma_mixlo_f16 %2, %12, %16, 0\n\tv_fma_mixhi_f16 %2, %13, %16, 0\n\t"
        "v_fma_mixlo_f16 %3, %14, %16, 0\n\tv_fma_mixhi_f16 %3, %15, %16, 0\n\t"
        "v_fma_mixlo_f16 %4, %8, %16, -%0 op_sel_hi:[0,0,1]\n\tv_fma_mixhi_f16 %4, %9, %16, -%0 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixlo_f16 %5, %10, %16, -%1 op_sel_hi:[0,0,1]\n\tv_fma_mixhi_f16 %5, %11, %16, -%1 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixlo_f16 %6, %12, %16, -%2 op_sel_hi:[0,0,1]\n\tv_fma_mixhi_f16 %6, %13, %16, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixlo_f16 %7, %14, %16, -%3 op_sel_hi:[0,0,1]\n\tv_fma_mixhi_f16 %7, %15, %16, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "s_nop 1"
        : "=&v"(h0), "=&v"(h1), "=&v"(h2), "=&v"(h3), "=&v"(l0), "=&v"(l1), "=&v"(l2), "=&v"(l3)
        : "v"(a.x), "v"(a.y), "v"(a.z), "v"(a.w), "v"(b.x), "v"(b.y), "v"(b.z), "v"(b.w), "v"(s));
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    hi = __builtin_bit_cast(h8, u4{h0, h1, h2, h3});
    lo = __builtin_bit_cast(h8, u4{l0, l1, l2, l3});
}

// m = max(m, |v|) in two v_max3_f32 with |.| source modifiers (fmaxf makes hipcc canonicalise every
// input first)
__device__ inline float fmax4_mix(float m, float4 v) {
    asm("v_max3_f32 %0, %0, |%1|, |%2|\n\tv_max3_f32 %0, %0, |%3|, |%4|" : "+v"(m) : "v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w));
    return m;
}

constexpr int NT_P_NMAX = 512;  // widest packed weight of the persistent NT kernels (their LDS scale / bias rows)

}  // namespace gemm

int64_t gemm_pack_npad(int64_t N);
// k_gemm_nt_p2<kc> (sirconv_gemm_nt2.hip) over C's 128 x 256 tiles, two blocks per CU (kc = K / KC: 4,
// 8 or 16); false, with nothing launched, if the tile count is out of range
bool launch_gemm_nt_p2(const float* A, int64_t lda, int64_t M, int kc, const void* packed, int N, const float* bias,
                       float* C, int64_t ldc, hipStream_t st, const Drop& drop);

}  // namespace sir
