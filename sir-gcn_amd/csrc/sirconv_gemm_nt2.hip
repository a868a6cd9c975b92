// sirconv_gemm_nt2.hip — the persistent NT projection GEMM as two independent 4-wave blocks per CU.
//
// k_gemm_nt_p (sirconv_gemm.hip) owns a CU with one 512-thread block: its eight waves run the same
// phase between barriers, so LDS latency, MFMA issue, memory latency and the epilogue follow one
// another.  Here a block is 256 threads (one wave per SIMD) on a 128 x 256 output tile, and two
// blocks are resident per CU: every SIMD still holds two multiplying waves, but they belong to
// blocks with separate barriers, LDS and tile positions, so one block's barrier waits, image
// writes, store bursts and exposed load latency are filled by the other block's MFMAs.
//
// Per output element the operations and their order are those of k_gemm_nt_p (the wave tile is its
// 128 x 64: TDT = 4, TFT = 2; the same fragment images, MFMA order, three-product split, running
// row scale and epilogue arithmetic): results are bit-identical.
//
// Staging.  A: as in k_gemm_nt_p, two loader threads per row, 16 floats each, split into a
// double-buffered 16-KiB image per 32-k chunk.  W: with one row group every 32-feature fragment of
// the packed weight is read by exactly one wave, and the packed order is the fragment order, so
// each wave loads its own fragments straight into the MFMA operand registers (one coalesced 1-KiB
// load per fragment, lane l's 16 bytes to lane l), one k16 step (4 fragments, 16 VGPRs) ahead of
// the step being multiplied: the weights take no LDS, no LDS instruction and no barrier, and the
// compiler counts every wait.  (Measured first with the fragments moved by LDS-DMA into a per-wave
// ring: equal to k_gemm_nt_p — 8 DMA issues and 8 more fragment reads per wave and chunk)
// The freed LDS holds the epilogue's image, so a tile's epilogue is four rounds of whole 1-KiB rows.
// Cost accepted: every 128-row tile streams the whole 256-KiB packed weight tile from L2, twice the
// weight traffic per output row of the 256-row tile.
#include <type_traits>

#include "sirconv_gemm_nt.h"

namespace sir {
namespace {
using namespace gemm;

__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <int NCT>
__global__ void __launch_bounds__(256, 2)
k_gemm_nt_p2(const float* __restrict__ A, int64_t lda, int64_t M, const u4v* __restrict__ Wp, int Npad,
             const float* __restrict__ inv_t, const float* __restrict__ bias, int N, float* __restrict__ C,
             int64_t ldc, int n_ftiles, int n_tiles, int tiles_per_block, Drop drop) {
    drop = drop_resolve(drop);
    constexpr int TDT = 4, TFT = 2;
    constexpr int NT = 256, BD = 128, BF = 256, TPR = NT / BD, FPT = KC / TPR;
    static_assert(TPR == 2 && NCT >= 4 && NCT % 2 == 0, "mapping");
    constexpr int D_BYTES = BD * 128;                 // A image of a chunk: [part][ks][rows in fimg order]
    constexpr int ASTAGE = D_BYTES + BD * 4;          // + the rows' rescale factors
    constexpr int FIN_OFF = 2 * ASTAGE;               // [2][BD]: 2^-se of the rows of the last two tiles
    constexpr int EPI_OFF = FIN_OFF + 2 * BD * 4;     // inv_t[NT_P_NMAX], bias[NT_P_NMAX]
    constexpr int IMG_OFF = EPI_OFF + 2 * NT_P_NMAX * 4;      // the epilogue's 32-row image
    constexpr int PITCH = BF * 4 + 16;
    constexpr int LDS_BYTES = IMG_OFF + 32 * PITCH;
    static_assert(2 * LDS_BYTES <= 160 * 1024 && LDS_BYTES <= 78 * 1024, "two blocks per CU");
    __shared__ __attribute__((aligned(16))) char lds[LDS_BYTES];

    const int t = threadIdx.x;
    // XCD-aware: consecutive ranges of tiles (adjacent rows of A and C) on one XCD
    const int bid = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const int tb = bid * tiles_per_block;
    const int te = (tb + tiles_per_block < n_tiles) ? tb + tiles_per_block : n_tiles;
    if (tb >= te) return;
    float* const inv_l = reinterpret_cast<float*>(lds + EPI_OFF);
    float* const bias_l = inv_l + NT_P_NMAX;
    float* const fin = reinterpret_cast<float*>(lds + FIN_OFF);
    // x + (-0) == x for every x (-0 included): without a bias the epilogue adds -0, which leaves
    // the result bit-identical to adding nothing (no branch around the stores)
    for (int n = t; n < Npad; n += NT) {          // visible after the prologue's barrier
        inv_l[n] = inv_t[n];
        bias_l[n] = (bias != nullptr && n < N) ? bias[n] : -0.f;
    }

    // loader role (A)
    const int rho = t / TPR, kp = t % TPR;
    const int aoff = (rho * (int)lda + kp * FPT) * 4;
    struct TileP { rsrc_t a; int64_t d0; int f0; int rows; };
    auto tile_p = [&](int tt) {   // a tile past the block's range loads zeros (0-record resource)
        TileP p;
        if (tt < te) {
            p.d0 = (int64_t)(tt / n_ftiles) * BD;
            p.f0 = (tt % n_ftiles) * BF;
            p.rows = (M - p.d0 < BD) ? (int)(M - p.d0) : BD;
            p.a = mk_rsrc(A + p.d0 * lda, (uint32_t)(p.rows * lda * 4));
        } else {
            p.d0 = 0;
            p.f0 = 0;
            p.rows = 0;
            p.a = mk_rsrc(A, 0u);
        }
        return p;
    };
    int se_run = SE_INIT;

    // compute role: wave w multiplies all 128 rows by features [64 w, 64 w + 64) of the tile
    const int w = t >> 6, l = t & 63, r = l & 31, h = l >> 5;
    const int f_w = w * TFT * 32;
    // the wave's weight fragments: lane l's 16 bytes of fragment (chunk c, part pt, step ks, a) are at
    // Wp + ((c 2 + pt) 2 + ks) Npad 32 + (f0 + f_w + 32 a) 32 + 16 l (fimg order = lane order)
    const int wvoff = f_w * 32 + l * 16;
    const rsrc_t wrsrc = mk_rsrc(Wp, (uint32_t)((int64_t)NCT * Npad * 128));

    float4 dv[2][FPT / 4];
    auto load_a = [&](int set, const TileP& p, int c) {
#pragma unroll
        for (int i = 0; i < FPT / 4; ++i) {
            const u4v u = __builtin_amdgcn_raw_buffer_load_b128(p.a, aoff + 16 * i, c * KC * 4, 0);
            dv[set][i] = make_float4(__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z),
                                     __uint_as_float(u.w));
        }
    };
    // the wave's 4 fragments of step ks of chunk c of the tile at f0, straight into the MFMA operand
    // registers of set ks (one coalesced 1-KiB load each)
    u4v wv[2][TFT][2];
    auto load_w = [&](const TileP& p, int c, int ks) {
#pragma unroll
        for (int pt = 0; pt < 2; ++pt)
#pragma unroll
            for (int a = 0; a < TFT; ++a)
                wv[ks][a][pt] = __builtin_amdgcn_raw_buffer_load_b128(
                    wrsrc, wvoff, (((c * 2 + pt) * 2 + ks) * Npad + p.f0 + 32 * a) * 32, 0);
    };
    // split chunk of register set `set` into stage `buf`; first: a tile's first chunk (fresh row
    // scale, factor 1); last: a tile's last chunk (its final row scale goes to fin[slot])
    auto store = [&](int set, int buf, bool first, bool last, int slot) {
        char* st = lds + buf * ASTAGE;
        float m = 0.f;
#pragma unroll
        for (int i = 0; i < FPT / 4; ++i) m = fmax4_mix(m, dv[set][i]);
        m = fmaxf(m, __shfl_xor(m, 1));
        const int se_old = first ? SE_INIT : se_run, se = next_se(se_old, bexp(m));
        se_run = se;
        const float s = pow2(se);
#pragma unroll
        for (int j = 0; j < FPT; j += 8) {
            const int kl = kp * FPT + j, ks = kl >> 4, pos = kl & 15;
            h8 hv, lv;
            split8_mix(dv[set][j / 4], dv[set][j / 4 + 1], s, hv, lv);
            *reinterpret_cast<h8*>(st + (0 * 2 + ks) * BD * 32 + fimg(rho, pos >> 3)) = hv;
            *reinterpret_cast<h8*>(st + (1 * 2 + ks) * BD * 32 + fimg(rho, pos >> 3)) = lv;
        }
        reinterpret_cast<float*>(st + D_BYTES)[rho] = first ? 1.f : pow2(se - se_old);
        if (last) {
            int rq = threadIdx.x;                     // recomputed here: see the epilogue
            asm volatile("" : "+v"(rq));
            fin[slot * BD + rq / TPR] = pow2(-se);
        }
    };

    f16v acc[TFT][TDT];
    auto rescale = [&](int buf) {
        const float* fac = reinterpret_cast<const float*>(lds + buf * ASTAGE + D_BYTES);
        float f[TDT];
        bool ch = false;
#pragma unroll
        for (int b = 0; b < TDT; ++b) { f[b] = fac[32 * b + r]; ch |= f[b] != 1.f; }
        if (__builtin_amdgcn_ballot_w64(ch) != 0) {
#pragma unroll
            for (int b = 0; b < TDT; ++b)
#pragma unroll
                for (int a = 0; a < TFT; ++a) acc[a][b] *= f[b];
        }
    };
    // one k16 step of the chunk in A stage `buf`; `after_read` runs once the step's fragments are
    // requested (it refills the weight slot)
    auto mfma_ks = [&](int buf, int ks, bool zinit) {
        const char* st = lds + buf * ASTAGE;
        const f16v zero = {};
        h8 wf[TFT][2], df[TDT][2];
#pragma unroll
        for (int pt = 0; pt < 2; ++pt) {
#pragma unroll
            for (int a = 0; a < TFT; ++a) wf[a][pt] = __builtin_bit_cast(h8, wv[ks][a][pt]);
#pragma unroll
            for (int b = 0; b < TDT; ++b)
                df[b][pt] = *reinterpret_cast<const h8*>(st + (pt * 2 + ks) * BD * 32 + fimg(32 * b + r, h));
        }
#pragma unroll
        for (int a = 0; a < TFT; ++a)
#pragma unroll
            for (int b = 0; b < TDT; ++b)
                acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[a][0], df[b][0], zinit ? zero : acc[a][b], 0, 0, 0);
#pragma unroll
        for (int a = 0; a < TFT; ++a)
#pragma unroll
            for (int b = 0; b < TDT; ++b)
                acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[a][0], df[b][1], acc[a][b], 0, 0, 0);
#pragma unroll
        for (int a = 0; a < TFT; ++a)
#pragma unroll
            for (int b = 0; b < TDT; ++b)
                acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[a][1], df[b][0], acc[a][b], 0, 0, 0);
    };
    // C[m][n] = acc * 2^-se(m) * inv_t[n] + bias[n].  Through LDS, as in k_gemm_nt_p: per round b every
    // wave writes its 32 rows x 64 features into a row-major image of the block's 32-row band (pitch
    // BF*4 + 16: conflict-free), then the block stores whole 1-KiB output rows.  The image has LDS of
    // its own (the weights take none), so the rounds need no barrier against the chunk pipeline and
    // the last round none after its stores: the next write to the image is a tile away.  The lane
    // indices are re-derived from an opaque copy of threadIdx.x, as in k_gemm_nt_p.  EPI_VM stores
    // per lane.
    constexpr int EPI_VM = TDT * 8;
    auto epilogue = [&](const TileP& p, int slot) {
        int tq = threadIdx.x;
        asm volatile("" : "+v"(tq));
        const int lq = tq & 63, rq = lq & 31, hq = lq >> 5, wq = tq >> 6;
        const int f_wq = wq * TFT * 32;
        char* const img = lds + IMG_OFF;
        const uint32_t ldc4 = (uint32_t)ldc * 4u;
        const uint32_t nrec = (uint32_t)p.rows * ldc4;
        const rsrc_t crs = mk_rsrc(C + p.d0 * ldc, nrec);
        const float* sc = fin + slot * BD;
        char* const wrow = img + rq * PITCH + (f_wq + 4 * hq) * 4;
#pragma unroll
        for (int b = 0; b < TDT; ++b) {
            const float is = sc[32 * b + rq];
#pragma unroll
            for (int a = 0; a < TFT; ++a) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int n = p.f0 + f_wq + 32 * a + 8 * g + 4 * hq;
                    const float4 it = *reinterpret_cast<const float4*>(inv_l + n);
                    const float4 bb = *reinterpret_cast<const float4*>(bias_l + n);   // -0 without bias
                    float4 o;
                    o.x = acc[a][b][4 * g + 0] * is * it.x + bb.x;
                    o.y = acc[a][b][4 * g + 1] * is * it.y + bb.y;
                    o.z = acc[a][b][4 * g + 2] * is * it.z + bb.z;
                    o.w = acc[a][b][4 * g + 3] * is * it.w + bb.w;
                    if (drop.on()) drop4(drop, p.d0 + 32 * b + rq, n, o);
                    *reinterpret_cast<float4*>(wrow + (32 * a + 8 * g) * 4) = o;
                }
            }
            lds_barrier();
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int ir = wq + 4 * i, c16 = lq;                 // image row, 16-B piece of it
                const u4v v = *reinterpret_cast<const u4v*>(img + ir * PITCH + c16 * 16);
                const int ml = 32 * b + ir;
                const uint32_t off = (p.f0 + 4 * c16 < N) ? (uint32_t)ml * ldc4 + (uint32_t)c16 * 16u : nrec;
                __builtin_amdgcn_raw_buffer_store_b128(v, crs, off, p.f0 * 4, 0);
                // the data registers of a 16-byte store are read over several cycles: keep the next
                // write to them away (see k_gemm_nt_p)
                __builtin_amdgcn_sched_barrier(0);
                asm volatile("s_nop 1" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
            }
            if (b + 1 < TDT) lds_barrier();
        }
    };

    TileP cur = tile_p(tb), nxt = tile_p(tb + 1);
    load_a(0, cur, 0);
    store(0, 0, true, false, 0);
    load_a(1, cur, 1);
    load_w(cur, 0, 0);
    load_w(cur, 0, 1);
    load_a(0, cur, 2);
    {
        // As many stores as a tile's epilogue issues, into an empty range (dropped by the range check):
        // the first tile's step 0 then sees the same operations behind its A loads as every later
        // tile's.  Without them the compiler's wait for chunk 1 at the head of the tile loop is the
        // stricter of its two predecessors', the prologue's, and drains every tile's stores.
        const rsrc_t nul = mk_rsrc(C, 0u);
#pragma unroll
        for (int i = 0; i < EPI_VM; ++i) {
            __builtin_amdgcn_raw_buffer_store_b128(u4v{0u, 0u, 0u, 0u}, nul, 16 * i, 0, 0);   // distinct: none merged
        }
    }
    lds_barrier();
    // step c: chunk c is multiplied out of A stage c&1 and the weight registers, one k16 step after the
    // other; after the first, chunk c+1 (registers, set (c+1)&1) is split into the other stage and
    // W(c+1, 0) is loaded into the registers step 0 has just used; after the second W(c+1, 1) is, then
    // A(c+3) into the freed set — in this order, so that the wait for a weight fragment leaves the A
    // chunk issued behind it in flight.  No load is conditional (see k_gemm_nt_p).  Chunks past the
    // tile's last belong to the next tile.  SK: 0 store chunk c+1 of this tile, 1 the same as the
    // tile's last chunk, 2 the next tile's chunk 0; WN / AN: W(c+1) / A(c+3) come from the next tile.
    typedef std::integral_constant<int, 0> I0;
    typedef std::integral_constant<int, 1> I1;
    typedef std::integral_constant<int, 2> I2;
    auto step = [&](int c, int j, const TileP& cu, const TileP& nx, auto P_, auto Z_, auto SK_, auto WN_, auto AN_) {
        constexpr int P = decltype(P_)::value, SK = decltype(SK_)::value;
        constexpr bool Z = decltype(Z_)::value != 0, WN = decltype(WN_)::value != 0, AN = decltype(AN_)::value != 0;
        if constexpr (!Z) rescale(P);
        mfma_ks(P, 0, Z);
        if constexpr (SK == 2) store(0, 0, true, false, 0);
        else store(P ^ 1, P ^ 1, false, SK == 1, j & 1);
        if constexpr (WN) load_w(nx, c + 1 - NCT, 0);
        else load_w(cu, c + 1, 0);
        __builtin_amdgcn_sched_barrier(0);            // step 1's fragments not loaded under step 0's MFMAs
        mfma_ks(P, 1, false);
        if constexpr (WN) load_w(nx, c + 1 - NCT, 1);
        else load_w(cu, c + 1, 1);
        if constexpr (AN) load_a(P ^ 1, nx, c + 3 - NCT);
        else load_a(P ^ 1, cu, c + 3);
        lds_barrier();
    };
    auto run = [&]() {
        TileP cu = cur, nx = nxt;
        for (int j = 0; tb + j < te; ++j) {
            const TileP nn = tile_p(tb + j + 2);
            step(0, j, cu, nx, I0(), I1(), I0(), I0(), I0());
#pragma unroll
            for (int c = 1; c + 1 <= NCT - 4; c += 2) {
                step(c, j, cu, nx, I1(), I0(), I0(), I0(), I0());
                step(c + 1, j, cu, nx, I0(), I0(), I0(), I0(), I0());
            }
            step(NCT - 3, j, cu, nx, I1(), I0(), I0(), I0(), I1());
            step(NCT - 2, j, cu, nx, I0(), I0(), I1(), I0(), I1());
            step(NCT - 1, j, cu, nx, I1(), I0(), I2(), I1(), I1());
            epilogue(cu, j & 1);
            cu = nx;
            nx = nn;
        }
    };
    run();
}

}  // namespace

bool launch_gemm_nt_p2(const float* A, int64_t lda, int64_t M, int kc, const void* packed, int N, const float* bias,
                       float* C, int64_t ldc, hipStream_t st, const Drop& drop) {
    const int np = (int)gemm_pack_npad(N);
    const u4v* wp = static_cast<const u4v*>(packed);
    const float* inv = reinterpret_cast<const float*>(static_cast<const char*>(packed) + (int64_t)kc * 4 * np * 32);
    constexpr int BD = 128, BF = 256;
    const int nft = (N + BF - 1) / BF;
    const int64_t ntiles = (M + BD - 1) / BD * nft;
    if (ntiles >= (int64_t)1 << 30) return false;
    const int nmax = 2 * device_cu_count();
    const int tpb = (int)((ntiles + nmax - 1) / nmax);
    const int nblk = (int)((ntiles + tpb - 1) / tpb);
    auto kern = kc == 4 ? k_gemm_nt_p2<4> : (kc == 8 ? k_gemm_nt_p2<8> : k_gemm_nt_p2<16>);
    hipLaunchKernelGGL(kern, dim3((unsigned)nblk), dim3(256), 0, st, A, lda, M, wp, np, inv, bias, N, C, ldc, nft,
                       (int)ntiles, tpb, drop);
    return true;
}

}  // namespace sir
