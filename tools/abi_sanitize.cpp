// Host-side AddressSanitizer / UndefinedBehaviorSanitizer run of the C ABI's argument validation
// (SURVEY §5 "ASan/UBSan build of the C-ABI shim").  Built by tools/build_abi_asan.sh with
// sirconv_abi.cpp instrumented (host code only: -fno-gpu-sanitize) and linked against the normally
// built kernel objects; needs no GPU: every call below must be rejected (or be a no-op on empty
// work) before anything is launched.  Exit status 0 = every expectation held and the sanitizers
// reported nothing.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sirconv.h"

static int failures = 0;

static void expect(const char* what, int got, int want, const char* needle = nullptr) {
    const char* msg = sir_last_error();
    const bool ok = got == want && (needle == nullptr || std::strstr(msg, needle) != nullptr);
    if (!ok) {
        std::printf("FAIL %-52s rc=%d (want %d) msg='%s'\n", what, got, want, msg);
        ++failures;
    }
}

int main() {
    if (sir_abi_version() != SIR_ABI_VERSION) {
        std::printf("FAIL abi version\n");
        return 1;
    }
    // host buffers only stand in for device pointers: no call below may dereference them
    std::vector<int32_t> buf(64, 0);
    int32_t* p = buf.data();
    float* f = reinterpret_cast<float*>(buf.data());
    void* v = buf.data();

    // edge passes
    expect("fwd: unknown dtype", sir_edge_agg_fwd(nullptr, nullptr, nullptr, 0, nullptr, 0, 256, 7, nullptr, 256,
                                                  nullptr, 256, nullptr, nullptr, 0, 2, 0.2f, nullptr, 256, nullptr,
                                                  nullptr, nullptr), SIR_EINVAL, "dtype");
    expect("fwd: bad agg", sir_edge_agg_fwd(nullptr, nullptr, nullptr, 0, nullptr, 0, 256, 0, nullptr, 256, nullptr, 256,
                                            nullptr, nullptr, 9, 2, 0.2f, nullptr, 256, nullptr, nullptr, nullptr),
           SIR_EINVAL, "agg");
    expect("fwd: H too large", sir_edge_agg_fwd(p, p, p, 1, nullptr, 0, 4096, 0, v, 4096, v, 4096, nullptr, nullptr, 0, 2,
                                                0.2f, v, 4096, nullptr, nullptr, nullptr), SIR_EINVAL, "H must be");
    expect("fwd: SYM without norms", sir_edge_agg_fwd(p, p, p, 1, nullptr, 0, 16, 0, v, 16, v, 16, nullptr, nullptr, 2, 2,
                                                      0.2f, v, 16, nullptr, nullptr, nullptr), SIR_EINVAL, "SYM");
    expect("fwd: ld < H", sir_edge_agg_fwd(p, p, p, 1, nullptr, 0, 16, 0, v, 8, v, 16, nullptr, nullptr, 0, 2, 0.2f, v, 16,
                                           nullptr, nullptr, nullptr), SIR_EINVAL, "leading");
    expect("fwd: split rows w/o partial", sir_edge_agg_fwd(p, p, p, 1, p, 1, 16, 0, v, 16, v, 16, nullptr, nullptr, 0, 2,
                                                           0.2f, v, 16, nullptr, nullptr, nullptr), SIR_EINVAL, "partial");
    expect("fwd: mask with GELU", sir_edge_agg_fwd(p, p, p, 1, nullptr, 0, 256, 0, v, 256, v, 256, nullptr, nullptr, 0, 3,
                                                   0.f, v, 256, reinterpret_cast<uint64_t*>(v), nullptr, nullptr),
           SIR_EUNSUPPORTED, "sign mask");
    for (int dt = 0; dt < 3; ++dt)
        expect("fwd: empty work is a no-op", sir_edge_agg_fwd(nullptr, nullptr, nullptr, 0, nullptr, 0, 256, dt, nullptr,
                                                               256, nullptr, 256, nullptr, nullptr, 0, 2, 0.2f, nullptr,
                                                               256, nullptr, nullptr, nullptr), SIR_OK);
    expect("dst: NULL G", sir_edge_agg_bwd_dst(p, p, p, 1, nullptr, 0, 64, 0, v, 64, v, 64, nullptr, nullptr, 64, nullptr,
                                               nullptr, 0, 2, 0.2f, v, 64, nullptr, 64, nullptr, nullptr, nullptr), SIR_EINVAL, "G must");
    expect("src: mask without perm", sir_edge_agg_bwd_src(p, p, nullptr, p, 1, nullptr, 0, 256, 0, nullptr, 256, nullptr,
                                                          256, reinterpret_cast<uint64_t*>(v), v, 256, nullptr, nullptr,
                                                          0, 2, 0.2f, v, 256, nullptr, nullptr, nullptr), SIR_EINVAL, "perm");
    expect("bwd (one launch): MEAN refused", sir_edge_agg_bwd(p, p, p, 1, nullptr, 0, p, p, p, p, 1, nullptr, 0, 256, 0,
                                                               reinterpret_cast<uint64_t*>(v), v, 256, nullptr, nullptr, 1,
                                                               2, 0.2f, v, 256, v, 256, nullptr, nullptr, nullptr, nullptr),
           SIR_EUNSUPPORTED, "MEAN");
    expect("bwd (one launch): needs mask", sir_edge_agg_bwd(p, p, p, 1, nullptr, 0, p, p, p, p, 1, nullptr, 0, 256, 0,
                                                             nullptr, v, 256, nullptr, nullptr, 0, 2, 0.2f, v, 256, v, 256,
                                                             nullptr, nullptr, nullptr, nullptr), SIR_EINVAL, "mask");
    // SIREConv edge term
    expect("e_fwd: 16-bit storage", sir_edge_e_agg_fwd(p, p, p, 1, nullptr, 0, 16, 1, v, 16, v, 16, v, 16, 1, nullptr,
                                                       nullptr, nullptr, 0, 2, 0.2f, v, 16, nullptr, nullptr, nullptr),
           SIR_EUNSUPPORTED, "F32");
    expect("e_fwd: GELU", sir_edge_e_agg_fwd(p, p, p, 1, nullptr, 0, 16, 0, v, 16, v, 16, v, 16, 1, nullptr, nullptr,
                                             nullptr, 0, 3, 0.f, v, 16, nullptr, nullptr, nullptr), SIR_EUNSUPPORTED, "RELU");
    expect("e_fwd: NULL Eh", sir_edge_e_agg_fwd(p, p, p, 1, nullptr, 0, 16, 0, v, 16, v, 16, nullptr, 16, 1, nullptr,
                                                nullptr, nullptr, 0, 2, 0.2f, v, 16, nullptr, nullptr, nullptr),
           SIR_EINVAL, "Q/K/Eh");
    expect("e_fwd: lde < H", sir_edge_e_agg_fwd(p, p, p, 1, nullptr, 0, 16, 0, v, 16, v, 16, v, 8, 1, nullptr, nullptr,
                                                nullptr, 0, 2, 0.2f, v, 16, nullptr, nullptr, nullptr), SIR_EINVAL, "leading");
    expect("e_fwd: no edge rows", sir_edge_e_agg_fwd(p, p, p, 1, nullptr, 0, 16, 0, v, 16, v, 16, v, 16, 0, nullptr,
                                                     nullptr, nullptr, 0, 2, 0.2f, v, 16, nullptr, nullptr, nullptr),
           SIR_EINVAL, "n_erows");
    expect("e_fwd: SYM without norms", sir_edge_e_agg_fwd(p, p, p, 1, nullptr, 0, 16, 0, v, 16, v, 16, v, 16, 1, nullptr,
                                                          nullptr, nullptr, 2, 2, 0.2f, v, 16, nullptr, nullptr, nullptr),
           SIR_EINVAL, "SYM");
    expect("e_fwd: empty work is a no-op", sir_edge_e_agg_fwd(nullptr, nullptr, nullptr, 0, nullptr, 0, 256, 0, nullptr,
                                                             256, nullptr, 256, nullptr, 256, 0, nullptr, nullptr, nullptr,
                                                             0, 2, 0.2f, nullptr, 256, nullptr, nullptr, nullptr), SIR_OK);
    expect("e_bwd: MEAN refused", sir_edge_e_bwd(p, p, p, 1, 16, 0, reinterpret_cast<uint64_t*>(v), v, 16, nullptr, nullptr,
                                                 1, 2, 0.2f, nullptr, 1, v, 16, nullptr), SIR_EUNSUPPORTED, "MEAN");
    expect("e_bwd: NULL mask", sir_edge_e_bwd(p, p, p, 1, 16, 0, nullptr, v, 16, nullptr, nullptr, 0, 2, 0.2f, nullptr, 1,
                                              v, 16, nullptr), SIR_EINVAL, "mask/G");
    expect("e_bwd: empty work is a no-op", sir_edge_e_bwd(nullptr, nullptr, nullptr, 0, 256, 0, nullptr, nullptr, 256,
                                                         nullptr, nullptr, 0, 2, 0.2f, nullptr, 0, nullptr, 256, nullptr),
           SIR_OK);
    expect("mask words", (int)sir_mask_words(300, SIR_ACT_LEAKY_RELU), 8);
    expect("mask words (GELU)", (int)sir_mask_words(256, SIR_ACT_GELU), 0);
    // generic path, GraphNorm, plan build
    expect("gather_add: F range", sir_edge_gather_add(p, p, p, 1, 0, f, 1, f, 1, f, 1, nullptr), SIR_EINVAL, "F must");
    expect("segment_sum: norm pairing", sir_segment_sum(p, p, nullptr, p, 1, nullptr, 0, 8, f, 8, f, nullptr, 0, f, 8,
                                                        nullptr, nullptr), SIR_EINVAL, "pairing");
    expect("segment_max: splits w/o ws", sir_segment_max(p, 1, p, 1, 8, f, 8, f, 8, p, 8, nullptr, nullptr, nullptr),
           SIR_EINVAL, "split");
    expect("graph_norm: bad F", sir_graph_norm_fwd(nullptr, 1, 0, f, 1, f, nullptr, nullptr, 1e-5f, f, 1, f, f, nullptr),
           SIR_EINVAL, "shape");
    expect("csr_build: chunk 0", sir_csr_build(nullptr, nullptr, 0, 4, 4, 0, p, p, nullptr, p, p, nullptr, v, 64, nullptr),
           SIR_EINVAL, "chunk");
    expect("csr_build: E >= 2^31", sir_csr_build(nullptr, nullptr, (int64_t)1 << 31, 4, 4, 256, p, p, nullptr, p, p,
                                                 nullptr, v, 64, nullptr), SIR_EINVAL, "2^31");
    expect("csr_build_workspace: negative", (int)sir_csr_build_workspace(-1, 4), -1);
    // GEMMs
    expect("gemm_nt: K % 4", sir_gemm_nt(f, 6, 1, 6, v, 8, nullptr, f, 8, nullptr, nullptr), SIR_EINVAL, "multiples");
    expect("gemm_nt: lda overflow", sir_gemm_nt(f, (int64_t)1 << 21, 1, 16, v, 16, nullptr, f, 16, nullptr, nullptr), SIR_EINVAL,
           "lda too large");
    expect("gemm_tn: ldb overflow", sir_gemm_tn(f, 16, f, (int64_t)1 << 21, 1, 16, 16, f, 16, nullptr, v, 1 << 20,
                                                nullptr), SIR_EINVAL, "too large");
    expect("gemm_pack: N range", sir_gemm_pack(f, 4, 0, 4, 0, v, nullptr), SIR_EINVAL, "N and K");
    expect("gemm_pack_bytes: range", (int)sir_gemm_pack_bytes(70000, 4), 0);
    // fused per-edge dense layer
    expect("mlp_fwd: act2 GELU", sir_edge_mlp_fwd(p, p, p, 1, nullptr, 0, 64, 64, f, 64, f, 64, nullptr, nullptr, 0, 1,
                                                  0.f, SIR_ACT_GELU, v, nullptr, f, 64, nullptr, 64, nullptr, nullptr,
                                                  nullptr), SIR_EUNSUPPORTED, "act2");
    expect("mlp_fwd: MAX needs arg", sir_edge_mlp_fwd(p, p, p, 1, nullptr, 0, 64, 64, f, 64, f, 64, nullptr, nullptr,
                                                      SIR_AGG_MAX, 1, 0.f, 0, v, nullptr, f, 64, nullptr, 64, nullptr,
                                                      nullptr, nullptr), SIR_EINVAL, "arg");
    expect("mlp_bwd_dst: H > 256", sir_edge_mlp_bwd_dst(p, p, p, 1, nullptr, 0, 260, 64, f, 260, f, 260, f, 64, nullptr,
                                                        nullptr, 0, 1, 0.f, 1, v, f, nullptr, f, 260, nullptr, nullptr,
                                                        f, nullptr), SIR_EUNSUPPORTED, "H");
    expect("mlp_bwd_parts: range", (int)sir_edge_mlp_bwd_parts(100, 64, 300), 0);
    expect("mlp_bwd_src: MAX refused", sir_edge_mlp_bwd_src(p, p, p, 1, nullptr, 0, 64, 64, f, 64, f, 64, f, 64, nullptr,
                                                            nullptr, SIR_AGG_MAX, 1, 0.f, 1, v, f, nullptr, f, 64,
                                                            nullptr, nullptr), SIR_EINVAL, "agg");
    expect("mlp_pack_bytes: range", (int)sir_edge_mlp_pack_bytes(1024, 64), 0);
    expect("max_bwd_dst: H > 256", sir_edge_max_bwd_dst(p, p, p, 1, nullptr, 0, 300, 64, f, 300, f, 300, f, 64, p, 64, 1,
                                                        0.f, f, f, 300, nullptr, f, nullptr), SIR_EUNSUPPORTED, "H");
    expect("max_bwd_src: NULL perm", sir_edge_max_bwd_src(p, p, nullptr, p, 1, nullptr, 0, 64, 64, f, 64, f, 64, f, 64,
                                                          p, 64, 1, 0.f, f, f, 64, nullptr, nullptr), SIR_EINVAL, "perm");
    // graph readout
    const int64_t* off = reinterpret_cast<const int64_t*>(buf.data());
    expect("pool_fwd: F out of range", sir_graph_pool_fwd(off, 2, 8, 65537, SIR_POOL_SUM, 0, v, 1 << 17, v, 1 << 17, nullptr,
                                                          nullptr, nullptr), SIR_EINVAL, "sir_graph_pool_fwd: F must be");
    expect("pool_fwd: negative B", sir_graph_pool_fwd(off, -1, 8, 8, SIR_POOL_SUM, 0, v, 8, v, 8, nullptr, nullptr, nullptr),
           SIR_EINVAL, "B and V");
    expect("pool_fwd: ld < F", sir_graph_pool_fwd(off, 2, 8, 8, SIR_POOL_SUM, 0, v, 7, v, 8, nullptr, nullptr, nullptr),
           SIR_EINVAL, "leading");
    expect("pool_fwd: bad op", sir_graph_pool_fwd(off, 2, 8, 8, 3, 0, v, 8, v, 8, p, nullptr, nullptr), SIR_EINVAL, "op must be");
    expect("pool_fwd: bad dtype", sir_graph_pool_fwd(off, 2, 8, 8, SIR_POOL_MEAN, 3, v, 8, v, 8, nullptr, nullptr, nullptr),
           SIR_EINVAL, "dtype must be");
    expect("pool_fwd: NULL P", sir_graph_pool_fwd(off, 2, 8, 8, SIR_POOL_MEAN, 0, v, 8, nullptr, 8, nullptr, nullptr, nullptr),
           SIR_EINVAL, "NULL");
    expect("pool_fwd: MAX needs arg", sir_graph_pool_fwd(off, 2, 8, 8, SIR_POOL_MAX, 1, v, 8, v, 8, nullptr, nullptr, nullptr),
           SIR_EINVAL, "MAX needs arg");
    expect("pool_fwd: work needed", sir_graph_pool_fwd(off, 2, SIR_POOL_SLAB_ROWS + 1, 8, SIR_POOL_MAX, 2, v, 8, v, 8, p, nullptr,
                                                       nullptr), SIR_EINVAL, "work needed");
    expect("pool_bwd: ld < F", sir_graph_pool_bwd(off, 2, 8, 8, SIR_POOL_SUM, 0, v, 8, nullptr, v, 7, nullptr), SIR_EINVAL,
           "sir_graph_pool_bwd: leading");
    expect("pool_bwd: NULL dP", sir_graph_pool_bwd(off, 2, 8, 8, SIR_POOL_SUM, 0, nullptr, 8, nullptr, v, 8, nullptr), SIR_EINVAL,
           "NULL");
    expect("pool_bwd: MAX needs arg", sir_graph_pool_bwd(off, 2, 8, 8, SIR_POOL_MAX, 0, v, 8, nullptr, v, 8, nullptr), SIR_EINVAL,
           "MAX needs arg");
    for (int op = 0; op < 3; ++op) {
        expect("pool_fwd: no graphs is a no-op", sir_graph_pool_fwd(nullptr, 0, 0, 75, op, 0, nullptr, 75, nullptr, 75, nullptr,
                                                                   nullptr, nullptr), SIR_OK);
        expect("pool_bwd: no graphs is a no-op", sir_graph_pool_bwd(nullptr, 0, 0, 75, op, 0, nullptr, 75, nullptr, nullptr, 75,
                                                                   nullptr), SIR_OK);
    }
    expect("pool_work_floats: range", (int)sir_graph_pool_work_floats(8, 2, 65537, SIR_POOL_SUM), -1);
    expect("pool_work_floats: one slab", (int)sir_graph_pool_work_floats(SIR_POOL_SLAB_ROWS, 2, 8, SIR_POOL_MAX), 0);
    // L1 / L2 parameter penalty: params / numel / grads are HOST arrays the validation reads (exactly T entries
    // each, so a read past the end is a sanitizer report); the addresses in them are never dereferenced
    {
        float* const a16 = reinterpret_cast<float*>(0x10000);             // fake device addresses
        std::vector<const float*> P = {a16, a16 + 16, a16 + 33};          // the last: 4-B aligned only
        std::vector<int64_t> N = {4, 0, 7};
        std::vector<float*> G = {a16 + 64, nullptr, a16 + 128};
        float* w = a16 + 1024;
        float* o = a16 + 2048;
        const int64_t wf = sir_param_norms_work_floats(2);
        auto fwd = [&](const std::vector<const float*>& p, const std::vector<int64_t>& n, int64_t T, float* work,
                       int64_t work_floats, float* out2) {
            return sir_param_norms_fwd(p.empty() ? nullptr : p.data(), n.empty() ? nullptr : n.data(), T, work,
                                       work_floats, out2, nullptr);
        };
        auto bwd = [&](const std::vector<const float*>& p, const std::vector<int64_t>& n, const std::vector<float*>& g,
                       int64_t T, const float* g1, const float* g2) {
            return sir_param_norms_bwd(p.empty() ? nullptr : p.data(), n.empty() ? nullptr : n.data(),
                                       g.empty() ? nullptr : g.data(), T, g1, g2, nullptr);
        };
        const std::vector<const float*> noP;
        const std::vector<int64_t> noN;
        const std::vector<float*> noG;
        expect("pn_fwd: negative T", fwd(P, N, -1, w, wf, o), SIR_EINVAL, "sir_param_norms_fwd: T must be");
        expect("pn_fwd: negative count", fwd(P, {4, -1, 7}, 3, w, wf, o), SIR_EINVAL, "negative element count");
        expect("pn_fwd: NULL params", fwd(noP, N, 3, w, wf, o), SIR_EINVAL, "NULL host array");
        expect("pn_fwd: NULL numel", fwd(P, noN, 3, w, wf, o), SIR_EINVAL, "NULL host array");
        expect("pn_fwd: NULL parameter", fwd({a16, nullptr, a16}, {4, 1, 7}, 3, w, wf, o), SIR_EINVAL, "NULL parameter");
        expect("pn_fwd: 2-B aligned", fwd({a16, a16, reinterpret_cast<const float*>(0x10002)}, N, 3, w, wf, o), SIR_EINVAL,
               "4-B aligned");
        expect("pn_fwd: small work", fwd(P, N, 3, w, wf - 1, o), SIR_EINVAL, "work smaller");
        expect("pn_fwd: NULL work", fwd(P, N, 3, nullptr, wf, o), SIR_EINVAL, "work smaller");
        expect("pn_fwd: NULL out2", fwd(P, N, 3, w, wf, nullptr), SIR_EINVAL, "out2");
        expect("pn_fwd: T = 0 is a no-op", fwd(noP, noN, 0, nullptr, 0, nullptr), SIR_OK);
        expect("pn_fwd: all counts 0 is a no-op", fwd({nullptr, a16, reinterpret_cast<const float*>(0x10002)}, {0, 0, 0}, 3,
                                                     nullptr, 0, nullptr), SIR_OK);
        expect("pn_bwd: negative T", bwd(P, N, G, -1, f, f), SIR_EINVAL, "sir_param_norms_bwd: T must be");
        expect("pn_bwd: negative count", bwd(P, {-4, 0, 7}, G, 3, f, f), SIR_EINVAL, "negative element count");
        expect("pn_bwd: NULL grads array", bwd(P, N, noG, 3, f, f), SIR_EINVAL, "NULL host array");
        expect("pn_bwd: NULL parameter", bwd({nullptr, a16, a16}, N, G, 3, f, f), SIR_EINVAL, "NULL parameter");
        expect("pn_bwd: 2-B aligned", bwd({reinterpret_cast<const float*>(0x10002), a16, a16}, N, G, 3, f, f), SIR_EINVAL,
               "4-B aligned");
        expect("pn_bwd: slot not 16-B aligned", bwd(P, N, {a16 + 64, nullptr, a16 + 129}, 3, f, f), SIR_EINVAL,
               "16-B aligned");
        expect("pn_bwd: no gradient at all", bwd(P, N, G, 3, nullptr, nullptr), SIR_EINVAL, "both NULL");
        expect("pn_bwd: T = 0 is a no-op", bwd(noP, noN, noG, 0, nullptr, nullptr), SIR_OK);
        expect("pn_bwd: all counts 0 is a no-op", bwd(P, {0, 0, 0}, {a16 + 1, nullptr, nullptr}, 3, f, nullptr), SIR_OK);
        expect("pn_work_floats: negative", (int)sir_param_norms_work_floats(-1), -1);
        expect("pn_work_floats: no chunks", (int)sir_param_norms_work_floats(0), 2);
        expect("pn_chunk", (int)sir_param_norms_chunk(), SIR_PARAM_NORMS_CHUNK);
        expect("pn_max_tensors", (int)sir_param_norms_max_tensors(), SIR_PARAM_NORMS_MAX_TENSORS);
    }
    // C&S label propagation: f / f2 / f3 stand for Y / Y0 / out (out must differ from Y)
    {
        float* f2 = f + 16;
        float* f3 = f + 32;
        const uint8_t* u8 = reinterpret_cast<const uint8_t*>(buf.data());
        auto lp = [&](int64_t V, int64_t F, const float* Y, int64_t ldy, const float* Y0, const float* norm, int agg, int post,
                      const uint8_t* fixed, const float* Yfix, int64_t ldf, float* out, int64_t ldo, int64_t n_splits,
                      float* partial) {
            return sir_label_prop_step(p, p, p, 8, n_splits ? p : nullptr, n_splits, V, F, Y, ldy, Y0, 8, norm, agg, 0.8f, 0.2f,
                                       post, 0.f, 1.f, fixed, Yfix, ldf, out, ldo, partial, nullptr);
        };
        const int S = SIR_AGG_SYM, N0 = SIR_LP_POST_NONE, FX = SIR_LP_POST_FIX;
        expect("label_prop: F out of range", lp(8, 65537, f, 1 << 17, f2, f, S, N0, nullptr, nullptr, 0, f3, 1 << 17, 0, nullptr),
               SIR_EINVAL, "sir_label_prop_step: F must be");
        expect("label_prop: negative V", lp(-1, 8, f, 8, f2, f, S, N0, nullptr, nullptr, 0, f3, 8, 0, nullptr), SIR_EINVAL,
               "sir_label_prop_step: V must be");
        expect("label_prop: ld < F", lp(8, 8, f, 7, f2, f, S, N0, nullptr, nullptr, 0, f3, 8, 0, nullptr), SIR_EINVAL, "leading");
        expect("label_prop: ldf < F", lp(8, 8, f, 8, f2, f, S, FX, u8, f2, 7, f3, 8, 0, nullptr), SIR_EINVAL, "leading");
        expect("label_prop: bad agg", lp(8, 8, f, 8, f2, f, 3, N0, nullptr, nullptr, 0, f3, 8, 0, nullptr), SIR_EINVAL, "agg must be");
        expect("label_prop: SYM needs norm", lp(8, 8, f, 8, f2, nullptr, S, N0, nullptr, nullptr, 0, f3, 8, 0, nullptr), SIR_EINVAL,
               "SYM needs norm");
        expect("label_prop: bad post", lp(8, 8, f, 8, f2, f, S, 3, nullptr, nullptr, 0, f3, 8, 0, nullptr), SIR_EINVAL, "post must be");
        expect("label_prop: FIX needs fixed", lp(8, 8, f, 8, f2, f, S, FX, nullptr, f2, 8, f3, 8, 0, nullptr), SIR_EINVAL, "FIX needs");
        expect("label_prop: FIX needs Yfix", lp(8, 8, f, 8, f2, f, S, FX, u8, nullptr, 8, f3, 8, 0, nullptr), SIR_EINVAL, "FIX needs");
        expect("label_prop: NULL Y", lp(8, 8, nullptr, 8, f2, f, S, N0, nullptr, nullptr, 0, f3, 8, 0, nullptr), SIR_EINVAL, "NULL");
        expect("label_prop: NULL out", lp(8, 8, f, 8, f2, f, S, N0, nullptr, nullptr, 0, nullptr, 8, 0, nullptr), SIR_EINVAL, "NULL");
        expect("label_prop: partial needed", lp(8, 8, f, 8, f2, f, S, N0, nullptr, nullptr, 0, f3, 8, 1, nullptr), SIR_EINVAL,
               "split rows need");
        expect("label_prop: out == Y", lp(8, 8, f, 8, f2, f, S, N0, nullptr, nullptr, 0, f, 8, 0, nullptr), SIR_EINVAL,
               "sir_label_prop_step: out must not alias Y");
        for (int agg = 0; agg < 3; ++agg)
            expect("label_prop: no rows is a no-op", sir_label_prop_step(nullptr, nullptr, nullptr, 0, nullptr, 0, 0, 40, nullptr, 40,
                                                                        nullptr, 40, nullptr, agg, 0.8f, 0.2f, N0, 0.f, 1.f, nullptr,
                                                                        nullptr, 0, nullptr, 40, nullptr, nullptr), SIR_OK);
    }
    // layer dropout fused into the norms
    const double* dd = reinterpret_cast<const double*>(buf.data());
    const double nan = std::nan("");
    const sir_dropout_t drop_ok = {5, 0.2, nullptr}, drop_nan = {5, nan, nullptr};
    expect("bn_drop_fwd: NaN p", sir_batch_norm_act_drop_fwd(f, 8, 4, 8, dd, dd, f, f, 2, 0.2f, nullptr, 0, f, 8, &drop_nan,
                                                             nullptr), SIR_EINVAL, "sir_batch_norm_act_drop_fwd: dropout p is NaN");
    expect("bn_drop_bwd: NaN p", sir_batch_norm_act_drop_bwd(f, 8, f, 8, 4, 8, dd, dd, f, f, 2, 0.2f, 1, f, 8, f, f, f, &drop_nan,
                                                             nullptr), SIR_EINVAL, "sir_batch_norm_act_drop_bwd: dropout p is NaN");
    expect("ln_drop_fwd: NaN p", sir_layer_norm_act_drop_fwd(f, 8, 4, 8, f, f, 1e-5f, 2, 0.2f, nullptr, 0, f, 8, f, f, &drop_nan,
                                                             nullptr), SIR_EINVAL, "sir_layer_norm_act_drop_fwd: dropout p is NaN");
    expect("ln_drop_bwd: NaN p", sir_layer_norm_act_drop_bwd(f, 8, f, 8, 4, 8, f, f, f, f, 2, 0.2f, f, 8, f, f, 8, &drop_nan,
                                                             nullptr), SIR_EINVAL, "sir_layer_norm_act_drop_bwd: dropout p is NaN");
    expect("gn_drop_fwd: NaN p", sir_graph_norm_act_drop_fwd(off, 2, 8, f, 8, f, f, f, 1e-5f, 2, 0.2f, nullptr, 0, f, 8, f, f,
                                                             &drop_nan, nullptr), SIR_EINVAL, "sir_graph_norm_act_drop_fwd: dropout p is NaN");
    expect("gn_drop_bwd: NaN p", sir_graph_norm_act_drop_bwd(off, 2, 8, f, 8, f, 8, f, f, f, f, f, 2, 0.2f, f, 8, f, f, f,
                                                             &drop_nan, nullptr), SIR_EINVAL, "sir_graph_norm_act_drop_bwd: dropout p is NaN");
    expect("bn_drop_fwd: ld < N", sir_batch_norm_act_drop_fwd(f, 7, 4, 8, dd, dd, f, f, 2, 0.2f, nullptr, 0, f, 8, &drop_ok, nullptr),
           SIR_EINVAL, "sir_batch_norm_act_drop_fwd: leading");
    expect("ln_drop_fwd: N out of range", sir_layer_norm_act_drop_fwd(f, 4096, 4, 1025, f, f, 1e-5f, 2, 0.2f, nullptr, 0, f, 4096, f,
                                                                      f, &drop_ok, nullptr), SIR_EINVAL, "N must be in [1, 1024]");
    expect("gn_drop_bwd: NULL dX", sir_graph_norm_act_drop_bwd(off, 2, 8, f, 8, f, 8, f, f, f, f, f, 2, 0.2f, nullptr, 8, f, f, f,
                                                               &drop_ok, nullptr), SIR_EINVAL, "NULL");
    expect("bn_drop_fwd: empty work is a no-op", sir_batch_norm_act_drop_fwd(nullptr, 8, 0, 8, nullptr, nullptr, nullptr, nullptr, 2,
                                                                            0.2f, nullptr, 0, nullptr, 8, &drop_ok, nullptr), SIR_OK);
    expect("gn_drop_fwd: no graphs is a no-op", sir_graph_norm_act_drop_fwd(nullptr, 0, 8, nullptr, 8, nullptr, nullptr, nullptr, 1e-5f,
                                                                           2, 0.2f, nullptr, 0, nullptr, 8, nullptr, nullptr, &drop_ok,
                                                                           nullptr), SIR_OK);
    std::printf("%s: %d failure(s)\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}
