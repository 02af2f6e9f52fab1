// Kernel self-test entries of the LM decode kernels (kernels/lm_decode.hip, kernels/lm_decode_q.hip;
// include/acestep_mi355x_selftest.h): one
// launch_lm_* call on host buffers, blocking, so that tests/lm_kernel_cases.py can compare each kernel with a float64
// reference of the same operation.  Built into libacestep_mi355x_selftest.so (Makefile target `selftest`) and, on top
// of tests/host/lm_emul.cpp, into the LM host library (tests/lmhostlib.py); not part of runtime/selftest.cpp, which the
// host library of tests/hostlib.py compiles without the LM kernels.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../../include/acestep_mi355x_selftest.h"
#include "../kernels.h"
#include "devmem.h"
#include "quant.h"

namespace {

using acemi::DevMem;

constexpr int D = 128;

// what check_post (lm_decode.hip) refuses, plus a row stride that holds the heads
bool post_args_ok(int B, int hq, int hkv, int capacity, int ld, const void* qkv, const void* k_norm, const void* cs,
                  const void* sn, const void* kc, const void* vc, const void* km) {
    return B >= 1 && B <= acemi::LM_MAX_BATCH && hq >= 1 && hkv >= 1 && capacity >= 1 &&
           (int64_t)ld >= (int64_t)(hq + 2 * hkv) * D && qkv && k_norm && cs && sn && kc && vc && km;
}

// ggml block rows -> the loader's planes (Loader::from_blocks) on the device
struct DevPlanes {
    DevMem q, s;
    int fmt;
    DevPlanes(acemi::quant::QType t, const std::vector<uint8_t>& qp, const std::vector<float>& sp)
        : q(qp.data(), qp.size()), s(sp.data(), sp.size() * 4),
          fmt(t == acemi::quant::Q8_0 ? acemi::WF_Q8_0 : (t == acemi::quant::Q4_K ? acemi::WF_Q4_K : acemi::WF_Q6_K)) {}
};

// qtype: the quant::QType ids 1 Q8_0, 2 Q4_K, 3 Q6_K (as ace_mi_quantize takes them)
bool plane_type_ok(int qtype, int K) {
    const auto t = static_cast<acemi::quant::QType>(qtype);
    return qtype >= 1 && qtype <= 3 && acemi::quant::has_planes(t) && K >= acemi::quant::block_values(t) &&
           K % acemi::quant::block_values(t) == 0;
}

}  // namespace

extern "C" {

ace_ggml_status ace_mi_kernel_lm_skinny_q(int32_t qtype, int32_t epi, int32_t B, int32_t N, int32_t w_rows, int32_t K,
                                          int32_t ldx, int32_t ldy, const uint16_t* x, const uint8_t* blocks,
                                          float* y_f32, uint16_t* y_u16, int32_t* chain) {
    using namespace acemi;
    if (!plane_type_ok(qtype, K) || B < 1 || B > LM_MAX_BATCH || N < 1 || w_rows < N || ldx % 8 != 0 || ldx < K || !x ||
        !blocks)
        return ACE_GGML_ERR_INVALID_ARG;
    const bool swiglu = epi == LM_EPI_SWIGLU;
    if (swiglu ? (N % 32 != 0 || !y_u16) : ((epi != LM_EPI_STORE && epi != LM_EPI_RESID) || !y_f32))
        return ACE_GGML_ERR_INVALID_ARG;
    if (ldy < (swiglu ? N / 2 : N)) return ACE_GGML_ERR_INVALID_ARG;
    try {
        const auto t = static_cast<quant::QType>(qtype);
        std::vector<uint8_t> qp(quant::q_plane_bytes(t, w_rows, K));
        std::vector<float> sp(quant::s_plane_floats(t, w_rows, K));
        quant::to_planes(t, blocks, w_rows, K, qp.data(), sp.data());
        const size_t ny = (size_t)B * ldy * (swiglu ? 2 : 4);
        void* y = swiglu ? (void*)y_u16 : (void*)y_f32;
        DevPlanes dW(t, qp, sp);
        DevMem dx(x, (size_t)B * ldx * 2), dy(y, ny);
        WeightView W;
        W.fmt = dW.fmt;
        W.q = dW.q.p;
        W.s = dW.s.as<float>();
        W.ld = K;
        launch_lm_skinny_q(dx.as<uint16_t>(), ldx, B, W, N, K, epi, swiglu ? nullptr : dy.as<float>(),
                           swiglu ? dy.as<uint16_t>() : nullptr, ldy, nullptr);
        ACEMI_HIP(hipDeviceSynchronize());
        dy.to_host(y, ny);
        if (chain) *chain = lm_skinny_q_chain(dW.fmt, K);
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "ace_mi_kernel_lm_skinny_q: %s\n", ex.what());
        return ACE_GGML_ERR;
    }
    return ACE_GGML_OK;
}

ace_ggml_status ace_mi_kernel_lm_embed_q(int32_t qtype, int32_t n, int32_t vocab, int32_t H, const uint8_t* blocks,
                                         const int32_t* ids, float* out) {
    using namespace acemi;
    if (!plane_type_ok(qtype, H) || n < 1 || vocab < 1 || !blocks || !ids || !out) return ACE_GGML_ERR_INVALID_ARG;
    try {
        const auto t = static_cast<quant::QType>(qtype);
        std::vector<uint8_t> qp(quant::q_plane_bytes(t, vocab, H));
        std::vector<float> sp(quant::s_plane_floats(t, vocab, H));
        quant::to_planes(t, blocks, vocab, H, qp.data(), sp.data());
        const size_t no = (size_t)n * H * 4;
        DevPlanes dW(t, qp, sp);
        DevMem di(ids, (size_t)n * 4), dout(out, no);
        launch_lm_embed_q(dW.fmt, dW.q.p, dW.s.as<float>(), di.as<int32_t>(), n, vocab, H, dout.as<float>(), nullptr);
        ACEMI_HIP(hipDeviceSynchronize());
        dout.to_host(out, no);
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "ace_mi_kernel_lm_embed_q: %s\n", ex.what());
        return ACE_GGML_ERR;
    }
    return ACE_GGML_OK;
}

ace_ggml_status ace_mi_kernel_lm_skinny(int32_t act_type, int32_t epi, int32_t B, int32_t N, int32_t K, int32_t ldx,
                                        int32_t ldy, const uint16_t* x, const uint16_t* W, float* y_f32,
                                        uint16_t* y_u16) {
    using namespace acemi;
    if ((act_type != 0 && act_type != 1) || B < 1 || B > LM_MAX_BATCH || N < 1 || K < 8 || K % 8 != 0 || ldx % 8 != 0 ||
        ldx < K || !x || !W)
        return ACE_GGML_ERR_INVALID_ARG;
    const bool swiglu = epi == LM_EPI_SWIGLU;
    if (swiglu ? (N % 32 != 0 || !y_u16) : ((epi != LM_EPI_STORE && epi != LM_EPI_RESID) || !y_f32))
        return ACE_GGML_ERR_INVALID_ARG;
    if (ldy < (swiglu ? N / 2 : N)) return ACE_GGML_ERR_INVALID_ARG;
    try {
        const size_t ny = (size_t)B * ldy * (swiglu ? 2 : 4);
        void* y = swiglu ? (void*)y_u16 : (void*)y_f32;
        DevMem dx(x, (size_t)B * ldx * 2), dW(W, (size_t)N * K * 2), dy(y, ny);
        launch_lm_skinny(act_type == 1 ? ActType::F16 : ActType::BF16, dx.as<uint16_t>(), ldx, B, dW.as<uint16_t>(), N, K,
                         epi, swiglu ? nullptr : dy.as<float>(), swiglu ? dy.as<uint16_t>() : nullptr, ldy, nullptr);
        ACEMI_HIP(hipDeviceSynchronize());
        dy.to_host(y, ny);
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "ace_mi_kernel_lm_skinny: %s\n", ex.what());
        return ACE_GGML_ERR;
    }
    return ACE_GGML_OK;
}

ace_ggml_status ace_mi_kernel_lm_embed(int32_t fmt, int32_t n, int32_t vocab, int32_t H, const uint16_t* table,
                                       const int32_t* ids, float* out) {
    using namespace acemi;
    if ((fmt != 0 && fmt != 1) || n < 1 || vocab < 1 || H < 8 || H % 8 != 0 || !table || !ids || !out)
        return ACE_GGML_ERR_INVALID_ARG;
    try {
        const size_t no = (size_t)n * H * 4;
        DevMem dt(table, (size_t)vocab * H * 2), di(ids, (size_t)n * 4), dout(out, no);
        launch_lm_embed(dt.p, fmt, di.as<int32_t>(), n, vocab, H, dout.as<float>(), nullptr);
        ACEMI_HIP(hipDeviceSynchronize());
        dout.to_host(out, no);
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "ace_mi_kernel_lm_embed: %s\n", ex.what());
        return ACE_GGML_ERR;
    }
    return ACE_GGML_OK;
}

ace_ggml_status ace_mi_kernel_lm_qkv_post(int32_t B, int32_t hq, int32_t hkv, int32_t capacity, int32_t pos, int32_t ld,
                                          float eps, const float* qkv, const float* q_norm, const float* k_norm,
                                          const float* rope_cos, const float* rope_sin, const int32_t* mask_new,
                                          float* q_out, uint16_t* k_cache, uint16_t* v_cache, int32_t* key_mask) {
    using namespace acemi;
    if (!post_args_ok(B, hq, hkv, capacity, ld, qkv, k_norm, rope_cos, rope_sin, k_cache, v_cache, key_mask) || !q_norm ||
        !q_out || pos < 0 || pos >= capacity)
        return ACE_GGML_ERR_INVALID_ARG;
    try {
        const size_t nc = (size_t)B * hkv * capacity * D * 2, nm = (size_t)B * capacity * 4, nq = (size_t)B * hq * D * 4;
        DevMem dqkv(qkv, (size_t)B * ld * 4), dqn(q_norm, D * 4), dkn(k_norm, D * 4);
        DevMem dcs(rope_cos, (size_t)capacity * 64 * 4), dsn(rope_sin, (size_t)capacity * 64 * 4);
        DevMem dmn(mask_new, (size_t)B * 4), dq(q_out, nq), dk(k_cache, nc), dv(v_cache, nc), dm(key_mask, nm);
        LmQkvPostArgs a;
        a.qkv = dqkv.as<float>();
        a.ld = ld;
        a.hq = hq;
        a.hkv = hkv;
        a.q_norm = dqn.as<float>();
        a.k_norm = dkn.as<float>();
        a.rope_cos = dcs.as<float>();
        a.rope_sin = dsn.as<float>();
        a.eps = eps;
        a.q_out = dq.as<float>();
        a.k_cache = dk.as<uint16_t>();
        a.v_cache = dv.as<uint16_t>();
        a.key_mask = dm.as<int32_t>();
        a.capacity = capacity;
        a.pos = pos;
        a.mask_new = mask_new ? dmn.as<int32_t>() : nullptr;
        launch_lm_qkv_post(a, B, nullptr);
        ACEMI_HIP(hipDeviceSynchronize());
        dq.to_host(q_out, nq);
        dk.to_host(k_cache, nc);
        dv.to_host(v_cache, nc);
        dm.to_host(key_mask, nm);
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "ace_mi_kernel_lm_qkv_post: %s\n", ex.what());
        return ACE_GGML_ERR;
    }
    return ACE_GGML_OK;
}

ace_ggml_status ace_mi_kernel_lm_prefill_kv(int32_t B, int32_t hq, int32_t hkv, int32_t capacity, int32_t n, int32_t ld,
                                            float eps, float* qkv, const float* k_norm, const float* rope_cos,
                                            const float* rope_sin, const int32_t* mask, uint16_t* k_cache,
                                            uint16_t* v_cache, int32_t* key_mask) {
    using namespace acemi;
    if (!post_args_ok(B, hq, hkv, capacity, ld, qkv, k_norm, rope_cos, rope_sin, k_cache, v_cache, key_mask) || n < 1 ||
        n > capacity || n > 65535)
        return ACE_GGML_ERR_INVALID_ARG;
    try {
        const size_t nc = (size_t)B * hkv * capacity * D * 2, nm = (size_t)B * capacity * 4;
        const size_t nx = (size_t)B * n * ld * 4;
        DevMem dqkv(qkv, nx), dkn(k_norm, D * 4);
        DevMem dcs(rope_cos, (size_t)capacity * 64 * 4), dsn(rope_sin, (size_t)capacity * 64 * 4);
        DevMem dmask(mask, (size_t)B * n * 4), dk(k_cache, nc), dv(v_cache, nc), dm(key_mask, nm);
        LmQkvPostArgs a;
        a.qkv = dqkv.as<float>();
        a.ld = ld;
        a.hq = hq;
        a.hkv = hkv;
        a.q_norm = dkn.as<float>();  // unused by the prefill fill; check_post wants a pointer
        a.k_norm = dkn.as<float>();
        a.rope_cos = dcs.as<float>();
        a.rope_sin = dsn.as<float>();
        a.eps = eps;
        a.k_cache = dk.as<uint16_t>();
        a.v_cache = dv.as<uint16_t>();
        a.key_mask = dm.as<int32_t>();
        a.capacity = capacity;
        launch_lm_prefill_kv(a, B, n, mask ? dmask.as<int32_t>() : nullptr, nullptr);
        ACEMI_HIP(hipDeviceSynchronize());
        dqkv.to_host(qkv, nx);
        dk.to_host(k_cache, nc);
        dv.to_host(v_cache, nc);
        dm.to_host(key_mask, nm);
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "ace_mi_kernel_lm_prefill_kv: %s\n", ex.what());
        return ACE_GGML_ERR;
    }
    return ACE_GGML_OK;
}

ace_ggml_status ace_mi_kernel_lm_select(const ace_mi_kernel_lm_select_args* g) {
    using namespace acemi;
    if (!g || g->B < 1 || g->B > LM_MAX_BATCH || g->vocab < 1 || g->ld_logits < g->vocab || !g->logits || !g->tokens ||
        g->token_stride < 1)
        return ACE_GGML_ERR_INVALID_ARG;
    const bool mix = g->cfg_scale > 1.0f;
    if (mix && g->B % 2 != 0) return ACE_GGML_ERR_INVALID_ARG;
    const int S = mix ? g->B / 2 : g->B;
    if ((g->allowed && g->n_allowed < 1) || g->stop_id >= g->vocab || (g->force_stop && g->stop_id < 0) ||
        (g->temperature > 0.0f && !g->uniform) || (g->seen && g->ld_seen < g->vocab) ||
        (g->processed && g->ld_processed < g->vocab))
        return ACE_GGML_ERR_INVALID_ARG;
    try {
        const int n_cand = lm_select_candidates(g->vocab, g->n_allowed, g->allowed != nullptr);
        const size_t n_seen = (size_t)S * g->ld_seen, n_tok = (size_t)S * g->token_stride * 4;
        const size_t n_proc = (size_t)S * g->ld_processed * 4;
        DevMem dl(g->logits, (size_t)g->B * g->ld_logits * 4), da(g->allowed, (size_t)g->n_allowed * 4);
        DevMem du(g->uniform, (size_t)S * 4), ds(g->seen, n_seen), dt(g->tokens, n_tok);
        DevMem dn(g->next_ids, (size_t)g->B * 4), dd(g->done, (size_t)(1 + S) * 4), dp(g->processed, n_proc);
        DevMem dw(lm_select_work_floats(S, n_cand) * 4);
        LmSelectArgs a;
        a.logits = dl.as<float>();
        a.ld_logits = g->ld_logits;
        a.vocab = g->vocab;
        a.S = S;
        a.cfg_scale = g->cfg_scale;
        a.allowed = g->allowed ? da.as<int32_t>() : nullptr;
        a.n_allowed = g->allowed ? g->n_allowed : 0;
        a.stop_id = g->stop_id < 0 ? -1 : g->stop_id;
        a.block_stop = g->block_stop != 0;
        a.force_stop = g->force_stop != 0;
        a.n_emitted = g->n_emitted;
        a.pre_temperature = g->pre_temperature;
        a.repetition_penalty = g->repetition_penalty;
        a.seen = g->seen ? ds.as<uint8_t>() : nullptr;
        a.ld_seen = g->ld_seen;
        a.top_k = g->top_k;
        a.top_p = g->top_p;
        a.temperature = g->temperature;
        a.uniform = g->uniform ? du.as<float>() : nullptr;
        a.work = dw.as<float>();
        a.tokens = dt.as<int32_t>();
        a.token_stride = g->token_stride;
        a.next_ids = g->next_ids ? dn.as<int32_t>() : nullptr;
        a.done = g->done ? dd.as<int32_t>() : nullptr;
        a.processed = g->processed ? dp.as<float>() : nullptr;
        a.ld_processed = g->ld_processed;
        launch_lm_select(a, nullptr);
        ACEMI_HIP(hipDeviceSynchronize());
        dt.to_host(g->tokens, n_tok);
        if (g->seen) ds.to_host(g->seen, n_seen);
        if (g->next_ids) dn.to_host(g->next_ids, (size_t)g->B * 4);
        if (g->done) dd.to_host(g->done, (size_t)(1 + S) * 4);
        if (g->processed) dp.to_host(g->processed, n_proc);
        if (g->chains) lm_select_chains(n_cand, g->chains);
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "ace_mi_kernel_lm_select: %s\n", ex.what());
        return ACE_GGML_ERR;
    }
    return ACE_GGML_OK;
}

ace_ggml_status ace_mi_kernel_lm_cache_fanout(int32_t layers, int32_t G, int32_t S, int32_t hkv, int32_t cap_src,
                                              int32_t cap_dst, int32_t n, uint16_t* k_src, uint16_t* v_src,
                                              int32_t* mask_src, uint16_t* k_dst, uint16_t* v_dst, int32_t* mask_dst) {
    using namespace acemi;
    if ((G != 1 && G != 2) || S < 1 || G * S > LM_MAX_BATCH || layers < 1 || hkv < 1 || (int64_t)layers * hkv > 65535 ||
        n < 1 || n > cap_src || n > cap_dst || !k_src || !v_src || !mask_src || !k_dst || !v_dst || !mask_dst)
        return ACE_GGML_ERR_INVALID_ARG;
    try {
        const size_t ns = (size_t)layers * G * hkv * cap_src * D * 2, ms = (size_t)G * cap_src * 4;
        const size_t nd = (size_t)layers * G * S * hkv * cap_dst * D * 2, md = (size_t)G * S * cap_dst * 4;
        DevMem dks(k_src, ns), dvs(v_src, ns), dms(mask_src, ms), dkd(k_dst, nd), dvd(v_dst, nd), dmd(mask_dst, md);
        LmFanoutArgs a;
        a.k_src = dks.as<uint16_t>();
        a.v_src = dvs.as<uint16_t>();
        a.mask_src = dms.as<int32_t>();
        a.k_dst = dkd.as<uint16_t>();
        a.v_dst = dvd.as<uint16_t>();
        a.mask_dst = dmd.as<int32_t>();
        a.layers = layers;
        a.G = G;
        a.S = S;
        a.hkv = hkv;
        a.cap_src = cap_src;
        a.cap_dst = cap_dst;
        a.n = n;
        launch_lm_cache_fanout(a, nullptr);
        ACEMI_HIP(hipDeviceSynchronize());
        dks.to_host(k_src, ns);
        dvs.to_host(v_src, ns);
        dms.to_host(mask_src, ms);
        dkd.to_host(k_dst, nd);
        dvd.to_host(v_dst, nd);
        dmd.to_host(mask_dst, md);
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "ace_mi_kernel_lm_cache_fanout: %s\n", ex.what());
        return ACE_GGML_ERR;
    }
    return ACE_GGML_OK;
}

ace_ggml_status ace_mi_kernel_lm_attention(int32_t out_type, int32_t B, int32_t hq, int32_t hkv, int32_t capacity,
                                           int32_t nk, float scale, const float* q, const uint16_t* k_cache,
                                           const uint16_t* v_cache, const int32_t* key_mask, uint16_t* out_u16) {
    using namespace acemi;
    if ((out_type != 0 && out_type != 1) || B < 1 || B > LM_MAX_BATCH || hkv < 1 || hq < 1 || hq % hkv != 0 || nk < 1 ||
        nk > capacity || !q || !k_cache || !v_cache || !key_mask || !out_u16)
        return ACE_GGML_ERR_INVALID_ARG;
    const int rep = hq / hkv;
    if (rep != 1 && rep != 2 && rep != 4) return ACE_GGML_ERR_INVALID_ARG;
    try {
        const size_t nc = (size_t)B * hkv * capacity * D * 2, no = (size_t)B * hq * D * 2;
        DevMem dq(q, (size_t)B * hq * D * 4), dk(k_cache, nc), dv(v_cache, nc), dm(key_mask, (size_t)B * capacity * 4);
        DevMem dout(out_u16, no), dpart(lm_attn_part_floats(B, hq, nk) * 4);
        LmAttnArgs a;
        a.q = dq.as<float>();
        a.k_cache = dk.as<uint16_t>();
        a.v_cache = dv.as<uint16_t>();
        a.key_mask = dm.as<int32_t>();
        a.hkv = hkv;
        a.capacity = capacity;
        a.nk = nk;
        a.scale = scale;
        a.out = dout.as<uint16_t>();
        a.part = dpart.as<float>();
        launch_lm_attention(out_type == 1 ? ActType::F16 : ActType::BF16, a, B, hq, nullptr);
        ACEMI_HIP(hipDeviceSynchronize());
        dout.to_host(out_u16, no);
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "ace_mi_kernel_lm_attention: %s\n", ex.what());
        return ACE_GGML_ERR;
    }
    return ACE_GGML_OK;
}

}  // extern "C"
