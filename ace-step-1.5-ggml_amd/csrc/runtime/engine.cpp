// DiT forward orchestration: the ggml graph of ace_dit::forward_dit
// (acestep_dit_model.cpp:1316-1560) as a fixed sequence of fused gfx950 kernels.
#include "engine.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <tuple>
#include <type_traits>

#include "../kernels/attn_probs_host.h"  // empty under hipcc; the host build's launch_attn_probs
#include "lora.h"
#include "operands.h"

namespace acemi {

DitEngine::DitEngine(int device) : device_(device) {
    // DiT: the f32-class f8c mode by default (hi/lo operands for Q.K and P.V, the correction products as block-scaled
    // e4m3 MFMAs): ggml runs both products in F32 (acestep_dit_model.cpp:1238-1251) and f8c is the fastest mode that
    // meets the literal 1e-3 one-layer bound at full width (DESIGN.md "Parity"); the condition / text encoders keep
    // the hi/lo fp16 `f32` default
    const AttnPrecision prec = attn_precision_from_env(AttnPrecision::F8C);
    set_attn_precision(prec);
    const char* u = std::getenv("ACE_MI_UNFUSED_PREP");
    fused_prep_ = !(u && u[0] && u[0] != '0');
    if (const char* pf = std::getenv("ACE_MI_WEIGHT_PREFETCH")) prefetch_blocks_ = std::max(0, std::atoi(pf));
    qact_ = quant_act_from_env();
    // TEST ONLY (self-test library builds): ACE_MI_TEST_FAULT, runtime/test_hooks.cpp
    if (!test_fault_from_env(fault_.layer, fault_.row, fault_.col, fault_.amp)) fault_.layer = -1;
}

DitEngine::~DitEngine() {  // (every DevBuf, and images_, frees itself)
    if (pf_stream_) {
        (void)hipStreamSynchronize(pf_stream_);
        (void)hipStreamDestroy(pf_stream_);
    }
    if (pf_ev_) (void)hipEventDestroy(pf_ev_);
    if (pf_done_) (void)hipEventDestroy(pf_done_);
    if (ev0_) (void)hipEventDestroy(ev0_);
    if (ev1_) (void)hipEventDestroy(ev1_);
    free_lora();
}

// Side-stream sweep of the 16-bit images layer li's GEMMs will read (ACE_MI_WEIGHT_PREFETCH), ordered after the work
// already queued on s; the forward joins the side stream before it returns.
void DitEngine::prefetch_layer(int li, hipStream_t s) {
    if (!pf_stream_) {
        ACEMI_HIP(hipStreamCreateWithFlags(&pf_stream_, hipStreamNonBlocking));
        ACEMI_HIP(hipEventCreateWithFlags(&pf_ev_, hipEventDisableTiming));
        ACEMI_HIP(hipEventCreateWithFlags(&pf_done_, hipEventDisableTiming));
    }
    ensure(pf_sink_, 256);
    const LayerViews lw = images_.views(li);
    const auto ws = model_.layers[li].block_weights();
    const void* ptrs[N_BLOCK_WEIGHTS];
    size_t bytes[N_BLOCK_WEIGHTS];
    int n = 0;
    for (int i = 0; i < N_BLOCK_WEIGHTS; ++i) {
        if (weight_quantized(lw[i].fmt) || !lw[i].q) continue;  // bf16 / fp16 images only
        ptrs[n] = lw[i].q;
        bytes[n++] = WeightImages::wbytes(*ws[i]);
    }
    if (n == 0) return;
    ACEMI_HIP(hipEventRecord(pf_ev_, s));
    ACEMI_HIP(hipStreamWaitEvent(pf_stream_, pf_ev_, 0));
    launch_prefetch(ptrs, bytes, n, prefetch_blocks_, get<unsigned>(pf_sink_), pf_stream_);
}

// Device table of every layer's cross-attention k-norm weights (PrepArgs::k_norm_layers), built once.
const float* const* DitEngine::cross_norm_table() {
    const size_t n = model_.layers.size();
    if (!knorm_tab_.p || knorm_tab_n_ != n) {
        std::vector<const float*> h(n);
        for (size_t i = 0; i < n; ++i) h[i] = model_.layers[i].ck_norm;
        ensure(knorm_tab_, n * sizeof(const float*));
        ACEMI_HIP(hipMemcpy(knorm_tab_.p, h.data(), n * sizeof(const float*), hipMemcpyHostToDevice));
        knorm_tab_n_ = n;
    }
    return static_cast<const float* const*>(knorm_tab_.p);
}

void DitEngine::set_profiling(bool on) {
    profiling_ = on;
    if (on && !ev0_) {
        ACEMI_HIP(hipEventCreate(&ev0_));
        ACEMI_HIP(hipEventCreate(&ev1_));
    }
}

void DitEngine::reset_times() { times_ = KernelTimes{}; }

void DitEngine::tic(hipStream_t s) {
    if (profiling_) ACEMI_HIP(hipEventRecord(ev0_, s));
}

void DitEngine::toc(const char* name, hipStream_t s) {
    if (!profiling_) return;
    ACEMI_HIP(hipEventRecord(ev1_, s));
    ACEMI_HIP(hipEventSynchronize(ev1_));
    float ms = 0.f;
    ACEMI_HIP(hipEventElapsedTime(&ms, ev0_, ev1_));
    for (size_t i = 0; i < times_.names.size(); ++i) {
        if (times_.names[i] == name) {
            times_.ms[i] += ms;
            times_.count[i] += 1;
            return;
        }
    }
    times_.names.emplace_back(name);
    times_.ms.push_back(ms);
    times_.count.push_back(1);
}

void DitEngine::prepare_shape(int B, int Np, int L) {
    const DitConfig& c = model_.cfg;
    const int H = c.hidden, I = c.intermediate, D = c.head_dim;
    const int64_t M = (int64_t)B * Np;
    const int64_t Npad = round_up(Np, 128);
    const int qd = c.hq * D, kd = c.hkv * D;
    const size_t act = 2;
    ensure(a0_, M * c.patch * c.in_channels * act * 3);                 // x3 layout for F32 proj_in
    ensure(act2_, M * std::max(I, 3 * H) * act);                        // also the x3 proj_out input
    ensure(x_, M * H * 4);
    ensure(act_, M * std::max(H, qd) * act);
    ensure(attn_, M * qd * act);
    ensure(qkv_, M * (qd + 2 * kd) * 4);
    ensure(qh_, (size_t)2 * B * c.hq * Npad * D * 2);   // hi + lo planes
    ensure(kh_, (size_t)2 * B * c.hkv * Npad * D * 2);
    ensure(vt_, (size_t)2 * B * c.hkv * D * Npad * 2);
    ensure(kbias_, (size_t)B * Npad * 4);
    ensure(attn_part_, attn_part_floats((size_t)B * Np * c.hq) * 4);
    if (L > 0) {
        const int64_t Lpad = round_up(L, 64);
        const int64_t Me = (int64_t)B * L;
        ensure(enc_act_, Me * H * act);
        ensure(encp_, Me * H * act);
        ensure(ckv_, Me * c.layers * 2 * kd * 4);  // all layers' cross k|v (one GEMM)
        const void* kc_old = kc_.p;
        const void* vc_old = vc_.p;
        ensure(kc_, (size_t)2 * c.layers * B * c.hkv * Lpad * D * 2);
        ensure(vc_, (size_t)2 * c.layers * B * c.hkv * D * Lpad * 2);
        if (kc_.p != kc_old || vc_.p != vc_old) cross_key_.valid = false;
        ensure(kbias_c_, (size_t)B * Lpad * 4);
    }
    ensure(freq_, (size_t)B * 256 * 4);
    ensure(freq_act_, (size_t)B * 256 * act);
    ensure(th_, (size_t)B * H * 4);
    ensure(th_act_, (size_t)B * H * act);
    ensure(temb_t_, (size_t)B * H * 4);
    ensure(temb_r_, (size_t)B * H * 4);
    ensure(temb_act_, (size_t)B * H * act);
    ensure(proj_, (size_t)B * 6 * H * 4);
    ensure(mods_, (size_t)c.layers * B * 6 * H * 4);
    ensure(outmod_, (size_t)B * 2 * H * 4);
}

void DitEngine::forward(const ForwardIO& io, hipStream_t s) {
    if (qact_)
        walk<true>(io, s);
    else
        walk<false>(io, s);
}

// The one walk of the DiT graph.  QACT = false is the product: bf16 activation rows (Row = uint16_t) through
// launch_gemm on the staged / imaged weights, attention at the engine's precision.  QACT = true is the
// ggml-arithmetic parity mode (engine_qact.cpp): f32 rows in one buffer (every Row* below is qf_), each linear through
// qlinear on the resident weights, attention at the f32 precision with f32 output.  The modes differ only in the
// `if constexpr` arms and the five small lambdas below; everything else is one sequence.
template <bool QACT>
void DitEngine::walk(const ForwardIO& io, hipStream_t s) {
    using Row = std::conditional_t<QACT, float, uint16_t>;
    const DitModel& m = model_;
    const DitConfig& c = m.cfg;
    const ActType at = m.act;
    const int B = io.B, T = io.T, L = io.L > 0 ? io.L : 0;
    const int P = c.patch, H = c.hidden, I = c.intermediate, D = c.head_dim;
    const int Np = (T + P - 1) / P;
    const int M = (int)((int64_t)B * Np);
    const int Npad = (int)round_up(Np, 128);
    const int Lpad = (int)round_up(std::max(L, 1), 64);
    const AttnDims dims{B, c.hq, c.hkv, D, Np, Npad, c.eps};
    const AttnPlanes planes = QACT ? AttnPlanes{true, true, false} : AttnPlanes{attn_split_, attn_pv_split_, attn_f8_};
    const int qd = dims.qd(), kd = dims.kd();
    const int64_t kc_layer = (int64_t)B * c.hkv * Lpad * D;  // one layer's cross K (or V^T) plane
    const int64_t kc_plane = c.layers * kc_layer;            // lo plane offset of kc_ / vc_
    ACEMI_CHECK(B >= 1 && B <= 8, "batch must be 1..8 per GPU");
    ACEMI_CHECK(T >= 1, "seq_len must be > 0");
    ACEMI_CHECK(L == 0 || io.enc != nullptr, "encoder_hidden_states required when enc_len > 0");
    const int kin = m.proj_in_w.k_mult(), kout = m.proj_out_w.k_mult();
    if constexpr (QACT)
        ACEMI_CHECK(kin == 1 && kout == 1,
                    "quantized-activation mode: F32 proj_in / proj_out (GGUF) are not supported");
    prepare_shape(B, Np, L);
    rope_.ensure(Np, c.head_dim, c.rope_theta, s);
    // parity: the cross K/V planes below are this mode's (f32 precision), not the cached ones
    if constexpr (QACT) cross_key_.valid = false;

    int n_layers = c.layers;
    if (io.max_layers > 0) n_layers = std::min(n_layers, io.max_layers);
    // capture request: every listed layer must run and own a cross block; an early exit ends the walk at the last one
    const bool capture = io.n_pairs > 0;
    const bool early_exit = capture && io.early_exit;
    if (capture) {
        ACEMI_CHECK(io.layers && io.heads && io.probs, "capture: null layers / heads / probs");
        ACEMI_CHECK(L > 0, "capture: enc_len must be > 0");
        int last = 0;
        for (int j = 0; j < io.n_pairs; ++j) {
            ACEMI_CHECK(io.layers[j] >= 0 && io.layers[j] < n_layers,
                        "capture: layer " + std::to_string(io.layers[j]) + " is outside the " +
                            std::to_string(n_layers) + " layers this forward runs");
            ACEMI_CHECK(m.layers[io.layers[j]].cross,
                        "capture: layer " + std::to_string(io.layers[j]) + " has no cross-attention block");
            ACEMI_CHECK(io.heads[j] >= 0 && io.heads[j] < c.hq,
                        "capture: head " + std::to_string(io.heads[j]) + " is outside [0, " + std::to_string(c.hq) + ")");
            last = std::max(last, io.layers[j]);
        }
        if (early_exit) n_layers = last + 1;
    }
    ACEMI_CHECK(early_exit || io.out != nullptr, "output buffer is null");
    // the product reads weight images (weight_images.h); parity multiplies the resident weights: nothing staged
    images_.begin_forward(QACT ? 0 : n_layers, io.reuse_stage, s);
    const int Kin = kin * P * c.in_channels;

    float* x = get<float>(x_);
    Row *a0, *act, *attn, *act2;  // packed input, norm output, attention output, SwiGLU output
    float* attn_f32 = nullptr;
    if constexpr (QACT) {
        ensure(qf_, (size_t)M * std::max({H, qd, I, Kin}) * 4);
        a0 = act = attn = act2 = attn_f32 = get<float>(qf_);
    } else {
        a0 = get<uint16_t>(a0_);
        act = get<uint16_t>(act_);
        attn = get<uint16_t>(attn_);
        act2 = get<uint16_t>(act2_);
    }

    // ---- the seam
    auto weight = [&](const DevWeight& w) { return QACT ? w.view() : images_.matrix(w, s); };
    auto linear = [&](const Row* in, int ld, int rows, const WeightView& w, int N, int K, const GemmEpilogue& e,
                      const char* name) {
        if constexpr (QACT) {
            qlinear(in, ld, rows, w, N, K, e, name, s);  // (times itself)
        } else {
            tic(s);
            launch_gemm(in, ld, w, rows, N, K, e, s);
            toc(name, s);
        }
    };
    // a projection feeding attention, with the operand prep `pa` in its epilogue (product: qkv_gemm's choice)
    auto project = [&](const WeightView& w, int N, const PrepArgs& pa, const char* name) {
        if constexpr (QACT)
            qlinear(act, H, M, w, N, H, epi_qkv_prep(pa), name, s);
        else
            qkv_gemm(act, w, M, N, pa, name, s);
    };
    auto norm = [&](ActType t, const float* w, const float* scale, const float* shift, int64_t stride, Row* out,
                    bool x3) {
        tic(s);
        if constexpr (QACT)
            launch_rmsnorm_mod_f32(x, M, H, w, scale, shift, stride, Np, c.eps, out, s);
        else
            launch_rmsnorm_mod(t, x, M, H, w, scale, shift, stride, Np, c.eps, out, s, x3);
        toc("rmsnorm_mod", s);
    };
    auto attention = [&](const uint16_t* k, const uint16_t* vt, const float* kbias, int nk, int nk_pad,
                         int64_t kv_plane, int window, const char* name) {
        tic(s);
        launch_attention(at,
                         attn_args(dims, planes, get<uint16_t>(qh_), k, vt, kbias, nk, nk_pad, kv_plane, window, false,
                                   get<float>(attn_part_), get<uint16_t>(attn_), attn_f32),
                         s);
        toc(name, s);
    };

    // ---- input pack + proj_in (:1343-1382)
    tic(s);
    if constexpr (QACT)
        launch_pack_input_f32(io.hidden, io.context, B, T, Np, P, c.audio_dim, c.ctx_dim(), a0, s);
    else
        launch_pack_input(m.proj_in_w.act(), io.hidden, io.context, B, T, Np, P, c.audio_dim, c.ctx_dim(), a0, s,
                          kin == 3);
    toc("pack_input", s);
    linear(a0, Kin, M, weight(m.proj_in_w), H, Kin, epi_store_f32(x, H, m.proj_in_b), "gemm_proj_in");

    // ---- timestep embeddings (:1416-1424, timestep_forward :1286-1308), or the sampler's precomputed rows, and the
    // key masks.  Parity leaves both out of the profile: its timestep linears time themselves (tic / toc do not nest)
    {
        if constexpr (!QACT) tic(s);
        const float* proj = io.ts_proj;
        const float* temb_t = io.ts_temb_t;
        const float* temb_r = io.ts_temb_r;
        if (!proj) {
            timestep_embed(io.t, io.r, B, get<float>(proj_), get<float>(temb_t_), get<float>(temb_r_), s);
            proj = get<float>(proj_);
            temb_t = get<float>(temb_t_);
            temb_r = get<float>(temb_r_);
        }
        launch_layer_mods(m.tables, proj, n_layers, B, H, get<float>(mods_), s);
        launch_out_mods(m.out_table, temb_t, temb_r, B, H, get<float>(outmod_), s);
        if constexpr (!QACT) {
            toc("timestep", s);
            tic(s);
        }
        launch_key_bias(io.mask, B, T, P, Np, Npad, get<float>(kbias_), s);
        if (L > 0) launch_key_bias(io.enc_mask, B, L, 1, L, Lpad, get<float>(kbias_c_), s);
        if constexpr (!QACT) toc("key_bias", s);
    }

    // ---- condition embedder (:1384-1414) + per-layer cross K/V (constant over the layer loop; the product reuses
    // the previous forward's on request)
    const bool reuse = !QACT && io.reuse_cross && cross_key_.valid && cross_key_.B == B && cross_key_.L == L &&
                       cross_key_.layers >= n_layers && cross_key_.enc == io.enc;
    if (L > 0 && !reuse) {
        const int Me = (int)((int64_t)B * L);
        Row* encp;
        if constexpr (QACT) {
            ensure(encf_, (size_t)Me * H * 4);
            encp = get<float>(encf_);
            qlinear(io.enc, H, Me, m.cond_w.view(), H, H, epi_store_f32(encp, H, m.cond_b), "gemm_condition", s);
        } else {
            cross_key_ = CrossKey{true, B, L, n_layers, io.enc};
            encp = get<uint16_t>(encp_);
            tic(s);
            launch_to_act(at, io.enc, (int64_t)Me * H, false, get<uint16_t>(enc_act_), s);
            launch_gemm(get<uint16_t>(enc_act_), H, weight(m.cond_w), Me, H, H, epi_store_act(encp, H, m.cond_b), s);
            toc("gemm_condition", s);
        }
        // one GEMM for every layer's cross k|v when the weights are fused: ckv [Me][n_layers*2kd]; the product then
        // re-lays all of them out in one launch too, parity runs one prep per layer
        const bool fused = m.w_ckv_all.q != nullptr;
        const bool one_prep = fused && !QACT;
        const int ld_ckv = fused ? n_layers * 2 * kd : 2 * kd;
        float* ckv = get<float>(ckv_);
        for (int li = 0; li < n_layers; ++li) {
            const DevLayer& ly = m.layers[li];
            if (li == 0 || !fused)  // (fused: the first n_layers layers)
                linear(encp, H, Me, weight(fused ? m.w_ckv_all : ly.w_ckv), ld_ckv, H, epi_store_f32(ckv, ld_ckv),
                       "gemm_cross_kv");
            tic(s);
            launch_attn_prep(cross_kv_prep(dims, planes, L, Lpad, ckv + (fused ? (size_t)li * 2 * kd : 0), ld_ckv,
                                           ly.ck_norm, get<uint16_t>(kc_) + li * kc_layer,
                                           get<uint16_t>(vc_) + li * kc_layer, kc_plane, n_layers,
                                           one_prep ? cross_norm_table() : nullptr),
                             s);
            toc("attn_prep", s);
            if (one_prep) break;
        }
    }

    const float* mods = get<float>(mods_);
    const int64_t mstride = 6LL * H;  // per item within a layer
    std::vector<int> cap_heads, cap_slots;  // capture: one layer's heads and their places in io.probs

    for (int li = 0; li < n_layers; ++li) {  // :1466-1535
        const DevLayer& ly = m.layers[li];
        if (images_.expanding()) tic(s);
        const LayerViews lw = images_.layer(li, s);  // (expands the layer's images first when this forward does)
        if (images_.expanding()) toc("dequant_stage", s);
        if (!QACT && prefetch_blocks_ > 0 && li + 1 < n_layers && !images_.expanding()) prefetch_layer(li + 1, s);
        const float* lm = mods + (size_t)li * B * 6 * H;
        const float* shift_msa = lm + 0 * H;
        const float* scale_msa = lm + 1 * H;
        const float* gate_msa = lm + 2 * H;
        const float* c_shift = lm + 3 * H;
        const float* c_scale = lm + 4 * H;
        const float* c_gate = lm + 5 * H;

        // self-attention block: the QKV projection with QK-RMSNorm, RoPE and the attention re-layout in its epilogue
        norm(at, ly.self_norm, scale_msa, shift_msa, mstride, act, false);
        project(lw[BW_QKV], qd + 2 * kd,
                self_prep(dims, planes, nullptr, 0, ly.sq_norm, ly.sk_norm, rope_.cos(), rope_.sin(),
                          get<uint16_t>(qh_), get<uint16_t>(kh_), get<uint16_t>(vt_)),
                "gemm_qkv");
        attention(get<uint16_t>(kh_), get<uint16_t>(vt_), io.mask ? get<float>(kbias_) : nullptr, Np, Npad,
                  dims.k_plane(), ly.sliding ? std::max(c.sliding_window, 0) : 0,  // padding keys: masked in-kernel
                  ly.sliding ? "attn_self_sliding" : "attn_self_full");
        linear(attn, qd, M, lw[BW_O], H, qd, epi_resid_gated(x, H, gate_msa, mstride, Np), "gemm_o");
        if (!QACT && li == fault_.layer)  // TEST ONLY: the injected fault must reach the norm that follows
            launch_fault_tile(x, H, M, fault_.row, fault_.col, fault_.amp, s);

        // cross-attention block (:1502-1520): no AdaLN, no gate, no RoPE
        if (ly.cross && L > 0) {
            norm(at, ly.cross_norm, nullptr, nullptr, 0, act, false);
            project(lw[BW_CQ], qd, cross_q_prep(dims, planes, ly.cq_norm, get<uint16_t>(qh_)), "gemm_cross_q");
            if (capture) {  // this layer's pairs in one launch: qh_ holds its cross queries until the next layer's QKV
                cap_heads.clear();
                cap_slots.clear();
                for (int j = 0; j < io.n_pairs; ++j)
                    if (io.layers[j] == li) {
                        cap_heads.push_back(io.heads[j]);
                        cap_slots.push_back(j);
                    }
                if (!cap_heads.empty()) {
                    tic(s);
                    launch_attn_probs(attn_prob_args(dims, get<uint16_t>(qh_), get<uint16_t>(kc_) + li * kc_layer,
                                                     io.enc_mask ? get<float>(kbias_c_) : nullptr, L, Lpad,
                                                     (int)cap_heads.size(), cap_heads.data(), cap_slots.data(),
                                                     io.probs),
                                      s);
                    toc("attn_probs", s);
                }
                if (early_exit && li + 1 == n_layers) break;  // nothing after the last capture is read
            }
            attention(get<uint16_t>(kc_) + li * kc_layer, get<uint16_t>(vc_) + li * kc_layer,
                      io.enc_mask ? get<float>(kbias_c_) : nullptr, L, Lpad, kc_plane, 0, "attn_cross");
            linear(attn, qd, M, lw[BW_CO], H, qd, epi_resid(x, H), "gemm_cross_o");
        }

        // MLP block (:1522-1534); parity's SwiGLU rows overwrite their own (already quantized) input
        norm(at, ly.mlp_norm, c_scale, c_shift, mstride, act, false);
        linear(act, H, M, lw[BW_GU], 2 * I, H, epi_swiglu(act2, I), "gemm_gate_up");
        linear(act2, I, M, lw[BW_DOWN], H, I, epi_resid_gated(x, H, c_gate, mstride, Np), "gemm_down");
    }

    // ---- output head (:1537-1559)
    if (!early_exit) {
        const float* om = get<float>(outmod_);
        Row* head_in = kout == 3 ? act2 : act;  // act2_ is sized for M x 3H too
        norm(m.proj_out_w.act(), m.norm_out, om + H, om, 2LL * H, head_in, kout == 3);
        linear(head_in, kout * H, M, weight(m.proj_out_w), P * c.audio_dim, kout * H,
               epi_proj_out(io.out, m.proj_out_b, Np, T, c.audio_dim, P), "gemm_proj_out");
    }
    images_.end_forward(s);
    if (pf_stream_) {  // the side stream's sweeps end before anything ordered after this forward on s
        ACEMI_HIP(hipEventRecord(pf_done_, pf_stream_));
        ACEMI_HIP(hipStreamWaitEvent(s, pf_done_, 0));
    }
}

void DitEngine::timestep_embed(const float* t, const float* r, int rows, float* proj, float* temb_t, float* temb_r,
                               hipStream_t s) {
    if (qact_) {
        timestep_embed_qact(t, r, rows, proj, temb_t, temb_r, s);
        return;
    }
    const DitModel& m = model_;
    const int H = m.cfg.hidden;
    const float log_max = std::log(10000.0f);
    ensure(freq_, (size_t)8 * 256 * 4);
    ensure(th_, (size_t)8 * H * 4);
    float* freq = get<float>(freq_);
    float* th = get<float>(th_);
    // rows are independent: chunks of up to 8 (the GEMV kernel's row limit), the same arithmetic per row
    for (int r0 = 0; r0 < rows; r0 += 8) {
        const int n = std::min(8, rows - r0);
        float* pr = proj + (size_t)r0 * 6 * H;
        for (int e = 0; e < 2; ++e) {
            float* temb = (e == 0 ? temb_t : temb_r) + (size_t)r0 * H;
            launch_timestep_freq(t + r0, e == 0 ? nullptr : r + r0, n, 256, 1000.0f, log_max, freq, s);
            const ActType ta = m.te[e].act;
            // each linear rounds its f32 input to the weight type itself (launch_gemv_f32 = to_act + gemv)
            launch_gemv_f32(ta, freq, false, n, m.te[e].w1, H, 256, m.te[e].b1, true, false, th, s);
            launch_gemv_f32(ta, th, false, n, m.te[e].w2, H, H, m.te[e].b2, false, false, temb, s);
            launch_gemv_f32(ta, temb, true, n, m.te[e].wp, 6 * H, H, m.te[e].bp, false, e == 1, pr, s);
        }
    }
}

DitEngine::TimestepRows DitEngine::precompute_timesteps(const float* t, const float* r, int rows, hipStream_t s) {
    const int H = model_.cfg.hidden;
    ensure(ts_proj_, (size_t)rows * 6 * H * 4);
    ensure(ts_temb_t_, (size_t)rows * H * 4);
    ensure(ts_temb_r_, (size_t)rows * H * 4);
    tic(s);
    timestep_embed(t, r, rows, get<float>(ts_proj_), get<float>(ts_temb_t_), get<float>(ts_temb_r_), s);
    toc("timestep_precompute", s);
    return TimestepRows{get<float>(ts_proj_), get<float>(ts_temb_t_), get<float>(ts_temb_r_)};
}

// A projection of the product walk feeding attention: with EPI_QKV_PREP the GEMM epilogue writes the attention
// operands of `prep` directly; the unfused path (ACE_MI_UNFUSED_PREP=1, A/B and debugging) stores f32 to qkv_
// and runs attn_prep over it.
void DitEngine::qkv_gemm(const uint16_t* act, const WeightView& w, int M, int N, PrepArgs prep, const char* name,
                         hipStream_t s) {
    const int H = model_.cfg.hidden;
    prep.src = fused_prep_ ? nullptr : get<float>(qkv_);
    prep.ld = fused_prep_ ? 0 : N;
    tic(s);
    launch_gemm(act, H, w, M, N, H, fused_prep_ ? epi_qkv_prep(prep) : epi_store_f32(get<float>(qkv_), N), s);
    toc(name, s);
    if (fused_prep_) return;
    tic(s);
    launch_attn_prep(prep, s);
    toc("attn_prep", s);
}

void DitEngine::encode(const EncodeIO& io, hipStream_t s) {
    const DitModel& m = model_;
    const DitConfig& c = m.cfg;
    const int H = c.hidden;
    const int B = io.B, n = io.n;
    ACEMI_CHECK(io.proj && io.proj->q, "encoder: input projection not loaded");
    ACEMI_CHECK(B >= 1 && n >= 1 && io.in && io.out, "encoder: bad arguments");
    ACEMI_CHECK(io.proj->rows == H && io.proj->k_mult() == 1, "encoder: projection weight shape mismatch");
    const int in_dim = io.proj->cols;
    const int64_t M = (int64_t)B * n;
    ensure(ein_, (size_t)M * in_dim * 2);
    uint16_t* ein = get<uint16_t>(ein_);
    launch_to_act(io.proj->act(), io.in, M * in_dim, false, ein, s);
    GemmEpilogue pe = epi_store_f32(nullptr, H, io.proj_b);
    if (!io.enc) {  // projection only (the text projector)
        ACEMI_CHECK(!io.first_only, "encoder: first_only needs an encoder");
        pe.c_f32 = io.out;
        launch_gemm(ein, in_dim, io.proj->view(), (int)M, H, in_dim, pe, s);
        return;
    }
    const DevEncoder& e = *io.enc;
    int n_layers = (int)e.layers.size();
    if (io.max_layers >= 0) n_layers = std::min(n_layers, io.max_layers);
    BlockShape sh;
    sh.hidden = H;
    sh.hq = c.hq;
    sh.hkv = c.hkv;
    sh.head_dim = c.head_dim;
    sh.intermediate = e.intermediate;
    sh.eps = c.eps;
    sh.rope_theta = c.rope_theta;
    sh.sliding_window = c.sliding_window;
    pe.c_f32 = cond_.x(M, H);
    launch_gemm(ein, in_dim, io.proj->view(), (int)M, H, in_dim, pe, s);  // x = in W^T + b
    // all-ones token mask (acestep_ggml.cpp:1692 / :1838), bidirectional
    cond_.run(sh, e.layers, n_layers, e.act, B, n, nullptr, false, s);
    cond_.finish(sh, e.norm, B, n, io.first_only, io.out, s);
}

void DitEngine::probe_gemm(int which, int M, int iters, hipStream_t s) {
    const DitModel& m = model_;
    const DitConfig& c = m.cfg;
    const int H = c.hidden, I = c.intermediate;
    prepare_shape(1, M, 0);
    const DevLayer& ly = m.layers[0];
    for (int it = 0; it < iters; ++it) {
        tic(s);
        if (which == 0) {
            launch_gemm(get<uint16_t>(act_), H, ly.w_gu.view(), M, 2 * I, H, epi_swiglu(get<uint16_t>(act2_), I), s);
            toc("probe_gemm_gate_up", s);
        } else {
            launch_gemm(get<uint16_t>(act2_), I, ly.w_down.view(), M, H, I,
                        epi_resid_gated(get<float>(x_), H, get<float>(mods_), 0, M), s);
            toc("probe_gemm_down", s);
        }
    }
}

// ---------------------------------------------------------------- LoRA adapters (engine.h)
void DitEngine::free_lora() {
    images_.adapted.clear();
    images_.adapter_on = false;
    lora_ab_.release();
    lora_a_.clear();
    lora_b_.clear();
    lora_.reset();
    lora_scale_ = 0.f;
    lora_merge_ms_ = 0.0;
}

DitEngine::LoraInfo DitEngine::lora_info() const {
    LoraInfo i;
    if (!lora_) return i;
    i.loaded = true;
    i.scale = lora_scale_;
    i.lora_alpha = lora_->lora_alpha;
    i.min_rank = lora_->min_rank;
    i.max_rank = lora_->max_rank;
    i.modules = (int)lora_->modules.size();
    for (const auto& kv : images_.adapted)
        if (kv.second.p) {
            ++i.images;
            i.image_bytes += kv.second.bytes;
        }
    i.merge_ms = lora_merge_ms_;
    return i;
}

// The images of the current adapter at the current scale, always from the base weights.  Everything that was
// computed from the previous views goes: the cached cross K/V and the staged slots (an adapted matrix's slot is left
// unwritten, so the next forward expands them again).
void DitEngine::rebuild_lora_images(hipStream_t s) {
    ACEMI_HIP(hipDeviceSynchronize());  // a forward in flight (on any stream) reads the current views
    cross_key_.valid = false;
    images_.invalidate();
    images_.adapter_on = false;
    lora_merge_ms_ = 0.0;
    if (!lora_ || lora_scale_ == 0.f) return;

    const DitModel& m = model_;
    const DitConfig& c = m.cfg;
    const int H = c.hidden, I = c.intermediate, qd = c.hq * c.head_dim, kd = c.hkv * c.head_dim;
    std::map<std::tuple<int, int, int>, int> index;
    for (size_t i = 0; i < lora_->modules.size(); ++i) {
        const LoraModule& lm = lora_->modules[i];
        index[std::make_tuple(lm.layer, lm.block, lm.proj)] = (int)i;
    }
    struct Slot {  // one module's rows inside a fused matrix
        int map, row_off, half, rows_mod, mod;
    };
    std::vector<std::pair<const DevWeight*, std::vector<Slot>>> mats;
    auto slot = [&](std::vector<Slot>& v, int li, int block, int proj, int map, int row_off, int half, int rows_mod) {
        const auto it = index.find(std::make_tuple(li, block, proj));
        v.push_back(Slot{map, row_off, half, rows_mod, it == index.end() ? -1 : it->second});
    };
    const bool ckv_fused = m.w_ckv_all.q != nullptr;
    std::vector<Slot> ckv_all;
    for (int li = 0; li < (int)m.layers.size(); ++li) {
        const DevLayer& ly = m.layers[li];
        std::vector<Slot> v;
        slot(v, li, LORA_SELF, LORA_Q, LORA_ROWS_PLAIN, 0, 0, qd);
        slot(v, li, LORA_SELF, LORA_K, LORA_ROWS_PLAIN, qd, 0, kd);
        slot(v, li, LORA_SELF, LORA_V, LORA_ROWS_PLAIN, qd + kd, 0, kd);
        mats.emplace_back(&ly.w_qkv, v);
        v.clear();
        slot(v, li, LORA_SELF, LORA_O, LORA_ROWS_PLAIN, 0, 0, H);
        mats.emplace_back(&ly.w_o, v);
        v.clear();
        slot(v, li, LORA_CROSS, LORA_Q, LORA_ROWS_PLAIN, 0, 0, qd);
        mats.emplace_back(&ly.w_cq, v);
        v.clear();
        std::vector<Slot>& kv = ckv_fused ? ckv_all : v;
        const int r0 = ckv_fused ? li * 2 * kd : 0;  // layer li's k|v rows inside w_ckv_all
        slot(kv, li, LORA_CROSS, LORA_K, LORA_ROWS_PLAIN, r0, 0, kd);
        slot(kv, li, LORA_CROSS, LORA_V, LORA_ROWS_PLAIN, r0 + kd, 0, kd);
        if (!ckv_fused) mats.emplace_back(&ly.w_ckv, v);
        v.clear();
        slot(v, li, LORA_CROSS, LORA_O, LORA_ROWS_PLAIN, 0, 0, H);
        mats.emplace_back(&ly.w_co, v);
        v.clear();
        slot(v, li, LORA_MLP, LORA_GATE, LORA_ROWS_INTERLEAVE, 0, 0, I);
        slot(v, li, LORA_MLP, LORA_UP, LORA_ROWS_INTERLEAVE, 0, 1, I);
        mats.emplace_back(&ly.w_gu, v);
        v.clear();
        slot(v, li, LORA_MLP, LORA_DOWN, LORA_ROWS_PLAIN, 0, 0, H);
        mats.emplace_back(&ly.w_down, v);
    }
    if (ckv_fused) mats.emplace_back(&m.w_ckv_all, ckv_all);

    // allocate first (ensure() synchronises the device), then launch everything in stream order
    std::vector<LoraMergeJob> jobs;
    std::vector<std::pair<const DevWeight*, uint16_t*>> expand;
    for (const auto& mt : mats) {
        const DevWeight& w = *mt.first;
        bool any = false;
        for (const Slot& sl : mt.second) any = any || sl.mod >= 0;
        if (!any) continue;
        ACEMI_CHECK(w.q && w.fmt != WF_F32X3, "lora: the targeted weight is not a 16-bit or block-format matrix");
        DevBuf& buf = images_.adapted[w.q];
        ensure(buf, WeightImages::wbytes(w));
        uint16_t* img = static_cast<uint16_t*>(buf.p);
        const bool quantized = weight_quantized(w.fmt);
        if (quantized) expand.emplace_back(&w, img);
        for (size_t k = 0; k < mt.second.size(); ++k) {
            const Slot& sl = mt.second[k];
            LoraMergeJob j;
            j.fmt = quantized ? WF_BF16 : w.fmt;
            j.base = quantized ? img : static_cast<const uint16_t*>(w.q);
            j.out = img;
            j.ld_base = j.ld_out = w.cols;
            j.cols = w.cols;
            j.map = sl.map;
            j.row_off = sl.row_off;
            j.half = sl.half;
            if (sl.map == LORA_ROWS_INTERLEAVE) {  // the job's range is the whole matrix; the other half is copied by
                j.row0 = 0;                        // its own job, or by this one when it has no adapter
                j.rows = w.rows;
                const Slot& other = mt.second[k ^ 1];
                j.copy_rest = other.mod < 0;
                if (sl.mod < 0) continue;
            } else {
                j.row0 = sl.row_off;
                j.rows = sl.rows_mod;
                j.copy_rest = sl.mod < 0;  // a module without an adapter: its rows are copied through
            }
            if (sl.mod >= 0) {
                const LoraModule& lm = lora_->modules[sl.mod];
                ACEMI_CHECK(lm.in == w.cols && lm.out == sl.rows_mod, "lora: module shape does not match the weight");
                j.A = lora_a_[sl.mod];
                j.B = lora_b_[sl.mod];
                j.r = lm.r;
                j.rows_mod = sl.rows_mod;
                j.eff = lora_scale_ * lm.unit;
            } else if (quantized) {
                continue;  // in place: the rows are in the image already
            }
            jobs.push_back(j);
        }
    }
    ACEMI_HIP(hipDeviceSynchronize());
    const auto t0 = std::chrono::steady_clock::now();
    for (const auto& e : expand) WeightImages::expand(*e.first, e.second, s);
    launch_lora_merge(jobs.data(), (int)jobs.size(), s);
    ACEMI_HIP(hipStreamSynchronize(s));
    lora_merge_ms_ = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    images_.adapter_on = true;
}

void DitEngine::load_lora(const std::string& dir, float scale, int max_layers, hipStream_t s) {
    if (qact_)
        throw Unsupported("lora: the quantized-activation parity mode (ACE_MI_QUANT_ACT=q8) multiplies the block "
                          "weights themselves and cannot run an adapter");
    auto ad = std::make_unique<LoraAdapter>(read_lora_adapter(dir, model_.cfg, max_layers));  // throws: state unchanged
    ACEMI_HIP(hipDeviceSynchronize());
    free_lora();
    // A and B of every module in one device buffer (256-byte aligned parts)
    size_t total = 0;
    auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
    for (const LoraModule& lm : ad->modules) total += al(lm.A.size() * 4) + al(lm.B.size() * 4);
    std::vector<char> host(total);
    lora_ab_.ensure(total);
    size_t off = 0;
    for (LoraModule& lm : ad->modules) {
        std::memcpy(&host[off], lm.A.data(), lm.A.size() * 4);
        lora_a_.push_back(reinterpret_cast<const float*>(lora_ab_.as<char>() + off));
        off += al(lm.A.size() * 4);
        std::memcpy(&host[off], lm.B.data(), lm.B.size() * 4);
        lora_b_.push_back(reinterpret_cast<const float*>(lora_ab_.as<char>() + off));
        off += al(lm.B.size() * 4);
        lm.A = std::vector<float>();
        lm.B = std::vector<float>();
    }
    ACEMI_HIP(hipMemcpy(lora_ab_.p, host.data(), total, hipMemcpyHostToDevice));
    ACEMI_HIP(hipDeviceSynchronize());  // null-stream copy: done before any stream reads it
    lora_ = std::move(ad);
    lora_scale_ = scale;
    try {
        rebuild_lora_images(s);
    } catch (...) {
        free_lora();
        throw;
    }
}

void DitEngine::set_lora_scale(float scale, hipStream_t s) {
    ACEMI_CHECK(lora_ != nullptr, "lora not loaded");
    lora_scale_ = scale;
    rebuild_lora_images(s);
}

void DitEngine::unload_lora(hipStream_t s) {
    ACEMI_HIP(hipDeviceSynchronize());
    free_lora();
    rebuild_lora_images(s);  // (nothing loaded: drops what was computed from the adapted views)
}

#ifndef __HIP__
// Host build of the runtime (no device compiler: the CPU tests' library, whose other launch_* are host loops too):
// launch_lora_merge as plain loops with the arithmetic of kernels.h, on "device" memory that is host memory.  The
// translation unit is compiled without FMA contraction, so each multiply and add below rounds on its own.
void launch_lora_merge(const LoraMergeJob* jobs, int n, hipStream_t) {
    auto widen = [](int fmt, uint16_t b) {
        if (fmt == WF_F16) return half_to_f32(b);
        const uint32_t u = (uint32_t)b << 16;
        float f;
        std::memcpy(&f, &u, 4);
        return f;
    };
    auto narrow = [](int fmt, float f) -> uint16_t {
        if (fmt == WF_F16) {
            const _Float16 h = (_Float16)f;
            uint16_t u;
            std::memcpy(&u, &h, 2);
            return u;
        }
        uint32_t u;
        std::memcpy(&u, &f, 4);
        if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 64u);
        u += 0x7fffu + ((u >> 16) & 1u);
        return (uint16_t)(u >> 16);
    };
    for (int ji = 0; ji < n; ++ji) {
        const LoraMergeJob& j = jobs[ji];
        ACEMI_CHECK((j.fmt == WF_BF16 || j.fmt == WF_F16) && j.base && j.out && j.rows > 0 && j.cols > 0 &&
                        j.r >= 0 && j.r <= LORA_MAX_RANK && (j.r == 0 || (j.A && j.B)),
                    "lora_merge: bad job");
        for (int fr = j.row0; fr < j.row0 + j.rows; ++fr) {
            const int o = lora_module_row(j.map, j.row_off, j.half, j.rows_mod, j.r, fr);
            const uint16_t* src = j.base + (int64_t)fr * j.ld_base;
            uint16_t* dst = j.out + (int64_t)fr * j.ld_out;
            if (o < 0) {
                if (j.copy_rest && src != dst) std::memmove(dst, src, (size_t)j.cols * 2);
                continue;
            }
            for (int i = 0; i < j.cols; ++i) {
                volatile float acc = 0.f;  // (volatile: one rounded f32 per step, whatever the optimiser prefers)
                for (int k = 0; k < j.r; ++k) {
                    const float p = j.B[(int64_t)o * j.r + k] * j.A[(int64_t)k * j.cols + i];
                    acc = acc + p;
                }
                const float t = j.eff * acc;
                dst[i] = narrow(j.fmt, widen(j.fmt, src[i]) + t);
            }
        }
    }
}
#endif

}  // namespace acemi
