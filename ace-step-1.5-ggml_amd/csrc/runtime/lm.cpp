// The 5 Hz audio-code language model on the engine: a HF Qwen3ForCausalLM with a KV cache (include/acestep_mi355x.h,
// ace_mi_load_lm / ace_mi_lm_*), driven like the reference's `pt` backend drives transformers
// (acestep/llm_inference.py:345-367): one prefill, then single-token steps.
//
//   prefill (n > 1, empty cache)  the text encoder's path: BlockRunner (MFMA GEMMs, causal flash attention, key mask);
//                                 its after-QKV hook stores every layer's post-norm, post-RoPE K and V into the cache.
//   decode step (n == 1)          kernels/lm_decode.hip: skinny products over the same fused matrices DevLayer holds,
//                                 QKV post-processing, decode attention over the cache.  A matrix in ggml block planes
//                                 (a GGUF checkpoint's Q8_0 / Q4_K / Q6_K tensors) goes through kernels/lm_decode_q.hip,
//                                 which multiplies the bf16 values the prefill's quantized GEMM multiplies.
// Rounding points follow BlockRunner::run: the residual stream stays f32, the input of every linear is rounded to
// the weights' 16-bit type, products accumulate in f32.  The one deviation: prefill attention reads Q, K, V as fp16
// hi + lo pairs (~22 bits), the decode step keeps Q in f32 and reads K and V from the cache as single fp16 values.
//
// This file holds both the engine and its C entries, so no other translation unit refers to the launch_lm_* kernels.
#include <cmath>
#include <cstdlib>
#include <random>
#include <vector>

#include "../kernels/lm_decode_q_host.h"  // empty under hipcc; the host build's launch_lm_skinny_q / launch_lm_embed_q
#include "../kernels/lm_fanout_host.h"    // empty under hipcc; the host build's launch_lm_cache_fanout
#include "../kernels/lm_sample_host.h"    // empty under hipcc; the host build's launch_lm_select
#include "context.h"
#include "safetensors.h"

namespace acemi {

// tokens between two host reads of the loop's stop word (ace_mi_lm_generate)
constexpr int LM_STOP_POLL = 16;

// the uniform stream of ace_mi_lm_generate / ace_mi_lm_uniforms: std::mt19937_64(seed), (x >> 40) * 2^-24 per output
inline void lm_uniform_stream(uint64_t seed, size_t n, float* out) {
    std::mt19937_64 gen(seed);
    for (size_t i = 0; i < n; ++i) out[i] = (float)(gen() >> 40) * (1.0f / 16777216.0f);
}

class LmEngine {
   public:
    TextModel& model() { return model_; }
    int batch() const { return batch_; }
    int capacity() const { return capacity_; }
    int len() const { return len_; }
    size_t cache_bytes() const { return kc_.bytes + vc_.bytes + kmask_.bytes; }
    void reset() { len_ = 0; }

    // bytes per position and sequence: K and V, fp16, every layer
    size_t token_bytes() const {
        const TextConfig& c = model_.cfg;
        return (size_t)c.layers * 2 * c.hkv * c.head_dim * 2;
    }

    void check_weights() const {
        auto ok = [](const DevWeight& w) { return (w.fmt == WF_BF16 || w.fmt == WF_F16 || weight_planes(w.fmt)) && w.q; };
        for (const DevLayer& ly : model_.layers)
            for (const DevWeight* w : {&ly.w_qkv, &ly.w_o, &ly.w_gu, &ly.w_down})
                if (!ok(*w)) throw Unsupported("LM weights must be dense BF16 / F16 or Q8_0 / Q4_K / Q6_K planes");
        if (!ok(model_.head)) throw Unsupported("LM head must be dense BF16 / F16 or Q8_0 / Q4_K / Q6_K planes");
        for (const DevLayer& ly : model_.layers)
            for (const DevWeight* w : {&ly.w_qkv, &ly.w_o, &ly.w_gu, &ly.w_down})
                if (weight_planes(w->fmt) && model_.act != ActType::BF16)
                    throw Unsupported("mixed LM weight types: block planes take BF16 activations");
    }

    void begin(int B, int cap) {
        const TextConfig& c = model_.cfg;
        ACEMI_HIP(hipDeviceSynchronize());  // nothing in flight reads the buffers that may move
        const size_t plane = (size_t)c.layers * B * c.hkv * cap * c.head_dim * 2;
        kc_.ensure(plane);
        vc_.ensure(plane);
        kmask_.ensure((size_t)B * cap * 4);
        rope_.ensure(cap, c.head_dim, c.rope_theta, nullptr);
        const int H = c.hidden, qd = c.hq * c.head_dim, kd = c.hkv * c.head_dim, I = c.intermediate;
        x_.ensure((size_t)LM_MAX_BATCH * H * 4);
        act_.ensure((size_t)LM_MAX_BATCH * std::max(H, qd) * 2);
        act2_.ensure((size_t)LM_MAX_BATCH * I * 2);
        qkv_.ensure((size_t)LM_MAX_BATCH * (qd + 2 * kd) * 4);
        q_.ensure((size_t)LM_MAX_BATCH * qd * 4);
        attn_.ensure((size_t)LM_MAX_BATCH * qd * 2);
        xn_.ensure((size_t)LM_MAX_BATCH * H * 4);
        xh_.ensure((size_t)LM_MAX_BATCH * H * 2);
        part_.ensure(lm_attn_part_floats(B, c.hq, cap) * 4);
        batch_ = B;
        capacity_ = cap;
        len_ = 0;
    }

    // The cache of batch_ = G sequences re-laid for G * copies sequences of `cap` positions (kernels/lm_fanout.hip):
    // sequence g * copies + s is a bit copy of sequence g, the logits rows follow, len_ stays.  The caller has checked
    // the arguments.  The new cache is allocated beside the old one, which is released once the copy has finished on
    // `s`; a throw before that leaves the engine as it was.
    void fanout(int copies, int cap, float* d_logits, hipStream_t s) {
        const TextConfig& c = model_.cfg;
        const int G = batch_, B = G * copies;
        if (copies == 1 && cap == capacity_) return;
        const size_t plane = (size_t)c.layers * B * c.hkv * cap * c.head_dim * 2;
        DevBuf kn, vn, mn;
        kn.ensure(plane);
        vn.ensure(plane);
        mn.ensure((size_t)B * cap * 4);
        rope_.ensure(cap, c.head_dim, c.rope_theta, s);
        part_.ensure(lm_attn_part_floats(B, c.hq, cap) * 4);
        LmFanoutArgs a;
        a.k_src = kc_.as<uint16_t>();
        a.v_src = vc_.as<uint16_t>();
        a.mask_src = kmask_.as<int32_t>();
        a.k_dst = kn.as<uint16_t>();
        a.v_dst = vn.as<uint16_t>();
        a.mask_dst = mn.as<int32_t>();
        a.layers = c.layers;
        a.G = G;
        a.S = copies;
        a.hkv = c.hkv;
        a.cap_src = capacity_;
        a.cap_dst = cap;
        a.n = len_;
        launch_lm_cache_fanout(a, s);
        if (d_logits)  // descending: row r is read only by rows >= r, all written before it is overwritten
            for (int r = B - 1; r > 0; --r)
                if (r / copies != r)
                    ACEMI_HIP(hipMemcpyAsync(d_logits + (size_t)r * c.vocab, d_logits + (size_t)(r / copies) * c.vocab,
                                             (size_t)c.vocab * 4, hipMemcpyDeviceToDevice, s));
        ACEMI_HIP(hipStreamSynchronize(s));  // the copy has read the old cache: it may go
        kc_ = std::move(kn);
        vc_ = std::move(vn);
        kmask_ = std::move(mn);
        batch_ = B;
        capacity_ = cap;
    }

    // the caller has checked batch, capacity and the prefill rule
    void forward(const int32_t* d_ids, const int32_t* d_mask, int n, float* d_logits, hipStream_t s) {
        if (n > 1)
            prefill(d_ids, d_mask, n, d_logits, s);
        else
            step(d_ids, d_mask, d_logits, s);
        len_ += n;
    }

    // The selection arguments shared by select() and generate(); `why` names what is wrong with them, if anything.
    // first_allowed: the list's first id when it has one entry (the caller read it), else -1.
    const char* check_sample(const ace_mi_lm_sample_params& p, int n_emitted, bool force_stop, int first_allowed) const {
        const int vocab = model_.cfg.vocab;
        if (p.cfg_scale > 1.0f && batch_ % 2 != 0) return "cfg_scale > 1 needs an even batch";
        if (p.d_allowed && p.n_allowed < 1) return "n_allowed < 1";
        if (p.stop_id >= vocab) return "stop_id outside the vocabulary";
        if (force_stop && p.stop_id < 0) return "force_stop without a stop_id";
        const bool blocked = p.stop_id >= 0 && n_emitted < p.min_tokens && !force_stop;
        if (blocked && (p.d_allowed ? (p.n_allowed == 1 && first_allowed == p.stop_id) : vocab == 1))
            return "the candidate set is empty";
        return nullptr;
    }

    LmSelectArgs select_args(const ace_mi_lm_sample_params& p, const float* d_logits, uint8_t* d_seen) {
        const int vocab = model_.cfg.vocab;
        LmSelectArgs a;
        a.logits = d_logits;
        a.ld_logits = vocab;
        a.vocab = vocab;
        a.S = p.cfg_scale > 1.0f ? batch_ / 2 : batch_;
        a.cfg_scale = p.cfg_scale;
        a.allowed = p.d_allowed;
        a.n_allowed = p.d_allowed ? p.n_allowed : 0;
        a.stop_id = p.stop_id < 0 ? -1 : p.stop_id;
        a.pre_temperature = p.pre_temperature;
        a.repetition_penalty = p.repetition_penalty;
        a.seen = d_seen;
        a.ld_seen = vocab;
        a.top_k = p.top_k;
        a.top_p = p.top_p;
        a.temperature = p.temperature;
        sel_work_.ensure(lm_select_work_floats(a.S, lm_select_candidates(vocab, p.n_allowed, p.d_allowed != nullptr)) * 4);
        a.work = sel_work_.as<float>();
        return a;
    }

    void select(const ace_mi_lm_sample_params& p, const float* d_logits, const float* d_uniform, uint8_t* d_seen,
                int n_emitted, bool force_stop, int32_t* d_tokens, hipStream_t s) {
        LmSelectArgs a = select_args(p, d_logits, d_seen);
        a.block_stop = a.stop_id >= 0 && n_emitted < p.min_tokens;
        a.force_stop = force_stop;
        a.n_emitted = n_emitted;
        a.uniform = d_uniform;
        a.tokens = d_tokens;
        launch_lm_select(a, s);
    }

    // the caller has checked the arguments and the capacity; returns *n_out
    int generate(const ace_mi_lm_sample_params& p, float* d_logits, int n_max, const float* d_uniform, uint8_t* d_seen,
                 int32_t* d_tokens, hipStream_t s) {
        LmSelectArgs a = select_args(p, d_logits, d_seen);
        sel_next_.ensure((size_t)LM_MAX_BATCH * 4);
        sel_done_.ensure((size_t)(1 + LM_MAX_BATCH) * 4);
        if (!d_uniform && p.temperature > 0.0f) {
            std::vector<float> u((size_t)n_max * a.S);
            lm_uniform_stream(p.seed, u.size(), u.data());
            sel_uni_.ensure(u.size() * 4);
            ACEMI_HIP(hipDeviceSynchronize());  // an earlier loop, on any stream, may still read the buffer
            ACEMI_HIP(hipMemcpy(sel_uni_.p, u.data(), u.size() * 4, hipMemcpyHostToDevice));
            d_uniform = sel_uni_.as<float>();
        }
        const bool stops = a.stop_id >= 0;
        const bool poll = stops && p.min_tokens < n_max;
        static const int32_t zeros[1 + LM_MAX_BATCH] = {};
        if (stops) ACEMI_HIP(hipMemcpyAsync(sel_done_.p, zeros, sizeof(zeros), hipMemcpyHostToDevice, s));
        a.next_ids = sel_next_.as<int32_t>();
        a.done = stops ? sel_done_.as<int32_t>() : nullptr;
        a.token_stride = n_max;
        int first_stop = 0;
        const int len0 = len_;
        try {
            first_stop = run_loop(a, p, d_logits, n_max, d_uniform, d_tokens, stops, poll, s);
        } catch (...) {
            len_ = len0;  // the entry reports ACE_GGML_ERR with the cache length it found; the slots past it are scratch
            throw;
        }
        return first_stop > 0 ? first_stop : n_max;
    }

   private:
    int run_loop(LmSelectArgs& a, const ace_mi_lm_sample_params& p, float* d_logits, int n_max, const float* d_uniform,
                 int32_t* d_tokens, bool stops, bool poll, hipStream_t s) {
        int first_stop = 0;
        for (int t = 0; t < n_max; ++t) {
            a.block_stop = stops && t < p.min_tokens;
            a.n_emitted = t;
            a.uniform = d_uniform ? d_uniform + (size_t)t * a.S : nullptr;
            a.tokens = d_tokens + t;
            launch_lm_select(a, s);
            if (poll && (t + 1) % LM_STOP_POLL == 0 && t + 1 < n_max && (first_stop = read_done(s)) != 0) break;
            if (t + 1 < n_max) {
                step(a.next_ids, nullptr, d_logits, s);
                ++len_;
            }
        }
        if (poll && first_stop == 0) first_stop = read_done(s);
        return first_stop;
    }

    // the `done` word of the loop through a pinned host word: async copy, event, wait
    int read_done(hipStream_t s) {
        if (!poll_.pinned) poll_.alloc();
        if (!poll_.ev) ACEMI_HIP(hipEventCreateWithFlags(&poll_.ev, hipEventDisableTiming));
        ACEMI_HIP(hipMemcpyAsync(poll_.pinned, sel_done_.p, 4, hipMemcpyDeviceToHost, s));
        ACEMI_HIP(hipEventRecord(poll_.ev, s));
        ACEMI_HIP(hipEventSynchronize(poll_.ev));
        return *poll_.pinned;
    }
    struct StopPoll {
        int32_t* pinned = nullptr;
        hipEvent_t ev = nullptr;
#ifdef __HIP__
        void alloc() { ACEMI_HIP(hipHostMalloc(reinterpret_cast<void**>(&pinned), 16, hipHostMallocDefault)); }
        ~StopPoll() {
            if (ev) (void)hipEventDestroy(ev);
            if (pinned) (void)hipHostFree(pinned);
        }
#else  // the host build has no pinned memory to ask for
        void alloc() { pinned = static_cast<int32_t*>(std::calloc(4, 4)); }
        ~StopPoll() {
            if (ev) (void)hipEventDestroy(ev);
            std::free(pinned);
        }
#endif
    };

    LmQkvPostArgs post_args(int li, const float* qkv, int ld) {
        const TextConfig& c = model_.cfg;
        const DevLayer& ly = model_.layers[li];
        const size_t layer = (size_t)batch_ * c.hkv * capacity_ * c.head_dim;
        LmQkvPostArgs a;
        a.qkv = qkv;
        a.ld = ld;
        a.hq = c.hq;
        a.hkv = c.hkv;
        a.q_norm = ly.sq_norm;
        a.k_norm = ly.sk_norm;
        a.rope_cos = rope_.cos();
        a.rope_sin = rope_.sin();
        a.eps = c.eps;
        a.q_out = q_.as<float>();
        a.k_cache = kc_.as<uint16_t>() + (size_t)li * layer;
        a.v_cache = vc_.as<uint16_t>() + (size_t)li * layer;
        a.key_mask = kmask_.as<int32_t>();
        a.capacity = capacity_;
        return a;
    }

    // one skinny product of the step, by the matrix's format: dense 16-bit rows or block planes
    void skinny(ActType t, const uint16_t* x, int ldx, const DevWeight& w, int N, int K, int epi, float* y_f32,
                uint16_t* y_act, int ldy, hipStream_t s) {
        if (weight_planes(w.fmt))
            launch_lm_skinny_q(x, ldx, batch_, w.view(), N, K, epi, y_f32, y_act, ldy, s);
        else
            launch_lm_skinny(t, x, ldx, batch_, static_cast<const uint16_t*>(w.q), N, K, epi, y_f32, y_act, ldy, s);
    }

    void embed(const int32_t* d_ids, int n, float* x, hipStream_t s) {
        const TextConfig& c = model_.cfg;
        if (model_.embed_fmt == 3)
            launch_lm_embed_q(model_.embed_q.fmt, model_.embed_q.q, model_.embed_q.s, d_ids, n, c.vocab, c.hidden, x, s);
        else if (model_.embed_fmt == 2)
            launch_lm_embed_q(LM_EMBED_F32, model_.embed, nullptr, d_ids, n, c.vocab, c.hidden, x, s);
        else
            launch_lm_embed(model_.embed, model_.embed_fmt, d_ids, n, c.vocab, c.hidden, x, s);
    }

    void head(const float* x_last, int64_t row_step, float* d_logits, hipStream_t s) {
        const TextConfig& c = model_.cfg;
        const ActType ht = model_.head.act();
        launch_rmsnorm_f32(x_last, batch_, row_step, c.hidden, model_.norm, c.eps, xn_.as<float>(), s);
        launch_to_act(ht, xn_.as<float>(), (int64_t)batch_ * c.hidden, false, xh_.as<uint16_t>(), s);
        skinny(ht, xh_.as<uint16_t>(), c.hidden, model_.head, c.vocab, c.hidden, LM_EPI_STORE, d_logits, nullptr, c.vocab, s);
    }

    BlockShape shape() const {
        const TextConfig& c = model_.cfg;
        BlockShape sh;
        sh.hidden = c.hidden;
        sh.hq = c.hq;
        sh.hkv = c.hkv;
        sh.head_dim = c.head_dim;
        sh.intermediate = c.intermediate;
        sh.eps = c.eps;
        sh.rope_theta = c.rope_theta;
        return sh;
    }

    void prefill(const int32_t* d_ids, const int32_t* d_mask, int n, float* d_logits, hipStream_t s) {
        const TextConfig& c = model_.cfg;
        const BlockShape sh = shape();
        const int M = batch_ * n;
        float* x = blocks_.x(M, sh.hidden);
        embed(d_ids, M, x, s);
        const BlockRunner::AfterQkv fill = [&](int li, float* qkv, int ld) {
            launch_lm_prefill_kv(post_args(li, qkv, ld), batch_, n, d_mask, s);
        };
        blocks_.run(sh, model_.layers, c.layers, model_.act, batch_, n, d_mask, true, s, &fill);
        head(x + (size_t)(n - 1) * sh.hidden, n, d_logits, s);
    }

    void step(const int32_t* d_ids, const int32_t* d_mask, float* d_logits, hipStream_t s) {
        const TextConfig& c = model_.cfg;
        const int B = batch_, H = c.hidden, D = c.head_dim, qd = c.hq * D, kd = c.hkv * D, I = c.intermediate;
        const ActType at = model_.act;
        float* x = x_.as<float>();
        uint16_t* act = act_.as<uint16_t>();
        uint16_t* act2 = act2_.as<uint16_t>();
        uint16_t* attn = attn_.as<uint16_t>();
        float* qkv = qkv_.as<float>();
        embed(d_ids, B, x, s);
        for (int li = 0; li < c.layers; ++li) {
            const DevLayer& ly = model_.layers[li];
            launch_rmsnorm_mod(at, x, B, H, ly.self_norm, nullptr, nullptr, 0, 1, c.eps, act, s);
            skinny(at, act, H, ly.w_qkv, qd + 2 * kd, H, LM_EPI_STORE, qkv, nullptr, qd + 2 * kd, s);
            LmQkvPostArgs pa = post_args(li, qkv, qd + 2 * kd);
            pa.pos = len_;
            pa.mask_new = d_mask;
            launch_lm_qkv_post(pa, B, s);
            LmAttnArgs aa;
            aa.q = q_.as<float>();
            aa.k_cache = pa.k_cache;
            aa.v_cache = pa.v_cache;
            aa.key_mask = pa.key_mask;
            aa.hkv = c.hkv;
            aa.capacity = capacity_;
            aa.nk = len_ + 1;
            aa.scale = 1.0f / std::sqrt((float)D);
            aa.out = attn;
            aa.part = part_.as<float>();
            launch_lm_attention(at, aa, B, c.hq, s);
            skinny(at, attn, qd, ly.w_o, H, qd, LM_EPI_RESID, x, nullptr, H, s);
            launch_rmsnorm_mod(at, x, B, H, ly.mlp_norm, nullptr, nullptr, 0, 1, c.eps, act, s);
            skinny(at, act, H, ly.w_gu, 2 * I, H, LM_EPI_SWIGLU, nullptr, act2, I, s);
            skinny(at, act2, I, ly.w_down, H, I, LM_EPI_RESID, x, nullptr, H, s);
        }
        head(x, 1, d_logits, s);
    }

    TextModel model_;
    BlockRunner blocks_;
    StopPoll poll_;  // declared before the buffers: the event and the pinned word go after the buffers are freed
    DevBuf kc_, vc_, kmask_, x_, act_, act2_, qkv_, q_, attn_, part_, xn_, xh_;
    DevBuf sel_work_, sel_next_, sel_done_, sel_uni_;  // selection scratch, the next step's ids, the stop words, uniforms
    RopeTable rope_;  // positions 0..capacity-1
    int batch_ = 0, capacity_ = 0, len_ = 0;
};

}  // namespace acemi

using namespace acemi_abi;

namespace {
acemi::LmEngine* lm_of(ace_ggml_context* ctx) { return static_cast<acemi::LmEngine*>(ctx->lm.get()); }
}  // namespace

extern "C" {

ace_ggml_status ace_mi_load_lm(ace_ggml_context* ctx, const char* model_dir) {
    if (!ctx || !model_dir) return ACE_GGML_ERR_INVALID_ARG;
    try {
        bind_device(ctx);
        ACEMI_HIP(hipStreamSynchronize(ctx->stream));
        ctx->lm.reset();  // the previous LM and its cache
        auto eng = std::make_shared<acemi::LmEngine>();
        acemi::TextLoadOptions opt;
        opt.model_prefix = true;
        opt.lm_head = true;
        opt.lm_checkpoint = true;
        acemi::load_text_model(model_dir, eng->model(), opt);
        eng->check_weights();
        ctx->lm = std::move(eng);
    } catch (const acemi::HipError& e) {
        return set_error(ctx, ACE_GGML_ERR, e.what());
    } catch (const acemi::Unsupported& e) {
        return set_error(ctx, ACE_GGML_ERR_UNSUPPORTED, e.what());
    } catch (const std::exception& e) {
        return set_error(ctx, ACE_GGML_ERR_IO, e.what());
    }
    return ACE_GGML_OK;
}

ace_ggml_status ace_mi_lm_get_info(ace_ggml_context* ctx, ace_mi_lm_info* out) {
    if (!ctx || !out) return ACE_GGML_ERR_INVALID_ARG;
    if (!ctx->lm) return set_error(ctx, ACE_GGML_ERR, "lm not loaded");
    acemi::LmEngine* e = lm_of(ctx);
    const acemi::TextConfig& c = e->model().cfg;
    out->vocab_size = c.vocab;
    out->hidden_size = c.hidden;
    out->num_layers = c.layers;
    out->num_heads = c.hq;
    out->num_kv_heads = c.hkv;
    out->head_dim = c.head_dim;
    out->max_positions = c.max_pos;
    out->tied = e->model().tied ? 1 : 0;
    out->act_type = e->model().act == acemi::ActType::F16 ? 1 : 0;
    out->batch = e->batch();
    out->capacity = e->capacity();
    out->cache_len = e->len();
    out->weight_bytes = (int64_t)e->model().arena.bytes();
    out->cache_bytes = (int64_t)e->cache_bytes();
    return ACE_GGML_OK;
}

ace_ggml_status ace_mi_lm_begin(ace_ggml_context* ctx, int32_t batch, int32_t capacity) {
    if (!ctx) return ACE_GGML_ERR_INVALID_ARG;
    if (!ctx->lm) return set_error(ctx, ACE_GGML_ERR, "lm not loaded");
    acemi::LmEngine* e = lm_of(ctx);
    if (batch < 1 || batch > acemi::LM_MAX_BATCH)
        return set_error(ctx, ACE_GGML_ERR_INVALID_ARG, "lm batch must be 1..8");
    if (capacity < 1 || capacity > e->model().cfg.max_pos)
        return set_error(ctx, ACE_GGML_ERR_INVALID_ARG, "lm capacity must be 1..max_position_embeddings");
    try {
        bind_device(ctx);
        e->begin(batch, capacity);
    } catch (const std::exception& ex) {
        return set_error(ctx, ACE_GGML_ERR, std::string("lm begin failed: ") + ex.what());
    }
    return ACE_GGML_OK;
}

ace_ggml_status ace_mi_lm_forward(ace_ggml_context* ctx, const int32_t* d_ids, const int32_t* d_mask, int32_t n,
                                  float* d_logits, void* stream) {
    if (!ctx) return ACE_GGML_ERR_INVALID_ARG;
    if (!ctx->lm) return set_error(ctx, ACE_GGML_ERR, "lm not loaded");
    if (!d_ids || !d_logits || n <= 0) return set_error(ctx, ACE_GGML_ERR_INVALID_ARG, "lm forward: null pointer or n <= 0");
    acemi::LmEngine* e = lm_of(ctx);
    if (e->batch() <= 0) return set_error(ctx, ACE_GGML_ERR_INVALID_ARG, "lm forward: ace_mi_lm_begin was not called");
    if ((int64_t)e->len() + n > e->capacity())
        return set_error(ctx, ACE_GGML_ERR_INVALID_ARG, "lm forward: exceeds the cache capacity");
    if (n > 1 && e->len() > 0)
        return set_error(ctx, ACE_GGML_ERR_INVALID_ARG, "lm forward: a prefill (n > 1) needs an empty cache");
    try {
        bind_device(ctx);
        acemi::gemm_splitk_check();
        hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
        e->forward(d_ids, d_mask, n, d_logits, s);
    } catch (const std::exception& ex) {
        return set_error(ctx, ACE_GGML_ERR, std::string("lm forward failed: ") + ex.what());
    }
    return ACE_GGML_OK;
}

namespace {
// the argument checks of ace_mi_lm_select / ace_mi_lm_generate; OK, or the status with the message set
ace_ggml_status lm_check_sample(ace_ggml_context* ctx, acemi::LmEngine* e, const ace_mi_lm_sample_params* p, int n_emitted,
                                bool force_stop, const char* where) {
    int first = -1;
    if (p->d_allowed && p->n_allowed == 1 && p->stop_id >= 0) {
        try {
            bind_device(ctx);
            ACEMI_HIP(hipMemcpy(&first, p->d_allowed, 4, hipMemcpyDeviceToHost));
        } catch (const std::exception& ex) {
            return set_error(ctx, ACE_GGML_ERR, std::string(where) + ": " + ex.what());
        }
    }
    if (const char* why = e->check_sample(*p, n_emitted, force_stop, first))
        return set_error(ctx, ACE_GGML_ERR_INVALID_ARG, std::string(where) + ": " + why);
    return ACE_GGML_OK;
}
}  // namespace

ace_ggml_status ace_mi_lm_select(ace_ggml_context* ctx, const ace_mi_lm_sample_params* params, const float* d_logits,
                                 const float* d_uniform, uint8_t* d_seen, int32_t n_emitted, int32_t force_stop,
                                 int32_t* d_tokens, void* stream) {
    if (!ctx) return ACE_GGML_ERR_INVALID_ARG;
    if (!ctx->lm) return set_error(ctx, ACE_GGML_ERR, "lm not loaded");
    if (!params || !d_logits || !d_tokens || n_emitted < 0 || (params->temperature > 0.0f && !d_uniform))
        return set_error(ctx, ACE_GGML_ERR_INVALID_ARG, "lm select: null pointer or n_emitted < 0");
    acemi::LmEngine* e = lm_of(ctx);
    if (e->batch() <= 0) return set_error(ctx, ACE_GGML_ERR_INVALID_ARG, "lm select: ace_mi_lm_begin was not called");
    const ace_ggml_status st = lm_check_sample(ctx, e, params, n_emitted, force_stop != 0, "lm select");
    if (st != ACE_GGML_OK) return st;
    try {
        bind_device(ctx);
        hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
        e->select(*params, d_logits, d_uniform, d_seen, n_emitted, force_stop != 0, d_tokens, s);
    } catch (const std::exception& ex) {
        return set_error(ctx, ACE_GGML_ERR, std::string("lm select failed: ") + ex.what());
    }
    return ACE_GGML_OK;
}

ace_ggml_status ace_mi_lm_generate(ace_ggml_context* ctx, const ace_mi_lm_sample_params* params, float* d_logits,
                                   int32_t n_max, const float* d_uniform, uint8_t* d_seen, int32_t* d_tokens,
                                   int32_t* n_out, void* stream) {
    if (!ctx) return ACE_GGML_ERR_INVALID_ARG;
    if (!ctx->lm) return set_error(ctx, ACE_GGML_ERR, "lm not loaded");
    if (!params || !d_logits || !d_tokens || !n_out)
        return set_error(ctx, ACE_GGML_ERR_INVALID_ARG, "lm generate: null pointer");
    acemi::LmEngine* e = lm_of(ctx);
    if (e->batch() <= 0) return set_error(ctx, ACE_GGML_ERR_INVALID_ARG, "lm generate: ace_mi_lm_begin was not called");
    if (n_max < 1) return set_error(ctx, ACE_GGML_ERR_INVALID_ARG, "lm generate: n_max < 1");
    if ((int64_t)e->len() + n_max - 1 > e->capacity())
        return set_error(ctx, ACE_GGML_ERR_INVALID_ARG, "lm generate: exceeds the cache capacity");
    const ace_ggml_status st = lm_check_sample(ctx, e, params, 0, false, "lm generate");
    if (st != ACE_GGML_OK) return st;
    try {
        bind_device(ctx);
        acemi::gemm_splitk_check();
        hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
        *n_out = e->generate(*params, d_logits, n_max, d_uniform, d_seen, d_tokens, s);
    } catch (const std::exception& ex) {
        return set_error(ctx, ACE_GGML_ERR, std::string("lm generate failed: ") + ex.what());
    }
    return ACE_GGML_OK;
}

ace_ggml_status ace_mi_lm_fanout(ace_ggml_context* ctx, int32_t copies, int32_t capacity, float* d_logits, void* stream) {
    if (!ctx) return ACE_GGML_ERR_INVALID_ARG;
    if (!ctx->lm) return set_error(ctx, ACE_GGML_ERR, "lm not loaded");
    acemi::LmEngine* e = lm_of(ctx);
    if (copies < 1) return set_error(ctx, ACE_GGML_ERR_INVALID_ARG, "lm fanout: copies < 1");
    if (e->batch() < 1 || e->batch() > 2)
        return set_error(ctx, ACE_GGML_ERR_INVALID_ARG, "lm fanout: the cache must hold 1 or 2 sequences");
    if ((int64_t)e->batch() * copies > acemi::LM_MAX_BATCH)
        return set_error(ctx, ACE_GGML_ERR_INVALID_ARG, "lm fanout: more than 8 sequences");
    if (e->len() < 1) return set_error(ctx, ACE_GGML_ERR_INVALID_ARG, "lm fanout: the cache is empty");
    if (capacity < e->len() || capacity > e->model().cfg.max_pos)
        return set_error(ctx, ACE_GGML_ERR_INVALID_ARG, "lm fanout: capacity must be cache_len..max_position_embeddings");
    try {
        bind_device(ctx);
        hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
        e->fanout(copies, capacity, d_logits, s);
    } catch (const std::exception& ex) {
        return set_error(ctx, ACE_GGML_ERR, std::string("lm fanout failed: ") + ex.what());
    }
    return ACE_GGML_OK;
}

ace_ggml_status ace_mi_lm_uniforms(uint64_t seed, int64_t n, float* out) {
    if (n < 0 || (n > 0 && !out)) return ACE_GGML_ERR_INVALID_ARG;
    acemi::lm_uniform_stream(seed, (size_t)n, out);
    return ACE_GGML_OK;
}

ace_ggml_status ace_mi_lm_reset(ace_ggml_context* ctx) {
    if (!ctx) return ACE_GGML_ERR_INVALID_ARG;
    if (!ctx->lm) return set_error(ctx, ACE_GGML_ERR, "lm not loaded");
    lm_of(ctx)->reset();
    return ACE_GGML_OK;
}

}  // extern "C"
