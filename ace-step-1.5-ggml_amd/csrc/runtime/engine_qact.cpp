// The arithmetic of the ggml-faithful quantized-activation mode (ACE_MI_QUANT_ACT=q8).  The mode walks the same graph
// as the product (DitEngine::walk in engine.cpp, its QACT arm); what differs is how a linear is computed, and that is
// here.  Every ggml_mul_mat against a Q8_0 / Q4_K / Q6_K weight (acestep_dit_model.cpp:1194-1196, 1257, 1295-1302,
// 1381, 1412, 1528-1531, 1551) converts its f32 input rows to Q8_0 / Q8_K blocks and sums d_w * d_a * (integer block
// dot) in f32 (kernels/gemm_a8.hip): qlinear, with q8_image for the bf16-MFMA form of Q8_0, and timestep_embed_qact
// for the timestep MLP.  The tensors between the mul_mats stay f32, as in the ggml graph (the walk keeps them in one
// f32 buffer), and attention runs at the f32 precision.  The product keeps bf16 activations and bf16(dequant(W)); this
// mode exists so the quantized configs can be checked against ggml's semantics within the oracle's floor
// (tests/test_gpu_qact.py).
#include <algorithm>
#include <cmath>

#include "engine.h"
#include "operands.h"

namespace acemi {

void DitEngine::qlinear(const float* x, int64_t ldx, int M, const WeightView& w, int N, int K, const GemmEpilogue& e,
                        const char* name, hipStream_t s, bool silu_in) {
    tic(s);
    if (weight_quantized(w.fmt) && gemm_a8_bf16_path(w.fmt, K)) {
        // Q8_0 on the bf16 MFMA: the activation blocks as bf16(q) rows, the weight as its bf16(q) image (same bits as
        // the i8 kernel below, kernels/gemm_a8.hip gemm_a8s_kernel)
        const int64_t ld_s = round_up(M, 128);
        ensure(qa16_, (size_t)M * K * 2);
        ensure(qs_, (size_t)(K / 32) * ld_s * 4);
        const uint16_t* w16 = q8_image(w, N, K, s);
        launch_quantize_act(QACT_Q8_0, x, ldx, M, K, silu_in, nullptr, get<float>(qs_), nullptr, ld_s, s,
                            get<uint16_t>(qa16_));
        QAct a;
        a.kind = QACT_Q8_0;
        a.q16 = get<uint16_t>(qa16_);
        a.s = get<float>(qs_);
        a.ld_s = ld_s;
        launch_gemm_a8(a, w, M, N, K, e, s, w16);
    } else if (weight_quantized(w.fmt)) {
        const int kind = qact_kind_for(w.fmt);
        const int64_t ld_s = round_up(M, 128);
        ensure(qa_, (size_t)M * K);
        ensure(qs_, (size_t)(K / 32) * ld_s * 4);
        ensure(qb_, (size_t)(K / 32) * ld_s * 4);
        launch_quantize_act(kind, x, ldx, M, K, silu_in, get<int8_t>(qa_), get<float>(qs_), get<float>(qb_), ld_s, s);
        QAct a;
        a.kind = kind;
        a.q = get<int8_t>(qa_);
        a.s = get<float>(qs_);
        a.bsum = get<float>(qb_);
        a.ld_s = ld_s;
        launch_gemm_a8(a, w, M, N, K, e, s);
    } else {
        // a 16-bit weight: ggml rounds the activation to the weight's type (its vec_dot_type) -- the dense GEMM
        ACEMI_CHECK(w.fmt == WF_BF16 || w.fmt == WF_F16, "quantized-activation mode: F32 2-D weights are not supported");
        ACEMI_CHECK(ldx == K && e.kind != EPI_SWIGLU_F32, "quantized-activation mode: unsupported dense linear");
        ensure(qa_, (size_t)M * K * 2);
        uint16_t* xa = get<uint16_t>(qa_);
        launch_to_act(weight_act(w.fmt), x, (int64_t)M * K, silu_in, xa, s);
        launch_gemm(xa, K, w, M, N, K, e, s);
    }
    toc(name, s);
}

// bf16(q) image of a Q8_0 weight's int8 plane, made once on the stream that first needs it and kept while the model is
// loaded (the engine is rebuilt with every load, so a plane pointer names one weight for the cache's lifetime)
const uint16_t* DitEngine::q8_image(const WeightView& w, int N, int K, hipStream_t s) {
    DevBuf& b = q8img_[w.q];
    if (!b.p) {
        ensure(b, (size_t)N * K * 2);
        launch_q8_image(static_cast<const int8_t*>(w.q), (int64_t)N * K, static_cast<uint16_t*>(b.p), s);
    }
    return static_cast<const uint16_t*>(b.p);
}

void DitEngine::timestep_embed_qact(const float* t, const float* r, int rows, float* proj, float* temb_t,
                                    float* temb_r, hipStream_t s) {
    const DitModel& m = model_;
    const int H = m.cfg.hidden;
    const float log_max = std::log(10000.0f);
    ensure(freq_, (size_t)8 * 256 * 4);
    ensure(th_, (size_t)8 * H * 4);
    float* freq = get<float>(freq_);
    float* th = get<float>(th_);
    for (int e = 0; e < 2; ++e)
        ACEMI_CHECK(m.te[e].q1.q && m.te[e].q2.q && m.te[e].qp.q,
                    "quantized-activation mode: load the model with ACE_MI_QUANT_ACT=q8 set");
    for (int r0 = 0; r0 < rows; r0 += 8) {
        const int n = std::min(8, rows - r0);
        float* pr = proj + (size_t)r0 * 6 * H;
        for (int e = 0; e < 2; ++e) {
            const DevTimestep& te = m.te[e];
            float* temb = (e == 0 ? temb_t : temb_r) + (size_t)r0 * H;
            // timestep_forward (:1286-1308): h = silu(W1 f + b1); temb = W2 h + b2; proj = Wp silu(temb) + bp,
            // proj of t - r added to that of t (:1420-1424); each silu is applied to the rows the next linear quantizes
            launch_timestep_freq(t + r0, e == 0 ? nullptr : r + r0, n, 256, 1000.0f, log_max, freq, s);
            qlinear(freq, 256, n, te.q1.view(), H, 256, epi_store_f32(th, H, te.b1), "timestep_l1", s);
            qlinear(th, H, n, te.q2.view(), H, H, epi_store_f32(temb, H, te.b2), "timestep_l2", s, true);
            GemmEpilogue e3 = epi_store_f32(pr, 6 * H, te.bp);
            if (e == 1) e3.kind = EPI_RESID;  // (with a bias: added to the product first)
            qlinear(temb, H, n, te.qp.view(), 6 * H, H, e3, "timestep_proj", s, true);
        }
    }
}

}  // namespace acemi
