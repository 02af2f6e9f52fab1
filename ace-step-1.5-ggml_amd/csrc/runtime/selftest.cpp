// Kernel self-test entries (include/acestep_mi355x.h, "test library"): run one gfx950 kernel on host buffers so
// the GPU parity tests can compare it with an fp64 / fp32 reference of the same op, and the kernel
// micro-benchmarks of tools/.  Built only into libacestep_mi355x_selftest.so (the product objects + this
// file, Makefile target `selftest`); the product library libacestep_mi355x.so does not contain them.
#include <algorithm>
#include <cstring>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../../include/acestep_mi355x_selftest.h"
#include "../gemm_variants.h"
#include "../kernels.h"
#include "devmem.h"
#include "quant.h"

using acemi::DevMem;

extern "C" {

ace_ggml_status ace_mi_kernel_gemm(int32_t act_type, int32_t epi, int32_t M, int32_t N, int32_t K, const uint16_t* A,
                                   const uint16_t* W, const float* bias, float* out_f32, uint16_t* out_u16) {
    using namespace acemi;
    if (!A || !W || M <= 0 || N % 128 != 0 || K % 64 != 0) return ACE_GGML_ERR_INVALID_ARG;
    const bool resid = epi == EPI_RESID || epi == EPI_RESID_GATED;
    if (epi != EPI_STORE_F32 && epi != EPI_SWIGLU && !resid) return ACE_GGML_ERR_UNSUPPORTED;
    if (((epi == EPI_STORE_F32 || resid) && !out_f32) || (epi == EPI_SWIGLU && !out_u16))
        return ACE_GGML_ERR_INVALID_ARG;
    if (epi == EPI_RESID_GATED && !bias) return ACE_GGML_ERR_INVALID_ARG;
    try {
        DevMem dA((size_t)M * K * 2), dW((size_t)N * K * 2), dB((size_t)N * 4), dC((size_t)M * N * 4);
        ACEMI_HIP(hipMemcpy(dA.p, A, (size_t)M * K * 2, hipMemcpyHostToDevice));
        ACEMI_HIP(hipMemcpy(dW.p, W, (size_t)N * K * 2, hipMemcpyHostToDevice));
        if (bias) ACEMI_HIP(hipMemcpy(dB.p, bias, (size_t)N * 4, hipMemcpyHostToDevice));
        GemmEpilogue e;
        e.kind = epi;
        e.bias = bias && !resid ? dB.as<float>() : nullptr;
        if (resid) {  // out_f32 holds x on entry: x += acc (* gate[n], the gate passed as `bias`)
            ACEMI_HIP(hipMemcpy(dC.p, out_f32, (size_t)M * N * 4, hipMemcpyHostToDevice));
            e.c_f32 = dC.as<float>();
            e.ldc = N;
            e.gate = epi == EPI_RESID_GATED ? dB.as<float>() : nullptr;
            e.gate_stride = 0;
            e.rows_per_item = M;
        } else if (epi == EPI_STORE_F32) {
            e.c_f32 = dC.as<float>();
            e.ldc = N;
        } else {
            e.c_act = dC.as<uint16_t>();
            e.ldc = N / 2;
        }
        launch_gemm(act_type == 1 ? ActType::F16 : ActType::BF16, dA.as<uint16_t>(), K, dW.as<uint16_t>(), K, M, N,
                    K, e, nullptr);
        ACEMI_HIP(hipDeviceSynchronize());
        if (epi == EPI_STORE_F32 || resid)
            ACEMI_HIP(hipMemcpy(out_f32, dC.p, (size_t)M * N * 4, hipMemcpyDeviceToHost));
        else
            ACEMI_HIP(hipMemcpy(out_u16, dC.p, (size_t)M * (N / 2) * 2, hipMemcpyDeviceToHost));
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "ace_mi_kernel_gemm: %s\n", ex.what());
        return ACE_GGML_ERR;
    }
    return ACE_GGML_OK;
}

}  // extern "C"

namespace {
// Device operands of one attention launch, prepared from host f32 q [B][nq][Hq*128] and kv
// [B][nk][2*Hkv*128] through the engine's own prep kernel (hi/lo planes, V^T, key bias).
struct AttnSetup {
    DevMem dq, dkv, dm, dqh, dkh, dvt, dkb, dout, dpart;
    acemi::AttnArgs a{};
    size_t nqf;
    AttnSetup(int B, int Hq, int Hkv, int nq, int nk, int window, float scale, int flags, const float* q,
              const float* kv, const int32_t* kmask)
        : dq((size_t)B * nq * Hq * 128 * 4), dkv((size_t)B * nk * 2 * Hkv * 128 * 4), dm((size_t)B * nk * 4),
          dqh((size_t)2 * B * Hq * acemi::round_up(nq, 128) * 128 * 2), dkh((size_t)2 * B * Hkv * acemi::round_up(nk, 128) * 128 * 2),
          dvt((size_t)2 * B * Hkv * 128 * acemi::round_up(nk, 128) * 2), dkb((size_t)B * acemi::round_up(nk, 128) * 4),
          dout((size_t)B * nq * Hq * 128 * 2), dpart(acemi::attn_part_floats((size_t)B * nq * Hq) * 4) {
        using namespace acemi;
        const int D = 128;
        const int nq_pad = (int)round_up(nq, 128), nk_pad = (int)round_up(nk, 128);
        ACEMI_HIP(hipMemset(dpart.p, 0, attn_part_floats((size_t)B * nq * Hq) * 4));  // the key-split tickets start at 0
        nqf = (size_t)B * nq * Hq * D;
        const size_t nkvf = (size_t)B * nk * 2 * Hkv * D;
        ACEMI_HIP(hipMemcpy(dq.p, q, nqf * 4, hipMemcpyHostToDevice));
        ACEMI_HIP(hipMemcpy(dkv.p, kv, nkvf * 4, hipMemcpyHostToDevice));
        if (kmask) ACEMI_HIP(hipMemcpy(dm.p, kmask, (size_t)B * nk * 4, hipMemcpyHostToDevice));
        const bool split = (flags & 1) != 0;
        PrepArgs pq{};
        pq.src = dq.as<float>();
        pq.ld = Hq * D;
        pq.q_col = 0;
        pq.k_col = -1;
        pq.v_col = -1;
        pq.hq = Hq;
        pq.hkv = Hkv;
        pq.n_tok = nq;
        pq.n_pad = nq_pad;
        pq.B = B;
        pq.qh = dqh.as<uint16_t>();
        const int64_t qpl = (int64_t)B * Hq * nq_pad * D, kpl = (int64_t)B * Hkv * nk_pad * D;
        pq.q_plane = split ? qpl : 0;
        const bool f8 = (flags & 8) && (flags & 16);  // f8c with split, pv8 without
        const bool pvs = (flags & 8) && (split || f8);
        pq.f8 = f8 ? 1 : 0;
        launch_attn_prep(pq, nullptr);
        PrepArgs pk{};
        pk.src = dkv.as<float>();
        pk.ld = 2 * Hkv * D;
        pk.q_col = -1;
        pk.k_col = 0;
        pk.v_col = Hkv * D;
        pk.hq = Hq;
        pk.hkv = Hkv;
        pk.n_tok = nk;
        pk.n_pad = nk_pad;
        pk.B = B;
        pk.kh = dkh.as<uint16_t>();
        pk.vt = dvt.as<uint16_t>();
        pk.k_plane = split ? kpl : 0;
        pk.v_plane = pvs || split ? kpl : 0;
        pk.f8 = f8 ? 1 : 0;
        launch_attn_prep(pk, nullptr);
        launch_key_bias(kmask ? dm.as<int32_t>() : nullptr, B, nk, 1, nk, nk_pad, dkb.as<float>(), nullptr);
        a.q = dqh.as<uint16_t>();
        a.k = dkh.as<uint16_t>();
        a.vt = dvt.as<uint16_t>();
        a.kbias = kmask ? dkb.as<float>() : nullptr;
        a.out = dout.as<uint16_t>();
        a.part = dpart.as<float>();
        a.B = B;
        a.Hq = Hq;
        a.Hkv = Hkv;
        a.nq = nq;
        a.nq_pad = nq_pad;
        a.nk = nk;
        a.nk_pad = nk_pad;
        a.window = window;
        a.scale = scale;
        a.split = split;
        a.causal = (flags & 2) != 0;
        a.pv_split = pvs;
        a.f8 = f8;
        a.q_plane = qpl;
        a.k_plane = kpl;
        a.v_plane = kpl;
        ACEMI_HIP(hipDeviceSynchronize());
    }
};
}  // namespace

extern "C" {

ace_ggml_status ace_mi_kernel_attention(int32_t B, int32_t Hq, int32_t Hkv, int32_t nq, int32_t nk, int32_t window,
                                        float scale, int32_t split, const float* q, const float* kv,
                                        const int32_t* kmask, float* out) {
    using namespace acemi;
    if (B <= 0 || Hq <= 0 || Hkv <= 0 || nq <= 0 || nk <= 0 || !q || !kv || !out) return ACE_GGML_ERR_INVALID_ARG;
    try {
        AttnSetup st(B, Hq, Hkv, nq, nk, window, scale, split, q, kv, kmask);
        launch_attention(ActType::BF16, st.a, nullptr);
        ACEMI_HIP(hipDeviceSynchronize());
        std::vector<uint16_t> h(st.nqf);
        ACEMI_HIP(hipMemcpy(h.data(), st.dout.p, st.nqf * 2, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < st.nqf; ++i) {
            const uint32_t u = (uint32_t)h[i] << 16;
            std::memcpy(&out[i], &u, 4);
        }
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "ace_mi_kernel_attention: %s\n", ex.what());
        return ACE_GGML_ERR;
    }
    return ACE_GGML_OK;
}

// Attention probabilities of the listed heads (kernels/attn_probs.hip): operands through the engine's prep kernel as
// above (no norm, no RoPE; the kernel reads the fp16 hi planes), one launch.  The device output sits between two
// guard runs of NaN-pattern words that the launch must leave alone.
ace_ggml_status ace_mi_kernel_attn_probs(int32_t B, int32_t Hq, int32_t Hkv, int32_t nq, int32_t nk, float scale,
                                         const float* q, const float* k, const int32_t* kmask, int32_t n_heads,
                                         const int32_t* heads, float* out) {
    using namespace acemi;
    if (B <= 0 || Hq <= 0 || Hkv <= 0 || Hq % Hkv != 0 || nq <= 0 || nk <= 0 || !q || !k || n_heads <= 0 || !heads ||
        !out)
        return ACE_GGML_ERR_INVALID_ARG;
    for (int i = 0; i < n_heads; ++i)
        if (heads[i] < 0 || heads[i] >= Hq) return ACE_GGML_ERR_INVALID_ARG;
    try {
        const int D = 128, G = 1024;
        const int nq_pad = (int)round_up(nq, 128), nk_pad = (int)round_up(nk, 64);
        const size_t nqf = (size_t)B * nq * Hq * D, nkf = (size_t)B * nk * Hkv * D;
        const size_t n_out = (size_t)n_heads * B * nq * nk;
        DevMem dq(nqf * 4), dk(nkf * 4), dm((size_t)B * nk * 4), dqh((size_t)B * Hq * nq_pad * D * 2),
            dkh((size_t)B * Hkv * nk_pad * D * 2), dkb((size_t)B * nk_pad * 4), dout((n_out + 2 * G) * 4);
        ACEMI_HIP(hipMemcpy(dq.p, q, nqf * 4, hipMemcpyHostToDevice));
        ACEMI_HIP(hipMemcpy(dk.p, k, nkf * 4, hipMemcpyHostToDevice));
        if (kmask) ACEMI_HIP(hipMemcpy(dm.p, kmask, (size_t)B * nk * 4, hipMemcpyHostToDevice));
        std::vector<uint32_t> guard((size_t)G, 0x7fc0a11cu);
        ACEMI_HIP(hipMemcpy(dout.as<float>(), guard.data(), (size_t)G * 4, hipMemcpyHostToDevice));
        ACEMI_HIP(hipMemcpy(dout.as<float>() + G, out, n_out * 4, hipMemcpyHostToDevice));
        ACEMI_HIP(hipMemcpy(dout.as<float>() + G + n_out, guard.data(), (size_t)G * 4, hipMemcpyHostToDevice));
        PrepArgs pq{};
        pq.src = dq.as<float>();
        pq.ld = Hq * D;
        pq.q_col = 0;
        pq.k_col = -1;
        pq.v_col = -1;
        pq.hq = Hq;
        pq.hkv = Hkv;
        pq.n_tok = nq;
        pq.n_pad = nq_pad;
        pq.B = B;
        pq.qh = dqh.as<uint16_t>();
        launch_attn_prep(pq, nullptr);
        PrepArgs pk{};
        pk.src = dk.as<float>();
        pk.ld = Hkv * D;
        pk.q_col = -1;
        pk.k_col = 0;
        pk.v_col = -1;
        pk.hq = Hq;
        pk.hkv = Hkv;
        pk.n_tok = nk;
        pk.n_pad = nk_pad;
        pk.B = B;
        pk.kh = dkh.as<uint16_t>();
        launch_attn_prep(pk, nullptr);
        launch_key_bias(kmask ? dm.as<int32_t>() : nullptr, B, nk, 1, nk, nk_pad, dkb.as<float>(), nullptr);
        AttnProbArgs a{};
        a.q = dqh.as<uint16_t>();
        a.k = dkh.as<uint16_t>();
        a.kbias = kmask ? dkb.as<float>() : nullptr;
        a.B = B;
        a.Hq = Hq;
        a.Hkv = Hkv;
        a.nq = nq;
        a.nq_pad = nq_pad;
        a.nk = nk;
        a.nk_pad = nk_pad;
        a.scale = scale;
        a.n_heads = n_heads;
        a.heads = heads;
        a.out = dout.as<float>() + G;
        launch_attn_probs(a, nullptr);
        ACEMI_HIP(hipDeviceSynchronize());
        std::vector<uint32_t> g0((size_t)G), g1((size_t)G);
        ACEMI_HIP(hipMemcpy(g0.data(), dout.as<float>(), (size_t)G * 4, hipMemcpyDeviceToHost));
        ACEMI_HIP(hipMemcpy(out, dout.as<float>() + G, n_out * 4, hipMemcpyDeviceToHost));
        ACEMI_HIP(hipMemcpy(g1.data(), dout.as<float>() + G + n_out, (size_t)G * 4, hipMemcpyDeviceToHost));
        if (g0 != guard || g1 != guard) throw std::runtime_error("a guard word outside the output was written");
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "ace_mi_kernel_attn_probs: %s\n", ex.what());
        return ACE_GGML_ERR;
    }
    return ACE_GGML_OK;
}

// Attention micro-benchmark: pseudo-random N(0,1)-like q / kv (fixed seed), average ms per launch over
// `iters` launches timed with hipEvents.  flags: bit 0 split (hi/lo) operands, bit 1 causal, bit 3 hi/lo P.V,
// bit 2 a key-padding mask (every 7th key masked), bit 4 the fp8 correction encoding (with bit 3: with bit 0 the f8c
// mode, without it pv8).
ace_ggml_status ace_mi_bench_attention(int32_t B, int32_t Hq, int32_t Hkv, int32_t nq, int32_t nk, int32_t window,
                                       int32_t flags, int32_t iters, float* avg_ms) {
    using namespace acemi;
    if (B <= 0 || Hq <= 0 || Hkv <= 0 || nq <= 0 || nk <= 0 || iters <= 0 || !avg_ms) return ACE_GGML_ERR_INVALID_ARG;
    try {
        std::vector<float> q((size_t)B * nq * Hq * 128), kv((size_t)B * nk * 2 * Hkv * 128);
        std::vector<int32_t> km((size_t)B * nk);
        uint32_t r = 2024u;
        auto rnd = [&]() {  // sum of 4 uniforms, centred: roughly N(0, 1/3)
            float acc = 0.f;
            for (int j = 0; j < 4; ++j) {
                r = r * 1664525u + 1013904223u;
                acc += (float)(r >> 8) * (1.0f / 16777216.0f);
            }
            return acc - 2.0f;
        };
        for (auto& v : q) v = 2.0f * rnd();
        for (auto& v : kv) v = rnd();
        for (size_t i = 0; i < km.size(); ++i) km[i] = (i % 7) != 6;
        AttnSetup st(B, Hq, Hkv, nq, nk, window, 1.0f / std::sqrt(128.0f), flags & 27, q.data(), kv.data(),
                     (flags & 4) ? km.data() : nullptr);
        hipEvent_t e0, e1;
        ACEMI_HIP(hipEventCreate(&e0));
        ACEMI_HIP(hipEventCreate(&e1));
        for (int i = 0; i < 2; ++i) launch_attention(ActType::BF16, st.a, nullptr);
        ACEMI_HIP(hipEventRecord(e0, nullptr));
        for (int i = 0; i < iters; ++i) launch_attention(ActType::BF16, st.a, nullptr);
        ACEMI_HIP(hipEventRecord(e1, nullptr));
        ACEMI_HIP(hipEventSynchronize(e1));
        float ms = 0.f;
        ACEMI_HIP(hipEventElapsedTime(&ms, e0, e1));
        *avg_ms = ms / (float)iters;
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "ace_mi_bench_attention: %s\n", ex.what());
        return ACE_GGML_ERR;
    }
    return ACE_GGML_OK;
}



}  // extern "C"

extern "C" {

// GEMM micro-benchmark (random bf16/fp16 operands, device-resident): average ms per launch over
// `iters` launches timed with hipEvents.  variant -1 = the engine's automatic choice.
ace_ggml_status ace_mi_bench_gemm(int32_t act_type, int32_t epi, int32_t variant, int32_t M, int32_t N, int32_t K,
                                  int32_t iters, float* avg_ms) {
    using namespace acemi;
    if (M <= 0 || N % 128 != 0 || K % 64 != 0 || iters <= 0 || !avg_ms) return ACE_GGML_ERR_INVALID_ARG;
    try {
        std::vector<uint16_t> ha((size_t)M * K), hw((size_t)N * K);
        uint32_t st = 12345u;
        auto rnd = [&]() {  // uniform in [-1, 1) as bf16 / fp16 bits
            st = st * 1664525u + 1013904223u;
            const float f = (float)(st >> 8) * (2.0f / 16777216.0f) - 1.0f;
            if (act_type == 1) {
                _Float16 h = (_Float16)f;
                return __builtin_bit_cast(uint16_t, h);
            }
            uint32_t u;
            std::memcpy(&u, &f, 4);
            return (uint16_t)(u >> 16);
        };
        for (auto& v : ha) v = rnd();
        for (auto& v : hw) v = rnd();
        DevMem dA(ha.size() * 2), dW(hw.size() * 2), dC((size_t)M * N * 4), dG((size_t)N * 4);
        ACEMI_HIP(hipMemcpy(dA.p, ha.data(), ha.size() * 2, hipMemcpyHostToDevice));
        ACEMI_HIP(hipMemcpy(dW.p, hw.data(), hw.size() * 2, hipMemcpyHostToDevice));
        ACEMI_HIP(hipMemset(dC.p, 0, (size_t)M * N * 4));
        ACEMI_HIP(hipMemset(dG.p, 0, (size_t)N * 4));
        GemmEpilogue e;
        e.kind = epi;
        e.ldc = (epi == EPI_SWIGLU) ? N / 2 : N;
        e.c_f32 = dC.as<float>();
        e.c_act = dC.as<uint16_t>();
        e.gate = dG.as<float>();
        e.rows_per_item = M;
        const ActType at = act_type == 1 ? ActType::F16 : ActType::BF16;
        // ACE_MI_BENCH_COLD=R: rotate over R device copies of W (R x |W| beyond the 256 MB MALL = weights cold in
        // every launch, as in a forward where each layer's weights were last read one step earlier)
        const char* ce = std::getenv("ACE_MI_BENCH_COLD");
        const int R = ce ? std::max(1, std::min(64, std::atoi(ce))) : 1;
        DevMem dWr((size_t)R * hw.size() * 2);
        for (int r = 0; r < R; ++r)
            ACEMI_HIP(hipMemcpy(dWr.as<uint16_t>() + (size_t)r * hw.size(), dW.p, hw.size() * 2, hipMemcpyDeviceToDevice));
        auto wptr = [&](int i) { return dWr.as<uint16_t>() + (size_t)(i % R) * hw.size(); };
        gemm_force_variant(variant);
        hipEvent_t e0, e1;
        ACEMI_HIP(hipEventCreate(&e0));
        ACEMI_HIP(hipEventCreate(&e1));
        for (int i = 0; i < 3; ++i) launch_gemm(at, dA.as<uint16_t>(), K, wptr(i), K, M, N, K, e, nullptr);
        ACEMI_HIP(hipEventRecord(e0, nullptr));
        for (int i = 0; i < iters; ++i)
            launch_gemm(at, dA.as<uint16_t>(), K, wptr(i + 3), K, M, N, K, e, nullptr);
        ACEMI_HIP(hipEventRecord(e1, nullptr));
        ACEMI_HIP(hipEventSynchronize(e1));
        float ms = 0.f;
        ACEMI_HIP(hipEventElapsedTime(&ms, e0, e1));
        *avg_ms = ms / iters;
        gemm_force_variant(-1);
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
    } catch (const std::exception& ex) {
        gemm_force_variant(-1);
        std::fprintf(stderr, "ace_mi_bench_gemm: %s\n", ex.what());
        return ACE_GGML_ERR;
    }
    return ACE_GGML_OK;
}

}  // extern "C"

extern "C" {

// Staged dequant kernel on ggml block rows W [N][K]: out = bf16 bits of bf16(dequant(W)) [N][K].
ace_ggml_status ace_mi_kernel_dequant(int32_t qtype, int32_t N, int32_t K, const uint8_t* W_blocks, uint16_t* out) {
    using namespace acemi;
    const auto t = static_cast<quant::QType>(qtype);
    if (!W_blocks || !out || N <= 0 || K <= 0) return ACE_GGML_ERR_INVALID_ARG;
    if (t != quant::Q8_0 && t != quant::Q4_K && t != quant::Q6_K) return ACE_GGML_ERR_INVALID_ARG;
    if (!quant::applies(t, K)) return ACE_GGML_ERR_INVALID_ARG;
    try {
        std::vector<uint8_t> qp(quant::q_plane_bytes(t, N, K));
        std::vector<float> sp(quant::s_plane_floats(t, N, K));
        quant::to_planes(t, W_blocks, N, K, qp.data(), sp.data());
        DevMem dq(qp.size()), ds(sp.size() * 4), dout((size_t)N * K * 2);
        ACEMI_HIP(hipMemcpy(dq.p, qp.data(), qp.size(), hipMemcpyHostToDevice));
        ACEMI_HIP(hipMemcpy(ds.p, sp.data(), sp.size() * 4, hipMemcpyHostToDevice));
        WeightView w;
        w.fmt = t == quant::Q8_0 ? WF_Q8_0 : t == quant::Q4_K ? WF_Q4_K : WF_Q6_K;
        w.q = dq.p;
        w.s = ds.as<float>();
        launch_dequant_bf16(w, N, K, dout.as<uint16_t>(), nullptr);
        ACEMI_HIP(hipDeviceSynchronize());
        ACEMI_HIP(hipMemcpy(out, dout.p, (size_t)N * K * 2, hipMemcpyDeviceToHost));
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "ace_mi_kernel_dequant: %s\n", ex.what());
        return ACE_GGML_ERR;
    }
    return ACE_GGML_OK;
}

// Raw-block expansion (kernels/dequant_blocks.hip) of n_segs row segments into one host matrix out [total_rows][K]
// of bf16 words, whose initial content is kept wherever no segment writes.  Blocks are host pointers.
ace_ggml_status ace_mi_kernel_dequant_segments(int32_t n_segs, const ace_mi_block_seg* segs, int32_t total_rows,
                                               int32_t K, uint16_t* out) {
    using namespace acemi;
    if (!segs || !out || n_segs <= 0 || total_rows <= 0 || K <= 0) return ACE_GGML_ERR_INVALID_ARG;
    for (int i = 0; i < n_segs; ++i) {  // every row a segment may write lies inside the host matrix
        const ace_mi_block_seg& g = segs[i];
        const quant::QType q = quant::from_ggml(g.type);
        if (q == quant::QNONE || !g.blocks || g.rows <= 0 || g.row0 < 0 || g.step < 1 || g.group < 1 ||
            !quant::applies(q, K))
            return ACE_GGML_ERR_INVALID_ARG;
        BlockSeg b;
        b.row0 = g.row0;
        b.step = g.step;
        b.group = g.group;
        for (int r = 0; r < g.rows; ++r)
            if (block_seg_row(b, r) >= total_rows) return ACE_GGML_ERR_INVALID_ARG;
    }
    try {
        std::vector<std::unique_ptr<DevMem>> src;
        DevMem dout((size_t)total_rows * K * 2);
        ACEMI_HIP(hipMemcpy(dout.p, out, (size_t)total_rows * K * 2, hipMemcpyHostToDevice));
        std::vector<DequantBlocksJob> jobs;
        for (int i = 0; i < n_segs; ++i) {
            const ace_mi_block_seg& g = segs[i];
            const size_t bytes = (size_t)g.rows * quant::row_bytes(quant::from_ggml(g.type), K);
            src.emplace_back(new DevMem(((bytes + 15) & ~size_t(15)) + 16));
            ACEMI_HIP(hipMemcpy(src.back()->p, g.blocks, bytes, hipMemcpyHostToDevice));
            DequantBlocksJob j;
            j.seg.type = g.type;
            j.seg.src = src.back()->p;
            j.seg.rows = g.rows;
            j.seg.row0 = g.row0;
            j.seg.step = g.step;
            j.seg.group = g.group;
            j.K = K;
            j.ld = K;
            j.out = dout.as<uint16_t>();
            jobs.push_back(j);
        }
        launch_dequant_blocks(jobs.data(), (int)jobs.size(), nullptr);
        ACEMI_HIP(hipDeviceSynchronize());
        ACEMI_HIP(hipMemcpy(out, dout.p, (size_t)total_rows * K * 2, hipMemcpyDeviceToHost));
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "ace_mi_kernel_dequant_segments: %s\n", ex.what());
        return ACE_GGML_ERR;
    }
    return ACE_GGML_OK;
}

// One matrix of one ggml type: out = bf16 words [N][K].
ace_ggml_status ace_mi_kernel_dequant_blocks(int32_t type, int32_t N, int32_t K, const uint8_t* blocks, uint16_t* out) {
    ace_mi_block_seg g{};
    g.type = type;
    g.rows = N;
    g.row0 = 0;
    g.step = 1;
    g.group = 1;
    g.blocks = blocks;
    return ace_mi_kernel_dequant_segments(1, &g, N, K, out);
}

// Time of one expansion of an [N][K] matrix, averaged over iters launches that rotate through enough copies of the
// blocks and of the image to exceed the memory-side cache: planes = 0 the raw-block kernel on ggml type `type`,
// planes = 1 the plane kernel (launch_dequant_bf16; Q8_0 / Q4_K / Q6_K).  The blocks are valid but arbitrary.
ace_ggml_status ace_mi_bench_dequant_blocks(int32_t type, int32_t planes, int32_t N, int32_t K, int32_t iters,
                                            float* avg_ms) {
    using namespace acemi;
    const quant::QType q = quant::from_ggml(type);
    if (!avg_ms || q == quant::QNONE || N <= 0 || iters <= 0 || !quant::applies(q, K) ||
        (planes && !quant::has_planes(q)))
        return ACE_GGML_ERR_INVALID_ARG;
    try {
        const size_t rb = quant::row_bytes(q, K), bytes = (size_t)N * rb;
        std::vector<uint8_t> blocks(bytes);
        for (size_t i = 0; i < bytes; ++i) blocks[i] = (uint8_t)(0x21u + (i * 37u) % 0x17u);  // fp16 fields: small, finite
        const size_t in_b = ((bytes + 15) & ~size_t(15)) + 16, out_b = (size_t)N * K * 2;
        const size_t qp_b = planes ? quant::q_plane_bytes(q, N, K) : 0, sp_b = planes ? quant::s_plane_floats(q, N, K) * 4 : 0;
        const size_t per = (planes ? qp_b + sp_b : in_b) + out_b;
        const int R = (int)std::max<size_t>(2, std::min<size_t>(32, ((size_t)640 << 20) / per + 1));
        std::vector<std::unique_ptr<DevMem>> in, in2, img;
        std::vector<uint8_t> qp(qp_b);
        std::vector<float> sp(sp_b / 4);
        if (planes) quant::to_planes(q, blocks.data(), N, K, qp.data(), sp.data());
        for (int r = 0; r < R; ++r) {
            img.emplace_back(new DevMem(out_b));
            if (planes) {
                in.emplace_back(new DevMem(qp_b));
                in2.emplace_back(new DevMem(sp_b));
                ACEMI_HIP(hipMemcpy(in.back()->p, qp.data(), qp_b, hipMemcpyHostToDevice));
                ACEMI_HIP(hipMemcpy(in2.back()->p, sp.data(), sp_b, hipMemcpyHostToDevice));
            } else {
                in.emplace_back(new DevMem(in_b));
                ACEMI_HIP(hipMemcpy(in.back()->p, blocks.data(), bytes, hipMemcpyHostToDevice));
            }
        }
        auto run = [&](int i) {
            const int r = i % R;
            if (planes) {
                WeightView w;
                w.fmt = q == quant::Q8_0 ? WF_Q8_0 : q == quant::Q4_K ? WF_Q4_K : WF_Q6_K;
                w.q = in[r]->p;
                w.s = in2[r]->as<float>();
                launch_dequant_bf16(w, N, K, img[r]->as<uint16_t>(), nullptr);
            } else {
                DequantBlocksJob j;
                j.seg.type = type;
                j.seg.src = in[r]->p;
                j.seg.rows = N;
                j.K = K;
                j.ld = K;
                j.out = img[r]->as<uint16_t>();
                launch_dequant_blocks(&j, 1, nullptr);
            }
        };
        hipEvent_t e0, e1;
        ACEMI_HIP(hipEventCreate(&e0));
        ACEMI_HIP(hipEventCreate(&e1));
        for (int i = 0; i < 3; ++i) run(i);
        ACEMI_HIP(hipEventRecord(e0, nullptr));
        for (int i = 0; i < iters; ++i) run(i + 3);
        ACEMI_HIP(hipEventRecord(e1, nullptr));
        ACEMI_HIP(hipEventSynchronize(e1));
        float ms = 0.f;
        ACEMI_HIP(hipEventElapsedTime(&ms, e0, e1));
        *avg_ms = ms / iters;
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "ace_mi_bench_dequant_blocks: %s\n", ex.what());
        return ACE_GGML_ERR;
    }
    return ACE_GGML_OK;
}

// LoRA merge kernel: n_jobs jobs of one launch on one host matrix pair (include/acestep_mi355x_selftest.h).
ace_ggml_status ace_mi_kernel_lora_merge(int32_t fmt, int32_t total_rows, int32_t cols, int32_t ld_base, int32_t ld_out,
                                         const uint16_t* base, uint16_t* out, const ace_mi_lora_job* jobs,
                                         int32_t n_jobs) {
    using namespace acemi;
    if (!out || !jobs || n_jobs <= 0 || total_rows <= 0 || cols <= 0 || ld_out < cols || (base && ld_base < cols) ||
        (fmt != 0 && fmt != 1))
        return ACE_GGML_ERR_INVALID_ARG;
    for (int i = 0; i < n_jobs; ++i) {  // every row a job may touch lies inside the host matrices
        const ace_mi_lora_job& j = jobs[i];
        if (j.row0 < 0 || j.rows <= 0 || j.row0 + j.rows > total_rows || j.r < 0 || (j.r > 0 && (!j.A || !j.B || j.rows_mod <= 0)))
            return ACE_GGML_ERR_INVALID_ARG;
    }
    try {
        const size_t nb = (size_t)total_rows * (base ? ld_base : ld_out) * 2, no = (size_t)total_rows * ld_out * 2;
        DevMem dbase(base ? nb : 16), dout(no);
        if (base) ACEMI_HIP(hipMemcpy(dbase.p, base, nb, hipMemcpyHostToDevice));
        ACEMI_HIP(hipMemcpy(dout.p, out, no, hipMemcpyHostToDevice));
        std::vector<std::unique_ptr<DevMem>> ab;
        std::vector<LoraMergeJob> lj(n_jobs);
        for (int i = 0; i < n_jobs; ++i) {
            const ace_mi_lora_job& j = jobs[i];
            LoraMergeJob& d = lj[i];
            d.fmt = fmt == 1 ? WF_F16 : WF_BF16;
            d.base = base ? dbase.as<uint16_t>() : dout.as<uint16_t>();
            d.ld_base = base ? ld_base : ld_out;
            d.out = dout.as<uint16_t>();
            d.ld_out = ld_out;
            d.row0 = j.row0;
            d.rows = j.rows;
            d.cols = cols;
            d.r = j.r;
            d.rows_mod = j.rows_mod;
            d.eff = j.eff;
            d.map = j.map;
            d.row_off = j.row_off;
            d.half = j.half;
            d.copy_rest = j.copy_rest != 0;
            if (j.r > 0) {
                const size_t na = (size_t)j.r * cols * 4, nbb = (size_t)j.rows_mod * j.r * 4;
                ab.emplace_back(new DevMem(na));
                ACEMI_HIP(hipMemcpy(ab.back()->p, j.A, na, hipMemcpyHostToDevice));
                d.A = ab.back()->as<float>();
                ab.emplace_back(new DevMem(nbb));
                ACEMI_HIP(hipMemcpy(ab.back()->p, j.B, nbb, hipMemcpyHostToDevice));
                d.B = ab.back()->as<float>();
            }
        }
        ACEMI_HIP(hipDeviceSynchronize());
        launch_lora_merge(lj.data(), n_jobs, nullptr);
        ACEMI_HIP(hipDeviceSynchronize());
        ACEMI_HIP(hipMemcpy(out, dout.p, no, hipMemcpyDeviceToHost));
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "ace_mi_kernel_lora_merge: %s\n", ex.what());
        return ACE_GGML_ERR;
    }
    return ACE_GGML_OK;
}

// Dequant-fused GEMM on ggml block rows W [N][K]: out = A(bf16) . bf16(dequant(W))^T (+ bias).
ace_ggml_status ace_mi_kernel_gemm_q(int32_t qtype, int32_t epi, int32_t variant, int32_t M, int32_t N, int32_t K,
                                     const uint16_t* A, const uint8_t* W_blocks, const float* bias, float* out_f32,
                                     uint16_t* out_u16) {
    using namespace acemi;
    const auto t = static_cast<quant::QType>(qtype);
    if (!A || !W_blocks || M <= 0 || N % 128 != 0 || K % 64 != 0) return ACE_GGML_ERR_INVALID_ARG;
    if (t != quant::Q8_0 && t != quant::Q4_K && t != quant::Q6_K) return ACE_GGML_ERR_INVALID_ARG;
    if (!quant::applies(t, K)) return ACE_GGML_ERR_INVALID_ARG;
    const bool resid = epi == EPI_RESID || epi == EPI_RESID_GATED;
    if (epi != EPI_STORE_F32 && epi != EPI_SWIGLU && !resid) return ACE_GGML_ERR_UNSUPPORTED;
    if (((epi == EPI_STORE_F32 || resid) && !out_f32) || (epi == EPI_SWIGLU && !out_u16))
        return ACE_GGML_ERR_INVALID_ARG;
    if (epi == EPI_RESID_GATED && !bias) return ACE_GGML_ERR_INVALID_ARG;
    if (!gemm_variant_arg_ok(variant, true)) return ACE_GGML_ERR_INVALID_ARG;  // (0x10000: past the support check)
    try {
        std::vector<uint8_t> qp(quant::q_plane_bytes(t, N, K));
        std::vector<float> sp(quant::s_plane_floats(t, N, K));
        quant::to_planes(t, W_blocks, N, K, qp.data(), sp.data());
        DevMem dA((size_t)M * K * 2), dQ(qp.size()), dS(sp.size() * 4), dB((size_t)N * 4), dC((size_t)M * N * 4);
        ACEMI_HIP(hipMemcpy(dA.p, A, (size_t)M * K * 2, hipMemcpyHostToDevice));
        ACEMI_HIP(hipMemcpy(dQ.p, qp.data(), qp.size(), hipMemcpyHostToDevice));
        ACEMI_HIP(hipMemcpy(dS.p, sp.data(), sp.size() * 4, hipMemcpyHostToDevice));
        if (bias) ACEMI_HIP(hipMemcpy(dB.p, bias, (size_t)N * 4, hipMemcpyHostToDevice));
        GemmEpilogue e;
        e.kind = epi;
        e.bias = bias && !resid ? dB.as<float>() : nullptr;
        if (resid) {  // out_f32 holds x on entry: x += acc (* gate[n], the gate passed as `bias`)
            ACEMI_HIP(hipMemcpy(dC.p, out_f32, (size_t)M * N * 4, hipMemcpyHostToDevice));
            e.c_f32 = dC.as<float>();
            e.ldc = N;
            e.gate = epi == EPI_RESID_GATED ? dB.as<float>() : nullptr;
            e.gate_stride = 0;
            e.rows_per_item = M;
        } else if (epi == EPI_STORE_F32) {
            e.c_f32 = dC.as<float>();
            e.ldc = N;
        } else {
            e.c_act = dC.as<uint16_t>();
            e.ldc = N / 2;
        }
        WeightView w;
        w.fmt = t == quant::Q8_0 ? WF_Q8_0 : (t == quant::Q4_K ? WF_Q4_K : WF_Q6_K);
        w.q = dQ.p;
        w.s = dS.as<float>();
        gemm_force_variant(variant);
        launch_gemm(dA.as<uint16_t>(), K, w, M, N, K, e, nullptr);
        gemm_force_variant(-1);
        ACEMI_HIP(hipDeviceSynchronize());
        if (epi == EPI_STORE_F32 || resid)
            ACEMI_HIP(hipMemcpy(out_f32, dC.p, (size_t)M * N * 4, hipMemcpyDeviceToHost));
        else
            ACEMI_HIP(hipMemcpy(out_u16, dC.p, (size_t)M * (N / 2) * 2, hipMemcpyDeviceToHost));
    } catch (const std::exception& ex) {
        gemm_force_variant(-1);
        std::fprintf(stderr, "ace_mi_kernel_gemm_q: %s\n", ex.what());
        return ACE_GGML_ERR;
    }
    return ACE_GGML_OK;
}

// ggml-faithful quantized-activation GEMM (kernels/gemm_a8.hip): x f32 [M][K] -> Q8_0 / Q8_K blocks on the device
// (returned in q_out [M][K], s_out [K/32][M], bsum_out [K/32][M] when non-null), then the integer-dot GEMM against
// ggml block rows W [N][K] with epilogue epi: 0 f32 store (+ bias), 3 residual (out_f32 holds x on entry; + bias),
// 7 SwiGLU f32 (out [M][N/2], gate|up interleaved in 16-column groups).
ace_ggml_status ace_mi_kernel_gemm_a8(int32_t qtype, int32_t epi, int32_t M, int32_t N, int32_t K, const float* x,
                                      const uint8_t* W_blocks, const float* bias, float* out_f32, int8_t* q_out,
                                      float* s_out, float* bsum_out) {
    using namespace acemi;
    const auto t = static_cast<quant::QType>(qtype);
    if (!x || !W_blocks || !out_f32 || M <= 0 || N % 128 != 0) return ACE_GGML_ERR_INVALID_ARG;
    if (t != quant::Q8_0 && t != quant::Q4_K && t != quant::Q6_K) return ACE_GGML_ERR_INVALID_ARG;
    if (!quant::applies(t, K)) return ACE_GGML_ERR_INVALID_ARG;
    if (epi != EPI_STORE_F32 && epi != EPI_RESID && epi != EPI_SWIGLU_F32) return ACE_GGML_ERR_UNSUPPORTED;
    try {
        const int64_t ld_s = (M + 127) / 128 * 128;
        const int nb = K / 32;
        const int ncol = epi == EPI_SWIGLU_F32 ? N / 2 : N;
        std::vector<uint8_t> qp(quant::q_plane_bytes(t, N, K));
        std::vector<float> sp(quant::s_plane_floats(t, N, K));
        quant::to_planes(t, W_blocks, N, K, qp.data(), sp.data());
        DevMem dX((size_t)M * K * 4), dQ(qp.size()), dS(sp.size() * 4), dB((size_t)N * 4), dC((size_t)M * ncol * 4),
            dAq((size_t)M * K), dAs((size_t)nb * ld_s * 4), dAb((size_t)nb * ld_s * 4);
        ACEMI_HIP(hipMemcpy(dX.p, x, (size_t)M * K * 4, hipMemcpyHostToDevice));
        ACEMI_HIP(hipMemcpy(dQ.p, qp.data(), qp.size(), hipMemcpyHostToDevice));
        ACEMI_HIP(hipMemcpy(dS.p, sp.data(), sp.size() * 4, hipMemcpyHostToDevice));
        ACEMI_HIP(hipMemset(dAs.p, 0, (size_t)nb * ld_s * 4));
        ACEMI_HIP(hipMemset(dAb.p, 0, (size_t)nb * ld_s * 4));
        if (bias) ACEMI_HIP(hipMemcpy(dB.p, bias, (size_t)N * 4, hipMemcpyHostToDevice));
        if (epi == EPI_RESID) ACEMI_HIP(hipMemcpy(dC.p, out_f32, (size_t)M * N * 4, hipMemcpyHostToDevice));
        ACEMI_HIP(hipDeviceSynchronize());
        QAct a;
        a.kind = t == quant::Q8_0 ? QACT_Q8_0 : QACT_Q8_K;
        a.q = dAq.as<int8_t>();
        a.s = dAs.as<float>();
        a.bsum = dAb.as<float>();
        a.ld_s = ld_s;
        // Q8_0 with K % 64 == 0 runs the bf16-MFMA form unless ace_mi_kernel_gemm_a8_mode(0) (or ACE_MI_QACT_GEMM=0)
        // keeps it on the i8 kernel: the int8 blocks are returned either way
        const bool bf16_path = gemm_a8_bf16_path(t == quant::Q8_0 ? WF_Q8_0 : WF_Q4_K, K);
        DevMem dA16(bf16_path ? (size_t)M * K * 2 : 16), dW16(bf16_path ? (size_t)N * K * 2 : 16);
        launch_quantize_act(a.kind, dX.as<float>(), K, M, K, false, dAq.as<int8_t>(), dAs.as<float>(), dAb.as<float>(),
                            ld_s, nullptr, bf16_path ? dA16.as<uint16_t>() : nullptr);
        if (bf16_path) {
            a.q16 = dA16.as<uint16_t>();
            launch_q8_image(dQ.as<int8_t>(), (int64_t)N * K, dW16.as<uint16_t>(), nullptr);
        }
        GemmEpilogue e;
        e.kind = epi;
        e.bias = bias ? dB.as<float>() : nullptr;
        e.c_f32 = dC.as<float>();
        e.ldc = ncol;
        WeightView w;
        w.fmt = t == quant::Q8_0 ? WF_Q8_0 : (t == quant::Q4_K ? WF_Q4_K : WF_Q6_K);
        w.q = dQ.p;
        w.s = dS.as<float>();
        launch_gemm_a8(a, w, M, N, K, e, nullptr, bf16_path ? dW16.as<uint16_t>() : nullptr);
        ACEMI_HIP(hipDeviceSynchronize());
        ACEMI_HIP(hipMemcpy(out_f32, dC.p, (size_t)M * ncol * 4, hipMemcpyDeviceToHost));
        if (q_out) ACEMI_HIP(hipMemcpy(q_out, dAq.p, (size_t)M * K, hipMemcpyDeviceToHost));
        for (int b = 0; b < nb; ++b) {
            if (s_out)
                ACEMI_HIP(hipMemcpy(s_out + (size_t)b * M, dAs.as<float>() + (size_t)b * ld_s, (size_t)M * 4,
                                    hipMemcpyDeviceToHost));
            if (bsum_out)
                ACEMI_HIP(hipMemcpy(bsum_out + (size_t)b * M, dAb.as<float>() + (size_t)b * ld_s, (size_t)M * 4,
                                    hipMemcpyDeviceToHost));
        }
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "ace_mi_kernel_gemm_a8: %s\n", ex.what());
        return ACE_GGML_ERR;
    }
    return ACE_GGML_OK;
}

// Which form ace_mi_kernel_gemm_a8 (and the q8 mode of this process) runs a Q8_0 GEMM in: -1 the environment / default
// (the bf16 MFMA), 0 the i8 kernel, 1 the bf16 MFMA.
ace_ggml_status ace_mi_kernel_gemm_a8_mode(int32_t mode) {
    if (mode < -1 || mode > 1) return ACE_GGML_ERR_INVALID_ARG;
    acemi::gemm_a8_mode(mode);
    return ACE_GGML_OK;
}

// Which kernel runs f8c attention in this process: -1 the environment / default policy, 0 attn2, 1 attn_kh_kernel.
ace_ggml_status ace_mi_kernel_attn_kh(int32_t mode) {
    if (mode < -1 || mode > 1) return ACE_GGML_ERR_INVALID_ARG;
    acemi::attn_kh_mode(mode);
    return ACE_GGML_OK;
}

// {ksplit_mode, tail, tail_min, xcd_order, kh, n_cu}, each -1 (unset) or inside its range
static bool attn_policy_fields_ok(const int32_t f[6], bool allow_unset) {
    const int32_t lo[6] = {0, 0, 2, 0, 0, 1}, hi[6] = {4, 1, 1 << 20, 1, 1, 1 << 20};
    for (int i = 0; i < 6; ++i) {
        const bool unset = f[i] == -1 && (allow_unset || i == 4);  // (kh = -1: the rule, also in a full policy)
        if (!unset && (f[i] < lo[i] || f[i] > hi[i])) return false;
    }
    return true;
}
static acemi::AttnPolicy attn_policy_of(const int32_t f[6]) { return {f[0], f[1], f[2], f[3], f[4], f[5]}; }

// The whole attention policy of this process (csrc/attn_plan.h): a field of -1 leaves the environment / the device in
// charge; all six -1 clears the override.
ace_ggml_status ace_mi_kernel_attn_policy(const int32_t fields[6]) {
    if (!fields || !attn_policy_fields_ok(fields, true)) return ACE_GGML_ERR_INVALID_ARG;
    acemi::attn_policy_override() = attn_policy_of(fields);
    return ACE_GGML_OK;
}

// The attention launch plan (csrc/attn_plan.h) for the CPU tests: pure, no device.
ace_ggml_status ace_mi_attn_plan(const int32_t shape[12], const int32_t policy[6], int32_t plan[8]) {
    using namespace acemi;
    if (!shape || !policy || !plan || !attn_policy_fields_ok(policy, false)) return ACE_GGML_ERR_INVALID_ARG;
    const AttnShape a{shape[0],      shape[1],      shape[2],      shape[3],      shape[4],       shape[5],
                      shape[6] != 0, shape[7] != 0, shape[8] != 0, shape[9] != 0, shape[10] != 0, shape[11] != 0};
    if (a.B < 1 || a.Hkv < 1 || a.Hq % a.Hkv != 0 || a.nq < 1 || a.nk < 1 || a.window < 0) return ACE_GGML_ERR_INVALID_ARG;
    const int rep = a.Hq / a.Hkv;
    if (rep != 1 && rep != 2 && rep != 4) return ACE_GGML_ERR_INVALID_ARG;
    const AttnPlan p = attn_plan(a, attn_policy_of(policy));
    const int32_t out[8] = {p.ksplit,        p.split_from,      p.xcd_order,      p.n_blk,
                            (int32_t)p.grid, (int32_t)p.kernel, (int32_t)p.merge, (int32_t)p.merge_grid};
    std::copy(out, out + 8, plan);
    return ACE_GGML_OK;
}

ace_ggml_status ace_mi_attn_plan_block(int32_t ksplit, int32_t split_from, int32_t xcd_order, int32_t n_blk, int32_t x,
                                       int32_t out[4]) {
    if (!out || ksplit < 1 || split_from < 0 || split_from > n_blk || n_blk < 1 || x < 0) return ACE_GGML_ERR_INVALID_ARG;
    const acemi::AttnBlock b = acemi::attn_block_of(ksplit, split_from, xcd_order, n_blk, x);
    const int32_t f[4] = {b.blk, b.part, b.parts, b.valid};
    std::copy(f, f + 4, out);
    return ACE_GGML_OK;
}

ace_ggml_status ace_mi_attn_plan_tiles(int32_t nk, int32_t window, int32_t causal, int32_t q0, int32_t qpb, int32_t part,
                                       int32_t parts, int32_t out[2]) {
    if (!out || nk < 1 || window < 0 || q0 < 0 || qpb < 1 || parts < 1 || part < 0 || part >= parts)
        return ACE_GGML_ERR_INVALID_ARG;
    const acemi::AttnKeyTiles t = acemi::attn_key_tiles(nk, window, causal != 0, q0, qpb, part, parts);
    out[0] = t.kt_begin;
    out[1] = t.n;
    return ACE_GGML_OK;
}

// Dequant-fused GEMM micro-benchmark (random N(0, 0.02) weights quantized with the loader's encoder).
ace_ggml_status ace_mi_bench_gemm_q(int32_t qtype, int32_t epi, int32_t variant, int32_t M, int32_t N, int32_t K,
                                    int32_t iters, float* avg_ms) {
    using namespace acemi;
    const auto t = static_cast<quant::QType>(qtype);
    if (M <= 0 || N % 128 != 0 || K % 64 != 0 || iters <= 0 || !avg_ms) return ACE_GGML_ERR_INVALID_ARG;
    if (t != quant::Q8_0 && t != quant::Q4_K && t != quant::Q6_K) return ACE_GGML_ERR_INVALID_ARG;
    if (!quant::applies(t, K)) return ACE_GGML_ERR_INVALID_ARG;
    try {
        uint32_t st = 777u;
        auto rnd = [&]() {
            st = st * 1664525u + 1013904223u;
            return ((float)(st >> 8) * (2.0f / 16777216.0f) - 1.0f);
        };
        std::vector<uint16_t> ha((size_t)M * K);
        for (auto& v : ha) {
            const float f = rnd();
            uint32_t u;
            std::memcpy(&u, &f, 4);
            v = (uint16_t)(u >> 16);
        }
        std::vector<float> hw((size_t)N * K);
        for (auto& v : hw) v = 0.02f * rnd();
        std::vector<uint8_t> blocks((size_t)N * quant::row_bytes(t, K));
        quant::quantize_rows(t, hw.data(), N, K, blocks.data());
        std::vector<uint8_t> qp(quant::q_plane_bytes(t, N, K));
        std::vector<float> sp(quant::s_plane_floats(t, N, K));
        quant::to_planes(t, blocks.data(), N, K, qp.data(), sp.data());
        DevMem dA(ha.size() * 2), dQ(qp.size()), dS(sp.size() * 4), dC((size_t)M * N * 4), dG((size_t)N * 4);
        ACEMI_HIP(hipMemcpy(dA.p, ha.data(), ha.size() * 2, hipMemcpyHostToDevice));
        ACEMI_HIP(hipMemcpy(dQ.p, qp.data(), qp.size(), hipMemcpyHostToDevice));
        ACEMI_HIP(hipMemcpy(dS.p, sp.data(), sp.size() * 4, hipMemcpyHostToDevice));
        ACEMI_HIP(hipMemset(dC.p, 0, (size_t)M * N * 4));
        ACEMI_HIP(hipMemset(dG.p, 0, (size_t)N * 4));
        GemmEpilogue e;
        e.kind = epi;
        e.ldc = (epi == EPI_SWIGLU) ? N / 2 : N;
        e.c_f32 = dC.as<float>();
        e.c_act = dC.as<uint16_t>();
        e.gate = dG.as<float>();
        e.rows_per_item = M;
        WeightView w;
        w.fmt = t == quant::Q8_0 ? WF_Q8_0 : (t == quant::Q4_K ? WF_Q4_K : WF_Q6_K);
        w.q = dQ.p;
        w.s = dS.as<float>();
        gemm_force_variant(variant);
        hipEvent_t e0, e1;
        ACEMI_HIP(hipEventCreate(&e0));
        ACEMI_HIP(hipEventCreate(&e1));
        for (int i = 0; i < 3; ++i) launch_gemm(dA.as<uint16_t>(), K, w, M, N, K, e, nullptr);
        ACEMI_HIP(hipEventRecord(e0, nullptr));
        for (int i = 0; i < iters; ++i) launch_gemm(dA.as<uint16_t>(), K, w, M, N, K, e, nullptr);
        ACEMI_HIP(hipEventRecord(e1, nullptr));
        ACEMI_HIP(hipEventSynchronize(e1));
        float ms = 0.f;
        ACEMI_HIP(hipEventElapsedTime(&ms, e0, e1));
        *avg_ms = ms / iters;
        gemm_force_variant(-1);
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
    } catch (const std::exception& ex) {
        gemm_force_variant(-1);
        std::fprintf(stderr, "ace_mi_bench_gemm_q: %s\n", ex.what());
        return ACE_GGML_ERR;
    }
    return ACE_GGML_OK;
}

// The GEMM variant table and picker (csrc/gemm_variants.h) for the CPU tests: pure, no device.
ace_ggml_status ace_mi_gemm_resolve(int32_t forced, int32_t override_v, int32_t M, int32_t N, int32_t K, int32_t wfmt,
                                    int32_t prep, int32_t* variant) {
    using namespace acemi;
    if (!variant || M < 1 || N < 1 || K < 1) return ACE_GGML_ERR_INVALID_ARG;
    const int v = gemm_resolve_variant(forced, override_v, M, N, K, weight_quantized(wfmt), wfmt);
    *variant = prep ? gemm_prep_sibling(v, forced >= 0) : v;
    return ACE_GGML_OK;
}

ace_ggml_status ace_mi_gemm_variant_row(int32_t id, int32_t fields[16], char* name, size_t name_size) {
    using namespace acemi;
    const GemmVariantRow* r = gemm_variant_row(id);
    if (!r || !fields) return ACE_GGML_ERR_INVALID_ARG;
    const GemmKernelSel* ks[2] = {&r->dense, &r->quant};
    for (int i = 0; i < 2; ++i) {
        const int32_t f[6] = {(int32_t)ks[i]->family, ks[i]->bm, ks[i]->bn, ks[i]->wm, ks[i]->wn, ks[i]->depth};
        std::copy(f, f + 6, fields + 6 * i);
    }
    fields[12] = r->dense_split;
    fields[13] = r->quant_split;
    fields[14] = r->prep_sibling;
    fields[15] = r->dense.needs_n256() || r->quant.needs_n256();
    if (name && name_size) {
        std::strncpy(name, r->name, name_size - 1);
        name[name_size - 1] = 0;
    }
    return ACE_GGML_OK;
}

ace_ggml_status ace_mi_gemm_variant_arg_ok(int32_t variant, int32_t allow_unchecked) {
    return acemi::gemm_variant_arg_ok(variant, allow_unchecked != 0) ? ACE_GGML_OK : ACE_GGML_ERR_INVALID_ARG;
}

}  // extern "C"

// ---- VAE conv kernels (kernels/vae.hip): one launch on host buffers, on a stream
namespace {

// a device copy of `n` elements of a host array (null host: null device pointer, nothing allocated)
template <typename T>
struct DevCopy {
    std::unique_ptr<DevMem> m;
    DevCopy(const T* host, size_t n) {
        if (!host) return;
        m = std::make_unique<DevMem>(n * sizeof(T));
        ACEMI_HIP(hipMemcpy(m->p, host, n * sizeof(T), hipMemcpyHostToDevice));
    }
    T* get() const { return m ? static_cast<T*>(m->p) : nullptr; }
};

struct Stream {
    hipStream_t s = nullptr;
    Stream() { ACEMI_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
    ~Stream() {
        if (s) (void)hipStreamDestroy(s);
    }
};

}  // namespace

extern "C" {

ace_ggml_status ace_mi_kernel_conv_gemm(const ace_mi_conv_gemm_args* g) {
    using namespace acemi;
    if (!g) return ACE_GGML_ERR_INVALID_ARG;
    // what the buffers are sized from; everything else is launch_conv_gemm's to refuse
    const int dims[] = {g->T_in, g->Cin, g->taps, g->M, g->N, g->Cout, g->T_out, g->items, g->up, g->in_stride};
    for (int d : dims)
        if (d < 1 || d > (1 << 24)) return ACE_GGML_ERR_INVALID_ARG;
    if (g->taps > 64 || g->guard < 0 || g->guard % 4 != 0 || g->guard > (1 << 24) || g->pad < 0 || g->crop < 0)
        return ACE_GGML_ERR_INVALID_ARG;
    if (!g->snake_ea != !g->snake_eb || !g->snake2_ea != !g->snake2_eb) return ACE_GGML_ERR_INVALID_ARG;
    const int64_t nS =(int64_t)g->items * g->T_in * g->Cin, nW = (int64_t)g->N * g->taps * g->Cin;
    const int64_t nP = (int64_t)g->items * g->T_out * g->Cout, nW2 = (int64_t)g->Cout * g->Cout;
    if (nS >= (1LL << 31) || nW >= (1LL << 31) || nP >= (1LL << 31) || nW2 >= (1LL << 31)) return ACE_GGML_ERR_INVALID_ARG;
    try {
        const size_t nO = (size_t)nP + 2 * (size_t)g->guard;
        DevCopy<uint16_t> dS(g->S, (size_t)nS), dW(g->W, (size_t)nW), dW2(g->W2, (size_t)nW2);
        DevCopy<float> dB(g->bias, (size_t)(g->up > 1 ? g->Cout : g->N)), dEa(g->snake_ea, (size_t)g->Cout),
            dEb(g->snake_eb, (size_t)g->Cout), dB2(g->bias2, (size_t)g->Cout), dEa2(g->snake2_ea, (size_t)g->N),
            dEb2(g->snake2_eb, (size_t)g->N);
        DevCopy<float> dX(g->X, nO);
        DevCopy<uint16_t> dSo(g->S_out, nO);
        DevMem zero(4096);  // VaeEngine::ensure(zero_, 4096)
        ACEMI_HIP(hipMemset(zero.p, 0, 4096));
        ACEMI_HIP(hipDeviceSynchronize());  // the uploads and the memset do not order against a non-blocking stream
        ConvGemmArgs a;
        a.S = dS.get();
        a.zero = zero.as<uint16_t>();
        a.W = dW.get();
        a.T_in = g->T_in;
        a.Cin = g->Cin;
        a.taps = g->taps;
        a.dil = g->dil;
        a.pad = g->pad;
        a.in_stride = g->in_stride;
        a.M = g->M;
        a.N = g->N;
        a.bias = dB.get();
        a.Cout = g->Cout;
        a.up = g->up;
        a.crop = g->crop;
        a.T_out = g->T_out;
        a.X = dX.get() ? dX.get() + g->guard : nullptr;
        a.resid = g->resid;
        a.store_x = g->store_x;
        a.S_out = dSo.get() ? dSo.get() + g->guard : nullptr;
        a.snake_ea = dEa.get();
        a.snake_eb = dEb.get();
        a.items = g->items;
        a.W2 = dW2.get();
        a.bias2 = dB2.get();
        a.snake2_ea = dEa2.get();
        a.snake2_eb = dEb2.get();
        Stream st;
        launch_conv_gemm(a, st.s);
        ACEMI_HIP(hipStreamSynchronize(st.s));
        if (g->X) ACEMI_HIP(hipMemcpy(g->X, dX.get(), nO * 4, hipMemcpyDeviceToHost));
        if (g->S_out) ACEMI_HIP(hipMemcpy(g->S_out, dSo.get(), nO * 2, hipMemcpyDeviceToHost));
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "ace_mi_kernel_conv_gemm: %s\n", ex.what());
        return ACE_GGML_ERR;
    }
    return ACE_GGML_OK;
}

ace_ggml_status ace_mi_kernel_conv_out(const uint16_t* S, int32_t T, int32_t items, const uint16_t* W, int32_t out_ch,
                                       float* out, int32_t guard) {
    using namespace acemi;
    if (!S || !W || !out || T < 1 || items < 1 || (out_ch != 1 && out_ch != 2) || guard < 0 || guard > (1 << 24) ||
        (int64_t)T * items >= (1LL << 24))
        return ACE_GGML_ERR_INVALID_ARG;
    try {
        const size_t nO = (size_t)T * items * out_ch + 2 * (size_t)guard;
        DevCopy<uint16_t> dS(S, (size_t)T * items * 128), dW(W, (size_t)out_ch * 7 * 128);
        DevCopy<float> dO(out, nO);
        ACEMI_HIP(hipDeviceSynchronize());
        Stream st;
        launch_conv_out(dS.get(), T, 128, dW.get(), out_ch, dO.get() + guard, st.s, items);
        ACEMI_HIP(hipStreamSynchronize(st.s));
        ACEMI_HIP(hipMemcpy(out, dO.get(), nO * 4, hipMemcpyDeviceToHost));
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "ace_mi_kernel_conv_out: %s\n", ex.what());
        return ACE_GGML_ERR;
    }
    return ACE_GGML_OK;
}

ace_ggml_status ace_mi_kernel_pack_f16(const float* x, int64_t rows, int32_t C, int32_t Cpad, uint16_t* y) {
    using namespace acemi;
    if (!x || !y || rows < 1 || C < 1 || Cpad < C || rows * Cpad >= (1LL << 31)) return ACE_GGML_ERR_INVALID_ARG;
    try {
        DevCopy<float> dx(x, (size_t)rows * C);
        DevCopy<uint16_t> dy(y, (size_t)rows * Cpad);
        ACEMI_HIP(hipDeviceSynchronize());
        Stream st;
        if (C == Cpad)
            launch_to_f16(dx.get(), rows * C, dy.get(), st.s);
        else
            launch_pack_f16(dx.get(), rows, C, Cpad, dy.get(), st.s);
        ACEMI_HIP(hipStreamSynchronize(st.s));
        ACEMI_HIP(hipMemcpy(y, dy.get(), (size_t)rows * Cpad * 2, hipMemcpyDeviceToHost));
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "ace_mi_kernel_pack_f16: %s\n", ex.what());
        return ACE_GGML_ERR;
    }
    return ACE_GGML_OK;
}

// ---- the RoPE table (runtime/devmem.h), without a kernel
ace_ggml_status ace_mi_rope_table_steps(int32_t steps, const int32_t* n, const int32_t* head_dim, const float* theta,
                                        int32_t* rows, float* cos_out, float* sin_out) {
    if (steps < 1 || !n || !head_dim || !theta || !rows || !cos_out || !sin_out) return ACE_GGML_ERR_INVALID_ARG;
    for (int i = 0; i < steps; ++i)
        if (n[i] < 1 || n[i] > (1 << 20) || head_dim[i] < 2 || head_dim[i] > 1024 || head_dim[i] % 2 != 0 ||
            !(theta[i] > 0.0f))
            return ACE_GGML_ERR_INVALID_ARG;
    try {
        acemi::RopeTable t;
        for (int i = 0; i < steps; ++i) {
            t.ensure(n[i], head_dim[i], theta[i], nullptr);
            rows[i] = t.rows();
        }
        const size_t bytes = (size_t)t.rows() * (head_dim[steps - 1] / 2) * 4;
        ACEMI_HIP(hipMemcpy(cos_out, t.cos(), bytes, hipMemcpyDeviceToHost));
        ACEMI_HIP(hipMemcpy(sin_out, t.sin(), bytes, hipMemcpyDeviceToHost));
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "ace_mi_rope_table: %s\n", ex.what());
        return ACE_GGML_ERR;
    }
    return ACE_GGML_OK;
}

ace_ggml_status ace_mi_rope_table(int32_t n, int32_t head_dim, float theta, float* cos_out, float* sin_out) {
    int32_t rows = 0;
    return ace_mi_rope_table_steps(1, &n, &head_dim, &theta, &rows, cos_out, sin_out);
}

}  // extern "C"
