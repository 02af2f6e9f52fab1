// BlockRunner (blocks.h): the encoder-layer loop of the condition encoders and the Qwen3 text encoder.
#include "blocks.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "operands.h"

namespace acemi {

BlockRunner::BlockRunner() {
    // the condition / text encoders (once per request) keep the f32-faithful default
    const AttnPrecision prec = attn_precision_from_env(AttnPrecision::F32);
    split_ = prec != AttnPrecision::FP16;
    pv_split_ = prec == AttnPrecision::F32;
}

float* BlockRunner::x(int64_t rows, int H) {
    ensure(x_, (size_t)rows * H * 4);
    return get<float>(x_);
}

void BlockRunner::run(const BlockShape& sh, const std::vector<DevLayer>& layers, int n_layers, ActType at, int B,
                      int n, const int32_t* key_mask, bool causal, hipStream_t s, const AfterQkv* after_qkv) {
    const int H = sh.hidden, D = sh.head_dim, I = sh.intermediate;
    ACEMI_CHECK(B >= 1 && n >= 1 && D == 128, "blocks: bad shape");
    ACEMI_CHECK(n_layers >= 0 && n_layers <= (int)layers.size(), "blocks: layer count");
    const int M = (int)((int64_t)B * n);
    const int Npad = (int)round_up(n, 128);
    const AttnDims dims{B, sh.hq, sh.hkv, D, n, Npad, sh.eps};
    const AttnPlanes planes{split_, pv_split_, false};
    const int qd = dims.qd(), kd = dims.kd();
    const int64_t q_plane = dims.q_plane(), k_plane = dims.k_plane();
    ACEMI_CHECK(x_.bytes >= (size_t)M * H * 4, "blocks: residual stream not initialised");
    ensure(act_, (size_t)M * std::max(H, qd) * 2);
    ensure(attn_, (size_t)M * qd * 2);
    ensure(act2_, (size_t)M * std::max(I, 1) * 2);
    ensure(qkv_, (size_t)M * (qd + 2 * kd) * 4);
    ensure(qh_, (size_t)2 * q_plane * 2);
    ensure(kh_, (size_t)2 * k_plane * 2);
    ensure(vt_, (size_t)2 * k_plane * 2);
    ensure(kbias_, (size_t)B * Npad * 4);
    rope_.ensure(n, D, sh.rope_theta, s);
    float* x = get<float>(x_);
    uint16_t* act = get<uint16_t>(act_);
    uint16_t* attn = get<uint16_t>(attn_);
    uint16_t* act2 = get<uint16_t>(act2_);
    float* qkv = get<float>(qkv_);
    uint16_t *qh = get<uint16_t>(qh_), *kh = get<uint16_t>(kh_), *vt = get<uint16_t>(vt_);
    launch_key_bias(key_mask, B, n, 1, n, Npad, get<float>(kbias_), s);
    const float* kbias = key_mask ? get<float>(kbias_) : nullptr;  // padding keys are masked in-kernel
    for (int li = 0; li < n_layers; ++li) {
        const DevLayer& ly = layers[li];
        launch_rmsnorm_mod(at, x, M, H, ly.self_norm, nullptr, nullptr, 0, n, sh.eps, act, s);
        launch_gemm(act, H, ly.w_qkv.view(), M, qd + 2 * kd, H, epi_store_f32(qkv, qd + 2 * kd), s);
        if (after_qkv) (*after_qkv)(li, qkv, qd + 2 * kd);
        launch_attn_prep(self_prep(dims, planes, qkv, qd + 2 * kd, ly.sq_norm, ly.sk_norm, rope_.cos(), rope_.sin(), qh,
                                   kh, vt),
                         s);
        launch_attention(at,
                         attn_args(dims, planes, qh, kh, vt, kbias, n, Npad, dims.k_plane(),
                                   ly.sliding ? std::max(sh.sliding_window, 0) : 0, causal, nullptr, attn),
                         s);
        launch_gemm(attn, qd, ly.w_o.view(), M, H, qd, epi_resid(x, H), s);  // h = x + o_proj(attn)
        launch_rmsnorm_mod(at, x, M, H, ly.mlp_norm, nullptr, nullptr, 0, n, sh.eps, act, s);
        launch_gemm(act, H, ly.w_gu.view(), M, 2 * I, H, epi_swiglu(act2, I), s);
        launch_gemm(act2, I, ly.w_down.view(), M, H, I, epi_resid(x, H), s);  // x = h + down(act)
    }
}

void BlockRunner::finish(const BlockShape& sh, const float* w, int B, int n, bool first_only, float* out,
                         hipStream_t s) {
    const int H = sh.hidden;
    const int rows = first_only ? B : B * n;
    const int64_t step = first_only ? n : 1;
    const float* x = get<float>(x_);
    if (w) {
        launch_rmsnorm_f32(x, rows, step, H, w, sh.eps, out, s);
    } else {
        ACEMI_HIP(hipMemcpy2DAsync(out, (size_t)H * 4, x, (size_t)step * H * 4, (size_t)H * 4, rows,
                                   hipMemcpyDeviceToDevice, s));
    }
}

}  // namespace acemi
