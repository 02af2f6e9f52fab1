// Plain C++ restatement of kernels/lm_decode_q.hip's launchers (launch_lm_skinny_q, launch_lm_embed_q,
// lm_skinny_q_chain of kernels.h) for a build of the runtime without a device compiler: the CPU tests' LM host library
// links runtime/lm.cpp with host loops for every other launch_* too.  Included by runtime/lm.cpp alone, so the
// definitions exist once; under hipcc (the product, where lm_decode_q.hip defines the three) this header is empty.
// Same weight values and rounding points as the kernels (the plane dequant as one f32 fma, RNE to bf16 for the
// product, unrounded for the gather); the sum runs in plain ascending k, so its addition chain is K long.
#pragma once

#ifndef __HIP__
#include <algorithm>
#include <cmath>
#include <cstring>

#include "../kernels.h"

namespace acemi {

namespace lmq_host {

inline float bf16_round(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) {
        u = (u | 0x00400000u) & 0xffff0000u;
    } else {
        u += 0x7fffu + ((u >> 16) & 1u);
        u &= 0xffff0000u;
    }
    std::memcpy(&f, &u, 4);
    return f;
}
inline float bf16_value(uint16_t h) {
    const uint32_t u = (uint32_t)h << 16;
    float r;
    std::memcpy(&r, &u, 4);
    return r;
}
inline uint16_t bf16_bits(float f) {
    f = bf16_round(f);
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return (uint16_t)(u >> 16);
}
inline bool k_ok(int fmt, int K) { return fmt == WF_Q8_0 ? (K >= 32 && K % 32 == 0) : (K >= 256 && K % 256 == 0); }

// the f32 plane dequant of W[row][k] (runtime/quant.h's layout; one rounding)
inline float plane_value(int fmt, const uint8_t* q, const float* s, int64_t row, int K, int k) {
    if (fmt == WF_Q4_K) {
        const int g = k / 32, kk = k % 32;  // byte i of the block's 16: low nibble k = 8(i/4) + i%4, high nibble k + 4
        const uint8_t byte = q[row * (K / 2) + (int64_t)g * 16 + 4 * (kk / 8) + kk % 4];
        const int nib = (kk % 8) < 4 ? (byte & 0xF) : (byte >> 4);
        const float* sm = s + (row * (K / 32) + g) * 2;
        return std::fma((float)nib, sm[0], -sm[1]);
    }
    const float sc = fmt == WF_Q8_0 ? s[row * (K / 32) + k / 32] : s[row * (K / 16) + k / 16];
    return (float)(int)(int8_t)q[row * K + k] * sc;  // the kernel's fma(u, s, -128 s) but for the sign of a zero
}

}  // namespace lmq_host

int lm_skinny_q_chain(int, int K) { return K; }

void launch_lm_skinny_q(const uint16_t* x, int ldx, int B, const WeightView& W, int N, int K, int epi, float* y_f32,
                        uint16_t* y_act, int ldy, hipStream_t) {
    using namespace lmq_host;
    ACEMI_CHECK(weight_planes(W.fmt) && W.q && W.s, "lm_skinny_q: the weight is not in block planes");
    ACEMI_CHECK(B >= 1 && B <= LM_MAX_BATCH && N >= 1 && k_ok(W.fmt, K) && ldx % 8 == 0 && ldx >= K && x,
                "lm_skinny_q: bad shape");
    ACEMI_CHECK(epi == LM_EPI_SWIGLU ? (N % 32 == 0 && y_act) : ((epi == LM_EPI_STORE || epi == LM_EPI_RESID) && y_f32),
                "lm_skinny_q: bad epilogue");
    const uint8_t* q = static_cast<const uint8_t*>(W.q);
    auto dot = [&](int b, int64_t row) {
        float acc = 0.f;
        for (int k = 0; k < K; ++k)
            acc = std::fma(bf16_round(plane_value(W.fmt, q, W.s, row, K, k)), bf16_value(x[(int64_t)b * ldx + k]), acc);
        return acc;
    };
    for (int b = 0; b < B; ++b) {
        if (epi == LM_EPI_SWIGLU) {
            for (int j = 0; j < N / 2; ++j) {
                const int64_t rg = (int64_t)(j >> 4) * 32 + (j & 15);
                const float g = dot(b, rg), u = dot(b, rg + 16);
                y_act[(int64_t)b * ldy + j] = bf16_bits(g / (1.0f + std::exp(-g)) * u);
            }
        } else {
            for (int n = 0; n < N; ++n) {
                const float v = dot(b, n);
                if (epi == LM_EPI_RESID)
                    y_f32[(int64_t)b * ldy + n] += v;
                else
                    y_f32[(int64_t)b * ldy + n] = v;
            }
        }
    }
}

void launch_lm_embed_q(int fmt, const void* q, const float* s, const int32_t* ids, int n, int vocab, int H, float* out,
                       hipStream_t) {
    using namespace lmq_host;
    ACEMI_CHECK(n >= 1 && vocab >= 1 && q && ids && out, "lm_embed_q: bad arguments");
    if (fmt == LM_EMBED_F32)
        ACEMI_CHECK(H >= 4 && H % 4 == 0, "lm_embed_q: bad row length");
    else
        ACEMI_CHECK(weight_planes(fmt) && s && k_ok(fmt, H), "lm_embed_q: bad format or row length");
    for (int t = 0; t < n; ++t) {
        const int64_t row = std::min(std::max(ids[t], 0), vocab - 1);
        for (int i = 0; i < H; ++i)
            out[(int64_t)t * H + i] = fmt == LM_EMBED_F32 ? static_cast<const float*>(q)[row * H + i]
                                                           : plane_value(fmt, static_cast<const uint8_t*>(q), s, row, H, i);
    }
}

}  // namespace acemi
#endif  // !__HIP__
