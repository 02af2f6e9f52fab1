// Plain C++ restatement of the chunk path's launchers (kernels.h: launch_lm_chunk_kv of kernels/lm_decode.hip,
// launch_lm_attention_chunk and lm_attn_chunk_part_floats of kernels/lm_attn_chunk.hip) for a build of the runtime
// without a device compiler, as lm_score_host.h is for the scoring kernel: included by runtime/lm.cpp alone, empty
// under hipcc.  The same launcher conditions, slots, masks and rounding points; the sums are those of the host build's
// launch_lm_attention (per range m, l and O in key order, the ranges joined in ascending order), so a row of a chunk
// gets what the host build's decode step gets for the same token.
#pragma once

#ifndef __HIP__
#include <algorithm>
#include <cmath>
#include <cstring>

#include "../kernels.h"

namespace acemi {

namespace lm_chunk_host {

inline float f16_value(uint16_t h) {
    _Float16 v;
    std::memcpy(&v, &h, 2);
    return (float)v;
}
inline uint16_t f16_sat(float f) {
    const _Float16 v = (_Float16)std::min(std::max(f, -65504.0f), 65504.0f);
    uint16_t h;
    std::memcpy(&h, &v, 2);
    return h;
}
inline uint16_t to_act(float v, bool f16) {
    if (f16) {
        const _Float16 hv = (_Float16)v;
        uint16_t w;
        std::memcpy(&w, &hv, 2);
        return w;
    }
    uint32_t u;
    std::memcpy(&u, &v, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 64u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
inline void norm_rope(float* v, const float* w, const float* cs, const float* sn, float eps) {
    float ss = 0.f;
    for (int i = 0; i < 128; ++i) ss += v[i] * v[i];
    const float sc = 1.0f / std::sqrt(ss / 128.0f + eps);
    for (int i = 0; i < 128; ++i) v[i] = (v[i] * sc) * w[i];
    for (int i = 0; i < 64; ++i) {
        const float a = v[i], b = v[64 + i];
        v[i] = a * cs[i] - b * sn[i];
        v[64 + i] = a * sn[i] + b * cs[i];
    }
}

}  // namespace lm_chunk_host

void launch_lm_chunk_kv(const LmQkvPostArgs& a, int B, int n, const int32_t* mask, hipStream_t) {
    using namespace lm_chunk_host;
    ACEMI_CHECK(B >= 1 && B <= LM_MAX_BATCH && n >= 1 && a.pos >= 0 && (int64_t)a.pos + n <= a.capacity && a.q_out,
                "lm_chunk_kv: rows outside the cache");
    for (int b = 0; b < B; ++b)
        for (int t = 0; t < n; ++t) {
            const int64_t m = (int64_t)b * n + t;
            const int slot = a.pos + t;
            const bool valid = mask ? mask[m] != 0 : true;
            a.key_mask[(int64_t)b * a.capacity + slot] = valid ? 1 : 0;
            float* row = const_cast<float*>(a.qkv) + m * a.ld;
            if (!valid) std::fill(row, row + (int64_t)(a.hq + 2 * a.hkv) * 128, 0.f);
            const float* cs = a.rope_cos + (int64_t)slot * 64;
            const float* sn = a.rope_sin + (int64_t)slot * 64;
            for (int h = 0; h < a.hq + 2 * a.hkv; ++h) {
                float v[128];
                std::memcpy(v, row + (int64_t)h * 128, sizeof(v));
                if (h < a.hq) {
                    if (valid) norm_rope(v, a.q_norm, cs, sn, a.eps);
                    std::memcpy(a.q_out + (m * a.hq + h) * 128, v, sizeof(v));
                    continue;
                }
                const bool is_k = h < a.hq + a.hkv;
                const int kh = is_k ? h - a.hq : h - a.hq - a.hkv;
                if (is_k && valid) norm_rope(v, a.k_norm, cs, sn, a.eps);
                uint16_t* dst = (is_k ? a.k_cache : a.v_cache) + (((int64_t)b * a.hkv + kh) * a.capacity + slot) * 128;
                for (int i = 0; i < 128; ++i) dst[i] = f16_sat(v[i]);
            }
        }
}

size_t lm_attn_chunk_part_floats(int B, int n, int hq, int nk) {
    return (size_t)B * n * hq * ceil_div(nk, LM_SPLIT_KEYS) * 130;
}

void launch_lm_attention_chunk(ActType out_t, const LmAttnChunkArgs& a, int B, int hq, hipStream_t) {
    using namespace lm_chunk_host;
    const int rep = lm_attn_chunk_check(a, B, hq);
    for (int b = 0; b < B; ++b)
        for (int t = 0; t < a.n; ++t)
            for (int head = 0; head < hq; ++head) {
                const int64_t orow = ((int64_t)b * a.n + t) * hq + head;
                const float* q = a.q + orow * 128;
                const int64_t base = ((int64_t)b * a.hkv + head / rep) * a.capacity;
                const int nk = a.past + t + 1;
                float M = -INFINITY, L = 0.f, O[128] = {};
                for (int k0 = 0; k0 < nk; k0 += LM_SPLIT_KEYS) {
                    const int k1 = std::min(nk, k0 + LM_SPLIT_KEYS);
                    float sc[LM_SPLIT_KEYS], m = -INFINITY;
                    for (int k = k0; k < k1; ++k) {
                        float d = 0.f;
                        for (int i = 0; i < 128; ++i) d = std::fma(q[i], f16_value(a.k_cache[(base + k) * 128 + i]), d);
                        sc[k - k0] = a.key_mask[(int64_t)b * a.capacity + k] ? d * a.scale : -INFINITY;
                        m = std::max(m, sc[k - k0]);
                    }
                    float l = 0.f, o[128] = {};
                    for (int k = k0; k < k1; ++k) {
                        if (sc[k - k0] == -INFINITY) continue;  // a masked key's V never reaches the result
                        const float p = std::exp(sc[k - k0] - m);
                        l += p;
                        for (int i = 0; i < 128; ++i) o[i] = std::fma(p, f16_value(a.v_cache[(base + k) * 128 + i]), o[i]);
                    }
                    const float Mn = std::max(M, m);
                    const float w0 = M == -INFINITY ? 0.f : std::exp(M - Mn), w1 = m == -INFINITY ? 0.f : std::exp(m - Mn);
                    L = L * w0 + l * w1;
                    for (int i = 0; i < 128; ++i) O[i] = O[i] * w0 + o[i] * w1;
                    M = Mn;
                }
                for (int i = 0; i < 128; ++i) a.out[orow * 128 + i] = to_act(L > 0.f ? O[i] / L : 0.f, out_t == ActType::F16);
            }
}

}  // namespace acemi
#endif  // !__HIP__
