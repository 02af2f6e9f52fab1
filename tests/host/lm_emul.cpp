// Host restatement of kernels/lm_decode.hip (the launch_lm_* entries of kernels.h) as plain loops, linked with
// tests/host/kernel_emul.cpp and the product's runtime/*.cpp + runtime/lm.cpp by tests/lmhostlib.py: the LM engine's
// control flow, cache indexing and rounding points run on the CPU (tests/test_lm_cpu.py, tests/host/lm_asan_driver.cpp).
// Same rounding points as the kernels; summation orders differ (f32 sums in index order here).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "kernels.h"

namespace acemi {

namespace {

float from16(uint16_t h, bool f16) {
    if (f16) {
        _Float16 v;
        std::memcpy(&v, &h, 2);
        return (float)v;
    }
    const uint32_t u = (uint32_t)h << 16;
    float r;
    std::memcpy(&r, &u, 4);
    return r;
}
uint16_t to16(float f, bool f16) {
    if (f16) {
        const _Float16 v = (_Float16)f;
        uint16_t h;
        std::memcpy(&h, &v, 2);
        return h;
    }
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 64u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
uint16_t f16_sat(float f) { return to16(std::min(std::max(f, -65504.0f), 65504.0f), true); }

void norm_rope(float* v, const float* w, const float* cs, const float* sn, float eps) {
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

void store_head(uint16_t* dst, const float* v) {
    for (int i = 0; i < 128; ++i) dst[i] = f16_sat(v[i]);
}

}  // namespace

void launch_lm_skinny(ActType t, const uint16_t* x, int ldx, int B, const uint16_t* W, int N, int K, int epi,
                      float* y_f32, uint16_t* y_act, int ldy, hipStream_t) {
    ACEMI_CHECK(B >= 1 && B <= LM_MAX_BATCH && K % 8 == 0 && ldx % 8 == 0, "lm_skinny: bad shape");
    const bool f16 = t == ActType::F16;
    auto dot = [&](int b, int64_t row) {
        float acc = 0.f;
        for (int k = 0; k < K; ++k) acc = std::fma(from16(W[row * K + k], f16), from16(x[(int64_t)b * ldx + k], f16), acc);
        return acc;
    };
    for (int b = 0; b < B; ++b) {
        if (epi == LM_EPI_SWIGLU) {
            for (int j = 0; j < N / 2; ++j) {
                const int64_t rg = (int64_t)(j >> 4) * 32 + (j & 15);
                const float g = dot(b, rg), u = dot(b, rg + 16);
                y_act[(int64_t)b * ldy + j] = to16(g / (1.0f + std::exp(-g)) * u, f16);
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

void launch_lm_embed(const void* table, int fmt, const int32_t* ids, int n, int vocab, int H, float* out, hipStream_t) {
    const uint16_t* tb = static_cast<const uint16_t*>(table);
    for (int t = 0; t < n; ++t) {
        const int64_t row = std::min(std::max(ids[t], 0), vocab - 1);
        for (int i = 0; i < H; ++i) out[(int64_t)t * H + i] = from16(tb[row * H + i], fmt == 1);
    }
}

void launch_lm_qkv_post(const LmQkvPostArgs& a, int B, hipStream_t) {
    ACEMI_CHECK(a.pos >= 0 && a.pos < a.capacity, "lm_qkv_post: position outside the cache");
    const float* cs = a.rope_cos + (int64_t)a.pos * 64;
    const float* sn = a.rope_sin + (int64_t)a.pos * 64;
    for (int b = 0; b < B; ++b) {
        a.key_mask[(int64_t)b * a.capacity + a.pos] = a.mask_new ? (a.mask_new[b] != 0) : 1;
        for (int h = 0; h < a.hq + 2 * a.hkv; ++h) {
            float v[128];
            std::memcpy(v, a.qkv + (int64_t)b * a.ld + (int64_t)h * 128, sizeof(v));
            if (h < a.hq) {
                norm_rope(v, a.q_norm, cs, sn, a.eps);
                std::memcpy(a.q_out + ((int64_t)b * a.hq + h) * 128, v, sizeof(v));
                continue;
            }
            const bool is_k = h < a.hq + a.hkv;
            const int kh = is_k ? h - a.hq : h - a.hq - a.hkv;
            if (is_k) norm_rope(v, a.k_norm, cs, sn, a.eps);
            store_head((is_k ? a.k_cache : a.v_cache) + (((int64_t)b * a.hkv + kh) * a.capacity + a.pos) * 128, v);
        }
    }
}

void launch_lm_prefill_kv(const LmQkvPostArgs& a, int B, int n, const int32_t* mask, hipStream_t) {
    ACEMI_CHECK(n >= 1 && n <= a.capacity, "lm_prefill_kv: rows outside the cache");
    for (int b = 0; b < B; ++b)
        for (int t = 0; t < n; ++t) {
            const int64_t m = (int64_t)b * n + t;
            const bool valid = mask ? mask[m] != 0 : true;
            a.key_mask[(int64_t)b * a.capacity + t] = valid ? 1 : 0;
            float* row = const_cast<float*>(a.qkv) + m * a.ld;
            if (!valid) std::fill(row, row + (int64_t)(a.hq + 2 * a.hkv) * 128, 0.f);
            for (int h = a.hq; h < a.hq + 2 * a.hkv; ++h) {
                float v[128];
                std::memcpy(v, row + (int64_t)h * 128, sizeof(v));
                const bool is_k = h < a.hq + a.hkv;
                const int kh = is_k ? h - a.hq : h - a.hq - a.hkv;
                if (is_k && valid) norm_rope(v, a.k_norm, a.rope_cos + (int64_t)t * 64, a.rope_sin + (int64_t)t * 64, a.eps);
                store_head((is_k ? a.k_cache : a.v_cache) + (((int64_t)b * a.hkv + kh) * a.capacity + t) * 128, v);
            }
        }
}

size_t lm_attn_part_floats(int B, int hq, int nk) { return (size_t)B * hq * ceil_div(nk, LM_SPLIT_KEYS) * 130; }

// the kernel's structure: per range of LM_SPLIT_KEYS keys (m, l, O), merged in ascending order
void launch_lm_attention(ActType out_t, const LmAttnArgs& a, int B, int hq, hipStream_t) {
    ACEMI_CHECK(a.nk >= 1 && a.nk <= a.capacity && hq % a.hkv == 0, "lm_attention: bad arguments");
    const int rep = hq / a.hkv, n_split = (int)ceil_div(a.nk, LM_SPLIT_KEYS);
    for (int b = 0; b < B; ++b)
        for (int head = 0; head < hq; ++head) {
            const float* q = a.q + ((int64_t)b * hq + head) * 128;
            const int64_t base = ((int64_t)b * a.hkv + head / rep) * a.capacity;
            float M = -INFINITY, L = 0.f;
            std::vector<float> O(128, 0.f);
            for (int sp = 0; sp < n_split; ++sp) {
                const int k0 = sp * LM_SPLIT_KEYS, k1 = std::min(a.nk, k0 + LM_SPLIT_KEYS);
                std::vector<float> s(k1 - k0);
                float m = -INFINITY;
                for (int k = k0; k < k1; ++k) {
                    float d = 0.f;
                    for (int i = 0; i < 128; ++i) d = std::fma(q[i], from16(a.k_cache[(base + k) * 128 + i], true), d);
                    s[k - k0] = a.key_mask[(int64_t)b * a.capacity + k] ? d * a.scale : -INFINITY;
                    m = std::max(m, s[k - k0]);
                }
                float l = 0.f;
                std::vector<float> o(128, 0.f);
                for (int k = k0; k < k1; ++k) {
                    const float p = s[k - k0] == -INFINITY ? 0.f : std::exp(s[k - k0] - m);
                    l += p;
                    for (int i = 0; i < 128; ++i) o[i] = std::fma(p, from16(a.v_cache[(base + k) * 128 + i], true), o[i]);
                }
                const float Mn = std::max(M, m);
                const float w0 = M == -INFINITY ? 0.f : std::exp(M - Mn), w1 = m == -INFINITY ? 0.f : std::exp(m - Mn);
                L = L * w0 + l * w1;
                for (int i = 0; i < 128; ++i) O[i] = O[i] * w0 + o[i] * w1;
                M = Mn;
            }
            for (int i = 0; i < 128; ++i)
                a.out[((int64_t)b * hq + head) * 128 + i] = to16(L > 0.f ? O[i] / L : 0.f, out_t == ActType::F16);
        }
}

}  // namespace acemi
