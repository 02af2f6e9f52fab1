// Plain C++ restatement of kernels/lm_decode.hip's launch_lm_attention_shared (kernels.h) for a build of the runtime
// without a device compiler, as lm_fanout_host.h is for the fan-out: included by runtime/lm.cpp alone, empty under
// hipcc.  The same launcher conditions and the same split of the key ranges: the n_shared / LM_SPLIT_KEYS ranges wholly
// inside the shared prefix are read from the group's first sequence, every other range from the sequence itself.  The
// sums are those of the host build's launch_lm_attention (per range m, l and O in key order, the ranges joined in
// ascending order), so on a cache that keeps the precondition the output equals that launcher's bit for bit, as the
// kernel's equals lm_attn_kernel's.
#pragma once

#ifndef __HIP__
#include <algorithm>
#include <cmath>
#include <cstring>

#include "../kernels.h"

namespace acemi {

void launch_lm_attention_shared(ActType out_t, const LmAttnArgs& a, int B, int hq, hipStream_t s) {
    ACEMI_CHECK(B >= 1 && B <= LM_MAX_BATCH && a.hkv >= 1 && hq % a.hkv == 0 && a.nk >= 1 && a.nk <= a.capacity &&
                    a.q && a.k_cache && a.v_cache && a.key_mask && a.out,
                "lm_attention: bad arguments");
    const int rep = hq / a.hkv;
    ACEMI_CHECK(rep == 1 || rep == 2 || rep == 4, "lm_attention: GQA ratio must be 1, 2 or 4");
    lm_attn_shared_check(a, B, rep);
    const int S = a.group_size, n_sh = a.n_shared / LM_SPLIT_KEYS;
    if (n_sh == 0 || S == 1 || a.nk <= LM_SPLIT_KEYS) return launch_lm_attention(out_t, a, B, hq, s);
    const int n_split = (int)ceil_div(a.nk, LM_SPLIT_KEYS);
    auto f16 = [](uint16_t h) {
        _Float16 v;
        std::memcpy(&v, &h, 2);
        return (float)v;
    };
    for (int b = 0; b < B; ++b)
        for (int head = 0; head < hq; ++head) {
            const float* q = a.q + ((int64_t)b * hq + head) * 128;
            float M = -INFINITY, L = 0.f, O[128] = {};
            for (int sp = 0; sp < n_split; ++sp) {
                const int src = sp < n_sh ? b / S * S : b;  // the sequence whose rows this range reads
                const int64_t base = ((int64_t)src * a.hkv + head / rep) * a.capacity;
                const int k0 = sp * LM_SPLIT_KEYS, k1 = std::min(a.nk, k0 + LM_SPLIT_KEYS);
                float sc[LM_SPLIT_KEYS], m = -INFINITY;
                for (int k = k0; k < k1; ++k) {
                    float d = 0.f;
                    for (int i = 0; i < 128; ++i) d = std::fma(q[i], f16(a.k_cache[(base + k) * 128 + i]), d);
                    sc[k - k0] = a.key_mask[(int64_t)src * a.capacity + k] ? d * a.scale : -INFINITY;
                    m = std::max(m, sc[k - k0]);
                }
                float l = 0.f, o[128] = {};
                for (int k = k0; k < k1; ++k) {
                    const float p = sc[k - k0] == -INFINITY ? 0.f : std::exp(sc[k - k0] - m);
                    l += p;
                    for (int i = 0; i < 128; ++i) o[i] = std::fma(p, f16(a.v_cache[(base + k) * 128 + i]), o[i]);
                }
                const float Mn = std::max(M, m);
                const float w0 = M == -INFINITY ? 0.f : std::exp(M - Mn), w1 = m == -INFINITY ? 0.f : std::exp(m - Mn);
                L = L * w0 + l * w1;
                for (int i = 0; i < 128; ++i) O[i] = O[i] * w0 + o[i] * w1;
                M = Mn;
            }
            for (int i = 0; i < 128; ++i) {
                const float v = L > 0.f ? O[i] / L : 0.f;
                uint16_t w;
                if (out_t == ActType::F16) {
                    const _Float16 hv = (_Float16)v;
                    std::memcpy(&w, &hv, 2);
                } else {
                    uint32_t u;
                    std::memcpy(&u, &v, 4);
                    if ((u & 0x7fffffffu) > 0x7f800000u) {
                        w = (uint16_t)((u >> 16) | 64u);
                    } else {
                        u += 0x7fffu + ((u >> 16) & 1u);
                        w = (uint16_t)(u >> 16);
                    }
                }
                a.out[((int64_t)b * hq + head) * 128 + i] = w;
            }
        }
}

}  // namespace acemi
#endif  // !__HIP__
