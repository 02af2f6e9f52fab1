// Plain C++ restatement of kernels/attn_probs.hip's launcher (launch_attn_probs of kernels.h) for a build of the
// runtime without a device compiler, as lm_sample_host.h is for token selection: included by runtime/engine.cpp alone,
// empty under hipcc.  The same operands (the fp16 hi planes, products exact in f32), the same checks and the same
// definition; the dot product and the row sum are f32 chains in index order (the host build compiles with
// -ffp-contract=off), the exponential is libm's expf.
#pragma once

#ifndef __HIP__
#include <cmath>
#include <cstring>
#include <vector>

#include "../kernels.h"

namespace acemi {

void launch_attn_probs(const AttnProbArgs& a, hipStream_t) {
    ACEMI_CHECK(a.q && a.k && a.out && a.heads, "attn_probs: null operand");
    ACEMI_CHECK(a.B >= 1 && a.Hq >= 1 && a.Hkv >= 1 && a.Hq % a.Hkv == 0, "attn_probs: bad head counts");
    ACEMI_CHECK(a.nq >= 1 && a.nq_pad >= a.nq && a.nq_pad % 128 == 0, "attn_probs: nq_pad must be a multiple of 128");
    ACEMI_CHECK(a.nk >= 1 && a.nk_pad >= a.nk && a.nk_pad % 64 == 0, "attn_probs: nk_pad must be a multiple of 64");
    ACEMI_CHECK(a.n_heads >= 1 && a.B <= 65535, "attn_probs: bad launch size");
    for (int i = 0; i < a.n_heads; ++i)
        ACEMI_CHECK(a.heads[i] >= 0 && a.heads[i] < a.Hq && (!a.slots || a.slots[i] >= 0),
                    "attn_probs: head index out of range");
    auto f16 = [](uint16_t bits) {
        _Float16 h;
        std::memcpy(&h, &bits, 2);
        return (float)h;
    };
    const int D = 128, rep = a.Hq / a.Hkv;
    std::vector<float> s((size_t)a.nk);
    for (int i = 0; i < a.n_heads; ++i)
        for (int b = 0; b < a.B; ++b) {
            const int h = a.heads[i], hk = h / rep;
            for (int q = 0; q < a.nq; ++q) {
                const uint16_t* qr = a.q + (((int64_t)b * a.Hq + h) * a.nq_pad + q) * D;
                float mx = -INFINITY;
                for (int k = 0; k < a.nk; ++k) {
                    const float bias = a.kbias ? a.kbias[(int64_t)b * a.nk_pad + k] : 0.f;
                    if (bias == -INFINITY) {
                        s[k] = -INFINITY;
                        continue;
                    }
                    const uint16_t* kr = a.k + (((int64_t)b * a.Hkv + hk) * a.nk_pad + k) * D;
                    float dot = 0.f;
                    for (int d = 0; d < D; ++d) dot += f16(qr[d]) * f16(kr[d]);
                    s[k] = dot * a.scale + bias;
                    mx = s[k] > mx ? s[k] : mx;
                }
                float sum = 0.f;
                for (int k = 0; k < a.nk; ++k)
                    if (s[k] != -INFINITY) sum += std::exp(s[k] - mx);
                float* out = a.out + (((int64_t)(a.slots ? a.slots[i] : i) * a.B + b) * a.nq + q) * a.nk;
                for (int k = 0; k < a.nk; ++k) out[k] = s[k] == -INFINITY ? 0.f : std::exp(s[k] - mx) / sum;
            }
        }
}

}  // namespace acemi
#endif  // !__HIP__
