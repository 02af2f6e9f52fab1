// Plain C++ restatement of kernels/lm_score.hip's launcher (launch_lm_score, lm_score_chain of kernels.h) for a build
// of the runtime without a device compiler, as lm_fanout_host.h is for the cache fan-out: included by runtime/lm.cpp
// alone, empty under hipcc.  The same operand values, the same clamp of the targets, the same cut of the vocabulary
// into splits x two 64-column halves of 128-column tiles, the same per-tile online (max, sum, count) update and the
// same merge order; a logit is the f32 sum of 32-value fma blocks in ascending k (lm_score_chain long, as on the
// device), computed by one function for l_t and for the sweep, so equal head rows give equal logits here as well.
#pragma once

#ifndef __HIP__
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "../kernels.h"

namespace acemi {

namespace lm_score_host {

inline float act_value(bool f16, uint16_t h) {
    uint32_t u;
    if (!f16) {
        u = (uint32_t)h << 16;
    } else {
        const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, f = h & 1023u;
        if (e == 31u) {
            u = sign | 0x7f800000u | (f << 13);
        } else if (e != 0u) {
            u = sign | ((e + 112u) << 23) | (f << 13);
        } else {
            const float sub = (float)f * 5.9604644775390625e-8f;  // f * 2^-24, exact
            std::memcpy(&u, &sub, 4);
            u |= sign;
        }
    }
    float r;
    std::memcpy(&r, &u, 4);
    return r;
}

}  // namespace lm_score_host

int lm_score_chain(int H) { return 31 + (H + 31) / 32; }

void launch_lm_score(ActType act, const LmScoreArgs& a, hipStream_t) {
    using namespace lm_score_host;
    lm_score_check(a);
    const bool f16 = act == ActType::F16;
    const int S = lm_score_splits(a.M, a.V, a.splits), P = 2 * S;
    const int tiles = (a.V + LM_SCORE_BN - 1) / LM_SCORE_BN;
    const float NEG_INF = -std::numeric_limits<float>::infinity();
    std::vector<float> xr(a.H), pm(P), ps(P);
    std::vector<int> pc(P);
    for (int m = 0; m < a.M; ++m) {
        const int t = std::min(std::max(a.target[(int64_t)(m / a.t_group) * a.t_stride + m % a.t_group], 0), a.V - 1);
        for (int k = 0; k < a.H; ++k) xr[k] = act_value(f16, a.x[(int64_t)m * a.ldx + k]);
        auto logit = [&](int j) {
            float acc = 0.f;  // 32 values per block as one MFMA takes them, then the blocks in ascending k
            for (int k0 = 0; k0 < a.H; k0 += 32) {
                float blk = 0.f;
                for (int k = k0; k < k0 + 32; ++k) blk = std::fma(xr[k], act_value(f16, a.w[(int64_t)j * a.ldw + k]), blk);
                acc += blk;
            }
            return acc;
        };
        const float lt = logit(t);
        for (int q = 0; q < P; ++q) {
            const int split = q / 2, half = q % 2;
            const int t_begin = (int)((int64_t)split * tiles / S), t_end = (int)((int64_t)(split + 1) * tiles / S);
            float mx = NEG_INF, sm = 0.f;
            int cnt = 0;
            for (int tile = t_begin; tile < t_end; ++tile) {
                const int n0 = tile * LM_SCORE_BN + half * 64, n1 = std::min(n0 + 64, a.V);
                if (n0 >= n1) continue;
                std::vector<float> v(n1 - n0);
                float tmax = NEG_INF;
                for (int n = n0; n < n1; ++n) {
                    v[n - n0] = logit(n);
                    tmax = std::max(tmax, v[n - n0]);
                    cnt += (n != t && (v[n - n0] > lt || (v[n - n0] == lt && n < t))) ? 1 : 0;
                }
                const float mnew = std::max(mx, tmax);
                float e = 0.f;
                for (float x : v) e += std::exp(x - mnew);
                sm = sm * std::exp(mx - mnew) + e;
                mx = mnew;
            }
            pm[q] = mx, ps[q] = sm, pc[q] = cnt;
        }
        // the merge: the maximum, lane l's triples l, l + 64, ... in order, then the butterfly over the 64 lanes
        float mx = NEG_INF;
        for (int q = 0; q < P; ++q) mx = std::max(mx, pm[q]);
        float ls[64] = {};
        int c = 0;
        for (int q = 0; q < P; ++q) {
            if (ps[q] > 0.f) ls[q % 64] += ps[q] * std::exp(pm[q] - mx);
            c += pc[q];
        }
        for (int off = 32; off > 0; off >>= 1)
            for (int l = 0; l < off; ++l) ls[l] += ls[l + off];
        a.logprob[m] = lt - (mx + std::log(ls[0]));
        a.rank[m] = c;
    }
}

}  // namespace acemi
#endif  // !__HIP__
