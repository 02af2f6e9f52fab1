// Plain C++ restatement of kernels/lm_sample.hip's launcher (launch_lm_select, lm_select_chains of kernels.h) for a
// build of the runtime without a device compiler, as lm_decode_q_host.h is for the plane kernels: included by
// runtime/lm.cpp alone, empty under hipcc.  Steps 1-4 (mix, candidates, phase temperature, penalty) round as the
// kernel does, one f32 operation at a time (the host build compiles with -ffp-contract=off); the top-k threshold is
// the k-th largest value; the top-p masses, the softmax of the draw and its cumulative sum are added in double, in
// plain candidate order, so the chains lm_select_chains reports are 1.
#pragma once

#ifndef __HIP__
#include <algorithm>
#include <cmath>
#include <functional>
#include <limits>
#include <vector>

#include "../kernels.h"

namespace acemi {

void lm_select_chains(int, int* chains) { chains[0] = chains[1] = chains[2] = 1; }

void launch_lm_select(const LmSelectArgs& a, hipStream_t) {
    ACEMI_CHECK(a.logits && a.tokens && a.work && a.vocab >= 1 && a.ld_logits >= a.vocab, "lm_select: bad arguments");
    ACEMI_CHECK(a.S >= 1 && a.S * (a.cfg_scale > 1.0f ? 2 : 1) <= LM_MAX_BATCH, "lm_select: bad batch");
    ACEMI_CHECK(!a.allowed || a.n_allowed >= 1, "lm_select: empty allowed list");
    ACEMI_CHECK(a.stop_id < a.vocab && (!a.force_stop || a.stop_id >= 0), "lm_select: bad stop id");
    ACEMI_CHECK(!(a.temperature > 0.0f) || a.uniform, "lm_select: sampling needs the uniforms");
    ACEMI_CHECK(!a.seen || a.ld_seen >= a.vocab, "lm_select: bad seen map");
    ACEMI_CHECK(!a.processed || a.ld_processed >= a.vocab, "lm_select: bad processed rows");
    const float ninf = -std::numeric_limits<float>::infinity();
    for (int s = 0; s < a.S; ++s) {
        const bool stopped = a.done && a.stop_id >= 0 && a.done[1 + s] != 0;
        const bool only_stop = a.force_stop || stopped;
        const int n = only_stop ? 1 : (a.allowed ? a.n_allowed : a.vocab);
        auto id_of = [&](int c) { return only_stop ? a.stop_id : (a.allowed ? a.allowed[c] : c); };
        std::vector<float> z((size_t)n);
        for (int c = 0; c < n; ++c) {
            const int id = id_of(c);
            float v = ninf;
            if (id >= 0 && id < a.vocab && !(a.block_stop && !a.force_stop && id == a.stop_id)) {
                v = a.logits[(int64_t)s * a.ld_logits + id];
                if (a.cfg_scale > 1.0f) {
                    const float u = a.logits[(int64_t)(s + a.S) * a.ld_logits + id];
                    const float d = v - u;
                    const float sd = a.cfg_scale * d;
                    v = u + sd;
                }
                if (v != v) v = ninf;
                if (a.pre_temperature > 0.0f) v = v / a.pre_temperature;
                if (a.seen && a.repetition_penalty != 1.0f && a.seen[(int64_t)s * a.ld_seen + id])
                    v = v < 0.0f ? v * a.repetition_penalty : v / a.repetition_penalty;
            }
            z[c] = v;
        }
        const float zmax = *std::max_element(z.begin(), z.end());
        const bool empty = !(zmax > ninf);
        std::vector<char> keep((size_t)n);
        for (int c = 0; c < n; ++c) keep[c] = !empty && z[c] > ninf;
        if (!empty && a.top_k > 0 && a.top_k < n) {
            std::vector<float> t(z);
            std::nth_element(t.begin(), t.begin() + (a.top_k - 1), t.end(), std::greater<float>());
            const float kth = t[a.top_k - 1];
            for (int c = 0; c < n; ++c) keep[c] = keep[c] && z[c] >= kth;
        }
        if (!empty && a.top_p > 0.0f && a.top_p < 1.0f) {
            std::vector<float> v;
            for (int c = 0; c < n; ++c)
                if (keep[c]) v.push_back(z[c]);
            std::sort(v.begin(), v.end(), std::greater<float>());
            double Z = 0.0;
            for (float x : v) Z += std::exp((double)x - (double)zmax);
            const double lim = (double)a.top_p * Z;
            double above = 0.0;  // mass of the values strictly larger than the group at i
            float cut = v[0];
            for (size_t i = 0; i < v.size();) {
                if (above > lim) break;
                cut = v[i];
                size_t j = i;
                double g = 0.0;
                for (; j < v.size() && v[j] == v[i]; ++j) g += std::exp((double)v[j] - (double)zmax);
                above += g;
                i = j;
            }
            for (int c = 0; c < n; ++c) keep[c] = keep[c] && z[c] >= cut;
        }
        if (a.processed) {
            float* out = a.processed + (int64_t)s * a.ld_processed;
            for (int v = 0; v < a.vocab; ++v) out[v] = ninf;
            for (int c = 0; c < n; ++c)
                if (keep[c]) out[id_of(c)] = z[c];
        }
        int pick = 0;
        if (empty) {
            pick = 0;
        } else if (!(a.temperature > 0.0f)) {
            for (int c = 0; c < n; ++c)
                if (z[c] == zmax) {
                    pick = c;
                    break;
                }
        } else {
            const double T = (double)a.temperature;
            std::vector<double> p((size_t)n, 0.0);
            double total = 0.0;
            int last = 0;
            for (int c = 0; c < n; ++c)
                if (keep[c]) {
                    p[c] = std::exp(((double)z[c] - (double)zmax) / T);
                    total += p[c];
                    last = c;
                }
            const double target = (double)a.uniform[s] * total;
            double cum = 0.0;
            pick = last;
            for (int c = 0; c < n; ++c)
                if (keep[c]) {
                    cum += p[c];
                    if (cum > target) {
                        pick = c;
                        break;
                    }
                }
        }
        int tok = id_of(pick);
        tok = tok < 0 ? 0 : (tok >= a.vocab ? a.vocab - 1 : tok);
        a.tokens[(int64_t)s * a.token_stride] = tok;
        if (a.next_ids) {
            a.next_ids[s] = tok;
            if (a.cfg_scale > 1.0f) a.next_ids[s + a.S] = tok;
        }
        if (a.seen) a.seen[(int64_t)s * a.ld_seen + tok] = 1;
        if (a.done && a.stop_id >= 0 && tok == a.stop_id) {
            a.done[1 + s] = 1;
            if (a.done[0] == 0) a.done[0] = a.n_emitted + 1;
        }
    }
}

}  // namespace acemi
#endif  // !__HIP__
