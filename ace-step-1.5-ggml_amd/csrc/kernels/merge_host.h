// Plain C++ restatement of the adapter merge launchers (launch_lora_merge / launch_lokr_merge of kernels.h) for a build
// of the runtime without a device compiler, as attn_probs_host.h is for the probability capture: included by
// runtime/engine.cpp alone (the two launchers are ordinary definitions: one translation unit), empty under hipcc.
// "Device" memory is host memory.  The arithmetic is the kernels' exactly
// (the CPU tests compare bits): the host build compiles with -ffp-contract=off, so each multiply and add below rounds
// on its own, and the 16-bit conversions are merge_common.h's.
#pragma once

#ifndef __HIP__
#include <cstring>

#include "merge_common.h"

namespace acemi {
namespace merge_host {

// every fused row of the target: copy-through rows are moved here, module row o goes to delta(o, i) for the f32 term
// of column i, which is added to the base word and rounded to the image's format
template <typename F>
void rows(const MergeTarget& t, int rows_mod, F delta) {
    const bool f16 = t.fmt == WF_F16;
    for (int fr = t.row0; fr < t.row0 + t.rows; ++fr) {
        const int o = merge_module_row(t, rows_mod, fr);
        const uint16_t* src = t.base + (int64_t)fr * t.ld_base;
        uint16_t* dst = t.out + (int64_t)fr * t.ld_out;
        if (o < 0) {
            if (t.copy_rest && src != dst) std::memmove(dst, src, (size_t)t.cols * 2);
            continue;
        }
        for (int i = 0; i < t.cols; ++i) dst[i] = f32_to_16(f16, f16_to_f32(f16, src[i]) + delta(o, i));
    }
}

// out [m][n] = L [m][r] . R [r][n] as the rank-ordered chain
inline void product(const float* L, const float* R, float* out, int m, int n, int r) {
    for (int o = 0; o < m; ++o)
        for (int i = 0; i < n; ++i) {
            volatile float acc = 0.f;  // (volatile: one rounded f32 per step, whatever the optimiser prefers)
            for (int k = 0; k < r; ++k) {
                const float p = L[(int64_t)o * r + k] * R[(int64_t)k * n + i];
                acc = acc + p;
            }
            out[(int64_t)o * n + i] = acc;
        }
}

}  // namespace merge_host

void launch_lora_merge(const LoraMergeJob* jobs, int n, hipStream_t) {
    for (int ji = 0; ji < n; ++ji) {
        const LoraMergeJob& j = jobs[ji];
        check_merge_target(j.t, "lora_merge");
        ACEMI_CHECK(j.r >= 0 && j.r <= LORA_MAX_RANK && (j.r == 0 || (j.A && j.B)), "lora_merge: bad job");
        merge_host::rows(j.t, j.r > 0 ? j.rows_mod : 0, [&](int o, int i) {
            volatile float acc = 0.f;
            for (int k = 0; k < j.r; ++k) {
                const float p = j.B[(int64_t)o * j.r + k] * j.A[(int64_t)k * j.t.cols + i];
                acc = acc + p;
            }
            return j.eff * acc;
        });
    }
}

// the product factors into the job's workspace, then one rounded multiply w1 * W2 and one by eff per weight
void launch_lokr_merge(const LokrMergeJob* jobs, int n, hipStream_t) {
    for (int ji = 0; ji < n; ++ji) {
        const LokrMergeJob& j = jobs[ji];
        check_merge_target(j.t, "lokr_merge");
        ACEMI_CHECK(j.a >= 0, "lokr_merge: bad job");
        const float *w1 = j.w1, *W2 = j.w2;
        if (j.a > 0) {
            ACEMI_CHECK(j.b > 0 && j.c > 0 && j.d > 0 && (int64_t)j.b * j.d == j.t.cols &&
                            (j.w1 || (j.w1a && j.w1b && j.r1 > 0)) && (j.w2 || (j.w2a && j.w2b && j.r2 > 0)) &&
                            (lokr_ws_floats(j) == 0 || j.ws),
                        "lokr_merge: bad factors");
            if (!W2) merge_host::product(j.w2a, j.w2b, j.ws, j.c, j.d, j.r2), W2 = j.ws;
            if (!w1) merge_host::product(j.w1a, j.w1b, j.ws + lokr_ws_w1_offset(j), j.a, j.b, j.r1), w1 = j.ws + lokr_ws_w1_offset(j);
        }
        merge_host::rows(j.t, j.a * j.c, [&](int o, int i) {
            volatile float v = w1[(int64_t)(o / j.c) * j.b + i / j.d] * W2[(int64_t)(o % j.c) * j.d + i % j.d];
            volatile float t = j.eff * v;
            return (float)t;
        });
    }
}

}  // namespace acemi
#endif
