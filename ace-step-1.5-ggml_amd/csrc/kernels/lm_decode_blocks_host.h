// Plain C++ restatement of kernels/lm_decode_blocks.hip's launchers (launch_lm_skinny_blocks, launch_lm_embed_blocks,
// lm_skinny_blocks_chain of kernels.h) for a build of the runtime without a device compiler, as lm_decode_q_host.h is
// for the plane kernels: included by runtime/lm.cpp alone, so the definitions exist once; under hipcc (the product, where
// lm_decode_blocks.hip defines the three) this header is empty.
// Same weight values and rounding points as the kernels: quant::dequantize_rows' f32 values, RNE to bf16 for the product
// (a zero's sign aside: ggml's -0 under a negative Q8_0 / Q6_K scale, which no sum that starts at +0 can show),
// unrounded for the gather; the sum runs in plain ascending k, so its addition chain is K long.
#pragma once

#ifndef __HIP__
#include <algorithm>
#include <cmath>
#include <vector>

#include "../kernels.h"
#include "../runtime/quant.h"
#include "lm_decode_q_host.h"

namespace acemi {

namespace lmb_host {

inline bool seg_ok(const BlockSeg& g, int K) {
    const quant::QType q = quant::from_ggml(g.type);
    return q != quant::QNONE && K >= quant::block_values(q) && quant::applies(q, K) && g.src && g.rows > 0 && g.row0 >= 0 &&
           g.step >= 1 && g.group >= 1;
}
// source row r of a segment as f32 values
inline void seg_row(const BlockSeg& g, int r, int K, float* out) {
    const quant::QType q = quant::from_ggml(g.type);
    quant::dequantize_rows(q, static_cast<const uint8_t*>(g.src) + (size_t)r * quant::row_bytes(q, K), 1, K, out);
}

}  // namespace lmb_host

int lm_skinny_blocks_chain(int, int K) { return K; }

void launch_lm_skinny_blocks(const uint16_t* x, int ldx, int B, const WeightView& W, int N, int K, int epi, float* y_f32,
                             uint16_t* y_act, int ldy, hipStream_t) {
    using namespace lmb_host;
    using lmq_host::bf16_bits;
    using lmq_host::bf16_round;
    using lmq_host::bf16_value;
    ACEMI_CHECK(W.fmt == WF_GGML_RAW && W.segs && W.n_segs >= 1, "lm_skinny_blocks: the weight is not in raw ggml blocks");
    ACEMI_CHECK(B >= 1 && B <= LM_MAX_BATCH && N >= 1 && K >= 32 && ldx % 8 == 0 && ldx >= K && x, "lm_skinny_blocks: bad shape");
    ACEMI_CHECK(epi == LM_EPI_SWIGLU ? (N % 32 == 0 && y_act) : ((epi == LM_EPI_STORE || epi == LM_EPI_RESID) && y_f32),
                "lm_skinny_blocks: bad epilogue");
    for (int i = 0; i < W.n_segs; ++i)
        ACEMI_CHECK(seg_ok(W.segs[i], K) && block_seg_row(W.segs[i], W.segs[i].rows - 1) < N, "lm_skinny_blocks: bad segment");
    if (epi == LM_EPI_SWIGLU) {
        const BlockSeg &a = W.segs[0], &b = W.segs[W.n_segs - 1];
        ACEMI_CHECK(W.n_segs == 2 && std::min(a.row0, b.row0) == 0 && std::max(a.row0, b.row0) == 16 && a.rows == N / 2 &&
                        b.rows == N / 2 && a.step == 2 && b.step == 2 && a.group == 16 && b.group == 16,
                    "lm_skinny_blocks: SwiGLU takes one gate and one up segment (group 16, step 2)");
    }
    // acc[b] of every fused row the segments hold, then the epilogue
    std::vector<float> dots((size_t)B * N, 0.f), row((size_t)K);
    for (int i = 0; i < W.n_segs; ++i) {
        const BlockSeg& g = W.segs[i];
        for (int r = 0; r < g.rows; ++r) {
            seg_row(g, r, K, row.data());
            for (int k = 0; k < K; ++k) row[(size_t)k] = bf16_round(row[(size_t)k]);
            const int fr = block_seg_row(g, r);
            for (int b = 0; b < B; ++b) {
                float acc = 0.f;
                for (int k = 0; k < K; ++k) acc = std::fma(row[(size_t)k], bf16_value(x[(int64_t)b * ldx + k]), acc);
                dots[(size_t)b * N + fr] = acc;
            }
        }
    }
    for (int b = 0; b < B; ++b) {
        if (epi == LM_EPI_SWIGLU) {
            for (int j = 0; j < N / 2; ++j) {
                const int64_t rg = (int64_t)(j >> 4) * 32 + (j & 15);
                const float g = dots[(size_t)b * N + rg], u = dots[(size_t)b * N + rg + 16];
                y_act[(int64_t)b * ldy + j] = bf16_bits(g / (1.0f + std::exp(-g)) * u);
            }
        } else {
            for (int i = 0; i < W.n_segs; ++i)
                for (int r = 0; r < W.segs[i].rows; ++r) {
                    const int n = block_seg_row(W.segs[i], r);
                    if (epi == LM_EPI_RESID)
                        y_f32[(int64_t)b * ldy + n] += dots[(size_t)b * N + n];
                    else
                        y_f32[(int64_t)b * ldy + n] = dots[(size_t)b * N + n];
                }
        }
    }
}

void launch_lm_embed_blocks(const WeightView& W, const int32_t* ids, int n, int vocab, int H, float* out, hipStream_t) {
    using namespace lmb_host;
    ACEMI_CHECK(W.fmt == WF_GGML_RAW && W.segs && W.n_segs == 1, "lm_embed_blocks: the table is not one raw-block segment");
    const BlockSeg& g = W.segs[0];
    ACEMI_CHECK(n >= 1 && vocab >= 1 && ids && out && seg_ok(g, H) && g.rows == vocab && g.row0 == 0 && g.step == 1,
                "lm_embed_blocks: bad arguments");
    for (int t = 0; t < n; ++t) seg_row(g, std::min(std::max(ids[t], 0), vocab - 1), H, out + (int64_t)t * H);
}

}  // namespace acemi
#endif  // !__HIP__
