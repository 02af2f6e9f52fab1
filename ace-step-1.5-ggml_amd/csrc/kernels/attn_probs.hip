// Cross-attention probabilities of a few chosen heads (launch_attn_probs of kernels.h): the flash kernels of
// attention.hip never hold a score matrix, so the maps the lyric-alignment features read are written here, from the
// same Q / K images those kernels read.
//
//   P[q][k] = exp(s - max_k s) / sum_k exp(s - max_k s),   s = scale * (q . k) + kbias[k]
//
// Operands: the fp16 hi planes only (present in the same layout in every attention precision mode; the lo planes hold
// fp8 bytes in the f8c mode), v_mfma_f32_16x16x32_f16 with f32 accumulate, S = Q . K^T with Q as the A operand: the
// accumulator of lane l then holds key l & 15 of a 16-key block and queries 4 (l >> 4) + i, so every store instruction
// writes runs of 16 consecutive keys (64 bytes) and the four blocks of a 64-key tile complete 256-byte row segments.
//
// A workgroup is four waves = 128 queries of one (listed head, item); a wave owns 32 queries (two 16-row blocks, Q
// fragments in registers for the whole kernel) and walks the key tiles twice, reading the K fragments straight from
// global memory (the 128 queries of a workgroup share them through the vector cache; nk is the encoder length, a few
// hundred keys):
//   sweep 1: every lane keeps the running maximum and the running sum of the keys it sees (k = l & 15 mod 16) for its
//            8 rows; the 16 lanes of a row are merged afterwards by xor butterflies (every lane gets the same bits);
//   sweep 2: the scores again, exp(s - max) / sum, stored.
// No LDS, no barrier, no atomics, a fixed reduction order: two runs give the same bits.  A masked key (kbias = -inf or
// k >= nk) is exactly +0; a row without an unmasked key is written as zeros.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../kernels.h"
#include "mfma_guard.h"
#include "prep_math.h"

namespace acemi {
namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

constexpr int D = 128;
constexpr int KT = 64;        // keys per tile
constexpr int QW = 32;        // queries per wave
constexpr int QB = 4 * QW;    // queries per workgroup

struct ProbParams {
    const uint16_t* q;
    const uint16_t* k;
    const float* kbias;
    float* out;
    int B, Hq, Hkv, nq, nq_pad, nk, nk_pad;
    float scale;
    int heads[ATTN_PROBS_MAX_HEADS];
    int slots[ATTN_PROBS_MAX_HEADS];  // listed head i writes out[slots[i]]
};

__global__ __launch_bounds__(256) void attn_probs_kernel(const ProbParams p) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int hi = blockIdx.y, b = blockIdx.z;
    const int q0 = blockIdx.x * QB + wid * QW;
    if (q0 >= p.nq) return;  // (no barrier in this kernel)
    const int h = p.heads[hi], hk = h / (p.Hq / p.Hkv);
    const int lr = lane & 15, lc = lane >> 4;
    const float ninf = -INFINITY;

    // rows q0 .. q0 + 31 exist in the image: q0 < nq <= nq_pad, q0 % 32 == 0, nq_pad % 128 == 0
    const uint16_t* Q = p.q + (((int64_t)b * p.Hq + h) * p.nq_pad + q0) * D;
    const uint16_t* K = p.k + ((int64_t)b * p.Hkv + hk) * p.nk_pad * D;
    const float* kb = p.kbias ? p.kbias + (int64_t)b * p.nk_pad : nullptr;
    uint4 qa[2][4];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) qa[mb][kk] = *(const uint4*)(Q + (mb * 16 + lr) * D + kk * 32 + lc * 8);

    // s[mb][nb][i]: query q0 + 16 mb + 4 lc + i, key 64 kt + 16 nb + lr (keys below nk_pad, a multiple of 64, exist)
    auto scores = [&](int kt, float (&s)[2][4][4]) {
        uint4 kf[4][4];
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
                kf[nb][kk] = *(const uint4*)(K + (int64_t)(kt * KT + nb * 16 + lr) * D + kk * 32 + lc * 8);
        float bias[4];
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const int key = kt * KT + nb * 16 + lr;
            bias[nb] = key < p.nk ? (kb ? kb[key] : 0.f) : ninf;
        }
        f32x4 acc[2][4];
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) acc[mb][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                for (int mb = 0; mb < 2; ++mb)
                    acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, qa[mb][kk]),
                                                                         __builtin_bit_cast(f16x8, kf[nb][kk]),
                                                                         acc[mb][nb], 0, 0, 0);
        mfma_war_retire(qa, kf);
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                for (int i = 0; i < 4; ++i)  // (a select: whatever a masked key's row holds never reaches a sum)
                    s[mb][nb][i] = bias[nb] == ninf ? ninf : rn_add(rn_mul(acc[mb][nb][i], p.scale), bias[nb]);
    };

    const int nt = (p.nk + KT - 1) / KT;
    float m[2][4], l[2][4];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            m[mb][i] = ninf;
            l[mb][i] = 0.f;
        }
    float s[2][4][4];
    for (int kt = 0; kt < nt; ++kt) {
        scores(kt, s);
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float mn = fmaxf(fmaxf(m[mb][i], fmaxf(s[mb][0][i], s[mb][1][i])),
                                       fmaxf(s[mb][2][i], s[mb][3][i]));
                if (mn > ninf) {  // expf(-inf) = 0: a lane's first unmasked key starts its sum at 0 * 0 + ...
                    float a = rn_mul(l[mb][i], expf(m[mb][i] - mn));
#pragma unroll
                    for (int nb = 0; nb < 4; ++nb) a = rn_add(a, expf(s[mb][nb][i] - mn));
                    l[mb][i] = a;
                    m[mb][i] = mn;
                }
            }
    }
    // the 16 lanes of a row (same lane >> 4): maximum, then the sums rescaled to it
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float mx = m[mb][i];
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
            float t = m[mb][i] > ninf ? rn_mul(l[mb][i], expf(m[mb][i] - mx)) : 0.f;
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) t = rn_add(t, __shfl_xor(t, o));
            m[mb][i] = mx;
            l[mb][i] = t;
        }

    float* out = p.out + ((int64_t)p.slots[hi] * p.B + b) * p.nq * p.nk;
    for (int kt = 0; kt < nt; ++kt) {
        scores(kt, s);
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = q0 + mb * 16 + lc * 4 + i;
                if (row >= p.nq) continue;
                float* orow = out + (int64_t)row * p.nk;
#pragma unroll
                for (int nb = 0; nb < 4; ++nb) {
                    const int key = kt * KT + nb * 16 + lr;
                    if (key >= p.nk) continue;
                    const float sv = s[mb][nb][i];
                    orow[key] = sv == ninf ? 0.f : rn_div(expf(sv - m[mb][i]), l[mb][i]);
                }
            }
    }
}

}  // namespace

void launch_attn_probs(const AttnProbArgs& a, hipStream_t s) {
    ACEMI_CHECK(a.q && a.k && a.out && a.heads, "attn_probs: null operand");
    ACEMI_CHECK(a.B >= 1 && a.Hq >= 1 && a.Hkv >= 1 && a.Hq % a.Hkv == 0, "attn_probs: bad head counts");
    ACEMI_CHECK(a.nq >= 1 && a.nq_pad >= a.nq && a.nq_pad % QB == 0, "attn_probs: nq_pad must be a multiple of 128");
    ACEMI_CHECK(a.nk >= 1 && a.nk_pad >= a.nk && a.nk_pad % KT == 0, "attn_probs: nk_pad must be a multiple of 64");
    ACEMI_CHECK(a.n_heads >= 1 && a.B <= 65535, "attn_probs: bad launch size");
    for (int i = 0; i < a.n_heads; ++i)
        ACEMI_CHECK(a.heads[i] >= 0 && a.heads[i] < a.Hq && (!a.slots || a.slots[i] >= 0),
                    "attn_probs: head index out of range");
    ProbParams p{};
    p.q = a.q;
    p.k = a.k;
    p.kbias = a.kbias;
    p.B = a.B;
    p.Hq = a.Hq;
    p.Hkv = a.Hkv;
    p.nq = a.nq;
    p.nq_pad = a.nq_pad;
    p.nk = a.nk;
    p.nk_pad = a.nk_pad;
    p.scale = a.scale;
    p.out = a.out;
    for (int h0 = 0; h0 < a.n_heads; h0 += ATTN_PROBS_MAX_HEADS) {  // the list travels by value
        const int n = a.n_heads - h0 < ATTN_PROBS_MAX_HEADS ? a.n_heads - h0 : ATTN_PROBS_MAX_HEADS;
        for (int i = 0; i < n; ++i) {
            p.heads[i] = a.heads[h0 + i];
            p.slots[i] = a.slots ? a.slots[h0 + i] : h0 + i;
        }
        hipLaunchKernelGGL(attn_probs_kernel, dim3((a.nq + QB - 1) / QB, n, a.B), dim3(256), 0, s, p);
        ACEMI_HIP(hipGetLastError());
    }
}

}  // namespace acemi
