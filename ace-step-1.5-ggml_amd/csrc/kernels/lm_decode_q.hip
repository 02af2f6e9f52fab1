// Decode step of the causal LM on block-quantized weights (runtime/lm.cpp): the skinny product and the embedding gather
// of lm_decode.hip for a weight held as ggml block planes (runtime/quant.h):
//   Q8_0: q int8 [N][K]        s f32 [N][K/32]     (d)             1.125 B per weight
//   Q4_K: q u8   [N][K/2]      s f32 [N][K/32][2]  (d*sc, dmin*m)  0.75  B per weight
//   Q6_K: q int8 [N][K] (q-32) s f32 [N][K/16]     (d*sc)          1.25  B per weight
//
//   lm_skinny_q_kernel  y[B][N] = x[B][K] . W[N][K]^T, x bf16, f32 accumulate.  The weight value multiplied is the one
//                       gemm_q.hip's dequant forms (deq_i8x4 / deq_u4x4): one f32 fma (q*d, d*sc*q - dmin*m, d*sc*(q-32)),
//                       RNE to bf16 -- so the prefill's GEMM and the step multiply the same weights.
//
// Lane mapping.  A lane reads 16 bytes of a row's q plane per trip (one global_load_dwordx4, consecutive lanes at
// consecutive 16-byte words: coalesced along the row) and the scale(s) of those bytes: 16 values of Q8_0 / Q6_K
// (VPL = 16), one whole 32-value block of Q4_K (VPL = 32).  LPR lanes share one output row (the gate row and its up
// row for SwiGLU) and make trips of LPR * VPL values:
//   K <= 32 * VPL (512 for Q8_0 / Q6_K, 1024 for Q4_K):  LPR = 32, two rows per wave, exactly one trip
//   larger K:                                            LPR = 64, one row per wave, ceil(K / (64 * VPL)) trips
// so Q4_K at K = 1024 fills the wave with two rows instead of leaving half of it idle.  A lane whose first value lies
// at or beyond K in the last trip skips the trip: it loads nothing.  Every plane byte is read once for all B rows; the
// activation rows (bf16, at most 8) come from L2.
// Reduction: lane-local over its k in ascending order (one fma per value), then the xor butterfly over the LPR lanes
// (offsets LPR/2 .. 1).  No atomics, no split along K: bit-identical between runs.  Longest f32 addition chain behind
// one output (lm_skinny_q_chain):  VPL * trips + log2(LPR)  =  VPL + 5 (LPR = 32),  VPL * ceil(K / (64 VPL)) + 6 (LPR = 64).
//
//   lm_embed_q_kernel   rows of the planes as ggml's get_rows returns them: the f32 dequant itself (one rounding, as
//                       quant::dequantize_rows), not rounded to bf16; ids clamped into the table.
//
// Built with -fno-slp-vectorize (Makefile): the packed form of these dequant fmas was not run-to-run stable in the GEMMs.
#include <hip/hip_runtime.h>

#include "../kernels.h"
#include "prep_math.h"

namespace acemi {

namespace {

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

__device__ __forceinline__ uint16_t q_f32_to_bf16_rne(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 64u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
__device__ __forceinline__ float q_silu(float x) { return x / (1.0f + expf(-x)); }

// RNE to bf16 and back to f32 (gemm_q.hip's pk_bf16: the hardware convert), two values per call
__device__ __forceinline__ void round2(float a, float b, float& ra, float& rb) {
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
    bf16x2_t v;
    v[0] = (__bf16)a;
    v[1] = (__bf16)b;
    const uint32_t w = __builtin_bit_cast(uint32_t, v);
    ra = __uint_as_float(w << 16);
    rb = __uint_as_float(w & 0xffff0000u);
}

// the four signed bytes of w (k order b0..b3) times s.  ROUND: (u - 128) * s = fma(u, s, -128 s), as gemm_q.hip's
// deq_i8x4.  The gather forms ggml's own product q * s instead: the same value, and ggml's -0 where q = 0 and s < 0.
template <bool ROUND>
__device__ __forceinline__ void deq_i8x4(uint32_t w, float s, float c, float* o) {
    if constexpr (!ROUND) {
        o[0] = (float)(int)(int8_t)(w & 0xffu) * s;
        o[1] = (float)(int)(int8_t)((w >> 8) & 0xffu) * s;
        o[2] = (float)(int)(int8_t)((w >> 16) & 0xffu) * s;
        o[3] = (float)(int)(int8_t)(w >> 24) * s;
        return;
    }
    const uint32_t u = w ^ 0x80808080u;
    const float f0 = fmaf((float)(u & 0xffu), s, c);
    const float f1 = fmaf((float)((u >> 8) & 0xffu), s, c);
    const float f2 = fmaf((float)((u >> 16) & 0xffu), s, c);
    const float f3 = fmaf((float)(u >> 24), s, c);
    if constexpr (ROUND) {
        round2(f0, f1, o[0], o[1]);
        round2(f2, f3, o[2], o[3]);
    } else {
        o[0] = f0, o[1] = f1, o[2] = f2, o[3] = f3;
    }
}
// four nibbles held as bytes (0..15) times d minus m, as gemm_q.hip's deq_u4x4
template <bool ROUND>
__device__ __forceinline__ void deq_u4x4(uint32_t w, float d, float nm, float* o) {
    const float f0 = fmaf((float)(w & 0xffu), d, nm);
    const float f1 = fmaf((float)((w >> 8) & 0xffu), d, nm);
    const float f2 = fmaf((float)((w >> 16) & 0xffu), d, nm);
    const float f3 = fmaf((float)(w >> 24), d, nm);
    if constexpr (ROUND) {
        round2(f0, f1, o[0], o[1]);
        round2(f2, f3, o[2], o[3]);
    } else {
        o[0] = f0, o[1] = f1, o[2] = f2, o[3] = f3;
    }
}

template <int FMT>
struct QLane {
    static constexpr int VPL = FMT == WF_Q4_K ? 32 : 16;  // values behind a lane's 16 bytes
};

// The VPL values, in ascending k, of 16-byte word `word` of row `row` (k = word * VPL ..).  ROUND: to bf16 and back.
template <int FMT, bool ROUND>
__device__ __forceinline__ void load_values(const uint8_t* __restrict__ q, const float* __restrict__ s, int64_t row, int K,
                                            int word, float* w) {
    if constexpr (FMT == WF_Q4_K) {
        const u32x4 v = *(const u32x4*)(q + row * (K / 2) + (int64_t)word * 16);
        const float2 sm = *(const float2*)(s + (row * (K / 32) + word) * 2);
        const float d = sm.x, nm = -sm.y;
#pragma unroll
        for (int i = 0; i < 4; ++i) {  // dword i: k = 8i .. 8i+3 in the low nibbles, 8i+4 .. 8i+7 in the high nibbles
            deq_u4x4<ROUND>(v[i] & 0x0f0f0f0fu, d, nm, w + 8 * i);
            deq_u4x4<ROUND>((v[i] >> 4) & 0x0f0f0f0fu, d, nm, w + 8 * i + 4);
        }
    } else {
        const u32x4 v = *(const u32x4*)(q + row * K + (int64_t)word * 16);
        const float sc = FMT == WF_Q8_0 ? s[row * (K / 32) + (word >> 1)] : s[row * (K / 16) + word];
        const float c = -128.0f * sc;
#pragma unroll
        for (int i = 0; i < 4; ++i) deq_i8x4<ROUND>(v[i], sc, c, w + 4 * i);
    }
}

__device__ __forceinline__ void unpack8_bf16(const uint4& w, float* f) {
    f[0] = __uint_as_float(w.x << 16), f[1] = __uint_as_float(w.x & 0xffff0000u);
    f[2] = __uint_as_float(w.y << 16), f[3] = __uint_as_float(w.y & 0xffff0000u);
    f[4] = __uint_as_float(w.z << 16), f[5] = __uint_as_float(w.z & 0xffff0000u);
    f[6] = __uint_as_float(w.w << 16), f[7] = __uint_as_float(w.w & 0xffff0000u);
}

// BT: the compiled batch bound (1, 2, 4, 8); rows b >= B (wave-uniform) are skipped and never read.
template <int FMT, int EPI, int LPR, int BT>
__global__ void __launch_bounds__(256) lm_skinny_q_kernel(const uint16_t* __restrict__ x, int ldx, int B,
                                                          const uint8_t* __restrict__ q, const float* __restrict__ s,
                                                          int N, int K, float* __restrict__ y_f32,
                                                          uint16_t* __restrict__ y_act, int ldy) {
    constexpr int ROWS = EPI == LM_EPI_SWIGLU ? 2 : 1;
    constexpr int VPL = QLane<FMT>::VPL;
    constexpr int GROUPS = 64 / LPR;  // output rows per wave
    const int lane = threadIdx.x & (LPR - 1);
    const int unit = (blockIdx.x * 4 + (threadIdx.x >> 6)) * GROUPS + ((threadIdx.x & 63) / LPR);
    const int n_units = N / ROWS;
    if (unit >= n_units) return;  // a whole group of LPR lanes: the butterfly below stays inside the group
    int64_t row[ROWS];
    if constexpr (EPI == LM_EPI_SWIGLU) {  // w_gu rows: [g0..15, u0..15, g16..31, ...]
        row[0] = (int64_t)(unit >> 4) * 32 + (unit & 15);
        row[1] = row[0] + 16;
    } else {
        row[0] = unit;
    }
    float acc[ROWS][BT];
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
        for (int b = 0; b < BT; ++b) acc[r][b] = 0.f;
    const int n_words = K / VPL;
    for (int word = lane; word < n_words; word += LPR) {
        float w[ROWS][VPL];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) load_values<FMT, true>(q, s, row[r], K, word, w[r]);
#pragma unroll
        for (int b = 0; b < BT; ++b) {
            if (b < B) {
                const uint16_t* xp = x + (int64_t)b * ldx + (int64_t)word * VPL;
#pragma unroll
                for (int c = 0; c < VPL / 8; ++c) {
                    float xv[8];
                    unpack8_bf16(*(const uint4*)(xp + 8 * c), xv);
#pragma unroll
                    for (int r = 0; r < ROWS; ++r)
#pragma unroll
                        for (int j = 0; j < 8; ++j) acc[r][b] = fmaf(w[r][8 * c + j], xv[j], acc[r][b]);
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
        for (int b = 0; b < BT; ++b)
#pragma unroll
            for (int o = LPR / 2; o >= 1; o >>= 1) acc[r][b] += __shfl_xor(acc[r][b], o);
    if (lane != 0) return;
#pragma unroll
    for (int b = 0; b < BT; ++b) {
        if (b < B) {
            if constexpr (EPI == LM_EPI_STORE) {
                y_f32[(int64_t)b * ldy + unit] = acc[0][b];
            } else if constexpr (EPI == LM_EPI_RESID) {
                y_f32[(int64_t)b * ldy + unit] += acc[0][b];
            } else {
                y_act[(int64_t)b * ldy + unit] = q_f32_to_bf16_rne(q_silu(acc[0][b]) * acc[1][b]);
            }
        }
    }
}

struct SkinnyQArgs {
    const uint16_t* x;
    int ldx, B;
    const uint8_t* q;
    const float* s;
    int N, K;
    float* y_f32;
    uint16_t* y_act;
    int ldy;
    hipStream_t stream;
};

template <int FMT, int EPI, int LPR, int BT>
void skinny_q_launch(const SkinnyQArgs& a) {
    const int units = EPI == LM_EPI_SWIGLU ? a.N / 2 : a.N;
    const dim3 grid((unsigned)ceil_div(units, 4 * (64 / LPR)));
    hipLaunchKernelGGL((lm_skinny_q_kernel<FMT, EPI, LPR, BT>), grid, dim3(256), 0, a.stream, a.x, a.ldx, a.B, a.q, a.s, a.N,
                       a.K, a.y_f32, a.y_act, a.ldy);
}

template <int FMT, int EPI, int LPR>
void skinny_q_b(const SkinnyQArgs& a) {
    if (a.B == 1)
        skinny_q_launch<FMT, EPI, LPR, 1>(a);
    else if (a.B == 2)
        skinny_q_launch<FMT, EPI, LPR, 2>(a);
    else if (a.B <= 4)
        skinny_q_launch<FMT, EPI, LPR, 4>(a);
    else
        skinny_q_launch<FMT, EPI, LPR, 8>(a);
}

template <int FMT, int EPI>
void skinny_q_lpr(const SkinnyQArgs& a) {
    if (a.K <= 32 * QLane<FMT>::VPL)
        skinny_q_b<FMT, EPI, 32>(a);
    else
        skinny_q_b<FMT, EPI, 64>(a);
}

template <int FMT>
void skinny_q_epi(int epi, const SkinnyQArgs& a) {
    if (epi == LM_EPI_STORE)
        skinny_q_lpr<FMT, LM_EPI_STORE>(a);
    else if (epi == LM_EPI_RESID)
        skinny_q_lpr<FMT, LM_EPI_RESID>(a);
    else
        skinny_q_lpr<FMT, LM_EPI_SWIGLU>(a);
}

// ------------------------------------------------------------------ embedding rows from the planes
// FMT: a plane format, or LM_EMBED_F32 (f32 table rows, 16 bytes = 4 values per thread and trip)
template <int FMT>
__global__ void __launch_bounds__(256) lm_embed_q_kernel(const uint8_t* __restrict__ q, const float* __restrict__ s,
                                                         const int32_t* __restrict__ ids, int vocab, int H,
                                                         float* __restrict__ out) {
    const int t = blockIdx.x;
    const int64_t row = min(max(ids[t], 0), vocab - 1);
    float* dst = out + (int64_t)t * H;
    if constexpr (FMT == LM_EMBED_F32) {
        const float* src = (const float*)q + row * H;
        for (int i = threadIdx.x * 4; i < H; i += 256 * 4) *(float4*)(dst + i) = *(const float4*)(src + i);
    } else {
        constexpr int VPL = QLane<FMT>::VPL;
        for (int word = threadIdx.x; word < H / VPL; word += 256) {
            float w[VPL];
            load_values<FMT, false>(q, s, row, H, word, w);
#pragma unroll
            for (int c = 0; c < VPL / 4; ++c)
                *(float4*)(dst + word * VPL + 4 * c) = make_float4(w[4 * c], w[4 * c + 1], w[4 * c + 2], w[4 * c + 3]);
        }
    }
}

bool planes_k_ok(int fmt, int K) { return fmt == WF_Q8_0 ? (K >= 32 && K % 32 == 0) : (K >= 256 && K % 256 == 0); }

}  // namespace

int lm_skinny_q_chain(int fmt, int K) {
    const int vpl = fmt == WF_Q4_K ? 32 : 16;
    if (K <= 32 * vpl) return vpl + 5;
    return vpl * (int)ceil_div(K, 64 * vpl) + 6;
}

void launch_lm_skinny_q(const uint16_t* x, int ldx, int B, const WeightView& W, int N, int K, int epi, float* y_f32,
                        uint16_t* y_act, int ldy, hipStream_t s) {
    ACEMI_CHECK(weight_planes(W.fmt) && W.q && W.s, "lm_skinny_q: the weight is not in block planes");
    ACEMI_CHECK(B >= 1 && B <= LM_MAX_BATCH && N >= 1 && planes_k_ok(W.fmt, K) && ldx % 8 == 0 && ldx >= K && x,
                "lm_skinny_q: bad shape");
    ACEMI_CHECK(epi == LM_EPI_SWIGLU ? (N % 32 == 0 && y_act) : ((epi == LM_EPI_STORE || epi == LM_EPI_RESID) && y_f32),
                "lm_skinny_q: bad epilogue");
    const SkinnyQArgs a{x, ldx, B, static_cast<const uint8_t*>(W.q), W.s, N, K, y_f32, y_act, ldy, s};
    if (W.fmt == WF_Q8_0)
        skinny_q_epi<WF_Q8_0>(epi, a);
    else if (W.fmt == WF_Q4_K)
        skinny_q_epi<WF_Q4_K>(epi, a);
    else
        skinny_q_epi<WF_Q6_K>(epi, a);
    ACEMI_HIP(hipGetLastError());
}

void launch_lm_embed_q(int fmt, const void* q, const float* s, const int32_t* ids, int n, int vocab, int H, float* out,
                       hipStream_t stream) {
    ACEMI_CHECK(n >= 1 && vocab >= 1 && q && ids && out, "lm_embed_q: bad arguments");
    const uint8_t* qb = static_cast<const uint8_t*>(q);
    if (fmt == LM_EMBED_F32) {
        ACEMI_CHECK(H >= 4 && H % 4 == 0, "lm_embed_q: bad row length");
        hipLaunchKernelGGL(lm_embed_q_kernel<LM_EMBED_F32>, dim3(n), dim3(256), 0, stream, qb, s, ids, vocab, H, out);
    } else {
        ACEMI_CHECK(weight_planes(fmt) && s && planes_k_ok(fmt, H), "lm_embed_q: bad format or row length");
        if (fmt == WF_Q8_0)
            hipLaunchKernelGGL(lm_embed_q_kernel<WF_Q8_0>, dim3(n), dim3(256), 0, stream, qb, s, ids, vocab, H, out);
        else if (fmt == WF_Q4_K)
            hipLaunchKernelGGL(lm_embed_q_kernel<WF_Q4_K>, dim3(n), dim3(256), 0, stream, qb, s, ids, vocab, H, out);
        else
            hipLaunchKernelGGL(lm_embed_q_kernel<WF_Q6_K>, dim3(n), dim3(256), 0, stream, qb, s, ids, vocab, H, out);
    }
    ACEMI_HIP(hipGetLastError());
}

}  // namespace acemi
