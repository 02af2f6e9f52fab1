// The per-type decoders of raw ggml blocks staged in LDS (device code), shared by kernels/dequant_blocks.hip (blocks ->
// bf16 image) and kernels/lm_decode_blocks.hip (the decode step's product and gather on the blocks themselves), so the
// two read a block the same way: the arithmetic of ggml's CPU dequantize_row_* (runtime/quant.cpp restates it on the
// host).  Every product is an fp16 scale times a small integer, exact in f32, so a value rounds once whether or not
// the compiler contracts the expression into an FMA.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace acemi {
namespace gblk {

// ggml type ids (runtime/gguf.h)
enum : int { T_Q4_0 = 2, T_Q4_1 = 3, T_Q5_0 = 6, T_Q5_1 = 7, T_Q8_0 = 8, T_Q2_K = 10, T_Q3_K = 11, T_Q4_K = 12,
             T_Q5_K = 13, T_Q6_K = 14, T_IQ4_NL = 20 };

template <int T> struct BlockOf;
template <> struct BlockOf<T_Q4_0> { static constexpr int BV = 32, BB = 18; };
template <> struct BlockOf<T_Q4_1> { static constexpr int BV = 32, BB = 20; };
template <> struct BlockOf<T_Q5_0> { static constexpr int BV = 32, BB = 22; };
template <> struct BlockOf<T_Q5_1> { static constexpr int BV = 32, BB = 24; };
template <> struct BlockOf<T_Q8_0> { static constexpr int BV = 32, BB = 34; };
template <> struct BlockOf<T_IQ4_NL> { static constexpr int BV = 32, BB = 18; };
template <> struct BlockOf<T_Q2_K> { static constexpr int BV = 256, BB = 84; };
template <> struct BlockOf<T_Q3_K> { static constexpr int BV = 256, BB = 110; };
template <> struct BlockOf<T_Q4_K> { static constexpr int BV = 256, BB = 144; };
template <> struct BlockOf<T_Q5_K> { static constexpr int BV = 256, BB = 176; };
template <> struct BlockOf<T_Q6_K> { static constexpr int BV = 256, BB = 210; };

// values / bytes per block of a type id; 0 for a type without a decoder here
__host__ __device__ inline int block_values_of(int type) {
    switch (type) {
        case T_Q4_0: case T_Q4_1: case T_Q5_0: case T_Q5_1: case T_Q8_0: case T_IQ4_NL: return 32;
        case T_Q2_K: case T_Q3_K: case T_Q4_K: case T_Q5_K: case T_Q6_K: return 256;
        default: return 0;
    }
}
__host__ __device__ inline int block_bytes_of(int type) {
    switch (type) {
        case T_Q4_0: case T_IQ4_NL: return 18;
        case T_Q4_1: return 20;
        case T_Q5_0: return 22;
        case T_Q5_1: return 24;
        case T_Q8_0: return 34;
        case T_Q2_K: return 84;
        case T_Q3_K: return 110;
        case T_Q4_K: return 144;
        case T_Q5_K: return 176;
        case T_Q6_K: return 210;
        default: return 0;
    }
}

// A block in the staged LDS words: s = the tile's words (16-byte aligned), o = the block's byte offset (even).  Every
// LDS read is an aligned 32-bit one, shifted into place: 16-bit reads of neighbouring fields were merged by the compiler
// into 64-bit reads at 2-byte alignment, which the LDS replays at 64 cycles per wave instruction.
struct lds_bytes {
    const uint32_t* s;
    int o;
};
__device__ __forceinline__ uint32_t rd8(lds_bytes p, int off) {
    const int a = p.o + off;
    return (p.s[a >> 2] >> ((a & 3) * 8)) & 0xffu;
}
__device__ __forceinline__ uint32_t rd16(lds_bytes p, int off) {  // (even offset: inside one word)
    const int a = p.o + off;
    return (p.s[a >> 2] >> ((a & 2) * 8)) & 0xffffu;
}
__device__ __forceinline__ uint32_t rd32(lds_bytes p, int off) {
    const int a = p.o + off;
    return __builtin_amdgcn_alignbyte(p.s[(a >> 2) + 1], p.s[a >> 2], (uint32_t)(a & 3));
}
__device__ __forceinline__ float rdh(lds_bytes p, int off) {
    const uint16_t h = (uint16_t)rd16(p, off);
    return (float)__builtin_bit_cast(_Float16, h);
}
__device__ __forceinline__ uint32_t pack_bf16(float lo, float hi) {
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
    bf16x2_t v;
    v[0] = (__bf16)lo;
    v[1] = (__bf16)hi;
    return __builtin_bit_cast(uint32_t, v);
}
// byte t (0..7) of the 8 bytes at off
__device__ __forceinline__ void rd8x8(lds_bytes p, int off, uint32_t (&b)[8]) {
    const int a = p.o + off;  // (the third word may lie past the block, never past the staged array)
    const uint32_t d0 = p.s[a >> 2], d1 = p.s[(a >> 2) + 1], d2 = p.s[(a >> 2) + 2];
    const uint32_t w0 = __builtin_amdgcn_alignbyte(d1, d0, (uint32_t)(a & 3));
    const uint32_t w1 = __builtin_amdgcn_alignbyte(d2, d1, (uint32_t)(a & 3));
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        b[t] = (w0 >> (8 * t)) & 0xffu;
        b[t + 4] = (w1 >> (8 * t)) & 0xffu;
    }
}
// get_scale_min_k4 of ggml (Q4_K / Q5_K): 6-bit scale and min of sub-block is (0..7) out of scales[12] at off
__device__ __forceinline__ void scale_min_k4(lds_bytes p, int off, int is, uint32_t& sc, uint32_t& m) {
    if (is < 4) {
        sc = rd8(p, off + is) & 63u;
        m = rd8(p, off + is + 4) & 63u;
    } else {
        const uint32_t a = rd8(p, off + is + 4);
        sc = (a & 0xFu) | ((rd8(p, off + is - 4) >> 6) << 4);
        m = (a >> 4) | ((rd8(p, off + is) >> 6) << 4);
    }
}

// Values 8j .. 8j+7 of the block at p (LDS), as ggml's dequantize_row_* computes them.  PLANE_ZERO: Q8_0 and Q6_K in the
// plane kernels' form fma(q + 128, s, -128 s) -- the same single rounding, but a zero is +0 as in those kernels, where
// ggml's d * q gives -0 under a negative scale; without it ggml's own product (what get_rows returns).
template <int T, bool PLANE_ZERO>
__device__ __forceinline__ void decode_values(lds_bytes p, int j, float (&f)[8]) {
    uint32_t b[8];
    if constexpr (T == T_Q4_0 || T == T_IQ4_NL) {  // {d, qs[16]}: value v < 16 low nibble of qs[v], else high of qs[v-16]
        const float d = rdh(p, 0);
        rd8x8(p, 2 + (j & 1) * 8, b);
        const int sh = (j >> 1) * 4;
        constexpr uint64_t kv_lo = 0xF6EADDCFBFAD9881ull, kv_hi = 0x7159453526190D01ull;  // kvalues_iq4nl as int8 bytes
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const uint32_t n = (b[t] >> sh) & 0xFu;
            if constexpr (T == T_Q4_0) {
                f[t] = (float)((int)n - 8) * d;
            } else {
                const int8_t kv = (int8_t)(((n & 8u) ? kv_hi : kv_lo) >> ((n & 7u) * 8));
                f[t] = d * (float)kv;
            }
        }
    } else if constexpr (T == T_Q4_1) {  // {d, m, qs[16]}
        const float d = rdh(p, 0), m = rdh(p, 2);
        rd8x8(p, 4 + (j & 1) * 8, b);
        const int sh = (j >> 1) * 4;
#pragma unroll
        for (int t = 0; t < 8; ++t) f[t] = (float)((b[t] >> sh) & 0xFu) * d + m;
    } else if constexpr (T == T_Q5_0 || T == T_Q5_1) {  // {d, [m,] qh[4], qs[16]}: bit v of qh = fifth bit of value v
        constexpr int O = T == T_Q5_0 ? 2 : 4;
        const float d = rdh(p, 0);
        const float m = T == T_Q5_1 ? rdh(p, 2) : 0.f;
        const uint32_t hb = (rd32(p, O) >> (8 * j)) & 0xffu;
        rd8x8(p, O + 4 + (j & 1) * 8, b);
        const int sh = (j >> 1) * 4;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const uint32_t q = ((b[t] >> sh) & 0xFu) | (((hb >> t) & 1u) << 4);
            if constexpr (T == T_Q5_0)
                f[t] = (float)((int)q - 16) * d;
            else
                f[t] = (float)q * d + m;
        }
    } else if constexpr (T == T_Q8_0) {  // {d, qs[32]}
        const float d = rdh(p, 0);
        rd8x8(p, 2 + 8 * j, b);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            if constexpr (PLANE_ZERO)
                f[t] = fmaf((float)(b[t] ^ 0x80u), d, -128.0f * d);  // = q * d (the plane kernel's form)
            else
                f[t] = (float)(int)(int8_t)b[t] * d;
        }
    } else if constexpr (T == T_Q2_K) {  // {scales[16], qs[64], d, dmin}
        const float d = rdh(p, 80), dmin = rdh(p, 82);
        const uint32_t sc = rd8(p, j >> 1);
        const float dl = d * (float)(sc & 0xFu), ml = dmin * (float)(sc >> 4);
        rd8x8(p, 16 + 32 * (j >> 4) + (j & 3) * 8, b);
        const int sh = 2 * ((j >> 2) & 3);
#pragma unroll
        for (int t = 0; t < 8; ++t) f[t] = dl * (float)((b[t] >> sh) & 3u) - ml;
    } else if constexpr (T == T_Q3_K) {  // {hmask[32], qs[64], scales[12], d}
        const float d_all = rdh(p, 108);
        const int is = j >> 1;
        const uint32_t lo = is < 8 ? (rd8(p, 96 + is) & 0xFu) : (rd8(p, 96 + is - 8) >> 4);
        const uint32_t hi = (rd8(p, 104 + (is & 3)) >> (2 * (is >> 2))) & 3u;
        const float dl = d_all * (float)((int)(lo | (hi << 4)) - 32);
        uint32_t hm[8];
        rd8x8(p, (j & 3) * 8, hm);
        rd8x8(p, 32 + 32 * (j >> 4) + (j & 3) * 8, b);
        const int jj = (j >> 2) & 3;
        const int hbit = 4 * (j >> 4) + jj;
#pragma unroll
        for (int t = 0; t < 8; ++t)
            f[t] = dl * (float)((int)((b[t] >> (2 * jj)) & 3u) - (((hm[t] >> hbit) & 1u) ? 0 : 4));
    } else if constexpr (T == T_Q4_K || T == T_Q5_K) {  // {d, dmin, scales[12], [qh[32],] qs[128]}
        const float d = rdh(p, 0), dmin = rdh(p, 2);
        const int is = j >> 2;
        uint32_t sc, m;
        scale_min_k4(p, 4, is, sc, m);
        const float d1 = d * (float)sc, m1 = dmin * (float)m;
        constexpr int QS = T == T_Q4_K ? 16 : 48;
        rd8x8(p, QS + 32 * (is >> 1) + (j & 3) * 8, b);
        const int sh = (is & 1) * 4;
        uint32_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if constexpr (T == T_Q5_K) rd8x8(p, 16 + (j & 3) * 8, h);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const uint32_t q = ((b[t] >> sh) & 0xFu) + (((h[t] >> is) & 1u) << 4);
            f[t] = d1 * (float)q - m1;
        }
    } else {  // T_Q6_K {ql[128], qh[64], scales[16] int8, d}
        const float d = rdh(p, 208);
        const int h = j >> 4, w = (j >> 2) & 3, l0 = (j & 3) * 8;
        const float ds = d * (float)(int)(int8_t)rd8(p, 192 + (j >> 1));
        uint32_t qh[8];
        rd8x8(p, 64 * h + l0 + (w & 1) * 32, b);
        rd8x8(p, 128 + 32 * h + l0, qh);
        const int sh = (w >> 1) * 4;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const uint32_t q = ((b[t] >> sh) & 0xFu) | (((qh[t] >> (2 * w)) & 3u) << 4);
            if constexpr (PLANE_ZERO)
                f[t] = fmaf((float)(q + 96u), ds, -128.0f * ds);  // = (q - 32) * ds (the plane kernel's form)
            else
                f[t] = ds * (float)((int)q - 32);
        }
    }
}

}  // namespace gblk
}  // namespace acemi
