// Raw ggml block rows -> dense bf16 image (gfx950): the expansion behind WF_GGML_RAW weights (kernels.h).
//
// The device holds the GGUF file's bytes.  A job is one row segment (BlockSeg): consecutive block rows of one ggml
// type, which are one contiguous byte stream, so a workgroup takes a run of TILE = 8192 values' blocks of it:
//   1. every thread loads up to three aligned 16-byte words of the run (a wave reads 1 KiB contiguous; blocks of 18,
//      22, 34 and 110 bytes are only 2-byte aligned, so the words are aligned to the allocation, not to the blocks,
//      and no global load is ever narrower than 16 bytes or misaligned) -- all loads before anything else;
//   2. the words go to LDS at the same address modulo 16, one barrier;
//   3. each thread decodes four 8-value chunks out of LDS with 16-bit reads (every block field sits at an even offset)
//      and the arithmetic of ggml's CPU dequantize_row_* (runtime/quant.cpp restates it on the host): every product is
//      an fp16 scale times a small integer, exact in f32, so a value rounds once whether or not the compiler contracts
//      the expression into an FMA; then RNE to bf16.  Q8_0 and Q6_K are written in the plane kernel's form,
//      fma(q + 128, s, -128 s): the same single rounding, and a zero is +0 as in that kernel (ggml's d * q gives -0 under
//      a negative scale), so a matrix expands to the same bits from raw blocks as from planes;
//   4. four 16-byte stores per thread, consecutive threads to consecutive 16 bytes of an output row.
// HBM-bound by design: bytes per weight read (0.5625 Q4_0 .. 1.0625 Q8_0) + 2 written.
#include <vector>

#include "../kernels.h"

namespace acemi {
namespace {

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

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) u32x4 global_u32x4;

constexpr int TILE = 8192;    // values per workgroup
constexpr int THREADS = 256;  // 4 chunks of 8 values per thread
constexpr int MAX_JOBS = 8;

struct BlocksBatch {  // up to 8 same-type segments expanded by one launch
    const char* src[MAX_JOBS];
    uint16_t* out[MAX_JOBS];
    int64_t ld[MAX_JOBS];
    int64_t blocks[MAX_JOBS];  // rows * K / BV
    int bpr[MAX_JOBS];         // blocks per row
    int row0[MAX_JOBS], step[MAX_JOBS], group[MAX_JOBS];
    int end[MAX_JOBS];         // exclusive prefix sums of the tile counts
    int n;
};

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
__device__ __forceinline__ uint4 pack8(const float (&f)[8]) {
    return uint4{pack_bf16(f[0], f[1]), pack_bf16(f[2], f[3]), pack_bf16(f[4], f[5]), pack_bf16(f[6], f[7])};
}
// byte t (0..7) of the 8 bytes at off
__device__ __forceinline__ void rd8x8(lds_bytes p, int off, uint32_t (&b)[8]) {
    const int a = p.o + off;  // (the third word may lie past the block, never past the staged array: WORDS)
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

// values 8j .. 8j+7 of the block at p (LDS), as ggml's dequantize_row_* computes them
template <int T>
__device__ __forceinline__ uint4 decode8(lds_bytes p, int j) {
    float f[8];
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
        for (int t = 0; t < 8; ++t) f[t] = fmaf((float)(b[t] ^ 0x80u), d, -128.0f * d);  // = q * d (the plane kernel's form)
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
            f[t] = fmaf((float)(q + 96u), ds, -128.0f * ds);  // = (q - 32) * ds (the plane kernel's form)
        }
    }
    return pack8(f);
}

template <int T>
__global__ void __launch_bounds__(THREADS) dequant_blocks_kernel(BlocksBatch bt) {
    constexpr int BV = BlockOf<T>::BV, BB = BlockOf<T>::BB;
    constexpr int NB = TILE / BV;                 // blocks per tile
    constexpr int WORDS = (NB * BB + 15) / 16 + 1;  // 16-byte words a tile can span (start anywhere in a word)
    static_assert(WORDS * 16 >= 14 + NB * BB + 2, "rd8x8 reads up to 4 bytes past a block's last 8");
    constexpr int LPT = (WORDS + THREADS - 1) / THREADS;
    __shared__ __attribute__((aligned(16))) uint8_t smem[WORDS * 16];

    int mi = 0;
    int tile = blockIdx.x;
#pragma unroll
    for (int i = 0; i < MAX_JOBS - 1; ++i) mi += (i + 1 < bt.n && tile >= bt.end[i]) ? 1 : 0;
    if (mi > 0) tile -= bt.end[mi - 1];
    const int64_t g0 = (int64_t)tile * NB;                             // first block of the tile in the segment
    const int nb = (int)min((int64_t)NB, bt.blocks[mi] - g0);          // its blocks (the last tile: fewer)
    const int64_t byte0 = g0 * BB, byte1 = byte0 + (int64_t)nb * BB;   // [byte0, byte1) of the segment
    const int64_t a0 = byte0 & ~(int64_t)15;
    const int nwords = (int)(((byte1 + 15) & ~(int64_t)15) - a0) >> 4;  // <= WORDS; the last one ends at most 15 bytes
                                                                        // after the segment (readable: kernels.h)
    const uint4* __restrict__ gsrc = reinterpret_cast<const uint4*>(bt.src[mi] + a0);
    // (three named registers, not an array: the compiler kept a conditionally written array in scratch / LDS)
    static_assert(LPT <= 3, "staging loads per thread");
    const int i0 = threadIdx.x, i1 = threadIdx.x + THREADS, i2 = threadIdx.x + 2 * THREADS;
    uint4 w0 = uint4{0, 0, 0, 0}, w1 = w0, w2 = w0;
    if (i0 < nwords) w0 = gsrc[i0];
    if constexpr (LPT > 1)
        if (i1 < nwords) w1 = gsrc[i1];
    if constexpr (LPT > 2)
        if (i2 < nwords) w2 = gsrc[i2];
    if (i0 < nwords) *reinterpret_cast<uint4*>(smem + 16 * i0) = w0;
    if constexpr (LPT > 1)
        if (i1 < nwords) *reinterpret_cast<uint4*>(smem + 16 * i1) = w1;
    if constexpr (LPT > 2)
        if (i2 < nwords) *reinterpret_cast<uint4*>(smem + 16 * i2) = w2;
    __syncthreads();

    const int skew = (int)(byte0 - a0);
    const uint32_t bpr = (uint32_t)bt.bpr[mi];
    const int r0 = (int)(g0 / bpr);                      // the tile's first row and block column (uniform)
    const uint32_t kb0 = (uint32_t)(g0 - (int64_t)r0 * bpr);
    const uint32_t grp = (uint32_t)bt.group[mi];
    constexpr int CPB = BV / 8;  // chunks per block
    uint4 o[TILE / 8 / THREADS];
    __attribute__((address_space(1))) uint16_t* dst[TILE / 8 / THREADS];
#pragma unroll
    for (int k = 0; k < TILE / 8 / THREADS; ++k) {
        const int c = threadIdx.x + k * THREADS;  // 8-value chunk of the tile
        const int bi = c / CPB, j = c % CPB;
        dst[k] = nullptr;
        if (bi < nb) {
            const uint32_t x = kb0 + (uint32_t)bi;
            const uint32_t r = (uint32_t)r0 + x / bpr, kb = x % bpr;
            const int64_t orow = bt.row0[mi] + (int64_t)(r / grp) * grp * bt.step[mi] + r % grp;
            o[k] = decode8<T>(lds_bytes{reinterpret_cast<const uint32_t*>(smem), skew + bi * BB}, j);
            dst[k] = (__attribute__((address_space(1))) uint16_t*)bt.out[mi] + orow * bt.ld[mi] + (int64_t)kb * BV + 8 * j;
        }
    }
#pragma unroll
    for (int k = 0; k < TILE / 8 / THREADS; ++k)
        if (dst[k]) *reinterpret_cast<global_u32x4*>(dst[k]) = u32x4{o[k].x, o[k].y, o[k].z, o[k].w};
}

int block_values_of(int type) {
    switch (type) {
        case T_Q4_0: case T_Q4_1: case T_Q5_0: case T_Q5_1: case T_Q8_0: case T_IQ4_NL: return 32;
        case T_Q2_K: case T_Q3_K: case T_Q4_K: case T_Q5_K: case T_Q6_K: return 256;
        default: return 0;
    }
}

void launch_batch(int type, const BlocksBatch& b, hipStream_t s) {
    const dim3 grid((unsigned)b.end[b.n - 1]);
#define ACEMI_DQB(TY) \
    case TY: hipLaunchKernelGGL((dequant_blocks_kernel<TY>), grid, dim3(THREADS), 0, s, b); break;
    switch (type) {
        ACEMI_DQB(T_Q4_0)
        ACEMI_DQB(T_Q4_1)
        ACEMI_DQB(T_Q5_0)
        ACEMI_DQB(T_Q5_1)
        ACEMI_DQB(T_Q8_0)
        ACEMI_DQB(T_Q2_K)
        ACEMI_DQB(T_Q3_K)
        ACEMI_DQB(T_Q4_K)
        ACEMI_DQB(T_Q5_K)
        ACEMI_DQB(T_Q6_K)
        ACEMI_DQB(T_IQ4_NL)
        default: throw std::runtime_error("dequant_blocks: bad type");
    }
#undef ACEMI_DQB
    ACEMI_HIP(hipGetLastError());
}

}  // namespace

void launch_dequant_blocks(const DequantBlocksJob* jobs, int n, hipStream_t s) {
    for (int i = 0; i < n; ++i) {
        const DequantBlocksJob& j = jobs[i];
        const int bv = block_values_of(j.seg.type);
        ACEMI_CHECK(bv > 0, "dequant_blocks: not a block-quantized ggml type");
        ACEMI_CHECK(j.seg.src && j.out && j.seg.rows > 0 && j.K > 0 && j.K % bv == 0 && j.ld >= j.K && j.ld % 8 == 0 &&
                        j.seg.row0 >= 0 && j.seg.step >= 1 && j.seg.group >= 1,
                    "dequant_blocks: bad job");
        ACEMI_CHECK((reinterpret_cast<uintptr_t>(j.seg.src) & 15) == 0 && (reinterpret_cast<uintptr_t>(j.out) & 15) == 0,
                    "dequant_blocks: src and out must be 16-byte aligned");
        ACEMI_CHECK((int64_t)j.seg.rows * j.K / TILE < (1 << 28), "dequant_blocks: segment too large");
    }
    // one launch per type (per 8 jobs of it), in the order the types first appear
    std::vector<char> done((size_t)n, 0);
    for (int i = 0; i < n; ++i) {
        if (done[i]) continue;
        const int type = jobs[i].seg.type;
        const int bv = block_values_of(type);
        BlocksBatch b{};
        auto flush = [&]() {
            if (b.n > 0) launch_batch(type, b, s);
            b = BlocksBatch{};
        };
        for (int k = i; k < n; ++k) {
            if (done[k] || jobs[k].seg.type != type) continue;
            done[k] = 1;
            const DequantBlocksJob& j = jobs[k];
            const int m = b.n++;
            b.src[m] = static_cast<const char*>(j.seg.src);
            b.out[m] = j.out;
            b.ld[m] = j.ld;
            b.bpr[m] = j.K / bv;
            b.blocks[m] = (int64_t)j.seg.rows * b.bpr[m];
            b.row0[m] = j.seg.row0;
            b.step[m] = j.seg.step;
            b.group[m] = j.seg.group;
            const int tiles = (int)((b.blocks[m] * bv + TILE - 1) / TILE);
            b.end[m] = (m > 0 ? b.end[m - 1] : 0) + tiles;
            if (b.n == MAX_JOBS) flush();
        }
        flush();
    }
}

}  // namespace acemi
