// Decode step of the causal LM on raw ggml blocks (runtime/lm.cpp, ACE_MI_LM_RAW_BLOCKS=1): the skinny product and the
// embedding gather of lm_decode.hip for a WF_GGML_RAW weight, whose rows are the GGUF file's own block rows in row
// segments (BlockSeg, kernels.h), each of one ggml type: Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q2_K, Q3_K, Q4_K, Q5_K, Q6_K,
// IQ4_NL (0.5625 .. 1.0625 bytes per weight, against 2 for the bf16 image such a matrix is expanded to by default).
//
//   lm_skinny_blocks_kernel  y[B][N] = x[B][K] . W[N][K]^T, x bf16, f32 accumulate.  The weight value multiplied is
//                            rne_bf16 of the f32 dequant, the bits launch_dequant_blocks writes (ggml_block_decode.h is
//                            shared with it, Q8_0 / Q6_K in the fma(q + 128, s, -128 s) form): the prefill's GEMM on
//                            the expanded image and the step multiply the same weights.
//
// Alignment.  A block row is K / BV * BB bytes and only 2-byte aligned (84, 110, 210 bytes at K = 256), so nothing is
// loaded relative to the row: the lanes that share a row load the aligned 16-byte words of the segment's allocation
// that cover the row's bytes (one global_load_dwordx4 each, consecutive lanes at consecutive words: coalesced), write
// them to LDS at the same address modulo 16, and the decoders read the blocks out of LDS with aligned 32-bit reads at
// the row's skew.  The first word starts at most 15 bytes before the row and the last ends at most 15 bytes after it:
// inside the segment, or inside the 16-byte-aligned extent of its allocation at either end (Loader::from_raw aligns
// every segment to 16 bytes and pads it to a multiple of 16; kernels.h).  No load is narrower than 16 bytes or
// misaligned.
// Work split.  One output unit (a row; for SwiGLU gate row j of one segment and up row j of the other, each with its
// own type) belongs to LPR lanes of a wave, four waves per workgroup:
//   K <= 256:  LPR = 32, two units per wave, one trip of 256 values (a 84 .. 272-byte row is 6 .. 18 words)
//   larger K:  LPR = 64, one unit per wave, trips of 2048 values (at most 137 words: up to three loads per lane, all
//              issued before the first LDS write), the last one partial
// Per trip: stage the rows' words, barrier, decode, barrier.  Lane l decodes the 8-value chunks l, l + LPR, .. of the
// trip, each one rd8x8 / scale read of its block, and multiplies it with the matching 16 bytes of each of the up to 8
// activation rows, which come from L2 (bf16 rows of K values: 2 .. 12 KB in all, read by every wave).
// Bytes.  A row's words are loaded once per launch, for all B rows; only the up to 30 bytes of slack at a row's two
// ends are touched by the neighbouring unit as well.
// Reduction: lane-local over its k in ascending order (one fma per value), then the xor butterfly over the LPR lanes
// (offsets LPR/2 .. 1).  No atomics, no split along K: bit-identical between runs.  A lane's values are k = 8 l + 512 i,
// lm_decode.hip's mapping, so on the same weights the two kernels return the same bits.  Longest f32 addition chain
// behind one output (lm_skinny_blocks_chain, any type):  8 + 5 (LPR = 32),  8 ceil(K / 512) + 6 (LPR = 64).
// Type dispatch: one launch serves up to 8 segments; a workgroup belongs to one segment, and the type selects, once per
// row and trip (a switch on a kernel argument: wave-uniform), a loop compiled for that type.  Nothing branches on the
// type per value.
// No MFMA: M <= 8 rows against a weight read once is bandwidth-bound (a 16-row tile would waste half of it and the
// decoders, not the multiplies, are the ALU work).
//
//   lm_embed_blocks_kernel   rows of a raw-block table as ggml's get_rows returns them: the f32 dequant itself (ggml's own
//                            products, quant::dequantize_rows' arithmetic: -0 where ggml gives -0), not rounded to
//                            bf16; ids clamped into the table.  One workgroup per id, the same staging.
//
// Built with -fno-slp-vectorize (Makefile), as dequant_blocks.hip is: the two must round every value alike.
#include <hip/hip_runtime.h>

#include "../kernels.h"
#include "ggml_block_decode.h"

namespace acemi {

namespace {

using namespace gblk;

constexpr int MAX_SEGS = 8;
constexpr int CV_SHORT = 256, CV_LONG = 2048;  // values per trip at LPR = 32 / 64
// LDS bytes of one staged row chunk of cv values of any type: the widest blocks (Q8_0, 34 bytes per 32 values), one
// word for the skew, and 16 bytes because rd8x8 reads the word after a block's last 8 bytes
constexpr int region_bytes(int cv) { return ((cv / 32 * 34 + 15) / 16 + 1) * 16 + 16; }

struct SkinnySegs {
    const uint8_t* src[MAX_SEGS];
    int type[MAX_SEGS], rows[MAX_SEGS], row0[MAX_SEGS], step[MAX_SEGS], group[MAX_SEGS];
    int end[MAX_SEGS];  // inclusive prefix sums of the segments' workgroup counts
    int n;
};

__device__ __forceinline__ uint16_t b_f32_to_bf16_rne(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 64u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
__device__ __forceinline__ float b_silu(float x) { return x / (1.0f + expf(-x)); }

__device__ __forceinline__ void unpack8_bf16(const uint4& w, float* f) {
    f[0] = __uint_as_float(w.x << 16), f[1] = __uint_as_float(w.x & 0xffff0000u);
    f[2] = __uint_as_float(w.y << 16), f[3] = __uint_as_float(w.y & 0xffff0000u);
    f[4] = __uint_as_float(w.z << 16), f[5] = __uint_as_float(w.z & 0xffff0000u);
    f[6] = __uint_as_float(w.w << 16), f[7] = __uint_as_float(w.w & 0xffff0000u);
}

// Bytes [b0, b0 + nbytes) of the allocation at src (16-byte aligned) into the LDS region, by NL lanes (this one: lane):
// the aligned words that cover them, at most LW per lane, every load before the first write.  Returns the skew, the
// offset of byte b0 in the region.
template <int NL, int LW>
__device__ __forceinline__ int stage_bytes(const uint8_t* __restrict__ src, int64_t b0, int nbytes, uint4* region, int lane) {
    const int64_t a0 = b0 & ~(int64_t)15;
    const int nwords = (int)((((b0 + nbytes + 15) & ~(int64_t)15) - a0) >> 4);
    const uint4* __restrict__ g = reinterpret_cast<const uint4*>(src + a0);
    uint4 w[LW];
#pragma unroll
    for (int i = 0; i < LW; ++i) {
        const int wi = lane + i * NL;
        w[i] = wi < nwords ? g[wi] : uint4{0, 0, 0, 0};
    }
#pragma unroll
    for (int i = 0; i < LW; ++i) {
        const int wi = lane + i * NL;
        if (wi < nwords) region[wi] = w[i];
    }
    return (int)(b0 - a0);
}

// One staged row chunk of nv values of type T against the B activation rows at xk (the chunk's first k): this lane's
// 8-value chunks in ascending k, one fma per value.
template <int T, int LPR, int BT>
__device__ __forceinline__ void row_pass(const uint4* region, int skew, int nv, int lane, const uint16_t* __restrict__ xk,
                                         int ldx, int B, float (&acc)[BT]) {
    constexpr int CPB = BlockOf<T>::BV / 8, BB = BlockOf<T>::BB;
    for (int c = lane; c < nv / 8; c += LPR) {
        float f[8], w[8];
        decode_values<T, true>(lds_bytes{reinterpret_cast<const uint32_t*>(region), skew + (c / CPB) * BB}, c % CPB, f);
#pragma unroll
        for (int i = 0; i < 4; ++i) {  // RNE to bf16 and back (the image's words)
            const uint32_t p = pack_bf16(f[2 * i], f[2 * i + 1]);
            w[2 * i] = __uint_as_float(p << 16);
            w[2 * i + 1] = __uint_as_float(p & 0xffff0000u);
        }
#pragma unroll
        for (int b = 0; b < BT; ++b) {
            if (b < B) {
                float xv[8];
                unpack8_bf16(*(const uint4*)(xk + (int64_t)b * ldx + 8 * c), xv);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[b] = fmaf(w[j], xv[j], acc[b]);
            }
        }
    }
}

#define ACEMI_BLOCK_TYPES(X) \
    X(T_Q4_0) X(T_Q4_1) X(T_Q5_0) X(T_Q5_1) X(T_Q8_0) X(T_Q2_K) X(T_Q3_K) X(T_Q4_K) X(T_Q5_K) X(T_Q6_K) X(T_IQ4_NL)

// ROWS 1: STORE / RESID over the segments of sg.  ROWS 2: SwiGLU, sg.src[0] / type[0] = the gate rows, [1] = the up
// rows, unit j = row j of both.  BT: the compiled batch bound (1, 2, 4, 8); rows b >= B are skipped and never read.
template <int ROWS, int LPR, int BT>
__global__ void __launch_bounds__(256) lm_skinny_blocks_kernel(const uint16_t* __restrict__ x, int ldx, int B, SkinnySegs sg,
                                                               int K, int epi, float* __restrict__ y_f32,
                                                               uint16_t* __restrict__ y_act, int ldy) {
    constexpr int GROUPS = 64 / LPR;  // units per wave
    constexpr int CV = LPR == 32 ? CV_SHORT : CV_LONG;
    constexpr int REGION = region_bytes(CV) / 16;  // uint4 words
    constexpr int LW = (REGION - 1 + LPR - 1) / LPR;
    __shared__ uint4 smem[4 * GROUPS * ROWS * REGION];

    int mi = 0, blk = blockIdx.x;
    if constexpr (ROWS == 1) {
#pragma unroll
        for (int i = 0; i < MAX_SEGS - 1; ++i) mi += (i + 1 < sg.n && blk >= sg.end[i]) ? 1 : 0;
        if (mi > 0) blk -= sg.end[mi - 1];
    }
    const int lane = threadIdx.x & (LPR - 1);
    const int slot = threadIdx.x / LPR;  // the unit's place in the workgroup
    const int unit = blk * 4 * GROUPS + slot;
    const bool active = unit < sg.rows[mi];  // (a whole group of LPR lanes)
    uint4* region = smem + slot * ROWS * REGION;

    float acc[ROWS][BT];
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
        for (int b = 0; b < BT; ++b) acc[r][b] = 0.f;
    for (int k0 = 0; k0 < K; k0 += CV) {  // (uniform over the workgroup: every thread reaches both barriers)
        const int nv = min(CV, K - k0);
        int skew[ROWS];
        if (k0 > 0) __syncthreads();  // the last trip's reads are done
        if (active) {
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                const int ty = sg.type[ROWS == 1 ? mi : r];
                const int bv = block_values_of(ty), bb = block_bytes_of(ty);
                const int64_t b0 = (int64_t)unit * (K / bv) * bb + (int64_t)(k0 / bv) * bb;
                skew[r] = stage_bytes<LPR, LW>(sg.src[ROWS == 1 ? mi : r], b0, nv / bv * bb, region + r * REGION, lane);
            }
        }
        __syncthreads();
        if (active) {
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                switch (sg.type[ROWS == 1 ? mi : r]) {
#define ACEMI_ROW_PASS(TY)                                                                               \
    case TY:                                                                                             \
        row_pass<TY, LPR, BT>(region + r * REGION, skew[r], nv, lane, x + k0, ldx, B, acc[r]);           \
        break;
                    ACEMI_BLOCK_TYPES(ACEMI_ROW_PASS)
#undef ACEMI_ROW_PASS
                    default: break;
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
    if (!active || lane != 0) return;
    const int g = sg.group[mi];
    const int64_t col = ROWS == 2 ? unit : sg.row0[mi] + (int64_t)(unit / g) * g * sg.step[mi] + unit % g;
#pragma unroll
    for (int b = 0; b < BT; ++b) {
        if (b < B) {
            if constexpr (ROWS == 2) {
                y_act[(int64_t)b * ldy + col] = b_f32_to_bf16_rne(b_silu(acc[0][b]) * acc[ROWS - 1][b]);
            } else if (epi == LM_EPI_RESID) {
                y_f32[(int64_t)b * ldy + col] += acc[0][b];
            } else {
                y_f32[(int64_t)b * ldy + col] = acc[0][b];
            }
        }
    }
}

struct SkinnyBlocksArgs {
    const uint16_t* x;
    int ldx, B;
    SkinnySegs sg;
    int K, epi;
    float* y_f32;
    uint16_t* y_act;
    int ldy;
    hipStream_t stream;
};

template <int ROWS, int LPR, int BT>
void skinny_blocks_launch(const SkinnyBlocksArgs& a) {
    hipLaunchKernelGGL((lm_skinny_blocks_kernel<ROWS, LPR, BT>), dim3((unsigned)a.sg.end[a.sg.n - 1]), dim3(256), 0, a.stream,
                       a.x, a.ldx, a.B, a.sg, a.K, a.epi, a.y_f32, a.y_act, a.ldy);
}
template <int ROWS, int LPR>
void skinny_blocks_b(const SkinnyBlocksArgs& a) {
    if (a.B == 1)
        skinny_blocks_launch<ROWS, LPR, 1>(a);
    else if (a.B == 2)
        skinny_blocks_launch<ROWS, LPR, 2>(a);
    else if (a.B <= 4)
        skinny_blocks_launch<ROWS, LPR, 4>(a);
    else
        skinny_blocks_launch<ROWS, LPR, 8>(a);
}
template <int ROWS>
void skinny_blocks_lpr(SkinnyBlocksArgs& a) {
    const int per_group = a.K <= CV_SHORT ? 8 : 4;  // units per workgroup
    for (int i = 0; i < a.sg.n; ++i) a.sg.end[i] = (i > 0 ? a.sg.end[i - 1] : 0) + (int)ceil_div(a.sg.rows[i], per_group);
    if (a.K <= CV_SHORT)
        skinny_blocks_b<ROWS, 32>(a);
    else
        skinny_blocks_b<ROWS, 64>(a);
}

// ------------------------------------------------------------------ embedding rows from the blocks
__global__ void __launch_bounds__(256) lm_embed_blocks_kernel(const uint8_t* __restrict__ src, int type,
                                                              const int32_t* __restrict__ ids, int vocab, int H,
                                                              float* __restrict__ out) {
    constexpr int REGION = region_bytes(CV_LONG) / 16;
    __shared__ uint4 region[REGION];
    const int64_t row = min(max(ids[blockIdx.x], 0), vocab - 1);
    float* dst = out + (int64_t)blockIdx.x * H;
    const int bv = block_values_of(type), bb = block_bytes_of(type);
    for (int k0 = 0; k0 < H; k0 += CV_LONG) {
        const int nv = min(CV_LONG, H - k0);
        if (k0 > 0) __syncthreads();
        const int skew = stage_bytes<256, 1>(src, row * (H / bv) * bb + (int64_t)(k0 / bv) * bb, nv / bv * bb, region,
                                             threadIdx.x);
        __syncthreads();
        const int c = threadIdx.x;  // CV_LONG / 8 chunks = one per thread
        if (c < nv / 8) {
            float f[8] = {};
            switch (type) {
#define ACEMI_EMBED_ROW(TY)                                                                                              \
    case TY:                                                                                                             \
        decode_values<TY, false>(lds_bytes{reinterpret_cast<const uint32_t*>(region),                                    \
                                           skew + (c / (BlockOf<TY>::BV / 8)) * BlockOf<TY>::BB},                        \
                                 c % (BlockOf<TY>::BV / 8), f);                                                          \
        break;
                ACEMI_BLOCK_TYPES(ACEMI_EMBED_ROW)
#undef ACEMI_EMBED_ROW
                default: break;  // (the launcher refuses other types)
            }
            *(float4*)(dst + k0 + 8 * c) = make_float4(f[0], f[1], f[2], f[3]);
            *(float4*)(dst + k0 + 8 * c + 4) = make_float4(f[4], f[5], f[6], f[7]);
        }
    }
}
static_assert(region_bytes(CV_LONG) / 16 - 1 <= 256 && CV_LONG / 8 == 256, "the gather stages and decodes a trip in one pass");

bool seg_ok(const BlockSeg& g, int K) {
    const int bv = block_values_of(g.type);
    return bv > 0 && K >= bv && K % bv == 0 && g.src && (reinterpret_cast<uintptr_t>(g.src) & 15) == 0 && g.rows > 0 &&
           g.row0 >= 0 && g.step >= 1 && g.group >= 1;
}

}  // namespace

int lm_skinny_blocks_chain(int, int K) { return K <= CV_SHORT ? 8 + 5 : 8 * (int)ceil_div(K, 512) + 6; }

void launch_lm_skinny_blocks(const uint16_t* x, int ldx, int B, const WeightView& W, int N, int K, int epi, float* y_f32,
                             uint16_t* y_act, int ldy, hipStream_t s) {
    ACEMI_CHECK(W.fmt == WF_GGML_RAW && W.segs && W.n_segs >= 1, "lm_skinny_blocks: the weight is not in raw ggml blocks");
    ACEMI_CHECK(B >= 1 && B <= LM_MAX_BATCH && N >= 1 && K >= 32 && ldx % 8 == 0 && ldx >= K && x &&
                    (reinterpret_cast<uintptr_t>(x) & 15) == 0,
                "lm_skinny_blocks: bad shape");
    ACEMI_CHECK(epi == LM_EPI_SWIGLU ? (N % 32 == 0 && y_act) : ((epi == LM_EPI_STORE || epi == LM_EPI_RESID) && y_f32),
                "lm_skinny_blocks: bad epilogue");
    for (int i = 0; i < W.n_segs; ++i)
        ACEMI_CHECK(seg_ok(W.segs[i], K) && block_seg_row(W.segs[i], W.segs[i].rows - 1) < N, "lm_skinny_blocks: bad segment");
    SkinnyBlocksArgs a{x, ldx, B, SkinnySegs{}, K, epi, y_f32, y_act, ldy, s};
    auto put = [&](const BlockSeg& g) {
        const int m = a.sg.n++;
        a.sg.src[m] = static_cast<const uint8_t*>(g.src);
        a.sg.type[m] = g.type;
        a.sg.rows[m] = g.rows;
        a.sg.row0[m] = g.row0;
        a.sg.step[m] = g.step;
        a.sg.group[m] = g.group;
    };
    if (epi == LM_EPI_SWIGLU) {  // the gate rows and the up rows of the 16-row interleave, one segment each
        const BlockSeg* gate = nullptr;
        const BlockSeg* up = nullptr;
        for (int i = 0; i < W.n_segs; ++i) (W.segs[i].row0 == 0 ? gate : up) = &W.segs[i];
        ACEMI_CHECK(W.n_segs == 2 && gate && up && up->row0 == 16 && gate->rows == N / 2 && up->rows == N / 2 &&
                        gate->step == 2 && up->step == 2 && gate->group == 16 && up->group == 16,
                    "lm_skinny_blocks: SwiGLU takes one gate and one up segment (group 16, step 2)");
        put(*gate);
        put(*up);
        a.sg.n = 1;  // one job of N / 2 units; [1] is read as the up rows
        skinny_blocks_lpr<2>(a);
    } else {
        for (int i0 = 0; i0 < W.n_segs; i0 += MAX_SEGS) {
            a.sg = SkinnySegs{};
            for (int i = i0; i < W.n_segs && i < i0 + MAX_SEGS; ++i) put(W.segs[i]);
            skinny_blocks_lpr<1>(a);
        }
    }
    ACEMI_HIP(hipGetLastError());
}

void launch_lm_embed_blocks(const WeightView& W, const int32_t* ids, int n, int vocab, int H, float* out, hipStream_t stream) {
    ACEMI_CHECK(W.fmt == WF_GGML_RAW && W.segs && W.n_segs == 1, "lm_embed_blocks: the table is not one raw-block segment");
    const BlockSeg& g = W.segs[0];
    ACEMI_CHECK(n >= 1 && vocab >= 1 && ids && out && seg_ok(g, H) && g.rows == vocab && g.row0 == 0 && g.step == 1 &&
                    (reinterpret_cast<uintptr_t>(out) & 15) == 0,
                "lm_embed_blocks: bad arguments");
    hipLaunchKernelGGL(lm_embed_blocks_kernel, dim3(n), dim3(256), 0, stream, static_cast<const uint8_t*>(g.src), g.type, ids,
                       vocab, H, out);
    ACEMI_HIP(hipGetLastError());
}

}  // namespace acemi
