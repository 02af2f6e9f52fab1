// LoRA merge (gfx950): the adapted 16-bit image of a weight matrix, out = rne16(f32(base) + eff * (B . A)), with the
// fixed arithmetic of kernels.h (LoraMergeJob): a rank-ordered chain of separately rounded f32 multiplies and adds,
// so every build of it (this kernel, the host loops of runtime/engine.cpp, numpy) gives the same bits.
//
// One workgroup merges a tile of 64 module rows x 256 columns: the A slice [r][256] and the B slice [64][r] pass
// through LDS in chunks of 32 ranks, each thread keeps 8 rows x 8 columns of f32 accumulators (two-wide packed
// multiplies and adds), reads its 8 base values per row with one 16-byte load and writes the 8 results with one
// 16-byte store.  2 B read + 2 B written per weight plus the (cached) A / B slices; the VALU chain is 2 r operations
// per weight, which bounds the kernel from r ~ 32 up (DESIGN.md "LoRA adapters").  Copy-through rows of a fused
// matrix (a module without an adapter) are moved by tiles of the same shape that only load and store.
#include <algorithm>

#include "../kernels.h"

// the chain is never contracted into FMAs (the kernel files build with -ffp-contract=fast-honor-pragmas)
#pragma clang fp contract(off)

namespace acemi {
namespace {

constexpr int TR = 64;    // rows per tile
constexpr int TC = 256;   // columns per tile
constexpr int RC = 32;    // ranks per LDS chunk
constexpr int BPAD = 4;   // padding of a Bs row (keeps 16-byte alignment)

typedef float v2f __attribute__((ext_vector_type(2)));

struct LoraBatch {
    LoraMergeJob job[8];
    int mod_tiles[8];  // tiles of module rows of job i
    int end[8];        // exclusive prefix sums of (module + copy) tiles
    int n;
};

__device__ __forceinline__ uint16_t f32_to_bf16_rne(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 64u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
__device__ __forceinline__ uint16_t f32_to_16(bool f16, float f) {
    if (f16) return __builtin_bit_cast(uint16_t, (_Float16)f);
    return f32_to_bf16_rne(f);
}
__device__ __forceinline__ float f16_to_f32(bool f16, uint16_t v) {
    if (f16) return (float)__builtin_bit_cast(_Float16, v);
    return __uint_as_float((uint32_t)v << 16);
}

__global__ void __launch_bounds__(256) lora_merge_kernel(LoraBatch b) {
    __shared__ __attribute__((aligned(16))) float As[RC][TC];
    __shared__ __attribute__((aligned(16))) float Bs[RC][TR + BPAD];

    int ji = 0;
#pragma unroll
    for (int i = 0; i < 7; ++i) ji += (i + 1 < b.n && (int)blockIdx.x >= b.end[i]) ? 1 : 0;
    const LoraMergeJob& jb = b.job[ji];
    int tile = (int)blockIdx.x - (ji > 0 ? b.end[ji - 1] : 0);
    const int col_tiles = (jb.cols + TC - 1) / TC;
    const bool copy_tile = tile >= b.mod_tiles[ji];
    if (copy_tile) tile -= b.mod_tiles[ji];
    const int c0 = (tile % col_tiles) * TC;
    const int r0 = (tile / col_tiles) * TR;  // first module row (merge tile) / first row of the range (copy tile)

    const int tid = threadIdx.x;
    const int cg = tid & 31, rg = tid >> 5;
    const int col = c0 + cg * 8;
    const bool col_ok = col < jb.cols;  // cols % 8 == 0: a thread's 8 columns are all inside or all outside
    const int row_end = jb.row0 + jb.rows;

    if (copy_tile) {  // rows of the range that belong to no module row: base -> out
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int fr = jb.row0 + r0 + rg * 8 + k;
            if (fr < row_end && col_ok &&
                lora_module_row(jb.map, jb.row_off, jb.half, jb.rows_mod, jb.r, fr) < 0) {
                const uint4 v = *reinterpret_cast<const uint4*>(jb.base + (int64_t)fr * jb.ld_base + col);
                *reinterpret_cast<uint4*>(jb.out + (int64_t)fr * jb.ld_out + col) = v;
            }
        }
        return;
    }

    const int r = jb.r;
    v2f acc[8][4];
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[k][i] = (v2f){0.f, 0.f};

    for (int jc = 0; jc < r; jc += RC) {
        const int nj = min(RC, r - jc);
        // A chunk [nj][TC]: 16-byte loads, zero outside the matrix (never used: those columns are not stored)
#pragma unroll
        for (int e = 0; e < RC * TC / 4 / 256; ++e) {
            const int idx = e * 256 + tid;
            const int jj = idx / (TC / 4), c4 = (idx % (TC / 4)) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (jj < nj && c0 + c4 < jb.cols)
                v = *reinterpret_cast<const float4*>(jb.A + (int64_t)(jc + jj) * jb.cols + c0 + c4);
            *reinterpret_cast<float4*>(&As[jj][c4]) = v;
        }
        // B chunk [TR][nj], transposed into Bs[jj][row]
#pragma unroll
        for (int e = 0; e < RC * TR / 256; ++e) {
            const int idx = e * 256 + tid;
            const int t = idx / RC, jj = idx % RC;
            const int o = r0 + t;
            float v = 0.f;
            if (jj < nj && o < jb.rows_mod) v = jb.B[(int64_t)o * r + jc + jj];
            Bs[jj][t] = v;
        }
        __syncthreads();
        for (int jj = 0; jj < nj; ++jj) {
            const float4 a0 = *reinterpret_cast<const float4*>(&As[jj][cg * 8]);
            const float4 a1 = *reinterpret_cast<const float4*>(&As[jj][cg * 8 + 4]);
            const float4 b0 = *reinterpret_cast<const float4*>(&Bs[jj][rg * 8]);
            const float4 b1 = *reinterpret_cast<const float4*>(&Bs[jj][rg * 8 + 4]);
            const v2f av[4] = {(v2f){a0.x, a0.y}, (v2f){a0.z, a0.w}, (v2f){a1.x, a1.y}, (v2f){a1.z, a1.w}};
            const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const v2f bb = (v2f){bv[k], bv[k]};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const v2f p = bb * av[i];      // rounded product
                    acc[k][i] = acc[k][i] + p;     // rounded sum (contract off: never an FMA)
                }
            }
        }
        __syncthreads();
    }

    const bool f16 = jb.fmt == WF_F16;
    const v2f eff = (v2f){jb.eff, jb.eff};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int o = r0 + rg * 8 + k;
        if (o >= jb.rows_mod || !col_ok) continue;
        const int fr = lora_fused_row(jb.map, jb.row_off, jb.half, o);
        if (fr < jb.row0 || fr >= row_end) continue;
        const uint4 w = *reinterpret_cast<const uint4*>(jb.base + (int64_t)fr * jb.ld_base + col);
        const uint32_t wi[4] = {w.x, w.y, w.z, w.w};
        uint32_t oi[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const v2f t = eff * acc[k][i];
            const v2f base = (v2f){f16_to_f32(f16, (uint16_t)(wi[i] & 0xffffu)), f16_to_f32(f16, (uint16_t)(wi[i] >> 16))};
            const v2f s = base + t;
            oi[i] = (uint32_t)f32_to_16(f16, s.x) | ((uint32_t)f32_to_16(f16, s.y) << 16);
        }
        *reinterpret_cast<uint4*>(jb.out + (int64_t)fr * jb.ld_out + col) = make_uint4(oi[0], oi[1], oi[2], oi[3]);
    }
}

}  // namespace

void launch_lora_merge(const LoraMergeJob* jobs, int n, hipStream_t s) {
    ACEMI_CHECK(n >= 0 && (n == 0 || jobs), "lora_merge: bad job list");
    for (int j0 = 0; j0 < n; j0 += 8) {
        LoraBatch b{};
        int tot = 0;
        b.n = std::min(8, n - j0);
        for (int i = 0; i < b.n; ++i) {
            const LoraMergeJob& jb = jobs[j0 + i];
            ACEMI_CHECK((jb.fmt == WF_BF16 || jb.fmt == WF_F16) && jb.base && jb.out, "lora_merge: dense 16-bit matrices");
            ACEMI_CHECK(jb.rows > 0 && jb.row0 >= 0 && jb.cols > 0 && jb.cols % 8 == 0 && jb.ld_base % 8 == 0 &&
                            jb.ld_out % 8 == 0 && jb.ld_base >= jb.cols && jb.ld_out >= jb.cols,
                        "lora_merge: cols and leading dimensions must be multiples of 8");
            ACEMI_CHECK(((uintptr_t)jb.base | (uintptr_t)jb.out | (uintptr_t)jb.A) % 16 == 0,
                        "lora_merge: 16-byte aligned base / out / A");
            ACEMI_CHECK(jb.r >= 0 && jb.r <= LORA_MAX_RANK && (jb.r == 0 || (jb.A && jb.B && jb.rows_mod > 0)),
                        "lora_merge: rank must be 0..128 with A and B");
            ACEMI_CHECK(jb.map == LORA_ROWS_PLAIN || (jb.map == LORA_ROWS_INTERLEAVE && (jb.half == 0 || jb.half == 1)),
                        "lora_merge: bad row map");
            const int col_tiles = (jb.cols + TC - 1) / TC;
            b.job[i] = jb;
            b.mod_tiles[i] = jb.r > 0 ? (jb.rows_mod + TR - 1) / TR * col_tiles : 0;
            const bool copies = jb.copy_rest && jb.base != jb.out;  // in place: the copy-through rows are there already
            tot += b.mod_tiles[i] + (copies ? (jb.rows + TR - 1) / TR * col_tiles : 0);
            b.end[i] = tot;
        }
        if (tot == 0) continue;
        hipLaunchKernelGGL(lora_merge_kernel, dim3((unsigned)tot), dim3(256), 0, s, b);
        ACEMI_HIP(hipGetLastError());
    }
}

}  // namespace acemi
