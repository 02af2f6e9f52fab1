// What the adapter merge kernels (lora.hip, lokr.hip) and their host restatements share:
//   the 16-bit <-> f32 conversions: bf16 / fp16 words of a weight image widened exactly, and f32 results rounded to
//       nearest even (a NaN stays a quiet NaN), callable on host and device;
//   the batch of up to 8 jobs one launch takes, with its tile accounting;
//   the walk from a workgroup to its (job, tile) and the copy-through tile.
// A tile is 8 * RPT module rows x 256 columns for 256 threads: 8 row groups of RPT rows, 32 column groups of 8
// columns (one 16-byte access per row).  LoRA uses RPT = 8, LoKr RPT = 4.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../kernels.h"

namespace acemi {

__host__ __device__ inline uint16_t f32_to_bf16_rne(float f) {
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 64u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
__host__ __device__ inline uint16_t f32_to_16(bool f16, float f) {
    if (f16) return __builtin_bit_cast(uint16_t, (_Float16)f);
    return f32_to_bf16_rne(f);
}
__host__ __device__ inline float f16_to_f32(bool f16, uint16_t v) {
    if (f16) return (float)__builtin_bit_cast(_Float16, v);
    return __builtin_bit_cast(float, (uint32_t)v << 16);
}

constexpr int MERGE_TC = 256;  // columns per tile

// One launch: Job is the kernel's own job type and holds its MergeTarget as member t.
template <int RPT, typename Job>
struct MergeBatch {
    static constexpr int TR = 8 * RPT;  // rows per tile
    Job job[8];
    int mod_tiles[8];  // tiles of module rows of job i
    int end[8];        // exclusive prefix sums of (module + copy) tiles
    int n;

    // host: job n's tiles for a module of rows_mod rows (0: none); returns the tiles of the batch so far
    int add(int rows_mod) {
        const MergeTarget& t = job[n].t;
        const int col_tiles = (t.cols + MERGE_TC - 1) / MERGE_TC;
        mod_tiles[n] = (rows_mod + TR - 1) / TR * col_tiles;
        const bool copies = t.copy_rest && t.base != t.out;  // in place: the copy-through rows are there already
        end[n] = (n > 0 ? end[n - 1] : 0) + mod_tiles[n] + (copies ? (t.rows + TR - 1) / TR * col_tiles : 0);
        return end[n++];
    }
};

struct MergeTile {
    int ji;          // job of the batch
    bool copy_tile;  // a copy-through tile (r0 counts rows of the range), else a merge tile (r0 counts module rows)
    int c0, r0;
};

template <int RPT, typename Job>
__device__ inline MergeTile merge_tile(const MergeBatch<RPT, Job>& b, int block) {
    MergeTile m;
    m.ji = 0;
#pragma unroll
    for (int i = 0; i < 7; ++i) m.ji += (i + 1 < b.n && block >= b.end[i]) ? 1 : 0;
    int tile = block - (m.ji > 0 ? b.end[m.ji - 1] : 0);
    const int col_tiles = (b.job[m.ji].t.cols + MERGE_TC - 1) / MERGE_TC;
    m.copy_tile = tile >= b.mod_tiles[m.ji];
    if (m.copy_tile) tile -= b.mod_tiles[m.ji];
    m.c0 = (tile % col_tiles) * MERGE_TC;
    m.r0 = (tile / col_tiles) * (8 * RPT);
    return m;
}

// the copy-through tile: rows of the range that belong to no module row, base -> out (row group rg, 8 columns at col)
template <int RPT>
__device__ inline void merge_copy_tile(const MergeTarget& t, int rows_mod, int r0, int rg, int col) {
    if (col >= t.cols) return;  // cols % 8 == 0: a thread's 8 columns are all inside or all outside
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
        const int fr = t.row0 + r0 + rg * RPT + k;
        if (fr < t.row0 + t.rows && merge_module_row(t, rows_mod, fr) < 0) {
            const uint4 v = *reinterpret_cast<const uint4*>(t.base + (int64_t)fr * t.ld_base + col);
            *reinterpret_cast<uint4*>(t.out + (int64_t)fr * t.ld_out + col) = v;
        }
    }
}

}  // namespace acemi
