// LoRA merge (gfx950): the adapted 16-bit image of a weight matrix, out = rne16(f32(base) + eff * (B . A)), with the
// fixed arithmetic of kernels.h (LoraMergeJob): a rank-ordered chain of separately rounded f32 multiplies and adds,
// so every build of it (this kernel, the host loops of kernels/merge_host.h, numpy) gives the same bits.
//
// One workgroup merges a tile of 64 module rows x 256 columns: the A slice [r][256] and the B slice [64][r] pass
// through LDS in chunks of 32 ranks, each thread keeps 8 rows x 8 columns of f32 accumulators (two-wide packed
// multiplies and adds), reads its 8 base values per row with one 16-byte load and writes the 8 results with one
// 16-byte store.  2 B read + 2 B written per weight plus the (cached) A / B slices; the VALU chain is 2 r operations
// per weight, which bounds the kernel from r ~ 32 up (DESIGN.md "LoRA adapters").  Copy-through rows of a fused
// matrix (a module without an adapter) are moved by tiles of the same shape that only load and store; the batch, the
// tile walk and that tile are merge_common.h's.
#include <algorithm>

#include "merge_common.h"

// the chain is never contracted into FMAs (the kernel files build with -ffp-contract=fast-honor-pragmas)
#pragma clang fp contract(off)

namespace acemi {
namespace {

constexpr int RPT = 8;    // rows per thread
constexpr int TR = 8 * RPT;
constexpr int TC = MERGE_TC;
constexpr int RC = 32;    // ranks per LDS chunk
constexpr int BPAD = 4;   // padding of a Bs row (keeps 16-byte alignment)

typedef float v2f __attribute__((ext_vector_type(2)));

using LoraBatch = MergeBatch<RPT, LoraMergeJob>;  // (a job without a module has rows_mod = 0 here)

__global__ void __launch_bounds__(256) lora_merge_kernel(LoraBatch b) {
    __shared__ __attribute__((aligned(16))) float As[RC][TC];
    __shared__ __attribute__((aligned(16))) float Bs[RC][TR + BPAD];

    const MergeTile mt = merge_tile(b, (int)blockIdx.x);
    // by value: the job's fields are fetched from the kernel argument once, here, instead of again inside every row's
    // branch of the epilogue (the compiler does not hoist a scalar load out of a conditional block)
    const LoraMergeJob jb = b.job[mt.ji];
    const MergeTarget& tg = jb.t;
    const int c0 = mt.c0, r0 = mt.r0;

    const int tid = threadIdx.x;
    const int cg = tid & 31, rg = tid >> 5;
    const int col = c0 + cg * 8;
    const bool col_ok = col < tg.cols;  // cols % 8 == 0: a thread's 8 columns are all inside or all outside
    const int row_end = tg.row0 + tg.rows;

    if (mt.copy_tile) return merge_copy_tile<RPT>(tg, jb.rows_mod, r0, rg, col);

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
            if (jj < nj && c0 + c4 < tg.cols)
                v = *reinterpret_cast<const float4*>(jb.A + (int64_t)(jc + jj) * tg.cols + c0 + c4);
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

    const bool f16 = tg.fmt == WF_F16;
    const v2f eff = (v2f){jb.eff, jb.eff};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int o = r0 + rg * 8 + k;
        if (o >= jb.rows_mod || !col_ok) continue;
        const int fr = merge_fused_row(tg, o);
        if (fr < tg.row0 || fr >= row_end) continue;
        const uint4 w = *reinterpret_cast<const uint4*>(tg.base + (int64_t)fr * tg.ld_base + col);
        const uint32_t wi[4] = {w.x, w.y, w.z, w.w};
        uint32_t oi[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const v2f t = eff * acc[k][i];
            const v2f base = (v2f){f16_to_f32(f16, (uint16_t)(wi[i] & 0xffffu)), f16_to_f32(f16, (uint16_t)(wi[i] >> 16))};
            const v2f s = base + t;
            oi[i] = (uint32_t)f32_to_16(f16, s.x) | ((uint32_t)f32_to_16(f16, s.y) << 16);
        }
        *reinterpret_cast<uint4*>(tg.out + (int64_t)fr * tg.ld_out + col) = make_uint4(oi[0], oi[1], oi[2], oi[3]);
    }
}

}  // namespace

void launch_lora_merge(const LoraMergeJob* jobs, int n, hipStream_t s) {
    ACEMI_CHECK(n >= 0 && (n == 0 || jobs), "lora_merge: bad job list");
    for (int j0 = 0; j0 < n; j0 += 8) {
        LoraBatch b{};
        int tot = 0;
        const int nb = std::min(8, n - j0);
        for (int i = 0; i < nb; ++i) {
            LoraMergeJob& jb = b.job[i] = jobs[j0 + i];
            check_merge_target(jb.t, "lora_merge");
            ACEMI_CHECK((uintptr_t)jb.A % 16 == 0, "lora_merge: 16-byte aligned base / out / A");
            ACEMI_CHECK(jb.r >= 0 && jb.r <= LORA_MAX_RANK && (jb.r == 0 || (jb.A && jb.B && jb.rows_mod > 0)),
                        "lora_merge: rank must be 0..128 with A and B");
            if (jb.r == 0) jb.rows_mod = 0;
            tot = b.add(jb.rows_mod);
        }
        if (tot == 0) continue;
        hipLaunchKernelGGL(lora_merge_kernel, dim3((unsigned)tot), dim3(256), 0, s, b);
        ACEMI_HIP(hipGetLastError());
    }
}

}  // namespace acemi
