// LoKr merge (gfx950): the adapted 16-bit image of a weight matrix under a LyCORIS Kronecker adapter,
// out[i*c + k][j*d + l] = rne16(f32(base) + eff * (w1[i][j] * W2[k][l])), with the fixed arithmetic of kernels.h
// (LokrMergeJob): every multiply and add rounded to f32 on its own, low-rank factors as rank-ordered chains, so every
// build of it (these kernels, the host loops of kernels/merge_host.h, numpy) gives the same bits.
//
// Two kernels per batch of up to 8 jobs:
//   lokr_factor_kernel  forms the factors that are stored as products (W2 = w2a . w2b, w1 = w1a . w1b) once per job
//       into the job's f32 workspace.  A tile of 16 x 64 entries per workgroup, the operand slices pass through LDS in
//       chunks of 32 ranks, four entries per thread.  The matrices are a few hundred entries a side and the chain is
//       fixed-order f32, so MFMA does not fit (its accumulation order and input formats are not this chain's); the
//       cost is nothing beside the merge, which reuses each W2 entry a*b (~1000) times.
//   lokr_merge_kernel   is the bandwidth-bound one: 2 B read + 2 B written per weight.  One workgroup owns 32 module
//       rows x 256 columns.  It stages into LDS the W2 rows and columns the tile touches (all c rows when c <= 32, else
//       the tile's own 32; all d columns when d <= 256, else the tile's own 256; rows padded by one word per 8 so that
//       lanes 8 columns apart read different banks: at most 36 KB) and the w1 entries of
//       the (i, j) blocks the tile overlaps.  Each thread then owns 4 rows x 8 consecutive columns: it finds the
//       (i, k) of its first row and the (j, l) of its first column with one division each and steps the rest, so
//       columns that straddle a j boundary (d % 8 != 0) and rows that cross an i boundary index per element; one
//       16-byte load and one 16-byte store per row.  Per element: two LDS reads, two multiplies, one add.
// Copy-through rows of a fused matrix (a module without an adapter) are moved by tiles of the same shape that only
// load and store; the batch, the tile walk and that tile are merge_common.h's.
#include <algorithm>
#include <climits>

#include "merge_common.h"

// the chain is never contracted into FMAs (the kernel files build with -ffp-contract=fast-honor-pragmas)
#pragma clang fp contract(off)

namespace acemi {
namespace {

constexpr int RPT = 4;    // rows per thread (8 row groups x 32 column groups of 8)
constexpr int TR = 8 * RPT;   // module rows per merge tile
constexpr int TC = MERGE_TC;  // columns per merge tile
constexpr int FR = 16;    // rows per factor tile
constexpr int FC = 64;    // columns per factor tile
constexpr int RC = 32;    // ranks per LDS chunk
constexpr int LPAD = 1;   // padding of an Ls row

struct LokrProduct {  // out [m][n] = L [m][r] . R [r][n]
    const float* L;
    const float* R;
    float* out;
    int m, n, r;
};
struct LokrFactorBatch {
    LokrProduct p[16];
    int end[16];  // exclusive prefix sums of tiles
    int n;
};

struct LokrTileJob {  // a LokrMergeJob with its factors resolved to whole matrices
    MergeTarget t;
    const float* w1;  // [a][b]
    const float* W2;  // [c][d]
    int rows_mod;     // a * c; 0: copy-only
    int a, b, c, d;
    float eff;
};
using LokrBatch = MergeBatch<RPT, LokrTileJob>;

__global__ void __launch_bounds__(256) lokr_factor_kernel(LokrFactorBatch b) {
    __shared__ __attribute__((aligned(16))) float Rs[RC][FC];
    __shared__ float Ls[RC][FR + LPAD];

    int pi = 0;
#pragma unroll
    for (int i = 0; i < 15; ++i) pi += (i + 1 < b.n && (int)blockIdx.x >= b.end[i]) ? 1 : 0;
    const LokrProduct& p = b.p[pi];
    const int tile = (int)blockIdx.x - (pi > 0 ? b.end[pi - 1] : 0);
    const int col_tiles = (p.n + FC - 1) / FC;
    const int c0 = (tile % col_tiles) * FC;
    const int r0 = (tile / col_tiles) * FR;
    const int tid = threadIdx.x;
    const int cg = tid & 15, rg = tid >> 4;  // 16 column groups of 4, 16 rows
    const int m = p.m, n = p.n, r = p.r;

    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int jc = 0; jc < r; jc += RC) {
        const int nj = min(RC, r - jc);
        // R chunk [nj][FC] (n need not be a multiple of 4: scalar loads), zero outside the matrix
#pragma unroll
        for (int e = 0; e < RC * FC / 256; ++e) {
            const int idx = e * 256 + tid;
            const int jj = idx / FC, cc = idx % FC;
            float v = 0.f;
            if (jj < nj && c0 + cc < n) v = p.R[(int64_t)(jc + jj) * n + c0 + cc];
            Rs[jj][cc] = v;
        }
        // L chunk [FR][nj], transposed into Ls[jj][row]
#pragma unroll
        for (int e = 0; e < RC * FR / 256; ++e) {
            const int idx = e * 256 + tid;
            const int t = idx / RC, jj = idx % RC;
            float v = 0.f;
            if (jj < nj && r0 + t < m) v = p.L[(int64_t)(r0 + t) * r + jc + jj];
            Ls[jj][t] = v;
        }
        __syncthreads();
        for (int jj = 0; jj < nj; ++jj) {
            const float4 rv = *reinterpret_cast<const float4*>(&Rs[jj][cg * 4]);
            const float l = Ls[jj][rg];
            const float pr[4] = {l * rv.x, l * rv.y, l * rv.z, l * rv.w};  // rounded products
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = acc[i] + pr[i];           // rounded sums (contract off)
        }
        __syncthreads();
    }
    const int o = r0 + rg;
    if (o >= m) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int col = c0 + cg * 4 + i;
        if (col < n) p.out[(int64_t)o * n + col] = acc[i];
    }
}

// LDS floats of a merge tile of a job: the staged W2 block and the largest w1 block a tile can overlap
__host__ __device__ inline int lokr_nk(int c) { return c < TR ? c : TR; }
__host__ __device__ inline int lokr_nl(int d) { return d < TC ? d : TC; }
// position of column slot v in a W2s row: one pad word per 8 slots, so that the lanes of a wave, whose columns are 8
// apart, read 32 different banks
__host__ __device__ inline int lokr_lpos(int v) { return v + (v >> 3); }
__host__ __device__ inline int lokr_row_words(int nl) { return lokr_lpos(nl - 1) + 1; }
inline int lokr_span(int tile, int f, int count) {  // blocks of width f a tile-aligned run of `tile` can overlap
    const int n = tile % f == 0 ? tile / f : (tile - 1) / f + 2;
    return std::min(n, count);
}

__global__ void __launch_bounds__(256) lokr_merge_kernel(LokrBatch b) {
    extern __shared__ __attribute__((aligned(16))) float lds[];

    const MergeTile mt = merge_tile(b, (int)blockIdx.x);
    // by value: the job's fields are fetched from the kernel argument once, here, instead of again inside every row's
    // branch (the compiler does not hoist a scalar load out of a conditional block)
    const LokrTileJob jb = b.job[mt.ji];
    const MergeTarget& tg = jb.t;
    const int c0 = mt.c0, r0 = mt.r0;

    const int tid = threadIdx.x;
    const int cg = tid & 31, rg = tid >> 5;
    const int col = c0 + cg * 8;
    const bool col_ok = col < tg.cols;  // cols % 8 == 0: a thread's 8 columns are all inside or all outside
    const int row_end = tg.row0 + tg.rows;

    if (mt.copy_tile) return merge_copy_tile<RPT>(tg, jb.rows_mod, r0, rg, col);

    const int c = jb.c, d = jb.d;
    const int nk = lokr_nk(c), nl = lokr_nl(d);
    const int rows_in = min(TR, jb.rows_mod - r0), cols_in = min(TC, tg.cols - c0);
    const int i0 = r0 / c, j0 = c0 / d;
    const int ni = (r0 + rows_in - 1) / c - i0 + 1, nj = (c0 + cols_in - 1) / d - j0 + 1;
    const int nlw = lokr_row_words(nl);
    float* W2s = lds;             // [nk][nlw]: slot s holds W2 row s (c <= TR) or the row of tile row s
    float* w1s = lds + nk * nlw;  // [ni][nj]: the blocks (i0 + ., j0 + .)
    for (int idx = tid; idx < nk * nl; idx += 256) {
        const int s = idx / nl, v = idx - s * nl;
        const int k = c <= TR ? s : (r0 + s) % c;
        const int l = d <= TC ? v : (c0 + v) % d;
        W2s[s * nlw + lokr_lpos(v)] = jb.W2[(int64_t)k * d + l];
    }
    for (int idx = tid; idx < ni * nj; idx += 256) {
        const int ii = idx / nj, jj = idx - ii * nj;
        w1s[idx] = jb.w1[(int64_t)(i0 + ii) * jb.b + j0 + jj];
    }
    __syncthreads();
    if (!col_ok) return;

    // this thread's 8 columns: slot of l in a W2s row, slot of j in a w1s row
    int lslot[8], jslot[8];
    {
        int j = col / d, l = col - j * d;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            lslot[e] = lokr_lpos(d <= TC ? l : col + e - c0);
            jslot[e] = j - j0;
            if (++l == d) l = 0, ++j;
        }
    }
    const bool f16 = tg.fmt == WF_F16;
    const float eff = jb.eff;
    int o = r0 + rg * RPT;
    int i = o / c, k = o - i * c;
#pragma unroll
    for (int kk = 0; kk < RPT; ++kk, ++o) {
        if (o >= jb.rows_mod) break;
        const float* w2r = W2s + (c <= TR ? k : o - r0) * nlw;
        const float* w1r = w1s + (i - i0) * nj;
        if (++k == c) k = 0, ++i;
        const int fr = merge_fused_row(tg, o);
        if (fr < tg.row0 || fr >= row_end) continue;
        const uint4 w = *reinterpret_cast<const uint4*>(tg.base + (int64_t)fr * tg.ld_base + col);
        const uint32_t wi[4] = {w.x, w.y, w.z, w.w};
        uint32_t oi[4];
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
            const float v0 = w1r[jslot[e]] * w2r[lslot[e]];          // rounded product
            const float v1 = w1r[jslot[e + 1]] * w2r[lslot[e + 1]];
            const float t0 = eff * v0, t1 = eff * v1;                // rounded scale
            const float s0 = f16_to_f32(f16, (uint16_t)(wi[e / 2] & 0xffffu)) + t0;  // rounded sum (never an FMA)
            const float s1 = f16_to_f32(f16, (uint16_t)(wi[e / 2] >> 16)) + t1;
            oi[e / 2] = (uint32_t)f32_to_16(f16, s0) | ((uint32_t)f32_to_16(f16, s1) << 16);
        }
        *reinterpret_cast<uint4*>(tg.out + (int64_t)fr * tg.ld_out + col) = make_uint4(oi[0], oi[1], oi[2], oi[3]);
    }
}

}  // namespace

void launch_lokr_merge(const LokrMergeJob* jobs, int n, hipStream_t s) {
    ACEMI_CHECK(n >= 0 && (n == 0 || jobs), "lokr_merge: bad job list");
    for (int j0 = 0; j0 < n; j0 += 8) {
        LokrBatch b{};
        LokrFactorBatch fb{};
        int tot = 0, ftot = 0, lds_floats = 0;
        const int nb = std::min(8, n - j0);
        auto product = [&](const float* L, const float* R, float* out, int m, int nn, int r) {
            const int tiles = ((m + FR - 1) / FR) * ((nn + FC - 1) / FC);
            fb.p[fb.n] = LokrProduct{L, R, out, m, nn, r};
            ftot += tiles;
            fb.end[fb.n++] = ftot;
        };
        for (int i = 0; i < nb; ++i) {
            const LokrMergeJob& jb = jobs[j0 + i];
            check_merge_target(jb.t, "lokr_merge");
            LokrTileJob& t = b.job[i];
            t.t = jb.t;
            t.eff = jb.eff;
            if (jb.a > 0) {
                ACEMI_CHECK(jb.b > 0 && jb.c > 0 && jb.d > 0 && (int64_t)jb.b * jb.d == jb.t.cols &&
                                (int64_t)jb.a * jb.c <= INT_MAX / 2,
                            "lokr_merge: kron([a][b], [c][d]) must have the job's columns");
                ACEMI_CHECK(jb.w1 || (jb.w1a && jb.w1b && jb.r1 >= 1 && jb.r1 <= LOKR_MAX_RANK),
                            "lokr_merge: w1, or w1a . w1b of rank 1..1024");
                ACEMI_CHECK(jb.w2 || (jb.w2a && jb.w2b && jb.r2 >= 1 && jb.r2 <= LOKR_MAX_RANK),
                            "lokr_merge: w2, or w2a . w2b of rank 1..1024");
                ACEMI_CHECK(lokr_ws_floats(jb) == 0 || jb.ws, "lokr_merge: a product factor needs the workspace");
                t.a = jb.a, t.b = jb.b, t.c = jb.c, t.d = jb.d;
                t.rows_mod = jb.a * jb.c;
                t.W2 = jb.w2, t.w1 = jb.w1;
                if (!jb.w2) {
                    product(jb.w2a, jb.w2b, jb.ws, jb.c, jb.d, jb.r2);
                    t.W2 = jb.ws;
                }
                if (!jb.w1) {
                    product(jb.w1a, jb.w1b, jb.ws + lokr_ws_w1_offset(jb), jb.a, jb.b, jb.r1);
                    t.w1 = jb.ws + lokr_ws_w1_offset(jb);
                }
                lds_floats = std::max(lds_floats, lokr_nk(jb.c) * lokr_row_words(lokr_nl(jb.d)) +
                                                      lokr_span(TR, jb.c, jb.a) * lokr_span(TC, jb.d, jb.b));
            }
            tot = b.add(t.rows_mod);
        }
        if (tot == 0) continue;
        ACEMI_CHECK(lds_floats * 4 <= 48 * 1024, "lokr_merge: tile LDS");
        if (ftot > 0) {
            hipLaunchKernelGGL(lokr_factor_kernel, dim3((unsigned)ftot), dim3(256), 0, s, fb);
            ACEMI_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(lokr_merge_kernel, dim3((unsigned)tot), dim3(256), (size_t)lds_floats * 4, s, b);
        ACEMI_HIP(hipGetLastError());
    }
}

}  // namespace acemi
