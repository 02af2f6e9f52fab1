// Teacher-forced scoring of the 5 Hz LM (runtime/lm.cpp, ace_mi_lm_score): the head product X [M][H] . W [V][H]^T with
// a reduction over the vocabulary for an epilogue, so that the [M][V] logits never leave the accumulators.  Per row m
// with target t:  logprob = l_t - logsumexp_j l_j  and  rank = #{ j != t : l_j > l_t or (l_j == l_t and j < t) }.
//
//   tile     64 rows x 128 vocabulary columns, k in steps of 64; 256 threads = 2 x 2 waves, each 32 rows x 64 columns
//            (2 x 4 accumulators of v_mfma_f32_16x16x32_{bf16,f16}).
//   LDS      two stages of (64 + 128) rows x 128 bytes, filled by LDS-DMA (1 KiB per wave instruction) with gemm.hip's
//            chunk swizzle on the source address and read back with ds_read_b128; the next (tile, k) step is in flight
//            while the current one multiplies, across tile boundaries too.  H % 64 == 32: the last step stages its
//            first half twice (never past a row's end) and issues half of its MFMAs.
//   lane     after a tile's last k step a lane holds 8 rows x 4 columns; the 16 lanes with the same lane >> 4 hold one
//            row's 64 columns.  Per row the lane keeps (max, sum of exp(l - max), count): the tile's maximum is reduced
//            over those 16 lanes (4 DPP steps), the sum is rescaled to the new maximum, the tile's exp sum and count
//            are reduced the same way and added.  Columns >= V read as -inf and never count.
//   splits   workgroup (row block, split) sweeps a contiguous run of tiles; each of its waves leaves one triple per
//            row (two column halves per split), and lm_score_merge -- one wave per row -- folds the 2 x splits triples:
//            the maximum first, then lane l adds triples l, l + 64, ... in that order and a butterfly adds the lanes.
//            No atomics; every sum has one fixed order.
//   l_t      lm_score_target runs the same loop once per row block over the gathered rows W[t(m)] and keeps the
//            diagonal: the same MFMA sequence over k as the sweep's column t, so the sweep's l_j == l_t holds for j = t
//            and for every head row with t's bytes (the tie rule then orders them by index).
#include <hip/hip_runtime.h>

#include "gemm_common.h"

namespace acemi {

namespace {

using namespace gemm_detail;

constexpr int BM = LM_SCORE_BM, BN = LM_SCORE_BN, BK = 64, ROWB = BK * 2;
constexpr int STAGE = (BM + BN) * ROWB;  // 24 KiB
constexpr int TM = 2, TN = 4;            // 16 x 16 accumulators per wave: 32 rows x 64 columns
constexpr int PIECES = (BM + BN) / 8 / 4;  // LDS-DMA pieces per wave and stage: 2 of X, 4 of W

struct ScoreParams {
    LmScoreArgs a;
    int splits;
    float* lt;    // [M]
    float* pmax;  // [M][2 * splits]
    float* psum;
    int32_t* pcnt;
};

__device__ __forceinline__ int target_of(const LmScoreArgs& a, int m) {
    const int t = a.target[(int64_t)(m / a.t_group) * a.t_stride + m % a.t_group];
    return min(max(t, 0), a.V - 1);
}

// all-reduce over the 16 lanes of a DPP row: quad swaps, then the two mirrors (each step pairs groups that already
// agree, so every lane ends with the same bits)
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false);
}
constexpr int DPP_X1 = 0xB1, DPP_X2 = 0x4E, DPP_HALF_MIRROR = 0x141, DPP_MIRROR = 0x140;
__device__ __forceinline__ float row_max(float v) {
    v = fmaxf(v, dpp_f<DPP_X1>(v));
    v = fmaxf(v, dpp_f<DPP_X2>(v));
    v = fmaxf(v, dpp_f<DPP_HALF_MIRROR>(v));
    return fmaxf(v, dpp_f<DPP_MIRROR>(v));
}
__device__ __forceinline__ float row_sum(float v) {
    v += dpp_f<DPP_X1>(v);
    v += dpp_f<DPP_X2>(v);
    v += dpp_f<DPP_HALF_MIRROR>(v);
    return v + dpp_f<DPP_MIRROR>(v);
}
__device__ __forceinline__ int row_sum(int v) {
    v += dpp_i<DPP_X1>(v);
    v += dpp_i<DPP_X2>(v);
    v += dpp_i<DPP_HALF_MIRROR>(v);
    return v + dpp_i<DPP_MIRROR>(v);
}

// The tile loop shared by both kernels: for tile = 0 .. n_tiles - 1 the 64 x 128 product of X rows m0.. with the 128
// head rows wrow(tile, c), then epi(tile, acc).  One flat loop over (tile, k step) with the next step's LDS-DMA issued
// before the current step's MFMAs.
template <bool F16, class RowW, class Epi>
__device__ __forceinline__ void score_loop(const LmScoreArgs& p, int m0, int n_tiles, char* smem, RowW wrow, Epi epi) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm0 = (wid >> 1) * 32, wn0 = (wid & 1) * 64;
    const int H = p.H, nk = (H + BK - 1) / BK;
    const bool half_tail = (H & 63) != 0;
    const int total = n_tiles * nk;
    if (total <= 0) return;

    // a lane's staging row of piece j is g * 8 + (lane >> 3), g = wid + 4 j; it fills chunk (lane & 7) of that LDS row
    // with source chunk (lane & 7) ^ swz(row)
    const uint16_t* xsrc[2];
    int koff[PIECES];
#pragma unroll
    for (int j = 0; j < PIECES; ++j) {
        const int row = (wid + 4 * j) * 8 + (lane >> 3);
        koff[j] = ((lane & 7) ^ swz(row)) * 8;
        if (j < 2) xsrc[j] = p.x + (int64_t)min(m0 + row, p.M - 1) * p.ldx;
    }
    const uint16_t* wsrc[PIECES - 2];
    auto tile_rows = [&](int tile) {
#pragma unroll
        for (int j = 2; j < PIECES; ++j)
            wsrc[j - 2] = p.w + (int64_t)wrow(tile, (wid + 4 * j) * 8 + (lane >> 3) - BM) * p.ldw;
    };
    int s_tile = 0, s_kt = 0;  // the (tile, k step) the next stage() call requests
    auto stage = [&](int buf) {
        if (s_kt == 0) tile_rows(s_tile);
        char* base = smem + buf * STAGE;
#pragma unroll
        for (int j = 0; j < PIECES; ++j) {
            int k = s_kt * BK + koff[j];
            if (k >= H) k -= 32;  // the half step of H % 64 == 32: its first half again, inside the row
            const uint16_t* src = (j < 2 ? xsrc[j] : wsrc[j - 2]) + k;
            __builtin_amdgcn_global_load_lds((const void*)src, (lds_void*)(base + (wid + 4 * j) * 1024), 16, 0, 0);
        }
        if (++s_kt == nk) s_kt = 0, ++s_tile;
    };

    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
    const int lrow = lane & 15, lchunk = lane >> 4;
    f32x4 acc[TM][TN];
    stage(0);
    wait_vmcnt<0>();
    __syncthreads();
    int tile = 0, kt = 0;
    for (int it = 0; it < total; ++it) {
        const int cur = it & 1;
        if (it + 1 < total) stage(cur ^ 1);
        uint4 a[TM][2], b[TN][2];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int ch = (kk * 4 + lchunk) ^ ((lrow >> 1) & 7);
            const uint32_t ab = lds0 + cur * STAGE + (wm0 + lrow) * ROWB + ch * 16;
            const uint32_t bb = lds0 + cur * STAGE + (BM + wn0 + lrow) * ROWB + ch * 16;
            ReadRows<0, TN, 16 * ROWB>::run(bb, b, kk);
            ReadRows<0, TM, 16 * ROWB>::run(ab, a, kk);
        }
        lds_wait_all();
        if (kt == 0) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = mfma16<F16>(a[i][0], b[j][0], acc[i][j]);
        if (!(half_tail && kt == nk - 1)) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = mfma16<F16>(a[i][1], b[j][1], acc[i][j]);
        }
        mfma_war_retire(a, b);
        if (kt == nk - 1) epi(tile, acc);
        if (++kt == nk) kt = 0, ++tile;
        wait_vmcnt<0>();
        __syncthreads();
    }
}

// l_t of the block's 64 rows: head row of tile column c is W[t(m0 + c % 64)], the value kept is the diagonal
template <bool F16>
__global__ void __launch_bounds__(256, 2) lm_score_target(ScoreParams p) {
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
    const LmScoreArgs& a = p.a;
    const int m0 = blockIdx.x * BM;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wm = wid >> 1, crow = (lane >> 4) * 4, ccol = lane & 15;
    score_loop<F16>(
        a, m0, 1, smem, [&](int, int c) { return target_of(a, min(m0 + (c & (BM - 1)), a.M - 1)); },
        [&](int, f32x4(&acc)[TM][TN]) {
            if (wid & 1) return;  // columns 64 .. 127 repeat 0 .. 63
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const f32x4 d = wm ? acc[i][2 + i] : acc[i][i];  // block row wm * 32 + i * 16 + .. sits in column group wm * 2 + i
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int m = m0 + wm * 32 + i * 16 + crow + r;
                    if (ccol == crow + r && m < a.M) p.lt[m] = d[r];
                }
            }
        });
}

template <bool F16>
__global__ void __launch_bounds__(256, 2) lm_score_sweep(ScoreParams p) {
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
    const LmScoreArgs& a = p.a;
    const int mblocks = (a.M + BM - 1) / BM;
    const int mb = blockIdx.x % mblocks, split = blockIdx.x / mblocks;  // the row blocks of one split are neighbours
    const int m0 = mb * BM;
    const int tiles = (a.V + BN - 1) / BN;
    const int t_begin = (int)((int64_t)split * tiles / p.splits), t_end = (int)((int64_t)(split + 1) * tiles / p.splits);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wm0 = (wid >> 1) * 32, wn0 = (wid & 1) * 64, crow = (lane >> 4) * 4, ccol = lane & 15;
    const float NEG_INF = -__builtin_inff();

    float lt[8], mx[8], sm[8];
    int tg[8], cnt[8];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = min(m0 + wm0 + i * 16 + crow + r, a.M - 1);
            lt[i * 4 + r] = p.lt[m];
            tg[i * 4 + r] = target_of(a, m);
            mx[i * 4 + r] = NEG_INF;
            sm[i * 4 + r] = 0.f;
            cnt[i * 4 + r] = 0;
        }

    score_loop<F16>(
        a, m0, t_end - t_begin, smem, [&](int tile, int c) { return min((t_begin + tile) * BN + c, a.V - 1); },
        [&](int tile, f32x4(&acc)[TM][TN]) {
            const int n0 = (t_begin + tile) * BN + wn0 + ccol;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ri = i * 4 + r;
                    float v[TN];
                    float tmax = NEG_INF;
                    int c = 0;
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        const int n = n0 + j * 16;
                        const bool valid = n < a.V;
                        v[j] = valid ? acc[i][j][r] : NEG_INF;
                        tmax = fmaxf(tmax, v[j]);
                        c += (valid && n != tg[ri] && (v[j] > lt[ri] || (v[j] == lt[ri] && n < tg[ri]))) ? 1 : 0;
                    }
                    tmax = row_max(tmax);
                    const float mnew = fmaxf(mx[ri], tmax);
                    const float mref = mnew == NEG_INF ? 0.f : mnew;  // a wave whose columns so far are all >= V
                    float e = 0.f;
#pragma unroll
                    for (int j = 0; j < TN; ++j) e += expf(v[j] - mref);
                    sm[ri] = sm[ri] * expf(mx[ri] - mref) + row_sum(e);
                    mx[ri] = mnew;
                    cnt[ri] += row_sum(c);
                }
        });

    if (ccol != 0) return;
    const int P = 2 * p.splits;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + wm0 + i * 16 + crow + r;
            if (m >= a.M) continue;
            const int64_t at = (int64_t)m * P + split * 2 + (wid & 1);
            p.pmax[at] = mx[i * 4 + r];
            p.psum[at] = sm[i * 4 + r];
            p.pcnt[at] = cnt[i * 4 + r];
        }
}

// one wave per row: the 2 x splits triples in the order described in the header
__global__ void __launch_bounds__(64) lm_score_merge(ScoreParams p) {
    const int m = blockIdx.x, lane = threadIdx.x, P = 2 * p.splits;
    const float* pm = p.pmax + (int64_t)m * P;
    const float* ps = p.psum + (int64_t)m * P;
    const int32_t* pc = p.pcnt + (int64_t)m * P;
    float mx = -__builtin_inff();
    for (int q = lane; q < P; q += 64) mx = fmaxf(mx, pm[q]);
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    float s = 0.f;
    int c = 0;
    for (int q = lane; q < P; q += 64) {
        if (ps[q] > 0.f) s += ps[q] * expf(pm[q] - mx);  // an empty triple is (-inf, 0, 0)
        c += pc[q];
    }
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_xor(s, off);
        c += __shfl_xor(c, off);
    }
    if (lane == 0) {
        p.a.logprob[m] = p.lt[m] - (mx + logf(s));
        p.a.rank[m] = c;
    }
}

template <bool F16>
void launch(const ScoreParams& p, hipStream_t s) {
    const int mblocks = (p.a.M + BM - 1) / BM;
    hipLaunchKernelGGL(lm_score_target<F16>, dim3(mblocks), dim3(256), 0, s, p);
    hipLaunchKernelGGL(lm_score_sweep<F16>, dim3(mblocks * p.splits), dim3(256), 0, s, p);
    hipLaunchKernelGGL(lm_score_merge, dim3(p.a.M), dim3(64), 0, s, p);
}

}  // namespace

int lm_score_chain(int H) { return 31 + (H + 31) / 32; }

void launch_lm_score(ActType act, const LmScoreArgs& a, hipStream_t s) {
    lm_score_check(a);
    ScoreParams p;
    p.a = a;
    p.splits = lm_score_splits(a.M, a.V, a.splits);
    const size_t n = (size_t)a.M * 2 * p.splits;
    p.lt = a.work;
    p.pmax = a.work + a.M;
    p.psum = p.pmax + n;
    p.pcnt = reinterpret_cast<int32_t*>(p.psum + n);
    if (act == ActType::F16)
        launch<true>(p, s);
    else
        launch<false>(p, s);
    ACEMI_HIP(hipGetLastError());
}

}  // namespace acemi
