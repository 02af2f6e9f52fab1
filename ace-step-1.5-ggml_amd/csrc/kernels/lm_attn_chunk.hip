// Chunk attention of the 5 Hz LM (runtime/lm.cpp, LmEngine::extend): n query tokens per sequence, appended at slots
// past .. past + n - 1 of a filled fp16 KV cache, attend to the cache and to themselves (causal inside the chunk).
// Row (b, t, head) sees the keys j <= past + t with key_mask[b][j] != 0; launch_lm_attention's rules otherwise.
//
//   rows     the rep = hq / hkv query heads of a kv head are stacked token-major along one 32-row tile
//            (row = t * rep + r): 32 tokens at rep 1, 16 at rep 2, 8 at rep 4.  The group shares one read of K and V.
//   grid     (key range of LM_SPLIT_KEYS keys) x (row tile) x (kv head, sequence); 256 threads = 4 waves, wave w owns
//            the keys [64 w, 64 w + 64) of the range, in two blocks of 32.  A block at or past the tile's last causal
//            limit is skipped (never read), a whole range there leaves the record (-inf, 0, 0).
//   products both on v_mfma_f32_16x16x32_f16, transposed so that P never leaves the registers:
//              S^T [key][row] = K . Q^T    A = K from LDS (ds_read_b128), B = Q as an fp16 hi + lo pair (two MFMAs per
//                                          k step), split once from the f32 Q and kept in registers for the kernel;
//              O^T [d][row]   = V^T . P^T  the S^T accumulator of a lane (row c, keys 4 g + r of both 16-key halves) IS
//                                          a B fragment once the MFMA's k slots are numbered (half, g, r): P goes from
//                                          accumulator to operand (fp16 hi + lo) without a shuffle.  A = V^T, keys
//                                          along k: the V block lies key-major in LDS, so a lane gathers its 8 keys of
//                                          one d with eight ds_read_u16 -- the gather was chosen over gfx950's
//                                          ds_read_b64_tr_b16; it costs 4 LDS instructions per MFMA at 2 bytes a lane,
//                                          conflict-free under the swizzle, and stays behind the 64 MFMAs of a block.
//   LDS      per wave one K and one V block (32 keys x 256 bytes each), filled by LDS-DMA (1 KiB = 4 key rows per wave
//            instruction) with the chunk swizzle on the source side: 16-byte chunk c of row r holds source chunk
//            c ^ (r & 15), gemm.hip's scheme widened to a 256-byte row.  Wave-private: no barrier in the key loop.
//   masks    a masked or out-of-range key's score becomes -inf by selection, and its V row is zeroed in LDS before the
//            gather (0 x NaN would poison the MFMA); rows past the tile's limit are staged from the last legal slot.
//   softmax  f32 online (running max and sum per row, replicated over the four lane groups); O is rescaled in place.
//   join     the four waves leave (m, l, O[32][128]) in LDS and are joined in ascending key order; the result is the
//            decode kernel's record (m, l, unnormalised O[128]) per (row, range), merged over the ranges by
//            lm_attn_merge_kernel (launch_lm_attn_merge) in ascending order, or -- one range -- the normalised output.
// No atomics, one fixed order for every sum: two launches give the same bytes.
#include <hip/hip_runtime.h>

#include "gemm_common.h"

namespace acemi {

namespace {

using namespace gemm_detail;

constexpr int CD = 128, TROWS = LM_CHUNK_ROWS, BLK = 32, WAVE_KEYS = LM_SPLIT_KEYS / 4;
constexpr int KV_BYTES = BLK * CD * 2;       // one block of K or of V: 8 KiB
constexpr int O_STRIDE = CD + 4;             // floats per row of a wave's O in LDS (the pad spreads the 16 rows of a store)
constexpr int WREG = TROWS * O_STRIDE * 4;   // a wave's LDS: K block | V block while it runs, its O at the join
static_assert(WREG >= 2 * KV_BYTES && WAVE_KEYS % BLK == 0, "chunk attention: LDS layout");

struct ChunkParams {
    LmAttnChunkArgs a;
    int rep, hq, n_split, f16out;
};

template <int OFF>
__device__ __forceinline__ uint32_t ds_read_u16_off(uint32_t addr) {
    uint32_t v;
    asm volatile("ds_read_u16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(OFF));
    return v;
}

__device__ __forceinline__ uint32_t f16_word(float a, float b) {
    return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)a) | ((uint32_t)__builtin_bit_cast(uint16_t, (_Float16)b) << 16);
}
__device__ __forceinline__ float f16_rest(float a) { return a - (float)(_Float16)a; }
// eight f32 -> their fp16 roundings and the fp16 roundings of what those leave
__device__ __forceinline__ void split8(const float (&x)[8], uint4& hi, uint4& lo) {
    hi = make_uint4(f16_word(x[0], x[1]), f16_word(x[2], x[3]), f16_word(x[4], x[5]), f16_word(x[6], x[7]));
    lo = make_uint4(f16_word(f16_rest(x[0]), f16_rest(x[1])), f16_word(f16_rest(x[2]), f16_rest(x[3])),
                    f16_word(f16_rest(x[4]), f16_rest(x[5])), f16_word(f16_rest(x[6]), f16_rest(x[7])));
}

__global__ void __launch_bounds__(256, 2) lm_attn_chunk_kernel(ChunkParams p) {
    __shared__ __attribute__((aligned(16))) char smem[4 * WREG];
    __shared__ float st_m[4][TROWS], st_l[4][TROWS];
    const LmAttnChunkArgs& a = p.a;
    const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int sp = blockIdx.x, tile = blockIdx.y, h = blockIdx.z % a.hkv, b = blockIdx.z / a.hkv;
    const int rep = p.rep, hq = p.hq, n = a.n;
    const float NEG_INF = -__builtin_inff();
    // the keys any row of the tile may see: [0, nk_tile)
    const int nk_tile = a.past + min(n - 1, (tile * TROWS + TROWS - 1) / rep) + 1;

    // Q^T fragments: lane (c, g) holds row qg * 16 + c, d = ks * 32 + g * 8 .. + 7
    uint4 qh[2][4], ql[2][4];
    int limit[2];
#pragma unroll
    for (int qg = 0; qg < 2; ++qg) {
        const int R = tile * TROWS + qg * 16 + c;
        const int t = min(R / rep, n - 1);  // a row past the chunk recomputes the last token and writes nothing
        limit[qg] = a.past + t;
        const float* qp = a.q + (((int64_t)b * n + t) * hq + h * rep + R % rep) * CD + g * 8;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const float4 x = *(const float4*)(qp + ks * 32), y = *(const float4*)(qp + ks * 32 + 4);
            const float f[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
            split8(f, qh[qg][ks], ql[qg][ks]);
        }
    }

    const int64_t kv0 = ((int64_t)b * a.hkv + h) * a.capacity;
    const int32_t* km = a.key_mask + (int64_t)b * a.capacity;
    char* wbase = smem + wid * WREG;
    const uint32_t kl = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)wbase, vl = kl + KV_BYTES;
    // V gather: row 4 g + jj of a half, chunk (2 dt + (c >> 3)) ^ (4 g + jj) = ((2 dt) ^ jj) ^ vx, 2-byte word c & 7
    const uint32_t vlane = vl + g * 1024 + (c & 7) * 2;
    const int vx = (g * 4) ^ (c >> 3);

    f32x4 o[8][2];
    float m[2] = {NEG_INF, NEG_INF}, l[2] = {0.f, 0.f};
#pragma unroll
    for (int dt = 0; dt < 8; ++dt)
#pragma unroll
        for (int qg = 0; qg < 2; ++qg) o[dt][qg] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int blk = 0; blk < WAVE_KEYS / BLK; ++blk) {
        const int kb = sp * LM_SPLIT_KEYS + wid * WAVE_KEYS + blk * BLK;
        if (kb >= nk_tile) break;  // wave-uniform
        // stage K and V: instruction i brings rows 4 i + g, this lane LDS chunk c = source chunk c ^ (row & 15)
#pragma unroll
        for (int i = 0; i < BLK / 4; ++i) {
            const int row = i * 4 + g;
            const int64_t src = (kv0 + min(kb + row, nk_tile - 1)) * CD + ((c ^ (row & 15)) << 3);
            __builtin_amdgcn_global_load_lds((const void*)(a.k_cache + src), (lds_void*)(wbase + i * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const void*)(a.v_cache + src), (lds_void*)(wbase + KV_BYTES + i * 1024), 16, 0,
                                             0);
        }
        // the lane's eight keys, slot j = (half, r): key kb + 16 half + 4 g + r -- its S^T rows and its P.V k slots
        int kmv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) kmv[j] = km[min(kb + (j >> 2) * 16 + g * 4 + (j & 3), nk_tile - 1)];
        bool on[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) on[j] = (kb + (j >> 2) * 16 + g * 4 + (j & 3) < nk_tile) & (kmv[j] != 0);
        wait_vmcnt<0>();
        __builtin_amdgcn_sched_barrier(0);
        // a key that is masked or past the tile contributes 0 x V: its V row must hold no NaN
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (!on[j]) *(uint4*)(wbase + KV_BYTES + ((j >> 2) * 16 + g * 4 + (j & 3)) * 256 + c * 16) = make_uint4(0, 0, 0, 0);
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);

        // S^T = K . Q^T: 2 halves of 16 keys x 2 row groups, 4 k steps of 32, hi then lo
        f32x4 s[2][2];
        {
            uint4 kf[2][4];
#pragma unroll
            for (int half = 0; half < 2; ++half)
#pragma unroll
                for (int ks = 0; ks < 4; ++ks)
                    kf[half][ks] = ds_read_b128_off<0>(kl + (half * 16 + c) * 256 + (((ks * 4 + g) ^ c) << 4));
            lds_wait_all();
#pragma unroll
            for (int qg = 0; qg < 2; ++qg)
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks) {
                        acc = mfma16<true>(kf[half][ks], qh[qg][ks], acc);
                        acc = mfma16<true>(kf[half][ks], ql[qg][ks], acc);
                    }
                    s[qg][half] = acc;
                }
            mfma_war_retire(kf, qh, ql);
        }

        // online softmax per row (the row's 32 keys of this block lie in the four lanes c, c + 16, c + 32, c + 48)
        uint4 ph[2], pl[2];
#pragma unroll
        for (int qg = 0; qg < 2; ++qg) {
            float sv[8];
            float bm = NEG_INF;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int key = kb + (j >> 2) * 16 + g * 4 + (j & 3);
                sv[j] = (on[j] && key <= limit[qg]) ? s[qg][j >> 2][j & 3] * a.scale : NEG_INF;
                bm = fmaxf(bm, sv[j]);
            }
            bm = fmaxf(bm, __shfl_xor(bm, 16));
            bm = fmaxf(bm, __shfl_xor(bm, 32));
            const float mn = fmaxf(m[qg], bm);
            const float alpha = m[qg] == NEG_INF ? 0.f : expf(m[qg] - mn);
            float pv[8], sum = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                pv[j] = sv[j] == NEG_INF ? 0.f : expf(sv[j] - mn);
                sum += pv[j];
            }
            l[qg] = l[qg] * alpha + sum;  // this lane's keys only; the four lanes of a row are added at the join
            m[qg] = mn;
#pragma unroll
            for (int dt = 0; dt < 8; ++dt) o[dt][qg] *= alpha;
            split8(pv, ph[qg], pl[qg]);
        }

        // O^T += V^T . P^T, four d tiles of 16 at a time
#pragma unroll
        for (int d0 = 0; d0 < 8; d0 += 4) {
            uint32_t w[4][8];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const uint32_t ad = vlane + (((((d0 + i) * 2) ^ jj) ^ vx) << 4);
                    if (jj == 0) {
                        w[i][0] = ds_read_u16_off<0>(ad);
                        w[i][4] = ds_read_u16_off<4096>(ad);
                    } else if (jj == 1) {
                        w[i][1] = ds_read_u16_off<256>(ad);
                        w[i][5] = ds_read_u16_off<4096 + 256>(ad);
                    } else if (jj == 2) {
                        w[i][2] = ds_read_u16_off<512>(ad);
                        w[i][6] = ds_read_u16_off<4096 + 512>(ad);
                    } else {
                        w[i][3] = ds_read_u16_off<768>(ad);
                        w[i][7] = ds_read_u16_off<4096 + 768>(ad);
                    }
                }
            lds_wait_all();
            uint4 vf[4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
                vf[i] = make_uint4(w[i][0] | (w[i][1] << 16), w[i][2] | (w[i][3] << 16), w[i][4] | (w[i][5] << 16),
                                   w[i][6] | (w[i][7] << 16));
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int qg = 0; qg < 2; ++qg) {
                    o[d0 + i][qg] = mfma16<true>(vf[i], ph[qg], o[d0 + i][qg]);
                    o[d0 + i][qg] = mfma16<true>(vf[i], pl[qg], o[d0 + i][qg]);
                }
            mfma_war_retire(vf, ph, pl);
        }
    }

    // the wave's record into its own LDS (its last reads have returned): O[row][d], lane (c, g) holds d = 16 dt + 4 g + r
#pragma unroll
    for (int qg = 0; qg < 2; ++qg) {
        float lr = l[qg];
        lr += __shfl_xor(lr, 16);
        lr += __shfl_xor(lr, 32);
        if (g == 0) {
            st_m[wid][qg * 16 + c] = m[qg];
            st_l[wid][qg * 16 + c] = lr;
        }
#pragma unroll
        for (int dt = 0; dt < 8; ++dt)
            *(float4*)(wbase + ((qg * 16 + c) * O_STRIDE + dt * 16 + g * 4) * 4) =
                make_float4(o[dt][qg][0], o[dt][qg][1], o[dt][qg][2], o[dt][qg][3]);
    }
    __syncthreads();

    // join the waves in ascending key order: thread (row, 16 d)
    const int row = tid >> 3, dd = (tid & 7) * 16;
    const int R = tile * TROWS + row, t = R / rep;
    if (t >= n) return;
    float M = NEG_INF;
#pragma unroll
    for (int w = 0; w < 4; ++w) M = fmaxf(M, st_m[w][row]);
    float L = 0.f, O[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) O[i] = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const float wt = st_m[w][row] == NEG_INF ? 0.f : expf(st_m[w][row] - M);
        L = fmaf(st_l[w][row], wt, L);
        const float* ow = (const float*)(smem + w * WREG) + row * O_STRIDE + dd;
#pragma unroll
        for (int i = 0; i < 16; ++i) O[i] = fmaf(ow[i], wt, O[i]);
    }
    const int64_t orow = ((int64_t)b * n + t) * hq + h * rep + R % rep;
    if (p.n_split == 1) {
        uint16_t* dst = a.out + orow * CD + dd;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float v = L > 0.f ? O[i] / L : 0.f;
            dst[i] = p.f16out ? to_act<true>(v) : to_act<false>(v);
        }
    } else {
        float* part = a.part + (orow * p.n_split + sp) * (CD + 2);
#pragma unroll
        for (int i = 0; i < 16; ++i) part[2 + dd + i] = O[i];
        if (dd == 0) {
            part[0] = M;
            part[1] = L;
        }
    }
}

}  // namespace

size_t lm_attn_chunk_part_floats(int B, int n, int hq, int nk) {
    return (size_t)B * n * hq * ceil_div(nk, LM_SPLIT_KEYS) * (CD + 2);
}

void launch_lm_attention_chunk(ActType out_t, const LmAttnChunkArgs& a, int B, int hq, hipStream_t s) {
    const int rep = lm_attn_chunk_check(a, B, hq);
    ChunkParams p;
    p.a = a;
    p.rep = rep;
    p.hq = hq;
    p.n_split = (int)ceil_div(a.past + a.n, LM_SPLIT_KEYS);
    p.f16out = out_t == ActType::F16;
    ACEMI_CHECK(p.n_split == 1 || a.part, "lm_attention_chunk: split workspace missing");
    const dim3 grid(p.n_split, (unsigned)ceil_div(a.n * rep, TROWS), a.hkv * B);
    hipLaunchKernelGGL(lm_attn_chunk_kernel, grid, dim3(256), 0, s, p);
    ACEMI_HIP(hipGetLastError());
    if (p.n_split > 1) launch_lm_attn_merge(out_t, a.part, B * a.n, hq, p.n_split, a.out, s);
}

}  // namespace acemi
