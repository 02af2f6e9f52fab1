// Token-by-token decode of the Qwen3 causal LM (runtime/lm.cpp): M = 1..8 rows per step, so every kernel here is
// bound by the bytes it reads (weights once per step, the KV cache once per layer), not by FLOPs.  No MFMA.
//
//   lm_skinny_kernel    y[B][N] = x[B][K] . W[N][K]^T, 16-bit x and W, f32 accumulate.  One wave per output row
//                       (the gate row and its up row for SwiGLU), lanes stride the row in 16-byte words (a wave
//                       instruction reads 1 KiB of one row, coalesced), every x row reuses the weight word in
//                       registers, so each weight byte is read once for all B sequences.  N = 1024 gives 256
//                       workgroups of four waves.  The reduction is lane-local over k in ascending order, then a
//                       fixed xor butterfly: no atomics, no split along K, bit-identical between runs.
//   lm_qkv_post_kernel  per head of the fused q|k|v row: RMSNorm (q, k) and NEOX RoPE at the slot position in f32
//                       (prep_math.h's operation order), Q kept in f32, K and V appended to the cache as fp16.
//   lm_prefill_kv_kernel the same K / V append for every row of a prefill (from the QKV GEMM's f32 output); rows of
//                       padding tokens (mask 0) are zeroed in the GEMM output and in the cache, so that a
//                       left-padded prompt never feeds a non-finite value into another row's attention.
//   lm_attn_kernel      one workgroup per (key range, kv head, sequence): the hq / hkv query heads of the kv head
//                       share one read of K and V; scores, f32 softmax and P.V over up to LM_SPLIT_KEYS keys.
//                       More keys: one workgroup per range of LM_SPLIT_KEYS writes (m, l, unnormalised O) and
//                       lm_attn_merge_kernel joins the ranges in ascending order (log-sum-exp), deterministically.
//
// KV cache: K and V [layer][B][hkv][capacity][128] fp16 (saturated to the fp16 range), key mask [B][capacity] int32.
#include <hip/hip_runtime.h>

#include "../kernels.h"
#include "prep_math.h"

namespace acemi {

namespace {

constexpr int LM_D = 128;

// the GEMM epilogues' roundings (gemm_common.h)
__device__ __forceinline__ uint16_t f32_to_bf16_rne(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 64u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
template <bool F16>
__device__ __forceinline__ uint16_t to_act(float f) {
    if constexpr (F16) return prep::f16_bits(f);
    return f32_to_bf16_rne(f);
}
__device__ __forceinline__ float silu_f(float x) { return x / (1.0f + expf(-x)); }

template <bool F16>
__device__ __forceinline__ void unpack2(uint32_t w, float& a, float& b) {
    if constexpr (F16) {
        a = (float)__builtin_bit_cast(_Float16, (uint16_t)(w & 0xffffu));
        b = (float)__builtin_bit_cast(_Float16, (uint16_t)(w >> 16));
    } else {
        a = __uint_as_float(w << 16);
        b = __uint_as_float(w & 0xffff0000u);
    }
}

template <bool F16>
__device__ __forceinline__ void unpack8(const uint4& w, float (&f)[8]) {
    unpack2<F16>(w.x, f[0], f[1]);
    unpack2<F16>(w.y, f[2], f[3]);
    unpack2<F16>(w.z, f[4], f[5]);
    unpack2<F16>(w.w, f[6], f[7]);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ uint16_t f16_sat(float f) {
    return prep::f16_bits(fminf(fmaxf(f, -65504.0f), 65504.0f));
}

// ------------------------------------------------------------------ skinny matrix product
template <bool F16, int B, int EPI>
__global__ void __launch_bounds__(256) lm_skinny_kernel(const uint16_t* __restrict__ x, int ldx,
                                                        const uint16_t* __restrict__ W, int N, int K,
                                                        float* __restrict__ y_f32, uint16_t* __restrict__ y_act,
                                                        int ldy) {
    constexpr int ROWS = EPI == LM_EPI_SWIGLU ? 2 : 1;
    const int lane = threadIdx.x & 63;
    const int unit = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int n_units = N / ROWS;
    if (unit >= n_units) return;  // wave-uniform
    int64_t row[ROWS];
    if constexpr (EPI == LM_EPI_SWIGLU) {  // w_gu rows: [g0..15, u0..15, g16..31, ...]
        row[0] = (int64_t)(unit >> 4) * 32 + (unit & 15);
        row[1] = row[0] + 16;
    } else {
        row[0] = unit;
    }
    float acc[ROWS][B];
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
        for (int b = 0; b < B; ++b) acc[r][b] = 0.f;
#pragma unroll 2
    for (int k = lane * 8; k < K; k += 512) {
        float w[ROWS][8];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) unpack8<F16>(*(const uint4*)(W + row[r] * K + k), w[r]);
#pragma unroll
        for (int b = 0; b < B; ++b) {
            float xv[8];
            unpack8<F16>(*(const uint4*)(x + (int64_t)b * ldx + k), xv);
#pragma unroll
            for (int r = 0; r < ROWS; ++r)
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[r][b] = fmaf(w[r][j], xv[j], acc[r][b]);
        }
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
        for (int b = 0; b < B; ++b) acc[r][b] = wave_sum(acc[r][b]);
    if (lane != 0) return;
#pragma unroll
    for (int b = 0; b < B; ++b) {
        if constexpr (EPI == LM_EPI_STORE) {
            y_f32[(int64_t)b * ldy + unit] = acc[0][b];
        } else if constexpr (EPI == LM_EPI_RESID) {
            y_f32[(int64_t)b * ldy + unit] += acc[0][b];
        } else {
            y_act[(int64_t)b * ldy + unit] = to_act<F16>(silu_f(acc[0][b]) * acc[1][b]);
        }
    }
}

template <bool F16, int B>
void skinny_epi(int epi, dim3 grid, hipStream_t s, const uint16_t* x, int ldx, const uint16_t* W, int N, int K,
                float* y_f32, uint16_t* y_act, int ldy) {
    if (epi == LM_EPI_STORE)
        hipLaunchKernelGGL((lm_skinny_kernel<F16, B, LM_EPI_STORE>), grid, dim3(256), 0, s, x, ldx, W, N, K, y_f32, y_act, ldy);
    else if (epi == LM_EPI_RESID)
        hipLaunchKernelGGL((lm_skinny_kernel<F16, B, LM_EPI_RESID>), grid, dim3(256), 0, s, x, ldx, W, N, K, y_f32, y_act, ldy);
    else
        hipLaunchKernelGGL((lm_skinny_kernel<F16, B, LM_EPI_SWIGLU>), grid, dim3(256), 0, s, x, ldx, W, N, K, y_f32, y_act, ldy);
}

template <bool F16>
void skinny_b(int B, int epi, dim3 grid, hipStream_t s, const uint16_t* x, int ldx, const uint16_t* W, int N, int K,
              float* y_f32, uint16_t* y_act, int ldy) {
    switch (B) {
        case 1: skinny_epi<F16, 1>(epi, grid, s, x, ldx, W, N, K, y_f32, y_act, ldy); break;
        case 2: skinny_epi<F16, 2>(epi, grid, s, x, ldx, W, N, K, y_f32, y_act, ldy); break;
        case 3: skinny_epi<F16, 3>(epi, grid, s, x, ldx, W, N, K, y_f32, y_act, ldy); break;
        case 4: skinny_epi<F16, 4>(epi, grid, s, x, ldx, W, N, K, y_f32, y_act, ldy); break;
        case 5: skinny_epi<F16, 5>(epi, grid, s, x, ldx, W, N, K, y_f32, y_act, ldy); break;
        case 6: skinny_epi<F16, 6>(epi, grid, s, x, ldx, W, N, K, y_f32, y_act, ldy); break;
        case 7: skinny_epi<F16, 7>(epi, grid, s, x, ldx, W, N, K, y_f32, y_act, ldy); break;
        default: skinny_epi<F16, 8>(epi, grid, s, x, ldx, W, N, K, y_f32, y_act, ldy); break;
    }
}

// ------------------------------------------------------------------ embedding rows (ids clamped into the table)
template <int FMT>
__global__ void __launch_bounds__(256) lm_embed_kernel(const uint16_t* __restrict__ table, const int32_t* __restrict__ ids,
                                                       int vocab, int H, float* __restrict__ out) {
    const int t = blockIdx.x;
    const int64_t row = min(max(ids[t], 0), vocab - 1);
    for (int i = threadIdx.x * 8; i < H; i += 256 * 8) {
        float f[8];
        unpack8<FMT == 1>(*(const uint4*)(table + row * H + i), f);
        *(float4*)(out + (int64_t)t * H + i) = make_float4(f[0], f[1], f[2], f[3]);
        *(float4*)(out + (int64_t)t * H + i + 4) = make_float4(f[4], f[5], f[6], f[7]);
    }
}

// ------------------------------------------------------------------ q/k norm + RoPE, cache append
// One head row of 128 by one wave: lane i holds dims i and i + 64 (the NEOX pair).  Returns the rotated pair.
__device__ __forceinline__ void norm_rope(float& a, float& b, const float* w, const float* cs, const float* sn,
                                          float eps, int lane) {
    const float ss = wave_sum(a * a + b * b);
    const float sc = 1.0f / sqrtf(ss / 128.0f + eps);
    a = rn_mul(rn_mul(a, sc), w[lane]);
    b = rn_mul(rn_mul(b, sc), w[64 + lane]);
    const float c = cs[lane], s = sn[lane];
    const float ra = rn_sub(rn_mul(a, c), rn_mul(b, s));
    const float rb = rn_add(rn_mul(a, s), rn_mul(b, c));
    a = ra;
    b = rb;
}

__global__ void __launch_bounds__(64) lm_qkv_post_kernel(LmQkvPostArgs a) {
    const int head = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const float* src = a.qkv + (int64_t)b * a.ld + (int64_t)head * LM_D;
    float v0 = src[lane], v1 = src[64 + lane];
    const float* cs = a.rope_cos + (int64_t)a.pos * 64;
    const float* sn = a.rope_sin + (int64_t)a.pos * 64;
    if (head < a.hq) {
        norm_rope(v0, v1, a.q_norm, cs, sn, a.eps, lane);
        float* q = a.q_out + ((int64_t)b * a.hq + head) * LM_D;
        q[lane] = v0;
        q[64 + lane] = v1;
        if (head == 0 && lane == 0) a.key_mask[(int64_t)b * a.capacity + a.pos] = a.mask_new ? (a.mask_new[b] != 0) : 1;
        return;
    }
    const bool is_k = head < a.hq + a.hkv;
    const int kh = is_k ? head - a.hq : head - a.hq - a.hkv;
    if (is_k) norm_rope(v0, v1, a.k_norm, cs, sn, a.eps, lane);
    uint16_t* dst = (is_k ? a.k_cache : a.v_cache) + (((int64_t)b * a.hkv + kh) * a.capacity + a.pos) * LM_D;
    dst[lane] = f16_sat(v0);
    dst[64 + lane] = f16_sat(v1);
}

// grid (hq + 2 hkv, n, B): row m = b * n + t of the prefill's QKV output
__global__ void __launch_bounds__(64) lm_prefill_kv_kernel(LmQkvPostArgs a, int n, const int32_t* __restrict__ mask) {
    const int head = blockIdx.x, t = blockIdx.y, b = blockIdx.z, lane = threadIdx.x;
    const int64_t m = (int64_t)b * n + t;
    const bool valid = mask ? mask[m] != 0 : true;
    float* src = const_cast<float*>(a.qkv) + m * a.ld + (int64_t)head * LM_D;
    if (!valid) {  // a padding row carries nothing into the attention of any other row
        src[lane] = 0.f;
        src[64 + lane] = 0.f;
    }
    if (head < a.hq) {
        if (head == 0 && lane == 0) a.key_mask[(int64_t)b * a.capacity + t] = valid ? 1 : 0;
        return;
    }
    const bool is_k = head < a.hq + a.hkv;
    const int kh = is_k ? head - a.hq : head - a.hq - a.hkv;
    float v0 = valid ? src[lane] : 0.f, v1 = valid ? src[64 + lane] : 0.f;
    if (is_k && valid) norm_rope(v0, v1, a.k_norm, a.rope_cos + (int64_t)t * 64, a.rope_sin + (int64_t)t * 64, a.eps, lane);
    uint16_t* dst = (is_k ? a.k_cache : a.v_cache) + (((int64_t)b * a.hkv + kh) * a.capacity + t) * LM_D;
    dst[lane] = f16_sat(v0);
    dst[64 + lane] = f16_sat(v1);
}

// ------------------------------------------------------------------ decode attention
__device__ __forceinline__ void unpack8_f16(const uint4& w, float (&f)[8]) { unpack8<true>(w, f); }

template <int REP, bool F16OUT>
__global__ void __launch_bounds__(256) lm_attn_kernel(LmAttnArgs a) {
    __shared__ float sc[REP][LM_SPLIT_KEYS];
    __shared__ float red[4][REP][LM_D];
    __shared__ float stat[REP][4];
    const int sp = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int sub = tid & 15, kg = tid >> 4;
    const int k0 = sp * LM_SPLIT_KEYS;
    const int cnt = min(a.nk - k0, LM_SPLIT_KEYS);
    const int hq = a.hkv * REP;
    const int64_t base = (((int64_t)b * a.hkv + h) * a.capacity + k0) * LM_D + sub * 8;
    const uint16_t* K = a.k_cache + base;
    const uint16_t* V = a.v_cache + base;
    const int32_t* km = a.key_mask + (int64_t)b * a.capacity + k0;

    float q[REP][8];
#pragma unroll
    for (int r = 0; r < REP; ++r) {
        const float* qp = a.q + ((int64_t)b * hq + h * REP + r) * LM_D + sub * 8;
        const float4 q0 = *(const float4*)qp, q1 = *(const float4*)(qp + 4);
        q[r][0] = q0.x, q[r][1] = q0.y, q[r][2] = q0.z, q[r][3] = q0.w;
        q[r][4] = q1.x, q[r][5] = q1.y, q[r][6] = q1.z, q[r][7] = q1.w;
    }
    // scores: 16 lanes per key, 16 keys per pass
    for (int j0 = 0; j0 < cnt; j0 += 16) {
        const int j = j0 + kg;
        const bool in = j < cnt;
        float kf[8];
        unpack8_f16(in ? *(const uint4*)(K + (int64_t)j * LM_D) : make_uint4(0, 0, 0, 0), kf);
#pragma unroll
        for (int r = 0; r < REP; ++r) {
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) s = fmaf(q[r][i], kf[i], s);
#pragma unroll
            for (int o = 8; o >= 1; o >>= 1) s += __shfl_xor(s, o);
            if (in && sub == 0) sc[r][j] = km[j] != 0 ? s * a.scale : -INFINITY;
        }
    }
    __syncthreads();
    // softmax statistics of the range: thread t owns key t
    float mloc[REP], p[REP];
#pragma unroll
    for (int r = 0; r < REP; ++r) {
        float m = tid < cnt ? sc[r][tid] : -INFINITY;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if (lane == 0) stat[r][wave] = m;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < REP; ++r) {
        mloc[r] = fmaxf(fmaxf(stat[r][0], stat[r][1]), fmaxf(stat[r][2], stat[r][3]));
        const float s = tid < cnt ? sc[r][tid] : -INFINITY;
        p[r] = (s == -INFINITY) ? 0.f : expf(s - mloc[r]);
    }
    __syncthreads();  // stat and sc are rewritten below
    float lsum[REP];
#pragma unroll
    for (int r = 0; r < REP; ++r) {
        if (tid < cnt) sc[r][tid] = p[r];
        const float l = wave_sum(p[r]);
        if (lane == 0) stat[r][wave] = l;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < REP; ++r) lsum[r] = (stat[r][0] + stat[r][1]) + (stat[r][2] + stat[r][3]);
    // P.V: thread (kg, sub) sums its keys j = kg, kg + 16, ... in ascending order
    float acc[REP][8];
#pragma unroll
    for (int r = 0; r < REP; ++r)
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[r][i] = 0.f;
    for (int j = kg; j < cnt; j += 16) {
        float vf[8];
        unpack8_f16(*(const uint4*)(V + (int64_t)j * LM_D), vf);
#pragma unroll
        for (int r = 0; r < REP; ++r) {
            const float pj = sc[r][j];
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[r][i] = fmaf(pj, vf[i], acc[r][i]);
        }
    }
#pragma unroll
    for (int r = 0; r < REP; ++r)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float v = acc[r][i];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            if (lane < 16) red[wave][r][sub * 8 + i] = v;
        }
    __syncthreads();
    for (int e = tid; e < REP * LM_D; e += 256) {
        const int r = e / LM_D, d = e % LM_D;
        const float o = (red[0][r][d] + red[1][r][d]) + (red[2][r][d] + red[3][r][d]);
        const int head = h * REP + r;
        if (a.n_split == 1) {
            const float v = lsum[r] > 0.f ? o / lsum[r] : 0.f;
            a.out[((int64_t)b * hq + head) * LM_D + d] = to_act<F16OUT>(v);
        } else {
            float* part = a.part + (((int64_t)b * hq + head) * a.n_split + sp) * (LM_D + 2);
            part[2 + d] = o;
            if (d == 0) {
                part[0] = mloc[r];
                part[1] = lsum[r];
            }
        }
    }
}

// grid (hq, B), 128 threads: joins the key ranges in ascending order
template <bool F16OUT>
__global__ void __launch_bounds__(128) lm_attn_merge_kernel(const float* __restrict__ part, int hq, int n_split,
                                                            uint16_t* __restrict__ out) {
    const int head = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
    const float* p = part + ((int64_t)b * hq + head) * n_split * (LM_D + 2);
    float M = -INFINITY;
    for (int s = 0; s < n_split; ++s) M = fmaxf(M, p[(int64_t)s * (LM_D + 2)]);
    float L = 0.f, O = 0.f;
    for (int s = 0; s < n_split; ++s) {
        const float* ps = p + (int64_t)s * (LM_D + 2);
        const float w = ps[0] == -INFINITY ? 0.f : expf(ps[0] - M);
        L = fmaf(ps[1], w, L);
        O = fmaf(ps[2 + d], w, O);
    }
    out[((int64_t)b * hq + head) * LM_D + d] = to_act<F16OUT>(L > 0.f ? O / L : 0.f);
}

}  // namespace

void launch_lm_skinny(ActType t, const uint16_t* x, int ldx, int B, const uint16_t* W, int N, int K, int epi,
                      float* y_f32, uint16_t* y_act, int ldy, hipStream_t s) {
    ACEMI_CHECK(B >= 1 && B <= LM_MAX_BATCH && N >= 1 && K >= 8 && K % 8 == 0 && ldx % 8 == 0 && x && W,
                "lm_skinny: bad shape");
    ACEMI_CHECK(epi == LM_EPI_SWIGLU ? (N % 32 == 0 && y_act) : ((epi == LM_EPI_STORE || epi == LM_EPI_RESID) && y_f32),
                "lm_skinny: bad epilogue");
    const int units = epi == LM_EPI_SWIGLU ? N / 2 : N;
    const dim3 grid((unsigned)ceil_div(units, 4));
    if (t == ActType::F16)
        skinny_b<true>(B, epi, grid, s, x, ldx, W, N, K, y_f32, y_act, ldy);
    else
        skinny_b<false>(B, epi, grid, s, x, ldx, W, N, K, y_f32, y_act, ldy);
    ACEMI_HIP(hipGetLastError());
}

void launch_lm_embed(const void* table, int fmt, const int32_t* ids, int n, int vocab, int H, float* out,
                     hipStream_t s) {
    ACEMI_CHECK((fmt == 0 || fmt == 1) && n >= 1 && vocab >= 1 && H % 8 == 0 && table && ids, "lm_embed: bad arguments");
    if (fmt == 0)
        hipLaunchKernelGGL(lm_embed_kernel<0>, dim3(n), dim3(256), 0, s, (const uint16_t*)table, ids, vocab, H, out);
    else
        hipLaunchKernelGGL(lm_embed_kernel<1>, dim3(n), dim3(256), 0, s, (const uint16_t*)table, ids, vocab, H, out);
    ACEMI_HIP(hipGetLastError());
}

static void check_post(const LmQkvPostArgs& a, int B) {
    ACEMI_CHECK(B >= 1 && B <= LM_MAX_BATCH && a.hq >= 1 && a.hkv >= 1 && a.capacity >= 1 && a.qkv && a.k_cache &&
                    a.v_cache && a.key_mask && a.rope_cos && a.rope_sin && a.q_norm && a.k_norm,
                "lm_qkv_post: bad arguments");
}

void launch_lm_qkv_post(const LmQkvPostArgs& a, int B, hipStream_t s) {
    check_post(a, B);
    ACEMI_CHECK(a.pos >= 0 && a.pos < a.capacity && a.q_out, "lm_qkv_post: position outside the cache");
    hipLaunchKernelGGL(lm_qkv_post_kernel, dim3(a.hq + 2 * a.hkv, B), dim3(64), 0, s, a);
    ACEMI_HIP(hipGetLastError());
}

void launch_lm_prefill_kv(const LmQkvPostArgs& a, int B, int n, const int32_t* mask, hipStream_t s) {
    check_post(a, B);
    ACEMI_CHECK(n >= 1 && n <= a.capacity && n <= 65535, "lm_prefill_kv: rows outside the cache");
    hipLaunchKernelGGL(lm_prefill_kv_kernel, dim3(a.hq + 2 * a.hkv, n, B), dim3(64), 0, s, a, n, mask);
    ACEMI_HIP(hipGetLastError());
}

size_t lm_attn_part_floats(int B, int hq, int nk) {
    return (size_t)B * hq * ceil_div(nk, LM_SPLIT_KEYS) * (LM_D + 2);
}

void launch_lm_attention(ActType out_t, const LmAttnArgs& a0, int B, int hq, hipStream_t s) {
    LmAttnArgs a = a0;
    ACEMI_CHECK(B >= 1 && B <= LM_MAX_BATCH && a.hkv >= 1 && hq % a.hkv == 0 && a.nk >= 1 && a.nk <= a.capacity &&
                    a.q && a.k_cache && a.v_cache && a.key_mask && a.out,
                "lm_attention: bad arguments");
    const int rep = hq / a.hkv;
    ACEMI_CHECK(rep == 1 || rep == 2 || rep == 4, "lm_attention: GQA ratio must be 1, 2 or 4");
    a.n_split = (int)ceil_div(a.nk, LM_SPLIT_KEYS);
    ACEMI_CHECK(a.n_split == 1 || a.part, "lm_attention: split workspace missing");
    const dim3 grid(a.n_split, a.hkv, B);
    const bool f16 = out_t == ActType::F16;
#define ACEMI_LM_ATTN(R)                                                                  \
    if (f16)                                                                              \
        hipLaunchKernelGGL((lm_attn_kernel<R, true>), grid, dim3(256), 0, s, a);          \
    else                                                                                  \
        hipLaunchKernelGGL((lm_attn_kernel<R, false>), grid, dim3(256), 0, s, a)
    if (rep == 1) {
        ACEMI_LM_ATTN(1);
    } else if (rep == 2) {
        ACEMI_LM_ATTN(2);
    } else {
        ACEMI_LM_ATTN(4);
    }
#undef ACEMI_LM_ATTN
    ACEMI_HIP(hipGetLastError());
    if (a.n_split > 1) {
        if (f16)
            hipLaunchKernelGGL(lm_attn_merge_kernel<true>, dim3(hq, B), dim3(128), 0, s, a.part, hq, a.n_split, a.out);
        else
            hipLaunchKernelGGL(lm_attn_merge_kernel<false>, dim3(hq, B), dim3(128), 0, s, a.part, hq, a.n_split, a.out);
        ACEMI_HIP(hipGetLastError());
    }
}

}  // namespace acemi
