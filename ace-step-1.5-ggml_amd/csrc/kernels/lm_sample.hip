// Token selection for the 5 Hz LM's decode loop (kernels.h launch_lm_select; semantics: include/acestep_mi355x.h,
// ace_mi_lm_select): logits of one forward -> one token per sampled sequence, in one launch.
//
// Mapping.  One workgroup of 1024 threads (16 waves) per sampled sequence, S <= 8 workgroups: the work of one sequence
// is a chain of dependent reductions over its candidates, so a second workgroup could only help through a grid-wide
// wait per reduction.  The candidates (the allowed list, else the vocabulary) are visited in passes of 1024: thread t
// takes candidates t, t + 1024, ... (coalesced).  The first pass writes the processed value z of every candidate to the
// scratch plane wz; later passes read that plane (it stays in L2) and a second plane we for exp values.  LDS holds one
// 256-bin histogram and 16-word reduction rows (about 1.2 KiB); no register array, so the 128 VGPRs that 16 waves per
// CU leave each thread are far from used.
//
// Thresholds by selection on key(z), the order-preserving uint32 image of the f32 value (-0 orders as +0):
//   top-k   a radix select of the k-th largest key: four passes, one byte each, counting into the LDS histogram with
//           integer atomics (lanes of a wave that hit the same bin are merged first, so the first byte, which most
//           logits share, does not serialise); integer counts do not depend on the order of arrival.
//   top-p   e = expf(z - max), Z = sum e, then a bisection on the key interval [smallest survivor, largest]: the
//           smallest key t with mass(key > t) <= top_p * Z, one mass reduction per step, at most 32 steps.  The mass
//           reduction adds in a fixed tree, and a fixed tree of non-negative terms is monotone in t, so the bisection
//           is well defined in f32.  Values equal to each other share a key: a group stays or goes as a whole.
// Sums: thread-sequential over its candidates, then an xor butterfly inside the wave (both partners compute the same
// commutative sum), then the 16 wave results added in wave order by every thread.  Chain behind a top-p mass:
// ceil(n / 1024) + 6 + 15 additions (lm_select_chains()[0]).
// Draw: wave w owns the contiguous candidates [w * seg, (w + 1) * seg), seg = ceil(n / 16), in rows of 64.  Pass A
// stores p' = expf(z / temperature - max / temperature) and reduces lane columns, wave, then waves in order (base of
// wave w = sum of the waves before it; total = all 16).  Pass B walks the rows with an inclusive wave scan (6 steps)
// on top of a running carry and takes the first kept candidate whose cumulative value exceeds u * total; the lowest
// such candidate over the waves wins (an integer minimum), the largest kept candidate if none does.  With rows =
// ceil(seg / 64), the chain behind the total is rows + 6 + 16 additions (lm_select_chains()[1]; 171 for the stock
// vocabulary of 151 936).  A cumulative value sits deeper: the base of the last wave is 15 wave totals (each rows + 6
// deep) added in order, the carry then takes one row total per row already walked (rows - 1), and the value itself is
// carry + scan: 2 * rows + 21 additions (lm_select_chains()[2]; 319 for the stock vocabulary).
// No float atomics anywhere; every reduction has a fixed shape, so two runs give the same bits.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../kernels.h"

#pragma clang fp contract(off)

namespace acemi {

namespace {

constexpr int SEL_THREADS = 1024;
constexpr int SEL_WAVES = SEL_THREADS / 64;
constexpr uint32_t KEY_NINF = 0x007fffffu;  // key(-inf): every finite value and +inf has a larger key

__device__ __forceinline__ uint32_t sel_key(float z) {
    uint32_t u = __float_as_uint(z);
    if ((u << 1) == 0u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float sel_unkey(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

struct SelShared {
    uint32_t hist[256];
    float fpart[SEL_WAVES];
    uint32_t upart[SEL_WAVES];
    uint32_t bin, krem;
};

__device__ __forceinline__ float wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o);
    return v;
}

__device__ float block_sum(float v, SelShared& sh) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh.fpart[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = sh.fpart[0];
    for (int i = 1; i < SEL_WAVES; ++i) t = t + sh.fpart[i];
    __syncthreads();
    return t;
}

template <bool MAX>
__device__ uint32_t block_minmax(uint32_t v, SelShared& sh) {
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t t = (uint32_t)__shfl_xor((int)v, o);
        v = MAX ? (t > v ? t : v) : (t < v ? t : v);
    }
    if ((threadIdx.x & 63) == 0) sh.upart[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t r = sh.upart[0];
    for (int i = 1; i < SEL_WAVES; ++i) {
        const uint32_t t = sh.upart[i];
        r = MAX ? (t > r ? t : r) : (t < r ? t : r);
    }
    __syncthreads();
    return r;
}

// steps 1-4 for one candidate id; an id outside the vocabulary (a list nobody validated) is never read
__device__ __forceinline__ float sel_value(const LmSelectArgs& a, int s, int id) {
    if (id < 0 || id >= a.vocab) return -INFINITY;
    if (a.block_stop && !a.force_stop && id == a.stop_id) return -INFINITY;
    float z = a.logits[(int64_t)s * a.ld_logits + id];
    if (a.cfg_scale > 1.0f) {
        const float u = a.logits[(int64_t)(s + a.S) * a.ld_logits + id];
        const float d = z - u;
        const float sd = a.cfg_scale * d;
        z = u + sd;
    }
    if (z != z) z = -INFINITY;
    if (a.pre_temperature > 0.0f) z = z / a.pre_temperature;
    if (a.seen && a.repetition_penalty != 1.0f && a.seen[(int64_t)s * a.ld_seen + id])
        z = z < 0.0f ? z * a.repetition_penalty : z / a.repetition_penalty;
    return z;
}

__global__ __launch_bounds__(SEL_THREADS) void lm_select_kernel(LmSelectArgs a) {
    __shared__ SelShared sh;
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const bool stopped = a.done && a.stop_id >= 0 && a.done[1 + s] != 0;
    const bool only_stop = a.force_stop || stopped;
    const int n_full = a.allowed ? a.n_allowed : a.vocab;
    const int n = only_stop ? 1 : n_full;
    float* wz = a.work + (size_t)s * 2 * n_full;
    float* we = wz + n_full;
    auto id_of = [&](int c) { return only_stop ? a.stop_id : (a.allowed ? a.allowed[c] : c); };

    // pass 0: the processed value of every candidate
    uint32_t kmax = 0;
    for (int base = 0; base < n; base += SEL_THREADS) {
        const int c = base + tid;
        if (c < n) {
            const float z = sel_value(a, s, id_of(c));
            wz[c] = z;
            const uint32_t k = sel_key(z);
            kmax = k > kmax ? k : kmax;
        }
    }
    kmax = block_minmax<true>(kmax, sh);  // its barriers also publish wz to the whole workgroup
    const bool empty = kmax <= KEY_NINF;
    uint32_t thr = KEY_NINF + 1;

    // step 5: the key of the k-th largest candidate
    if (!empty && a.top_k > 0 && a.top_k < n) {
        uint32_t prefix = 0, mask = 0, krem = (uint32_t)a.top_k;
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) sh.hist[tid] = 0;
            __syncthreads();
            for (int base = 0; base < n; base += SEL_THREADS) {
                const int c = base + tid;
                uint32_t bin = 0;
                bool act = false;
                if (c < n) {
                    const uint32_t k = sel_key(wz[c]);
                    act = (k & mask) == prefix;
                    bin = (k >> shift) & 255u;
                }
                for (int it = 0; it < 4; ++it) {  // merge the lanes that share the bin of the first waiting lane
                    const unsigned long long m = __ballot(act);
                    if (!m) break;
                    const int leader = __ffsll((long long)m) - 1;
                    const uint32_t b0 = (uint32_t)__shfl((int)bin, leader);
                    const unsigned long long same = __ballot(act && bin == b0);
                    if (lane == leader) atomicAdd(&sh.hist[b0], (uint32_t)__popcll(same));
                    if (bin == b0) act = false;
                }
                if (act) atomicAdd(&sh.hist[bin], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                uint32_t acc = 0;
                int b = 255;
                for (; b > 0; --b) {
                    if (acc + sh.hist[b] >= krem) break;
                    acc += sh.hist[b];
                }
                sh.bin = (uint32_t)b;
                sh.krem = krem - acc;
            }
            __syncthreads();
            prefix |= sh.bin << shift;
            mask |= 255u << shift;
            krem = sh.krem;
            __syncthreads();
        }
        thr = prefix > thr ? prefix : thr;
    }

    // step 6: the smallest key whose mass of strictly larger survivors is within top_p
    const float zmax = sel_unkey(kmax);
    if (!empty && a.top_p > 0.0f && a.top_p < 1.0f) {
        float acc = 0.0f;
        uint32_t kmin = 0xffffffffu;
        for (int base = 0; base < n; base += SEL_THREADS) {
            const int c = base + tid;
            if (c < n) {
                const float z = wz[c];
                const uint32_t k = sel_key(z);
                if (k >= thr) {
                    const float e = expf(z - zmax);
                    we[c] = e;
                    acc = acc + e;
                    kmin = k < kmin ? k : kmin;
                }
            }
        }
        const float Z = block_sum(acc, sh);
        kmin = block_minmax<false>(kmin, sh);
        const float lim = a.top_p * Z;
        uint32_t lo = kmin, hi = kmax;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            float m = 0.0f;
            for (int base = 0; base < n; base += SEL_THREADS) {
                const int c = base + tid;
                if (c < n && sel_key(wz[c]) > mid) m = m + we[c];  // mid >= kmin >= thr: a survivor
            }
            m = block_sum(m, sh);
            if (m <= lim)
                hi = mid;
            else
                lo = mid + 1;
        }
        thr = lo;
    }

    if (a.processed) {
        float* out = a.processed + (int64_t)s * a.ld_processed;
        for (int v = tid; v < a.vocab; v += SEL_THREADS) out[v] = -INFINITY;
        __syncthreads();
        if (!empty)
            for (int c = tid; c < n; c += SEL_THREADS) {
                const float z = wz[c];
                if (sel_key(z) >= thr) out[id_of(c)] = z;
            }
    }

    // step 7
    uint32_t pick = 0;
    if (empty) {
        pick = 0;
    } else if (!(a.temperature > 0.0f)) {
        uint32_t cmin = 0xffffffffu;
        for (int c = tid; c < n; c += SEL_THREADS)
            if (sel_key(wz[c]) == kmax) cmin = (uint32_t)c < cmin ? (uint32_t)c : cmin;
        pick = block_minmax<false>(cmin, sh);
    } else {
        const float T = a.temperature;
        const float m2 = zmax / T;
        const int seg = (n + SEL_WAVES - 1) / SEL_WAVES;
        const int rows = (seg + 63) / 64;
        const int c0 = w * seg;
        float col = 0.0f;
        uint32_t clast = 0;
        for (int r = 0; r < rows; ++r) {
            const int i = r * 64 + lane, c = c0 + i;
            if (i < seg && c < n) {
                const float z = wz[c];
                float e = 0.0f;
                if (sel_key(z) >= thr) {
                    e = expf(z / T - m2);
                    clast = (uint32_t)c;
                }
                we[c] = e;
                col = col + e;
            }
        }
        col = wave_sum(col);
        if (lane == 0) sh.fpart[w] = col;
        clast = block_minmax<true>(clast, sh);  // barriers: fpart and we are visible
        float wbase = 0.0f, total = 0.0f;
        for (int i = 0; i < SEL_WAVES; ++i) {
            if (i == w) wbase = total;
            total = total + sh.fpart[i];
        }
        const float target = a.uniform[s] * total;
        uint32_t found = 0xffffffffu;
        float carry = wbase;
        for (int r = 0; r < rows; ++r) {
            const int i = r * 64 + lane, c = c0 + i;
            const bool valid = i < seg && c < n;
            float e = 0.0f;
            bool kept = false;
            if (valid) {
                e = we[c];
                kept = sel_key(wz[c]) >= thr;
            }
            float incl = e;
            for (int o = 1; o < 64; o <<= 1) {
                const float t = __shfl_up(incl, o);
                if (lane >= o) incl = incl + t;
            }
            const float cum = carry + incl;
            const unsigned long long hit = __ballot(kept && cum > target);
            if (hit) {
                found = (uint32_t)(c0 + r * 64 + (__ffsll((long long)hit) - 1));
                break;
            }
            carry = carry + __shfl(incl, 63);
        }
        found = block_minmax<false>(found, sh);
        pick = found != 0xffffffffu ? found : clast;
    }

    if (tid == 0) {
        int tok = id_of((int)pick);
        tok = tok < 0 ? 0 : (tok >= a.vocab ? a.vocab - 1 : tok);
        a.tokens[(int64_t)s * a.token_stride] = tok;
        if (a.next_ids) {
            a.next_ids[s] = tok;
            if (a.cfg_scale > 1.0f) a.next_ids[s + a.S] = tok;
        }
        if (a.seen) a.seen[(int64_t)s * a.ld_seen + tok] = 1;
        if (a.done && a.stop_id >= 0 && tok == a.stop_id) {
            a.done[1 + s] = 1;
            if (a.done[0] == 0) a.done[0] = a.n_emitted + 1;  // every workgroup of this launch writes the same value
        }
    }
}

}  // namespace

void lm_select_chains(int n_cand, int* chains) {
    const int seg = (n_cand + SEL_WAVES - 1) / SEL_WAVES;
    chains[0] = (n_cand + SEL_THREADS - 1) / SEL_THREADS + 6 + (SEL_WAVES - 1);
    const int rows = (seg + 63) / 64;
    chains[1] = rows + 6 + SEL_WAVES;
    chains[2] = (rows + 6 + (SEL_WAVES - 1)) + (rows - 1) + 1;
}

void launch_lm_select(const LmSelectArgs& a, hipStream_t s) {
    ACEMI_CHECK(a.logits && a.tokens && a.work && a.vocab >= 1 && a.ld_logits >= a.vocab, "lm_select: bad arguments");
    ACEMI_CHECK(a.S >= 1 && a.S * (a.cfg_scale > 1.0f ? 2 : 1) <= LM_MAX_BATCH, "lm_select: bad batch");
    ACEMI_CHECK(!a.allowed || a.n_allowed >= 1, "lm_select: empty allowed list");
    ACEMI_CHECK(a.stop_id < a.vocab && (!a.force_stop || a.stop_id >= 0), "lm_select: bad stop id");
    ACEMI_CHECK(!(a.temperature > 0.0f) || a.uniform, "lm_select: sampling needs the uniforms");
    ACEMI_CHECK(!a.seen || a.ld_seen >= a.vocab, "lm_select: bad seen map");
    ACEMI_CHECK(!a.processed || a.ld_processed >= a.vocab, "lm_select: bad processed rows");
    hipLaunchKernelGGL(lm_select_kernel, dim3(a.S), dim3(SEL_THREADS), 0, s, a);
    ACEMI_HIP(hipGetLastError());
}

}  // namespace acemi
