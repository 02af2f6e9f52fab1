// Host emulation of the gfx950 kernels (TEST INFRASTRUCTURE, never shipped): every launch_* entry of
// csrc/kernels.h restated as plain C++ loops over "device" memory that is host memory, plus stub HIP
// runtime functions.  Linked with the real runtime/*.cpp into libacestep_mi355x_host.so it runs the
// product's host orchestration (ABI validation, loaders, buffer sizing, pointer offsets, the order and
// arguments of every launch) on the CPU, so tests can compare whole forwards with the oracle without a
// GPU.  The arithmetic follows each kernel's documented contract (bf16/fp16 operand rounding, f32
// epilogues) with double accumulation; it says nothing about the kernels' own correctness, which the
// -m gpu tests check.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kernels.h"

extern "C" {
hipError_t hipMalloc(void** p, size_t n) {
    *p = std::calloc(1, n ? n : 1);
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipFree(void* p) {
    std::free(p);
    return hipSuccess;
}
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) {
    std::memmove(d, s, n);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t) {
    std::memmove(d, s, n);
    return hipSuccess;
}
hipError_t hipMemcpy2DAsync(void* d, size_t dp, const void* s, size_t sp, size_t w, size_t h, hipMemcpyKind,
                            hipStream_t) {
    for (size_t r = 0; r < h; ++r) std::memmove((char*)d + r * dp, (const char*)s + r * sp, w);
    return hipSuccess;
}
hipError_t hipMemset(void* d, int v, size_t n) {
    std::memset(d, v, n);
    return hipSuccess;
}
hipError_t hipDeviceSynchronize() { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int) {
    *s = reinterpret_cast<hipStream_t>(0x1);
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t) { return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetDeviceCount(int* n) {
    *n = 1;
    return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* e) {
    *e = reinterpret_cast<hipEvent_t>(0x1);
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned int) {
    *e = reinterpret_cast<hipEvent_t>(0x1);
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned int) { return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) {
    *ms = 0.f;
    return hipSuccess;
}
const char* hipGetErrorString(hipError_t) { return "host emulation"; }
}

namespace acemi {
namespace {

float bf16f(uint16_t b) {
    uint32_t u = (uint32_t)b << 16;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
float f16f(uint16_t b) {
    _Float16 h;
    std::memcpy(&h, &b, 2);
    return (float)h;
}
uint16_t to_bf16(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 64u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
uint16_t to_f16(float f) {
    _Float16 h = (_Float16)f;
    uint16_t u;
    std::memcpy(&u, &h, 2);
    return u;
}
float act_val(bool f16, uint16_t b) { return f16 ? f16f(b) : bf16f(b); }
uint16_t to_act(bool f16, float f) { return f16 ? to_f16(f) : to_bf16(f); }
float silu(float x) { return x / (1.0f + expf(-x)); }
int vperm(int k) {
    const int w = k & 15, g = w >> 2;
    const int gp = (g == 1) ? 2 : (g == 2 ? 1 : g);
    return (k & ~15) | (gp << 2) | (w & 3);
}

// weight element (n, k) as the MFMA sees it
float weight_val(const WeightView& W, int K, int n, int k) {
    switch (W.fmt) {
        case WF_BF16: return bf16f(((const uint16_t*)W.q)[(int64_t)n * W.ld + k]);
        case WF_F16: return f16f(((const uint16_t*)W.q)[(int64_t)n * W.ld + k]);
        case WF_Q8_0: {
            const int8_t q = ((const int8_t*)W.q)[(int64_t)n * K + k];
            return bf16f(to_bf16((float)q * W.s[(int64_t)n * (K / 32) + k / 32]));
        }
        case WF_Q6_K: {
            const int8_t q = ((const int8_t*)W.q)[(int64_t)n * K + k];
            return bf16f(to_bf16((float)q * W.s[(int64_t)n * (K / 16) + k / 16]));
        }
        case WF_Q4_K: {
            const int blk = k / 32, i = k % 32;
            const int dw = i / 8, r = i % 8;  // dword dw: low nibbles k 0..3, high nibbles k 4..7
            const uint8_t byte = ((const uint8_t*)W.q)[(int64_t)n * (K / 2) + blk * 16 + dw * 4 + (r & 3)];
            const int q = r < 4 ? (byte & 0xF) : (byte >> 4);
            const float* sm = W.s + ((int64_t)n * (K / 32) + blk) * 2;
            return bf16f(to_bf16(fmaf((float)q, sm[0], -sm[1])));
        }
        default: throw std::runtime_error("emul gemm: bad weight format");
    }
}

}  // namespace

void gemm_force_variant(int) {}

void launch_dequant_bf16(const WeightView& W, int N, int K, uint16_t* out, hipStream_t) {
    ACEMI_CHECK(weight_quantized(W.fmt) && K % 32 == 0, "dequant: quantized [N][K] weight");
    for (int n = 0; n < N; ++n)
        for (int k = 0; k < K; ++k) out[(int64_t)n * K + k] = to_bf16(weight_val(W, K, n, k));
}
void launch_dequant_bf16_batch(const DequantJob* jobs, int n, hipStream_t s) {
    for (int i = 0; i < n; ++i) launch_dequant_bf16(jobs[i].w, jobs[i].N, jobs[i].K, jobs[i].out, s);
}

void launch_gemm(const uint16_t* A, int lda, const WeightView& W, int M, int N, int K, const GemmEpilogue& e,
                 hipStream_t) {
    ACEMI_CHECK(M >= 1 && N % 128 == 0 && K % 64 == 0 && K >= 64, "gemm: unsupported shape");
    const bool af16 = W.fmt == WF_F16;  // activation type of the kernel; quantized weights -> bf16
    std::vector<float> wcol((size_t)K);
    std::vector<double> acc((size_t)M * N);
    std::vector<float> arow((size_t)K);
    std::vector<float> wt((size_t)N * K);
    for (int n = 0; n < N; ++n)
        for (int k = 0; k < K; ++k) wt[(size_t)n * K + k] = weight_val(W, K, n, k);
    for (int m = 0; m < M; ++m) {
        for (int k = 0; k < K; ++k) arow[k] = act_val(af16, A[(int64_t)m * lda + k]);
        for (int n = 0; n < N; ++n) {
            double s = 0;
            const float* w = &wt[(size_t)n * K];
            for (int k = 0; k < K; ++k) s += (double)arow[k] * w[k];
            acc[(size_t)m * N + n] = s;
        }
    }
    if (e.kind == EPI_QKV_PREP) {  // the f32 result through the attn_prep contract
        std::vector<float> tmp((size_t)M * N);
        for (size_t i = 0; i < tmp.size(); ++i) tmp[i] = (float)acc[i];
        PrepArgs pa = e.prep;
        pa.src = tmp.data();
        pa.ld = N;
        launch_attn_prep(pa, nullptr);
        return;
    }
    for (int m = 0; m < M; ++m) {
        if (e.kind == EPI_SWIGLU) {
            for (int n = 0; n < N; n += 32)
                for (int j = 0; j < 16; ++j) {
                    const float g = (float)acc[(size_t)m * N + n + j], u = (float)acc[(size_t)m * N + n + 16 + j];
                    e.c_act[(int64_t)m * e.ldc + (n >> 1) + j] = to_act(af16, silu(g) * u);
                }
            continue;
        }
        for (int n = 0; n < N; ++n) {
            float v = (float)acc[(size_t)m * N + n];
            switch (e.kind) {
                case EPI_STORE_F32:
                    if (e.bias) v += e.bias[n];
                    e.c_f32[(int64_t)m * e.ldc + n] = v;
                    break;
                case EPI_STORE_ACT:
                    if (e.bias) v += e.bias[n];
                    e.c_act[(int64_t)m * e.ldc + n] = to_act(af16, v);
                    break;
                case EPI_RESID_GATED: {
                    const int item = m / e.rows_per_item;
                    float* xp = e.c_f32 + (int64_t)m * e.ldc + n;
                    *xp = *xp + v * e.gate[(int64_t)item * e.gate_stride + n];
                    break;
                }
                case EPI_RESID: e.c_f32[(int64_t)m * e.ldc + n] += v; break;
                case EPI_PROJ_OUT: {
                    const int item = m / e.rows_per_item, pp = m - item * e.rows_per_item;
                    const int kpos = n / e.out_ch, c = n - kpos * e.out_ch, t = pp * e.patch + kpos;
                    if (t < e.out_T) e.c_f32[((int64_t)item * e.out_T + t) * e.out_ch + c] = v + e.bias[c];
                    break;
                }
                default: throw std::runtime_error("emul gemm: bad epilogue");
            }
        }
    }
}

void launch_gemm(ActType t, const uint16_t* A, int lda, const uint16_t* W, int ldw, int M, int N, int K,
                 const GemmEpilogue& epi, hipStream_t s) {
    WeightView w;
    w.fmt = t == ActType::F16 ? WF_F16 : WF_BF16;
    w.q = W;
    w.ld = ldw;
    launch_gemm(A, lda, w, M, N, K, epi, s);
}

// Read the first and last element of the range the real kernel touches, so that an allocation smaller
// than the kernel's footprint (padded rows, lo planes) is an AddressSanitizer report in the host runs.
template <typename T>
void touch(const T* p, int64_t n) {
    if (n <= 0) return;
    volatile T x = p[0];
    x = p[n - 1];
    (void)x;
}

void attn_kh_mode(int) {}

void launch_attention(ActType out_t, const AttnArgs& a, hipStream_t) {
    attn_check_args(a);
    // the real launcher's plan, for a 256-CU device unless the override says otherwise (the environment is not read)
    const AttnPlan plan = attn_plan(attn_shape_of(a), attn_policy_with(attn_policy_default(256), attn_policy_override()));
    const int D = 128, rep = a.Hq / a.Hkv;
    // the partials the split kernels and the merge go through: ksplit planes of O rows, then (max, sum) per row
    if (plan.ksplit > 1) touch(a.part, (int64_t)plan.ksplit * a.B * a.nq * a.Hq * (D + 2));
    {  // attn_kernel footprint: Q rows up to nq_pad, K / V^T tiles up to nk_pad, both planes when split
        const int64_t nq = (int64_t)a.B * a.Hq * a.nq_pad * D, nk = (int64_t)a.B * a.Hkv * a.nk_pad * D;
        touch(a.q, a.split ? a.q_plane + nq : nq);
        touch(a.k, a.split ? a.k_plane + nk : nk);
        touch(a.vt, a.pv_split ? a.v_plane + nk : nk);
        if (a.kbias) touch(a.kbias, (int64_t)a.B * a.nk_pad);
        if (a.out_f32)
            touch(a.out_f32, (int64_t)a.B * a.nq * a.Hq * D);
        else
            touch(a.out, (int64_t)a.B * a.nq * a.Hq * D);
    }
    std::vector<double> s((size_t)a.nk_pad), o((size_t)D);
    auto val = [&](const uint16_t* base, int64_t idx, int64_t plane) {
        double v = f16f(base[idx]);
        if (a.split && plane > 0) v += f16f(base[idx + plane]);
        return v;
    };
    for (int b = 0; b < a.B; ++b)
        for (int h = 0; h < a.Hq; ++h) {
            const int hk = h / rep;
            for (int q = 0; q < a.nq; ++q) {
                const int64_t qb = (((int64_t)b * a.Hq + h) * a.nq_pad + q) * D;
                double mx = -INFINITY;
                for (int k = 0; k < a.nk_pad; ++k) {
                    double bias = a.kbias ? a.kbias[(int64_t)b * a.nk_pad + k] : (k < a.nk ? 0.0 : -INFINITY);
                    if (a.window > 0 && std::abs(q - k) > a.window) bias = -INFINITY;
                    if (a.causal && k > q) bias = -INFINITY;
                    if (std::isinf(bias)) {
                        s[k] = -INFINITY;
                        continue;
                    }
                    const int64_t kb = (((int64_t)b * a.Hkv + hk) * a.nk_pad + k) * D;
                    double dot = 0;
                    for (int d = 0; d < D; ++d) dot += val(a.q, qb + d, a.q_plane) * val(a.k, kb + d, a.k_plane);
                    s[k] = dot * a.scale + bias;
                    mx = std::max(mx, s[k]);
                }
                std::fill(o.begin(), o.end(), 0.0);
                double sum = 0;
                for (int k = 0; k < a.nk_pad; ++k) {
                    if (std::isinf(s[k])) continue;
                    const double p = std::exp(s[k] - mx);
                    sum += p;
                    const int pk = vperm(k % 16) + (k / 16) * 16;  // V^T keys are stored permuted in 16-groups
                    for (int d = 0; d < D; ++d)
                        o[d] += p * val(a.vt, (((int64_t)b * a.Hkv + hk) * D + d) * a.nk_pad + pk,
                                        a.pv_split ? a.v_plane : 0);
                }
                if (a.out_f32) {  // f32 output (quantized-activation mode)
                    float* of = a.out_f32 + ((int64_t)b * a.nq + q) * a.Hq * D + h * D;
                    for (int d = 0; d < D; ++d) of[d] = (float)(o[d] / sum);
                    continue;
                }
                uint16_t* out = a.out + ((int64_t)b * a.nq + q) * a.Hq * D + h * D;
                for (int d = 0; d < D; ++d) out[d] = to_act(out_t == ActType::F16, (float)(o[d] / sum));  // 0/0 -> NaN
            }
        }
}

// ---- quantized-activation mode (kernels/gemm_a8.hip), restated
void launch_quantize_act(int kind, const float* x, int64_t ldx, int M, int K, bool sl, int8_t* q_out, float* s,
                         float* bs, int64_t ld_s, hipStream_t, uint16_t* q16) {
    ACEMI_CHECK(M >= 1 && ld_s >= M && ldx >= K && (q_out || q16), "quantize_act: bad shape");
    ACEMI_CHECK(kind == QACT_Q8_0 || (q_out && !q16), "quantize_act: Q8_K has the int8 form only");
    std::vector<int8_t> qtmp((size_t)K);
    const int QK = kind == QACT_Q8_0 ? 32 : 256;
    ACEMI_CHECK(K % QK == 0, "quantize_act: K");
    for (int m = 0; m < M; ++m)
        for (int b0 = 0; b0 < K; b0 += QK) {
            float v[256];
            float amax = 0.f, mx = 0.f;
            for (int i = 0; i < QK; ++i) {
                v[i] = sl ? silu(x[(int64_t)m * ldx + b0 + i]) : x[(int64_t)m * ldx + b0 + i];
                if (std::fabs(v[i]) > amax) {
                    amax = std::fabs(v[i]);
                    mx = v[i];
                }
            }
            int8_t* qr = q_out ? q_out + (int64_t)m * K + b0 : qtmp.data() + b0;
            if (kind == QACT_Q8_0) {
                const float d = amax / 127.0f, id = amax != 0.f ? 127.0f / amax : 0.f;
                for (int i = 0; i < 32; ++i) qr[i] = (int8_t)std::nearbyint(v[i] * id);
                if (q16)  // bf16(q): the integer exactly
                    for (int i = 0; i < 32; ++i) q16[(int64_t)m * K + b0 + i] = to_bf16((float)qr[i]);
                s[(int64_t)(b0 / 32) * ld_s + m] = f16f(to_f16(d));
                continue;
            }
            const float iscale = amax != 0.f ? -127.0f / mx : 0.f;
            for (int j = 0; j < 8; ++j) {
                int sum = 0;
                for (int i = 32 * j; i < 32 * j + 32; ++i) {
                    qr[i] = amax != 0.f ? (int8_t)std::min(127, (int)std::nearbyint(iscale * v[i])) : 0;
                    sum += qr[i];
                }
                s[(int64_t)(b0 / 32 + j) * ld_s + m] = amax != 0.f ? 1.0f / iscale : 0.f;
                bs[(int64_t)(b0 / 32 + j) * ld_s + m] = (float)sum;
            }
        }
}

static int g_a8_mode = -1;
void gemm_a8_mode(int mode) { g_a8_mode = mode; }
bool gemm_a8_bf16_path(int fmt, int K) {
    const char* e = std::getenv("ACE_MI_QACT_GEMM");
    const int mode = g_a8_mode >= 0 ? g_a8_mode : ((e && e[0] == '0') ? 0 : 1);
    return mode == 1 && fmt == WF_Q8_0 && K % 64 == 0;
}
void launch_q8_image(const int8_t* q, int64_t n, uint16_t* out, hipStream_t) {
    ACEMI_CHECK(n % 16 == 0, "q8_image: n % 16 == 0");
    for (int64_t i = 0; i < n; ++i) out[i] = to_bf16((float)q[i]);
}

void launch_gemm_a8(const QAct& a, const WeightView& W, int M, int N, int K, const GemmEpilogue& e, hipStream_t st,
                    const uint16_t* w16) {
    ACEMI_CHECK(weight_quantized(W.fmt) && a.kind == qact_kind_for(W.fmt), "gemm_a8: format mismatch");
    ACEMI_CHECK(a.q || (a.q16 && w16 && W.fmt == WF_Q8_0 && K % 64 == 0), "gemm_a8: operand forms");
    if (a.q16 && w16) touch(w16, (int64_t)N * K);
    auto aq = [&](int64_t i) { return a.q16 && w16 ? bf16f(a.q16[i]) : (float)a.q[i]; };
    ACEMI_CHECK(M >= 1 && N % 128 == 0 && a.ld_s >= (M + 127) / 128 * 128, "gemm_a8: bad shape");
    touch(a.s, (int64_t)(K / 32 - 1) * a.ld_s + (M + 127) / 128 * 128);
    std::vector<float> acc((size_t)M * N);
    const int nb = K / 32;
    for (int m = 0; m < M; ++m)
        for (int n = 0; n < N; ++n) {
            double sum = 0;
            for (int b = 0; b < nb; ++b) {
                const float da = a.s[(int64_t)b * a.ld_s + m];
                for (int k = 32 * b; k < 32 * b + 32; ++k) {
                    float w;  // the dequantized weight element in f32 (not rounded to bf16)
                    if (W.fmt == WF_Q8_0) {
                        const float qw = a.q16 && w16 ? bf16f(w16[(int64_t)n * K + k]) : (float)((const int8_t*)W.q)[(int64_t)n * K + k];
                        w = qw * W.s[(int64_t)n * nb + b];
                    } else if (W.fmt == WF_Q6_K) {
                        w = (float)((const int8_t*)W.q)[(int64_t)n * K + k] * W.s[(int64_t)n * (K / 16) + k / 16];
                    } else {
                        const int i = k % 32, dw = i / 8, r = i % 8;
                        const uint8_t byte = ((const uint8_t*)W.q)[(int64_t)n * (K / 2) + b * 16 + dw * 4 + (r & 3)];
                        const int qv = r < 4 ? (byte & 0xF) : (byte >> 4);
                        const float* sm = W.s + ((int64_t)n * nb + b) * 2;
                        w = (float)qv * sm[0] - sm[1];
                    }
                    sum += (double)aq((int64_t)m * K + k) * da * w;
                }
            }
            acc[(size_t)m * N + n] = (float)sum;
        }
    if (e.kind == EPI_QKV_PREP) {
        PrepArgs pa = e.prep;
        pa.src = acc.data();
        pa.ld = N;
        launch_attn_prep(pa, st);
        return;
    }
    for (int m = 0; m < M; ++m) {
        if (e.kind == EPI_SWIGLU_F32 || e.kind == EPI_SWIGLU) {
            for (int n = 0; n < N; n += 32)
                for (int j = 0; j < 16; ++j) {
                    const float g = acc[(size_t)m * N + n + j], u = acc[(size_t)m * N + n + 16 + j];
                    if (e.kind == EPI_SWIGLU_F32)
                        e.c_f32[(int64_t)m * e.ldc + (n >> 1) + j] = silu(g) * u;
                    else
                        e.c_act[(int64_t)m * e.ldc + (n >> 1) + j] = to_bf16(silu(g) * u);
                }
            continue;
        }
        for (int n = 0; n < N; ++n) {
            float v = acc[(size_t)m * N + n];
            switch (e.kind) {
                case EPI_STORE_F32:
                    e.c_f32[(int64_t)m * e.ldc + n] = e.bias ? v + e.bias[n] : v;
                    break;
                case EPI_RESID_GATED: {
                    if (e.bias) v += e.bias[n];
                    float* xp = e.c_f32 + (int64_t)m * e.ldc + n;
                    *xp = *xp + v * e.gate[(int64_t)(m / e.rows_per_item) * e.gate_stride + n];
                    break;
                }
                case EPI_RESID:
                    e.c_f32[(int64_t)m * e.ldc + n] += e.bias ? v + e.bias[n] : v;
                    break;
                case EPI_PROJ_OUT: {
                    const int item = m / e.rows_per_item, pp = m - item * e.rows_per_item;
                    const int kpos = n / e.out_ch, c = n - kpos * e.out_ch, t = pp * e.patch + kpos;
                    if (t < e.out_T) e.c_f32[((int64_t)item * e.out_T + t) * e.out_ch + c] = v + e.bias[c];
                    break;
                }
                default: throw std::runtime_error("emul gemm_a8: bad epilogue");
            }
        }
    }
}

void launch_rmsnorm_mod_f32(const float* x, int M, int H, const float* w, const float* scale, const float* shift,
                            int64_t mod_stride, int rows_per_item, float eps, float* out, hipStream_t) {
    for (int m = 0; m < M; ++m) {
        const float* xr = x + (int64_t)m * H;
        double ss = 0;
        for (int i = 0; i < H; ++i) ss += (double)xr[i] * xr[i];
        const float sc = 1.0f / sqrtf((float)(ss / H) + eps);
        const int item = m / rows_per_item;
        for (int i = 0; i < H; ++i) {
            float y = xr[i] * sc * w[i];
            if (scale) y = y * (scale[(int64_t)item * mod_stride + i] + 1.0f) + shift[(int64_t)item * mod_stride + i];
            out[(int64_t)m * H + i] = y;
        }
    }
}

void launch_pack_input_f32(const float* hidden, const float* context, int B, int T, int Np, int P, int audio, int cdim,
                           float* out, hipStream_t) {
    const int cin = audio + cdim;
    for (int b = 0; b < B; ++b)
        for (int p = 0; p < Np; ++p)
            for (int k = 0; k < P; ++k)
                for (int c = 0; c < cin; ++c) {
                    const int tt = p * P + k;
                    float v = 0.f;
                    if (tt < T) {
                        if (c < cdim) {
                            if (context) v = context[((int64_t)b * T + tt) * cdim + c];
                        } else if (hidden) {
                            v = hidden[((int64_t)b * T + tt) * audio + (c - cdim)];
                        }
                    }
                    out[((int64_t)b * Np + p) * P * cin + (int64_t)k * cin + c] = v;
                }
}

void launch_pack_input(ActType t, const float* hidden, const float* context, int B, int T, int Np, int P, int audio,
                       int cdim, uint16_t* out, hipStream_t, bool x3) {
    const int cin = audio + cdim, rowlen = P * cin;
    for (int b = 0; b < B; ++b)
        for (int p = 0; p < Np; ++p)
            for (int k = 0; k < P; ++k)
                for (int c = 0; c < cin; ++c) {
                    const int tt = p * P + k;
                    float v = 0.f;
                    if (tt < T) {
                        if (c < cdim) {
                            if (context) v = context[((int64_t)b * T + tt) * cdim + c];
                        } else if (hidden) {
                            v = hidden[((int64_t)b * T + tt) * audio + (c - cdim)];
                        }
                    }
                    const int64_t row = (int64_t)b * Np + p, col = (int64_t)k * cin + c;
                    if (x3) {
                        uint16_t* o = out + row * 3 * rowlen + col;
                        o[0] = o[rowlen] = to_f16(v);
                        o[2 * rowlen] = to_f16(v - f16f(o[0]));
                    } else {
                        out[row * rowlen + col] = to_act(t == ActType::F16, v);
                    }
                }
}

void launch_to_act(ActType t, const float* in, int64_t n, bool sl, uint16_t* out, hipStream_t) {
    for (int64_t i = 0; i < n; ++i) out[i] = to_act(t == ActType::F16, sl ? silu(in[i]) : in[i]);
}

void launch_rmsnorm_mod(ActType t, const float* x, int M, int H, const float* w, const float* scale, const float* shift,
                        int64_t mod_stride, int rows_per_item, float eps, uint16_t* out, hipStream_t, bool x3) {
    for (int m = 0; m < M; ++m) {
        const float* xr = x + (int64_t)m * H;
        double ss = 0;
        for (int i = 0; i < H; ++i) ss += (double)xr[i] * xr[i];
        const float sc = 1.0f / sqrtf((float)(ss / H) + eps);
        const int item = m / rows_per_item;
        uint16_t* o = out + (int64_t)m * H * (x3 ? 3 : 1);
        for (int i = 0; i < H; ++i) {
            float y = xr[i] * sc * w[i];
            if (scale) y = y * (scale[(int64_t)item * mod_stride + i] + 1.0f) + shift[(int64_t)item * mod_stride + i];
            if (x3) {
                o[i] = o[H + i] = to_f16(y);
                o[2 * H + i] = to_f16(y - f16f(o[i]));
            } else {
                o[i] = to_act(t == ActType::F16, y);
            }
        }
    }
}

void launch_rmsnorm_f32(const float* x, int rows, int64_t row_step, int H, const float* w, float eps, float* out,
                        hipStream_t) {
    for (int m = 0; m < rows; ++m) {
        const float* xr = x + (int64_t)m * row_step * H;
        double ss = 0;
        for (int i = 0; i < H; ++i) ss += (double)xr[i] * xr[i];
        const float sc = 1.0f / sqrtf((float)(ss / H) + eps);
        for (int i = 0; i < H; ++i) out[(int64_t)m * H + i] = xr[i] * sc * w[i];
    }
}

void launch_embed_rows(const void* table, int fmt, const int32_t* ids, int n, int H, float* out, hipStream_t) {
    for (int t = 0; t < n; ++t)
        for (int i = 0; i < H; ++i) {
            const int64_t k = (int64_t)ids[t] * H + i;
            float v;
            if (fmt == 2) {
                v = ((const float*)table)[k];
            } else if (fmt == 0) {
                const uint32_t u = (uint32_t)((const uint16_t*)table)[k] << 16;
                std::memcpy(&v, &u, 4);
            } else {
                v = f16f(((const uint16_t*)table)[k]);
            }
            out[(int64_t)t * H + i] = v;
        }
}

void launch_attn_prep(const PrepArgs& a, hipStream_t) {
    if (a.layers > 1) {  // PrepArgs::layers: the layers one after another
        for (int l = 0; l < a.layers; ++l) {
            PrepArgs p = a;
            p.layers = 1;
            p.src += l * a.src_layer;
            p.kh += l * a.kh_layer;
            p.vt += l * a.vt_layer;
            p.k_norm = a.k_norm_layers[l];
            launch_attn_prep(p, nullptr);
        }
        return;
    }
    auto head = [&](bool isq, int b, int h) {
        const float* w = isq ? a.q_norm : a.k_norm;
        const int col = (isq ? a.q_col : a.k_col) + h * 128;
        uint16_t* base = isq ? a.qh + ((int64_t)b * a.hq + h) * a.n_pad * 128 : a.kh + ((int64_t)b * a.hkv + h) * a.n_pad * 128;
        const int64_t plane = isq ? a.q_plane : a.k_plane;
        for (int n = 0; n < a.n_pad; ++n) {
            float y[128] = {};
            if (n < a.n_tok) {
                const float* row = a.src + ((int64_t)b * a.n_tok + n) * a.ld + col;
                float ss = 0;
                for (int d = 0; d < 128; ++d) ss += row[d] * row[d];
                const float sc = 1.0f / sqrtf(ss / 128.0f + a.eps);
                for (int d = 0; d < 128; ++d) y[d] = w ? row[d] * sc * w[d] : row[d];
                if (a.rope_cos) {
                    for (int d = 0; d < 64; ++d) {
                        const float c = a.rope_cos[(int64_t)n * 64 + d], s = a.rope_sin[(int64_t)n * 64 + d];
                        const float y0 = y[d], y1 = y[d + 64];
                        y[d] = y0 * c - y1 * s;
                        y[d + 64] = y0 * s + y1 * c;
                    }
                }
            }
            uint16_t* dst = base + (int64_t)n * 128;
            for (int d = 0; d < 128; ++d) {
                dst[d] = to_f16(y[d]);
                if (plane > 0) dst[plane + d] = to_f16(y[d] - f16f(dst[d]));
            }
        }
    };
    for (int b = 0; b < a.B; ++b) {
        if (a.q_col >= 0)
            for (int h = 0; h < a.hq; ++h) head(true, b, h);
        if (a.k_col >= 0)
            for (int h = 0; h < a.hkv; ++h) head(false, b, h);
        if (a.v_col >= 0)
            for (int h = 0; h < a.hkv; ++h)
                for (int d = 0; d < 128; ++d) {
                    uint16_t* dst = a.vt + (((int64_t)b * a.hkv + h) * 128 + d) * a.n_pad;
                    for (int p = 0; p < a.n_pad; ++p) {
                        const int n = (p / 16) * 16 + vperm(p % 16);
                        const float v = n < a.n_tok ? a.src[((int64_t)b * a.n_tok + n) * a.ld + a.v_col + h * 128 + d] : 0.f;
                        dst[p] = to_f16(v);
                        if (a.v_plane > 0) dst[a.v_plane + p] = to_f16(v - f16f(dst[p]));
                    }
                }
    }
}

void launch_key_bias(const int32_t* mask, int B, int frames, int patch, int nk, int nk_pad, float* kbias, hipStream_t) {
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < nk_pad; ++k) {
            bool ok = k < nk;
            if (ok && mask) {
                bool any = false;
                for (int j = 0; j < patch; ++j) {
                    const int f = k * patch + j;
                    if (f < frames && mask[(int64_t)b * frames + f] != 0) any = true;
                }
                ok = any;
            }
            kbias[(int64_t)b * nk_pad + k] = ok ? 0.f : -INFINITY;
        }
}

void launch_timestep_freq(const float* t, const float* r, int B, int dim, float scale, float log_max, float* f,
                          hipStream_t) {
    const int half = dim / 2;
    for (int b = 0; b < B; ++b) {
        float tv = t[b];
        if (r) tv = tv - r[b];
        const float ts = tv * scale;
        for (int i = 0; i < half; ++i) {
            const float arg = ts * (float)std::exp((double)((-log_max * (float)i) / (float)half));
            f[(int64_t)b * dim + i] = (float)std::cos((double)arg);
            f[(int64_t)b * dim + i + half] = (float)std::sin((double)arg);
        }
        if (dim & 1) f[(int64_t)b * dim + dim - 1] = 0.f;
    }
}

void launch_gemv(ActType t, const uint16_t* x, int M, const uint16_t* W, int N, int K, const float* bias, bool sl,
                 bool accumulate, float* y, hipStream_t) {
    const bool f16 = t == ActType::F16;
    for (int m = 0; m < M; ++m)
        for (int n = 0; n < N; ++n) {
            double s = 0;
            for (int k = 0; k < K; ++k) s += (double)act_val(f16, x[(int64_t)m * K + k]) * act_val(f16, W[(int64_t)n * K + k]);
            float v = (float)s;
            if (bias) v += bias[n];
            if (sl) v = silu(v);
            float* yp = y + (int64_t)m * N + n;
            *yp = accumulate ? *yp + v : v;
        }
}

void launch_gemv_f32(ActType t, const float* x, bool silu_in, int M, const uint16_t* W, int N, int K, const float* bias,
                     bool sl, bool accumulate, float* y, hipStream_t) {
    std::vector<uint16_t> xa((size_t)M * K);
    launch_to_act(t, x, (int64_t)M * K, silu_in, xa.data(), nullptr);
    launch_gemv(t, xa.data(), M, W, N, K, bias, sl, accumulate, y, nullptr);
}

void launch_layer_mods(const float* tables, const float* proj, int L, int B, int H, float* mod, hipStream_t) {
    for (int l = 0; l < L; ++l)
        for (int b = 0; b < B; ++b)
            for (int j = 0; j < 6; ++j)
                for (int c = 0; c < H; ++c)
                    mod[(((int64_t)l * B + b) * 6 + j) * H + c] = tables[((int64_t)l * 6 + j) * H + c] + proj[((int64_t)b * 6 + j) * H + c];
}

void launch_out_mods(const float* table, const float* tt, const float* tr, int B, int H, float* om, hipStream_t) {
    for (int b = 0; b < B; ++b)
        for (int j = 0; j < 2; ++j)
            for (int c = 0; c < H; ++c)
                om[((int64_t)b * 2 + j) * H + c] = table[(int64_t)j * H + c] + (tt[(int64_t)b * H + c] + tr[(int64_t)b * H + c]);
}

void gemm_splitk_check() {}
void gemm_splitk_release(hipStream_t) {}

void launch_fault_tile(float* x, int ld, int rows, int row0, int col0, float amp, hipStream_t) {
    for (int r = row0; r < row0 + 16 && r < rows; ++r)
        for (int c = col0; c < col0 + 128; ++c) x[(int64_t)r * ld + c] += amp;
}

// the weight prefetch only warms caches: nothing to restate
void launch_prefetch(const void* const*, const size_t*, int, int, unsigned*, hipStream_t) {}

void launch_euler(float* xt, const float* v, int64_t n, float dt, hipStream_t) {
    for (int64_t i = 0; i < n; ++i) xt[i] = xt[i] - v[i] * dt;
}

void launch_sde(float* xt, const float* v, const float* noise, int64_t n, float t, float t_next, hipStream_t) {
    for (int64_t i = 0; i < n; ++i) {
        const float x0 = xt[i] - v[i] * t;
        xt[i] = t_next * noise[i] + (1.0f - t_next) * x0;
    }
}

// ---------------------------------------------------------------- VAE
void launch_conv_gemm(const ConvGemmArgs& a, hipStream_t) {
    ACEMI_CHECK(a.Cin % 64 == 0 && a.N % 128 == 0 && a.M >= 1 && a.taps >= 1, "conv_gemm: unsupported shape");
    // the rest of what the kernel's launch refuses
    ACEMI_CHECK(a.S && a.W && a.zero, "conv_gemm: null operand");
    ACEMI_CHECK(a.up <= 1 || a.N == a.up * a.Cout, "conv_gemm: transposed conv needs N = stride * Cout");
    ACEMI_CHECK(a.up > 1 || a.N == a.Cout, "conv_gemm: N must equal Cout");
    ACEMI_CHECK(!(a.resid || a.store_x) || a.X, "conv_gemm: null X");
    ACEMI_CHECK(a.items >= 1 && a.M % a.items == 0, "conv_gemm: rows must split evenly into the sequences");
    ACEMI_CHECK(a.Cout % 4 == 0, "conv_gemm: output channels must be a multiple of 4");
    if (a.W2)
        ACEMI_CHECK(a.N == 128 && a.Cout == 128 && a.up <= 1 && a.snake2_ea && a.snake2_eb,
                    "conv_gemm: the fused k1 conv needs Cout = N = 128 and a Snake between the convs");
    // out-of-range rows are staged from the zero buffer: 64 halves (chunk * 8, chunk < 8) by the generic staging,
    // 128 halves (hc * 8, hc < 16) by the halo staging; an epilogue without a residual reads 4 floats of it
    touch(a.zero, 128);
    const int K = a.taps * a.Cin;
    const int Mi = a.M / a.items;
    std::vector<float> row((size_t)K);
    for (int mg = 0; mg < a.M; ++mg) {
        const int item = mg / Mi, m = mg - item * Mi;
        const uint16_t* S = a.S + (int64_t)item * a.T_in * a.Cin;
        const int64_t obase = (int64_t)item * a.T_out;
        for (int tap = 0; tap < a.taps; ++tap) {
            const int t = m * a.in_stride + tap * a.dil - a.pad;
            for (int c = 0; c < a.Cin; ++c)
                row[(size_t)tap * a.Cin + c] = (t >= 0 && t < a.T_in) ? f16f(S[(int64_t)t * a.Cin + c]) : 0.f;
        }
        std::vector<float> z;  // fused k1 conv: z = W2 . fp16(Snake2(acc + bias)) (ConvGemmArgs::W2)
        if (a.W2) {
            std::vector<float> y((size_t)a.N);
            for (int n = 0; n < a.N; ++n) {
                double s = 0;
                const uint16_t* w = a.W + (int64_t)n * K;
                for (int k = 0; k < K; ++k) s += (double)row[k] * f16f(w[k]);
                const float v = (float)s + (a.bias ? a.bias[n] : 0.f);
                const float sv = sinf(a.snake2_ea[n] * v);
                y[n] = f16f(to_f16(v + (sv * sv) / a.snake2_eb[n]));
            }
            z.resize((size_t)a.N);
            for (int n = 0; n < a.N; ++n) {
                double s = 0;
                for (int k = 0; k < a.N; ++k) s += (double)y[k] * f16f(a.W2[(int64_t)n * a.N + k]);
                z[n] = (float)s;
            }
        }
        for (int n = 0; n < a.N; ++n) {
            double s = 0;
            if (a.W2) {
                s = z[n];
            } else {
                const uint16_t* w = a.W + (int64_t)n * K;
                for (int k = 0; k < K; ++k) s += (double)row[k] * f16f(w[k]);
            }
            int u, co;
            if (a.up > 1) {
                const int rr = n / a.Cout;
                co = n - rr * a.Cout;
                u = m * a.up + rr - a.crop;
            } else {
                co = n;
                u = m;
            }
            if (u < 0 || u >= a.T_out) continue;
            float v = (float)s;
            const float* bias = a.W2 ? a.bias2 : a.bias;
            if (bias) v += bias[co];
            const int64_t o = (obase + u) * a.Cout + co;
            if (a.resid) v = a.X[o] + v;
            if (a.store_x) a.X[o] = v;
            if (a.S_out) {
                float y = v;
                if (a.snake_ea) {
                    float sv = sinf(a.snake_ea[co] * v);
                    y = v + (sv * sv) / a.snake_eb[co];
                }
                a.S_out[o] = to_f16(y);
            }
        }
    }
}

void launch_to_f16(const float* x, int64_t n, uint16_t* y, hipStream_t) {
    for (int64_t i = 0; i < n; ++i) y[i] = to_f16(x[i]);
}

void launch_pack_f16(const float* x, int64_t rows, int C, int Cpad, uint16_t* y, hipStream_t) {
    for (int64_t r = 0; r < rows; ++r)
        for (int c = 0; c < Cpad; ++c) y[r * Cpad + c] = c < C ? to_f16(x[r * C + c]) : (uint16_t)0;
}

void launch_conv_out(const uint16_t* S0, int T, int C, const uint16_t* W, int out_ch, float* out0, hipStream_t,
                     int items) {
    for (int item = 0; item < items; ++item) {
        const uint16_t* S = S0 + (int64_t)item * T * C;
        float* out = out0 + (int64_t)item * T * out_ch;
        for (int t = 0; t < T; ++t)
            for (int o = 0; o < out_ch; ++o) {
                double s = 0;
                for (int k = 0; k < 7; ++k) {
                    const int ti = t + k - 3;
                    if (ti < 0 || ti >= T) continue;
                    for (int c = 0; c < C; ++c)
                        s += (double)f16f(S[(int64_t)ti * C + c]) * f16f(W[((int64_t)o * 7 + k) * C + c]);
                }
                out[(int64_t)t * out_ch + o] = (float)s;
            }
    }
}

}  // namespace acemi
