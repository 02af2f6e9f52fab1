// Host-side launch wrappers for the gfx950 kernels (all stream-ordered, no
// allocation, no synchronisation: safe to capture into a hipGraph).
#pragma once

#include <cstdlib>
#include <stdexcept>
#include <string>

#include "attn_plan.h"
#include "common.h"

namespace acemi {

// Per-head RMSNorm (+ NEOX RoPE) of the q/k sections and f16 re-layout for attention.
struct PrepArgs {
    const float* src;
    int ld;
    int q_col, k_col, v_col;  // -1: section absent
    int hq, hkv;
    int n_tok, n_pad, B;
    const float* q_norm;
    const float* k_norm;
    const float* rope_cos;  // [n_tok][64] or null
    const float* rope_sin;
    float eps;
    uint16_t* qh;
    uint16_t* kh;
    uint16_t* vt;
    int64_t q_plane = 0, k_plane = 0, v_plane = 0;  // >0: also write lo = f16(x - f16(x)) planes
    int f8 = 0;  // 1: the lo planes hold the fp8 operands of the f8c attention mode instead (prep_math.h)
    // > 1 (k / v sections only): one launch for `layers` consecutive layers, layer l reading src + l*src_layer,
    // writing kh + l*kh_layer / vt + l*vt_layer, normalising by k_norm_layers[l] (a device table)
    int layers = 1;
    int64_t src_layer = 0, kh_layer = 0, vt_layer = 0;
    const float* const* k_norm_layers = nullptr;
};

// ---------------------------------------------------------------- GEMM
// C[M][N] = A[M][K] . W[N][K]^T   (A, W: 16-bit act type, f32 accumulate)
// followed by a fused epilogue.  N % 128 == 0, K % 64 == 0, M >= 1.
enum GemmEpiKind : int {
    EPI_STORE_F32 = 0,      // c_f32[m*ldc+n] = acc (+ bias[n])
    EPI_STORE_ACT = 1,      // c_act[m*ldc+n] = act(acc (+ bias[n]))
    EPI_RESID_GATED = 2,    // c_f32[m*ldc+n] += acc * gate[(m / rows_per_item)*gate_stride + n]
    EPI_RESID = 3,          // c_f32[m*ldc+n] += acc
    EPI_SWIGLU = 4,         // columns interleaved [g0..15,u0..15,g16..]: c_act[m*ldc + n'] = act(silu(g)*u)
    EPI_PROJ_OUT = 5,       // c_f32[b][2p+k][c] = acc[m=(b,p)][n = c + k*out_ch] + bias[c], cropped to T
    EPI_QKV_PREP = 6,       // attn_prep fused: column tile n0/128 = one head of [q heads | k heads | v heads]
                            // (sections present per prep.q_col / k_col / v_col >= 0), written straight into
                            // the attention layouts of `prep` (QK-RMSNorm, RoPE, fp16 hi/lo, V^T); 128-wide
                            // column tiles only, no bias
    EPI_SWIGLU_F32 = 7,     // EPI_SWIGLU with an f32 output c_f32 (the quantized-activation GEMM only)
};

struct GemmEpilogue {
    int kind = EPI_STORE_F32;
    const float* bias = nullptr;
    float* c_f32 = nullptr;
    uint16_t* c_act = nullptr;
    int ldc = 0;
    const float* gate = nullptr;
    int64_t gate_stride = 0;
    int rows_per_item = 1;
    int out_T = 0;        // EPI_PROJ_OUT: frames per item
    int out_ch = 0;       // EPI_PROJ_OUT: channels (64)
    int patch = 2;        // EPI_PROJ_OUT
    PrepArgs prep{};      // EPI_QKV_PREP (src / ld unused)
};

// Weight operand.  Dense: 16-bit [N][ld] in the activation type.  Quantized (ggml block formats
// re-laid out at load, runtime/quant.h): q = int8 / nibble plane, s = f32 scales; the kernel
// dequantizes each 32-value block to bf16 while staging it into LDS and multiplies it with a bf16
// activation (`Q -> bf16 dequant-fused` MFMA GEMM).
// WF_F32X3: an F32 weight as the fp16 triple [hi | lo | hi] along K (ld = 3K), multiplied with an
// activation written as [hi | hi | lo] (Ah.Wh + Ah.Wl + Al.Wh) by the plain fp16 GEMM over 3K.
// WF_GGML_RAW: raw ggml block rows exactly as the GGUF file holds them, as a list of row segments (BlockSeg below),
// each with its own ggml type.  No GEMM reads this format: launch_dequant_blocks expands it to the dense bf16 image
// first (the staged-dequant scopes of runtime/engine.h), and a bf16 activation multiplies that image.
enum WeightFormat : int {
    WF_BF16 = 0, WF_F16 = 1, WF_Q8_0 = 2, WF_Q4_K = 3, WF_Q6_K = 4, WF_F32X3 = 5, WF_GGML_RAW = 6
};
struct BlockSeg;
struct WeightView {
    int fmt = WF_BF16;
    const void* q = nullptr;   // dense uint16 [N][ld] | Q8_0/Q6_K int8 [N][K] | Q4_K u8 [N][K/2] | raw: the blocks
    const float* s = nullptr;  // Q8_0 [N][K/32] | Q4_K [N][K/32][2] (d*sc, dmin*m) | Q6_K [N][K/16]
    int ld = 0;                // dense leading dimension (elements)
    const BlockSeg* segs = nullptr;  // WF_GGML_RAW: the matrix's row segments (host array owned by the DevWeight)
    int n_segs = 0;
};
inline ActType weight_act(int fmt) { return (fmt == WF_F16 || fmt == WF_F32X3) ? ActType::F16 : ActType::BF16; }
inline bool weight_quantized(int fmt) { return fmt >= WF_Q8_0; }
inline bool weight_planes(int fmt) { return fmt == WF_Q8_0 || fmt == WF_Q4_K || fmt == WF_Q6_K; }

void launch_gemm(const uint16_t* A, int lda, const WeightView& W, int M, int N, int K, const GemmEpilogue& epi,
                 hipStream_t s);
// dense shorthand: W 16-bit of type t
void launch_gemm(ActType t, const uint16_t* A, int lda, const uint16_t* W, int ldw, int M, int N, int K,
                 const GemmEpilogue& epi, hipStream_t s);
// -1 = automatic tile choice; else force a variant of gemm_variants.h (dense ids 0..16 and 18, quantized 0..5, 7 and
// 20..25, + 100 * S for split-K over S = 2..4 blocks per tile) wherever it handles the shape (micro-benchmarks / tests)
void gemm_force_variant(int v);
// Throws (once) if a split-K GEMM join on the current device timed out since the last check: reads a per-device
// host-pinned error word, no stream is synchronised (called at the library's synchronisation points and on entry).
void gemm_splitk_check();
// free the split-K workspace of stream s on the current device (before the owner destroys s)
void gemm_splitk_release(hipStream_t s);
// bf16 image [N][K] (ld K) of a quantized weight: bit-identical to what the dequant-fused GEMM feeds its MFMAs
void launch_dequant_bf16(const WeightView& W, int N, int K, uint16_t* out, hipStream_t s);
// the same for 1..8 matrices of one format in one launch
struct DequantJob {
    WeightView w;
    int N = 0, K = 0;
    uint16_t* out = nullptr;
};
void launch_dequant_bf16_batch(const DequantJob* jobs, int n, hipStream_t s);

// ------------------------------------------------- raw ggml blocks -> bf16 image (kernels/dequant_blocks.hip)
// One run of `rows` consecutive block rows of one ggml type (runtime/gguf.h ids: Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q2_K,
// Q3_K, Q4_K, Q5_K, Q6_K, IQ4_NL), source row r at src + r * row_bytes, expanded to output row
//   row0 + (r / group) * group * step + r % group
// of a dense bf16 matrix [.][ld] with K values per row: step 1 = a concatenated part starting at row0; step 2 with
// group 16 and row0 = 0 / 16 = the gate / up rows of the interleaved w_gu.  Every value is rne_bf16 of ggml's CPU
// dequantize_row_* f32 value (runtime/quant.h) -- for Q8_0 / Q4_K / Q6_K the bits of launch_dequant_bf16 on the same
// blocks, whose zeros are always +0.  src is 16-byte aligned and readable up to the next 16-byte boundary
// after its last block (the kernel stages whole aligned 16-byte words); out is 16-byte aligned, K % 8 == 0 beyond
// K % block == 0, ld % 8 == 0.
struct BlockSeg {
    int type = 0;            // ggml type id
    const void* src = nullptr;
    int rows = 0;
    int row0 = 0, step = 1, group = 1;
};
inline int block_seg_row(const BlockSeg& g, int r) { return g.row0 + (r / g.group) * g.group * g.step + r % g.group; }
struct DequantBlocksJob {
    BlockSeg seg;
    int K = 0;
    int64_t ld = 0;
    uint16_t* out = nullptr;
};
// any number of jobs: grouped by type, up to 8 jobs per launch; jobs of one call must not write the same rows
void launch_dequant_blocks(const DequantBlocksJob* jobs, int n, hipStream_t s);

// ------------------------------------------------- LoRA merge (kernels/lora.hip)
// The adapted 16-bit image of a (possibly fused) weight matrix: for module row o and column i
//   acc = 0; for j = 0 .. r-1 ascending: acc = acc + B[o][j] * A[j][i]   (multiply and add each rounded to f32,
//   never contracted);  t = eff * acc;  out = rne16(f32(base) + t)  in the matrix's own 16-bit format,
// so numpy restates it bit for bit (acestep_mi355x/synthetic.py lora_delta_bits).  A job covers the fused rows
// [row0, row0 + rows) of base / out; the row map places module row o at a fused row inside that range, and the
// rows of the range that the map does not reach are copied from base when copy_rest is set (left untouched
// otherwise).  out == base (in place) is allowed; columns >= cols of a row and rows outside the range are never
// written.  cols, ld_base, ld_out % 8 == 0 and 16-byte aligned base / out / A (16-byte accesses on the matrix).
enum LoraRowMap : int {
    LORA_ROWS_PLAIN = 0,       // fused row = row_off + o (row_off: the module's offset inside a q|k|v or k|v concatenation)
    LORA_ROWS_INTERLEAVE = 1,  // w_gu: fused row = (o / 16) * 32 + half * 16 + o % 16 (half 0 = gate, 1 = up)
};
struct LoraMergeJob {
    int fmt = WF_BF16;  // WF_BF16 | WF_F16, of base and out
    const uint16_t* base = nullptr;
    int64_t ld_base = 0;
    uint16_t* out = nullptr;
    int64_t ld_out = 0;
    int row0 = 0, rows = 0, cols = 0;
    const float* A = nullptr;  // [r][cols]; null (r = 0): no module, the whole range is copy-through
    const float* B = nullptr;  // [rows_mod][r]
    int r = 0, rows_mod = 0;
    float eff = 0.f;
    int map = LORA_ROWS_PLAIN;
    int row_off = 0;  // LORA_ROWS_PLAIN
    int half = 0;     // LORA_ROWS_INTERLEAVE
    bool copy_rest = false;
};
constexpr int LORA_MAX_RANK = 128;
// module row of fused row fr, or -1 when fr belongs to no row of the job's module
__host__ __device__ inline int lora_module_row(int map, int row_off, int half, int rows_mod, int r, int fr) {
    if (r <= 0) return -1;
    int o;
    if (map == LORA_ROWS_INTERLEAVE) {
        if (((fr >> 4) & 1) != half) return -1;
        o = (fr >> 5) * 16 + (fr & 15);
    } else {
        o = fr - row_off;
    }
    return (o >= 0 && o < rows_mod) ? o : -1;
}
// fused row of module row o (the inverse of lora_module_row)
__host__ __device__ inline int lora_fused_row(int map, int row_off, int half, int o) {
    return map == LORA_ROWS_INTERLEAVE ? (o >> 4) * 32 + half * 16 + (o & 15) : row_off + o;
}
// any number of jobs (launches of up to 8 jobs each); jobs of one call must not write the same rows
void launch_lora_merge(const LoraMergeJob* jobs, int n, hipStream_t s);

// ------------------------------------------------- ggml-faithful quantized activations (kernels/gemm_a8.hip)
// ggml's mul_mat against a quantized weight first converts the f32 activation rows to the weight's vec_dot_type
// (Q8_0 blocks for Q8_0 weights, Q8_K for K-quants) and takes integer dot products per block
// (ggml-metal-embed.metal:222-227, 3110-3128; ggml-cpu quantize_row_q8_0 / quantize_row_q8_K_ref / vec_dot_*).
// ACE_MI_QUANT_ACT=q8 runs the DiT that way (the QACT arm of DitEngine::walk, runtime/engine_qact.cpp).
// Activation blocks on the device: q int8 [M][K]; s f32 [K/32][ld_s] per 32-value block (Q8_0: fp16(d);
// Q8_K: the 256-block's d in each of its eight 32-blocks); bsum f32 [K/32][ld_s] = sum of the block's q (Q8_K
// only: the Q4_K min term).  ld_s >= M rounded up to 128 (the GEMM reads whole 128-row tiles of s / bsum).
enum QActKind : int { QACT_Q8_0 = 0, QACT_Q8_K = 1 };
struct QAct {
    int kind = QACT_Q8_0;
    const int8_t* q = nullptr;
    const uint16_t* q16 = nullptr;  // Q8_0: bf16(q) [M][K] (exact integers) for the bf16-MFMA form of the GEMM
    const float* s = nullptr;
    const float* bsum = nullptr;
    int64_t ld_s = 0;
};
inline int qact_kind_for(int weight_fmt) { return weight_fmt == WF_Q8_0 ? QACT_Q8_0 : QACT_Q8_K; }
// x f32 [M][ldx] (silu first when silu_in) -> the blocks of `kind` in q / s / bsum (layout above)
// (q16: Q8_0 only, bf16(q) rows as well / instead -- either output may be null, not both)
void launch_quantize_act(int kind, const float* x, int64_t ldx, int M, int K, bool silu_in, int8_t* q, float* s,
                         float* bsum, int64_t ld_s, hipStream_t st, uint16_t* q16 = nullptr);
// C = dequant(A blocks) . dequant(W)^T with ggml's per-block integer dot products (v_mfma_i32_16x16x32_i8) and an
// f32 sum of d_w * d_a * isum over the blocks; W quantized (WF_Q8_0 with QACT_Q8_0, WF_Q4_K / WF_Q6_K with
// QACT_Q8_K); the epilogues of launch_gemm plus EPI_SWIGLU_F32 (a bias on EPI_RESID adds to the product first).
// N % 128 == 0, K % 32 (Q8_0) / % 256 (K-quants) == 0.
// With a.q16 and w16 (the bf16(q) image of W's int8 plane, launch_q8_image) a Q8_0 GEMM runs on the bf16 MFMA
// (gemm_a8s_kernel: each 32-value block's integer dot is exact there; same bits as the i8 kernel), K % 64 == 0.
void launch_gemm_a8(const QAct& a, const WeightView& W, int M, int N, int K, const GemmEpilogue& epi, hipStream_t s,
                    const uint16_t* w16 = nullptr);
// int8 plane [n] -> bf16 image [n] (exact integers), n % 16 == 0
void launch_q8_image(const int8_t* q, int64_t n, uint16_t* out, hipStream_t s);
// whether the q8 mode runs a GEMM with this weight format / depth on the bf16 MFMA: ACE_MI_QACT_GEMM=0 (or
// gemm_a8_mode(0)) keeps every one on the i8 kernel; gemm_a8_mode(-1) = the environment / default (on)
bool gemm_a8_bf16_path(int fmt, int K);
void gemm_a8_mode(int mode);
// launch_rmsnorm_mod's operator with an f32 output [M][H]
void launch_rmsnorm_mod_f32(const float* x, int M, int H, const float* w, const float* scale, const float* shift,
                            int64_t mod_stride, int rows_per_item, float eps, float* out, hipStream_t s);
// launch_pack_input's packing with f32 output [B*Np][P*Cin]
void launch_pack_input_f32(const float* hidden, const float* context, int B, int T, int Np, int P, int audio_dim,
                           int ctx_dim, float* out, hipStream_t s);

// ------------------------------------------------------------ attention
// Flash-style fp16 attention, f32 softmax/accumulate.  D = 128.
// Qh [B][Hq][nq_pad][128] f16, Kh [B][Hkv][nk_pad][128] f16,
// Vt [B][Hkv][128][nk_pad] f16 (keys permuted within groups of 16, see ops.hip),
// kbias [B][nk_pad] f32 additive (0 / -inf) or null, out act [B*nq][Hq*128].
struct AttnArgs {
    const uint16_t* q;
    const uint16_t* k;
    const uint16_t* vt;
    const float* kbias;
    uint16_t* out;
    int B, Hq, Hkv;
    int nq, nq_pad, nk, nk_pad;
    int window;  // >0: bidirectional sliding window |q-k| <= window
    bool causal = false;  // key k > query q masked (Qwen3 text encoder)
    float scale;
    bool split = true;                 // hi/lo fp16 Q.K operands (see attention.hip)
    bool pv_split = false;             // hi/lo fp16 P.V operands too (needs split)
    int64_t q_plane = 0, k_plane = 0, v_plane = 0;  // element offset of the lo planes
    // Optional f32 workspace of attn_part_floats(): with it, a grid too small to fill the chip in whole rounds
    // splits block key ranges in two or four parts, merged by attn_merge_kernel.
    float* part = nullptr;
    int ksplit = 1;  // set by launch_attention
    int xcd_order = 1;  // set by launch_attention: XCD-aware block order
    int split_from = 0;  // set by launch_attention: > 0 = tail split (blocks [0, split_from) whole, the rest in two
                         // key-range parts; ksplit = 2 gives the partials' layout)
    // f32 output [B*nq][Hq*128] instead of `out` (the ggml-faithful quantized-activation mode, whose next linear
    // quantizes the f32 rows), under the same key-split policy: whole blocks and the merges write f32 rows
    float* out_f32 = nullptr;
    bool f8 = false;  // f8c mode (needs split + pv_split): the lo planes hold fp8 hi / lo operands (prep_math.h), the
                      // correction products Kl.Qh + Kh.Ql and Vl.Ph + Vh.Pl run as block-scaled fp8 MFMAs
};
// launch_attention's argument checks (the host emulation applies the same ones)
inline void attn_check_args(const AttnArgs& a) {
    ACEMI_CHECK(a.Hkv > 0 && a.Hq % a.Hkv == 0, "attention: Hq must be a multiple of Hkv");
    const int rep = a.Hq / a.Hkv;
    ACEMI_CHECK(rep == 1 || rep == 2 || rep == 4, "attention: n_rep must be 1, 2 or 4");
    ACEMI_CHECK(a.nk_pad % ATTN_KT == 0 && a.nk_pad >= a.nk, "attention: nk_pad");
    const int qpb = 128 / rep;
    const int n_qt = (a.nq + qpb - 1) / qpb;
    ACEMI_CHECK(a.nq_pad >= n_qt * qpb, "attention: nq_pad too small");
    ACEMI_CHECK(!a.f8 || a.pv_split, "attention: the fp8 correction modes need pv_split");
    if (a.split) {
        ACEMI_CHECK(a.q_plane > 0 && a.k_plane > 0, "attention: split mode needs lo planes");
        ACEMI_CHECK(!a.pv_split || a.v_plane > 0, "attention: hi/lo P.V needs the V lo plane");
    } else if (a.pv_split) {
        ACEMI_CHECK(a.f8 && a.v_plane > 0, "attention: pv8 mode needs the fp8 V lo plane");
    }
}
inline AttnShape attn_shape_of(const AttnArgs& a) {
    return {a.B,     a.Hq,       a.Hkv, a.nq,  a.nk, a.window, a.causal, a.part != nullptr,
            a.split, a.pv_split, a.f8,  a.out_f32 != nullptr};
}
// The tests' override of this process's attention policy (attn_plan.h): every field that is not -1 replaces what the
// environment / the device says; ATTN_POLICY_UNSET clears it.
inline AttnPolicy& attn_policy_override() {
    static AttnPolicy over = ATTN_POLICY_UNSET;
    return over;
}
// Which kernel runs the f8c mode (the override's kh field alone): -1 = ACE_MI_ATTN_KH (0 never, 1 always) / default
// (attn_kh_kernel, two waves per SIMD, for blocks of >= 16 key tiles; attn2 below that), 0 = attn2 always,
// 1 = attn_kh_kernel always
void attn_kh_mode(int mode);
// Operand precision of the attention MFMAs: FP16 = single fp16 operands (two workgroups per CU),
// SPLIT = hi/lo fp16 Q.K (three MFMAs per product) with fp16 P.V, F32 = hi/lo fp16 for both products
// (~22-bit operands, the f32-faithful mode), F8C = hi/lo for both products with the two correction products as
// block-scaled e4m3 MFMAs (hi x hi in fp16, Kl.Qh + Kh.Ql and Vl.Ph + Vh.Pl at e4m3 precision: ~2^-15 relative
// per product instead of F32's ~2^-22, at 2/3 of F32's matrix-core time).  ACE_MI_ATTN_PRECISION=fp16|split|f32 overrides `dflt`;
// the legacy ACE_MI_ATTN_FAST=1 means fp16.
// PV8 = fp16 Q.K with F8C's hi/lo P.V (the P.V roundings carry most of fp16 attention's excess over the f32 graph;
// measured in tests/test_gpu_parity_strict.py), 3/4 of F8C's matrix-core time.
enum class AttnPrecision { FP16, SPLIT, F32, F8C, PV8 };
inline AttnPrecision attn_precision_from_env(AttnPrecision dflt) {
    const char* f = std::getenv("ACE_MI_ATTN_FAST");
    if (f && f[0] && f[0] != '0') return AttnPrecision::FP16;
    const char* e = std::getenv("ACE_MI_ATTN_PRECISION");
    if (!e || !e[0]) return dflt;
    const std::string v(e);
    if (v == "fp16") return AttnPrecision::FP16;
    if (v == "split") return AttnPrecision::SPLIT;
    if (v == "f32") return AttnPrecision::F32;
    if (v == "f8c") return AttnPrecision::F8C;
    if (v == "pv8") return AttnPrecision::PV8;
    throw std::runtime_error("ACE_MI_ATTN_PRECISION must be fp16, split, f32, f8c or pv8");
}
void launch_attention(ActType out_t, const AttnArgs& a, hipStream_t s);

// ------------------------------------------------------------ attention probabilities (kernels/attn_probs.hip)
// The softmax the flash kernels never materialise, for a list of query heads (the lyric-alignment features read the
// cross-attention maps): for every listed head h, with its KV head h / (Hq / Hkv),
//   out[i][b][q][k] = exp(s - max_k s) / sum_k exp(s - max_k s),  s = scale * (q . k) + kbias[b][k],  h = heads[i],
// from the fp16 HI planes of the Q / K images of AttnArgs alone (the lo planes, which hold fp8 bytes in the f8c mode,
// are not read): fp16-operand precision, f32 accumulate.  out is dense f32 [n_heads][B][nq][nk]; a masked key
// (kbias -inf, or k >= nk) is exactly +0, a row without an unmasked key is all zeros (not NaN).  The list may repeat
// a head and be in any order.  nq_pad % 128 == 0, nk_pad % 64 == 0.  Fixed reduction order: bit-identical between runs.
constexpr int ATTN_PROBS_MAX_HEADS = 32;  // per launch; a longer list takes several launches
struct AttnProbArgs {
    const uint16_t* q = nullptr;   // [B][Hq][nq_pad][128]
    const uint16_t* k = nullptr;   // [B][Hkv][nk_pad][128]
    const float* kbias = nullptr;  // [B][nk_pad] additive (0 / -inf) or null
    int B = 0, Hq = 0, Hkv = 0;
    int nq = 0, nq_pad = 0, nk = 0, nk_pad = 0;
    float scale = 0.f;
    int n_heads = 0;
    const int* heads = nullptr;  // host array [n_heads]: passed to the kernel by value
    const int* slots = nullptr;  // host array [n_heads] or null: listed head i writes out[slots[i]] instead of out[i]
                                 // (out then holds max(slots) + 1 maps; two entries may not share a slot)
    float* out = nullptr;
};
void launch_attn_probs(const AttnProbArgs& a, hipStream_t s);

// ------------------------------------------------------------ elementwise
// Pack [context | hidden] frames into patches: out act [B*Np][P*Cin].
// x3: write the f32 value as the fp16 triple [hi | hi | lo] per row (input of a WF_F32X3 weight).
void launch_pack_input(ActType t, const float* hidden, const float* context, int B, int T, int Np, int P,
                       int audio_dim, int ctx_dim, uint16_t* out, hipStream_t s, bool x3 = false);
// f32 -> act conversion (row-major copy), optionally act(silu(x)).
void launch_to_act(ActType t, const float* in, int64_t n, bool silu, uint16_t* out, hipStream_t s);
// y = act( RMSNorm(x) * w * (1 + scale) + shift ); scale/shift optional, per item
// (item = row / rows_per_item, stride mod_stride floats).
void launch_rmsnorm_mod(ActType t, const float* x, int M, int H, const float* w, const float* scale,
                        const float* shift, int64_t mod_stride, int rows_per_item, float eps, uint16_t* out,
                        hipStream_t s, bool x3 = false);
// out[r] = RMSNorm(x[r * row_step]) * w in f32 for r < rows (the condition encoders' final norm,
// acestep_dit_model.cpp:1642-1644 / :1727-1729; row_step > 1 picks every item's first token).
void launch_rmsnorm_f32(const float* x, int rows, int64_t row_step, int H, const float* w, float eps, float* out,
                        hipStream_t s);
// out[t] = f32(table[ids[t]]) for t < n (ggml_get_rows + cast_f32, qwen_model.cpp:563-564):
// table [rows][H] as bf16 (fmt 0), fp16 (1) or f32 (2) values.
void launch_embed_rows(const void* table, int fmt, const int32_t* ids, int n, int H, float* out, hipStream_t s);
void launch_attn_prep(const PrepArgs& a, hipStream_t s);
// kbias[b][k] = (k < nk && pooled mask) ? 0 : -inf ; mask [B][nk*patch-ish frames] or null.
void launch_key_bias(const int32_t* mask, int B, int frames, int patch, int nk, int nk_pad, float* kbias,
                     hipStream_t s);
// Sinusoidal timestep features f[b][256] of t[b] - (r ? r[b] : 0) (acestep_dit_model.cpp:1261-1284).
// log_max = logf(10000) evaluated on the host exactly as the reference does.
void launch_timestep_freq(const float* t, const float* r, int B, int dim, float scale, float log_max, float* f,
                          hipStream_t s);
// Small-M GEMV (timestep MLPs): v = sum_k x_act[m][k] W[n][k] + bias[n]; v = silu(v) if silu_out;
// y[m][n] = accumulate ? y[m][n] + v : v.  M <= 8, K % 512 == 0.
void launch_gemv(ActType t, const uint16_t* x_act, int M, const uint16_t* W, int N, int K, const float* bias,
                 bool silu_out, bool accumulate, float* y, hipStream_t s);
// Same with f32 x rounded to the act type in the kernel (after silu when silu_in): launch_to_act + launch_gemv
// in one launch, same bits.
void launch_gemv_f32(ActType t, const float* x, bool silu_in, int M, const uint16_t* W, int N, int K,
                     const float* bias, bool silu_out, bool accumulate, float* y, hipStream_t s);
// mod[l][b][j][c] = table[l][j][c] + proj[b][j*H + c]  (j < 6)
void launch_layer_mods(const float* tables, const float* proj, int n_layers, int B, int H, float* mod,
                       hipStream_t s);
// outmod[b][j][c] = out_table[j][c] + (temb_t[b][c] + temb_r[b][c]) (j < 2)
void launch_out_mods(const float* out_table, const float* temb_t, const float* temb_r, int B, int H,
                     float* outmod, hipStream_t s);
// TEST ONLY (fault injection for the parity negative control): x[r][c] += amp for r in [row0, row0 + 16),
// c in [col0, col0 + 128)
void launch_fault_tile(float* x, int ld, int rows, int row0, int col0, float amp, hipStream_t s);
// Test-only hooks (runtime/test_hooks.cpp): read from the environment in the self-test library only; the product
// library's versions return "off"
bool test_fault_from_env(int& layer, int& row, int& col, float& amp);
bool test_vae_fault_from_env(int& block, int& row, int& col, float& amp);
int gemm_override_from_env(int N, int K);
// xt -= v * dt
void launch_euler(float* xt, const float* v, int64_t n, float dt, hipStream_t s);
// Read-only sweep of up to 6 device ranges (weights of the next layer) on a side stream, so they sit in the
// memory-side cache (MALL) when the layer's GEMMs read them; `blocks` workgroups.  Nothing is written except
// one word of `sink` in a case that never occurs (keeps the loads).
void launch_prefetch(const void* const* ptrs, const size_t* bytes, int n, int blocks, unsigned* sink, hipStream_t s);
// SDE re-noise step: xt = t_next * noise + (1 - t_next) * (xt - v * t)
void launch_sde(float* xt, const float* v, const float* noise, int64_t n, float t, float t_next, hipStream_t s);

// ------------------------------------------------------------ LM decode step (kernels/lm_decode.hip)
// The M = 1..8 regime of the causal LM's token-by-token decode (runtime/lm.cpp): HBM-bound, no MFMA.
constexpr int LM_MAX_BATCH = 8;
// keys per decode-attention workgroup; a step over more keys splits into ranges of this size and merges them
constexpr int LM_SPLIT_KEYS = 256;
enum LmEpi : int {
    LM_EPI_STORE = 0,   // y_f32[b*ldy + n] = acc
    LM_EPI_RESID = 1,   // y_f32[b*ldy + n] += acc
    LM_EPI_SWIGLU = 2,  // W = the 16-row interleaved gate|up matrix [N][K]: y_act[b*ldy + j] = act(silu(g_j) * u_j), j < N/2
};
// y[B][N] = x[B][K] . W[N][K]^T: x, W 16-bit of type t (W dense, ld K), f32 accumulate, B <= 8, K % 8 == 0, ldx % 8 == 0.
// Every weight byte is read once for all B rows; fixed reduction order (bit-identical between runs).
void launch_lm_skinny(ActType t, const uint16_t* x, int ldx, int B, const uint16_t* W, int N, int K, int epi,
                      float* y_f32, uint16_t* y_act, int ldy, hipStream_t s);
// launch_embed_rows for a 16-bit table (fmt 0 bf16, 1 fp16) with the ids (device values nobody validated) clamped
// into [0, vocab)
void launch_lm_embed(const void* table, int fmt, const int32_t* ids, int n, int vocab, int H, float* out, hipStream_t s);
// The same two operations on a weight in ggml block planes (kernels/lm_decode_q.hip; plane layout: runtime/quant.h).
// launch_lm_skinny_q: x bf16, W.fmt WF_Q8_0 / WF_Q4_K / WF_Q6_K, K % 32 == 0 (Q8_0) or K % 256 == 0 (K-quants); the
// weight value multiplied is the bf16 rounding of the plane dequant (the value the quantized GEMMs of gemm_q.hip
// multiply), the epilogues and the fixed reduction order are launch_lm_skinny's.
void launch_lm_skinny_q(const uint16_t* x, int ldx, int B, const WeightView& W, int N, int K, int epi, float* y_f32,
                        uint16_t* y_act, int ldy, hipStream_t s);
// longest f32 addition chain behind one output of launch_lm_skinny_q (its lane mapping: lm_decode_q.hip's header)
int lm_skinny_q_chain(int fmt, int K);
// launch_lm_embed_q: rows of the planes as ggml's get_rows returns them (the f32 dequant, not rounded to bf16), ids
// clamped into [0, vocab).  fmt LM_EMBED_F32: `q` is an f32 table [vocab][H] (a table without a plane layout).
constexpr int LM_EMBED_F32 = 100;
void launch_lm_embed_q(int fmt, const void* q, const float* s, const int32_t* ids, int n, int vocab, int H, float* out,
                       hipStream_t stream);
// KV cache of one layer: k_cache / v_cache [B][hkv][capacity][128] fp16, key_mask [B][capacity] int32 (shared by the
// layers).  qkv: the fused projection's f32 rows [.][ld] = [q heads | k heads | v heads]; rope_cos / rope_sin
// [capacity][64].
struct LmQkvPostArgs {
    const float* qkv = nullptr;
    int ld = 0;
    int hq = 0, hkv = 0;
    const float* q_norm = nullptr;
    const float* k_norm = nullptr;
    const float* rope_cos = nullptr;
    const float* rope_sin = nullptr;
    float eps = 1e-6f;
    float* q_out = nullptr;  // decode: [B][hq][128] f32, normalised and rotated
    uint16_t* k_cache = nullptr;
    uint16_t* v_cache = nullptr;
    int32_t* key_mask = nullptr;
    int capacity = 0;
    int pos = 0;                        // decode: the slot every sequence appends at
    const int32_t* mask_new = nullptr;  // decode: [B] mask of the appended token, or null = valid
};
// decode: one row per sequence (qkv [B][ld]) at slot a.pos
void launch_lm_qkv_post(const LmQkvPostArgs& a, int B, hipStream_t s);
// prefill: rows b*n + t of qkv -> slots t < n; mask [B][n] or null; the q|k|v values of a padding row (mask 0) are
// zeroed in place and in the cache (q_out, pos and mask_new unused)
void launch_lm_prefill_kv(const LmQkvPostArgs& a, int B, int n, const int32_t* mask, hipStream_t s);
struct LmAttnArgs {
    const float* q = nullptr;  // [B][hq][128] f32
    const uint16_t* k_cache = nullptr;
    const uint16_t* v_cache = nullptr;
    const int32_t* key_mask = nullptr;
    int hkv = 0, capacity = 0;
    int nk = 0;  // keys 0 .. nk-1 (the appended one included)
    float scale = 0.f;
    uint16_t* out = nullptr;  // [B][hq*128] in the act type
    float* part = nullptr;    // lm_attn_part_floats() floats when nk > LM_SPLIT_KEYS
    int n_split = 1;          // set by launch_lm_attention
};
size_t lm_attn_part_floats(int B, int hq, int nk);
// out = softmax(scale q.k over the keys with key_mask != 0) . V; a masked key's K and V never reach the result, slots
// >= nk are not read, and a sequence whose keys are all masked gets exactly +0 in every output word of either type.
void launch_lm_attention(ActType out_t, const LmAttnArgs& a, int B, int hq, hipStream_t s);

// ------------------------------------------------------------ LM cache fan-out (kernels/lm_fanout.hip)
// A prefilled cache of G = 1 or 2 sequences re-laid for G * S sequences: destination sequence g * S + s is a bit copy of
// source sequence g over positions [0, n); positions [n, cap_dst) of the destination are not written.  Source K and V
// [layers][G][hkv][cap_src][128] fp16 with key mask [G][cap_src]; destination [layers][G * S][hkv][cap_dst][128] with
// [G * S][cap_dst].  The two caches must be different allocations.
struct LmFanoutArgs {
    const uint16_t* k_src = nullptr;
    const uint16_t* v_src = nullptr;
    const int32_t* mask_src = nullptr;
    uint16_t* k_dst = nullptr;
    uint16_t* v_dst = nullptr;
    int32_t* mask_dst = nullptr;
    int layers = 0, G = 0, S = 0, hkv = 0;
    int cap_src = 0, cap_dst = 0;
    int n = 0;  // positions held by the source
};
inline void lm_fanout_check(const LmFanoutArgs& a) {
    ACEMI_CHECK(a.k_src && a.v_src && a.mask_src && a.k_dst && a.v_dst && a.mask_dst && a.k_src != a.k_dst &&
                    a.v_src != a.v_dst && a.mask_src != a.mask_dst,
                "lm_cache_fanout: null or aliased buffers");
    ACEMI_CHECK((a.G == 1 || a.G == 2) && a.S >= 1 && a.G * a.S <= LM_MAX_BATCH && a.layers >= 1 && a.hkv >= 1 &&
                    (int64_t)a.layers * a.hkv <= 65535,
                "lm_cache_fanout: bad batch or layer shape");
    ACEMI_CHECK(a.n >= 1 && a.n <= a.cap_src && a.n <= a.cap_dst, "lm_cache_fanout: positions outside a cache");
}
void launch_lm_cache_fanout(const LmFanoutArgs& a, hipStream_t s);

// ------------------------------------------------------------ LM token selection (kernels/lm_sample.hip)
// One token per sampled sequence from the f32 logits of a forward: CFG mix, candidate set, phase temperature,
// repetition penalty, top-k, top-p, then a draw (or the argmax) -- the codes-phase pipeline of the reference's loops.
// Every step up to the top-p cut is a separately rounded f32 operation (semantics and order: include/acestep_mi355x.h,
// ace_mi_lm_select); the thresholds come from selection, never from a sort; one launch; bit-identical between runs.
struct LmSelectArgs {
    const float* logits = nullptr;  // [B][ld_logits]; S sampled sequences: cfg_scale > 1 -> S = B/2, row s cond, s+S uncond
    int64_t ld_logits = 0;
    int vocab = 0;
    int S = 0;
    float cfg_scale = 1.f;           // > 1: mix
    const int32_t* allowed = nullptr;  // ascending ids, or null = the whole vocabulary
    int n_allowed = 0;
    int stop_id = -1;
    int block_stop = 0;   // the caller's n_emitted < min_tokens
    int force_stop = 0;   // only stop_id is a candidate
    int n_emitted = 0;    // index of this token (written to done[0] as n_emitted + 1 on the first stop)
    float pre_temperature = 0.f;
    float repetition_penalty = 1.f;
    uint8_t* seen = nullptr;  // [S][ld_seen] byte map or null; the chosen id's byte is set
    int64_t ld_seen = 0;
    int top_k = 0;
    float top_p = 1.f;
    float temperature = 1.f;         // <= 0: argmax
    const float* uniform = nullptr;  // [S] in [0, 1) (temperature > 0)
    float* work = nullptr;           // lm_select_work_floats() floats of scratch
    int32_t* tokens = nullptr;       // token of sequence s -> tokens[s * token_stride]
    int64_t token_stride = 1;
    int32_t* next_ids = nullptr;  // or null; [B]: rows s and (mixing) s + S
    int32_t* done = nullptr;      // or null; [1 + S] words: [0] = 1 + index of the first token at which a sequence emitted
                                  // stop_id (0 = none yet), [1 + s] != 0 = sequence s has stopped and keeps emitting it
    float* processed = nullptr;   // or null; [S][ld_processed]: the logits as they stand after the top-p cut, -inf
    int64_t ld_processed = 0;     // where removed
};
// candidates of one sequence (the allowed list, else the vocabulary) and the scratch floats launch_lm_select needs
inline int lm_select_candidates(int vocab, int n_allowed, bool has_list) { return has_list ? n_allowed : vocab; }
inline size_t lm_select_work_floats(int S, int n_cand) { return (size_t)2 * S * n_cand; }
void launch_lm_select(const LmSelectArgs& a, hipStream_t s);
// longest f32 addition chains of launch_lm_select over n_cand candidates, three ints: [0] behind a top-p mass (and
// behind the top-p total), [1] behind the draw's total, [2] behind a cumulative value of the draw
void lm_select_chains(int n_cand, int* chains);

// ------------------------------------------------------------ VAE decoder (kernels/vae.hip)
// Implicit-GEMM conv on fp16 time-major activations.  A row (m, tap) = S[m + tap*dil - pad]
// (zero row outside [0, T_in)); W [N][taps*Cin] fp16.  up == 1: conv, (m, n) -> (u = m, co = n);
// up = s > 1: transposed conv, n = r*Cout + co -> u = s*m + r - crop.  Epilogue on v = acc + bias:
// resid: v = X[u][co] + v; store_x: X[u][co] = v; S_out: S_out[u][co] = f16(snake(v)) (or f16(v)
// when snake_ea is null).
struct ConvGemmArgs {
    const uint16_t* S = nullptr;
    const uint16_t* zero = nullptr;
    const uint16_t* W = nullptr;
    int T_in = 0, Cin = 0, taps = 1, dil = 1, pad = 0;
    int in_stride = 1;  // strided conv: A row (m, tap) = S[m*in_stride + tap*dil - pad]
    int M = 0, N = 0;
    const float* bias = nullptr;
    int Cout = 0, up = 1, crop = 0, T_out = 0;
    float* X = nullptr;
    int resid = 0, store_x = 0;
    uint16_t* S_out = nullptr;
    const float* snake_ea = nullptr;
    const float* snake_eb = nullptr;
    // independent sequences in one launch (windows of the tiled decode): the M rows split into
    // `items` equal runs; S is [items][T_in][Cin], X / S_out are [items][T_out][Cout]
    int items = 1;
    // Fused second conv of a residual unit (residual_forward, acestep_vae_model.cpp:724-733) when
    // Cout = N = 128: the tile's conv output y = Snake2(acc + bias) goes through LDS as fp16 into
    // z = y . W2^T + bias2 (the k1 conv), and the residual / store / S_out epilogue applies to z.
    const uint16_t* W2 = nullptr;  // [Cout][Cout] fp16
    const float* bias2 = nullptr;
    const float* snake2_ea = nullptr;
    const float* snake2_eb = nullptr;
};
void launch_conv_gemm(const ConvGemmArgs& a, hipStream_t s);
void launch_to_f16(const float* x, int64_t n, uint16_t* y, hipStream_t s);
// x [rows][C] f32 -> y [rows][Cpad] fp16, channels >= C zero
void launch_pack_f16(const float* x, int64_t rows, int C, int Cpad, uint16_t* y, hipStream_t s);
// out[t][o] = sum_k sum_c W[o][k][c] * S[t + k - 3][c]   (kernel 7, pad 3, no bias), f32 out
// (items sequences of T rows each: S [items][T][C], out [items][T][out_ch])
void launch_conv_out(const uint16_t* S, int T, int C, const uint16_t* W, int out_ch, float* out, hipStream_t s,
                     int items = 1);

}  // namespace acemi
