/* Kernel self-test and micro-benchmark entries of the TEST library libacestep_mi355x_selftest.so (the product
 * library's objects + csrc/runtime/selftest.cpp; Makefile target `selftest`).  Not part of the product
 * library libacestep_mi355x.so: the -m gpu parity tests and tools/ call single gfx950 kernels through these on
 * host buffers (blocking) and compare them with fp64 / fp32 references of the same op. */
#ifndef ACESTEP_MI355X_SELFTEST_H
#define ACESTEP_MI355X_SELFTEST_H

#include "acestep_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- kernel self-test entries (blocking, host buffers; used by the -m gpu parity tests) ----
 * GEMM: C = A[M][K] . W[N][K]^T with A, W raw 16-bit words of act_type (0 bf16, 1 fp16).
 * epi 0: out_f32[M][N] = C (+ bias[N] if bias != NULL);
 * epi 4: SwiGLU on 16-column interleaved gate|up weights, out_u16[M][N/2] raw act words;
 * epi 3 / 2: residual update in place, out_f32[M][N] holds x on entry: x += C (epi 3) or
 * x += C * gate[N] (epi 2, the gate passed in `bias`). */
ACE_GGML_API ace_ggml_status ace_mi_kernel_gemm(int32_t act_type, int32_t epi, int32_t M, int32_t N, int32_t K,
                                                const uint16_t* A, const uint16_t* W, const float* bias,
                                                float* out_f32, uint16_t* out_u16);
/* Attention core only (no norm/RoPE): q [B][nq][Hq*128] f32, kv [B][nk][2*Hkv*128] f32 (K then V),
 * kmask [B][nk] int32 or NULL, window > 0 = sliding |q-k| <= window; `split` is a flag word: bit 0 =
 * hi/lo fp16 operands (default engine mode; clear = single fp16), bit 1 = causal (key k > query q
 * masked); out [B][nq][Hq*128] f32 (the kernel's bf16 output widened). */
ACE_GGML_API ace_ggml_status ace_mi_kernel_attention(int32_t B, int32_t Hq, int32_t Hkv, int32_t nq, int32_t nk,
                                                     int32_t window, float scale, int32_t split, const float* q,
                                                     const float* kv, const int32_t* kmask, float* out);
/* Attention probabilities of the listed query heads (kernels/attn_probs.hip, one launch; no norm / RoPE): q
 * [B][nq][Hq*128] f32, k [B][nk][Hkv*128] f32, prepared as ace_mi_kernel_attention prepares its operands (the kernel
 * reads their fp16 roundings), kmask [B][nk] int32 or NULL, heads [n_heads] query heads (any order, repeats allowed).
 * out f32 [n_heads][B][nq][nk] is copied to the device before the launch and back after it, so a caller's sentinels
 * show an element the kernel did not write; the device buffer carries 1024 guard floats on either side of the payload,
 * and ACE_GGML_ERR is returned when the launch changed one of them. */
ACE_GGML_API ace_ggml_status ace_mi_kernel_attn_probs(int32_t B, int32_t Hq, int32_t Hkv, int32_t nq, int32_t nk,
                                                      float scale, const float* q, const float* k,
                                                      const int32_t* kmask, int32_t n_heads, const int32_t* heads,
                                                      float* out);

/* Attention micro-benchmark on pseudo-random device operands (fixed seed): average ms per launch (HIP
 * events) of the engine's attention kernel; flags bit 0 = hi/lo operands, bit 1 = causal, bit 2 = a
 * key-padding mask (every 7th key masked). */
ACE_GGML_API ace_ggml_status ace_mi_bench_attention(int32_t B, int32_t Hq, int32_t Hkv, int32_t nq, int32_t nk,
                                                    int32_t window, int32_t flags, int32_t iters, float* avg_ms);

/* GEMM micro-benchmark on random device operands: average ms per launch (HIP events) of the
 * engine's GEMM for act_type (0 bf16, 1 fp16), epilogue `epi` (0 f32 store, 2 gated residual,
 * 4 SwiGLU), kernel `variant` (-1 automatic; forced: a dense id of csrc/gemm_variants.h, 0..16 or 18, + 100 S for
 * split-K over S = 2..4 parts where the row allows it). */
ACE_GGML_API ace_ggml_status ace_mi_bench_gemm(int32_t act_type, int32_t epi, int32_t variant, int32_t M, int32_t N,
                                               int32_t K, int32_t iters, float* avg_ms);
/* Dequant-fused GEMM on ggml block rows W [N][K]: out = A . bf16(dequant(W))^T (+ bias), A bf16 [M][K];
 * epi 0 (f32 store) or 4 (SwiGLU, bf16 out [M][N/2]); variant -1 automatic; forced: a quantized id of
 * csrc/gemm_variants.h -- 0..5 and 7 (round 1's ds_write dequant tiles), 20..24 (the LDS-staged dequant tiles; 22, 23
 * + 100 S: split-K), 25 (warp-specialized); + 0x10000: launched without the picker's support check. */
ACE_GGML_API ace_ggml_status ace_mi_kernel_gemm_q(int32_t qtype, int32_t epi, int32_t variant, int32_t M, int32_t N,
                                                  int32_t K, const uint16_t* A, const uint8_t* W_blocks,
                                                  const float* bias, float* out_f32, uint16_t* out_u16);
/* Staged dequant kernel (the bf16 weight image the DiT's staged-dequant ring multiplies): out = bf16 bits of
 * bf16(dequant(W)) [N][K] for ggml block rows W [N][K]. */
ACE_GGML_API ace_ggml_status ace_mi_kernel_dequant(int32_t qtype, int32_t N, int32_t K, const uint8_t* W_blocks,
                                                   uint16_t* out);
/* Raw ggml block rows -> bf16 image (the expansion of a raw-block weight, csrc/kernels/dequant_blocks.hip): ggml type ids
 * 2 Q4_0, 3 Q4_1, 6 Q5_0, 7 Q5_1, 8 Q8_0, 10 Q2_K, 11 Q3_K, 12 Q4_K, 13 Q5_K, 14 Q6_K, 20 IQ4_NL.  out = bf16 bits
 * of rne_bf16(ggml dequantize_row_*(blocks)) [N][K]. */
ACE_GGML_API ace_ggml_status ace_mi_kernel_dequant_blocks(int32_t type, int32_t N, int32_t K, const uint8_t* blocks,
                                                          uint16_t* out);
/* The segment form: source row r of segment i lands at row  row0 + (r / group) * group * step + r % group  of the host
 * matrix out [total_rows][K] (bf16 words), which keeps its content wherever no segment writes; all segments in one call
 * of the launch entry (one launch per type). */
typedef struct ace_mi_block_seg {
    int32_t type, rows, row0, step, group;
    const uint8_t* blocks; /* [rows][K / block][block bytes] */
} ace_mi_block_seg;
ACE_GGML_API ace_ggml_status ace_mi_kernel_dequant_segments(int32_t n_segs, const ace_mi_block_seg* segs,
                                                            int32_t total_rows, int32_t K, uint16_t* out);
/* Average time (ms) of one [N][K] expansion over iters launches on rotating buffers: planes 0 = the raw-block kernel,
 * 1 = the plane kernel of ace_mi_kernel_dequant on the same blocks (types 8, 12, 14). */
ACE_GGML_API ace_ggml_status ace_mi_bench_dequant_blocks(int32_t type, int32_t planes, int32_t N, int32_t K,
                                                         int32_t iters, float* avg_ms);
/* ggml-faithful quantized-activation GEMM (ACE_MI_QUANT_ACT=q8): x f32 [M][K] quantized on the device to Q8_0
 * (Q8_0 weights) or Q8_K (K-quants) blocks -- returned as q_out int8 [M][K], s_out f32 [K/32][M] (block scale d),
 * bsum_out f32 [K/32][M] (sum of q per 32, Q8_K) when non-null -- then ggml's per-block integer dot products against
 * the ggml block rows W [N][K].  epi 0: out [M][N] = acc (+ bias); 3: out += acc (+ bias); 7: out [M][N/2] =
 * silu(g) * u (gate|up interleaved in 16-column groups). */
ACE_GGML_API ace_ggml_status ace_mi_kernel_gemm_a8(int32_t qtype, int32_t epi, int32_t M, int32_t N, int32_t K,
                                                   const float* x, const uint8_t* W_blocks, const float* bias,
                                                   float* out_f32, int8_t* q_out, float* s_out, float* bsum_out);
/* The form ace_mi_kernel_gemm_a8 and the q8 mode of this process run Q8_0 GEMMs in (K % 64 == 0): -1 = the
 * environment (ACE_MI_QACT_GEMM=0: i8) / default (bf16 MFMA over exact integer bf16 operands), 0 = the i8-MFMA kernel,
 * 1 = the bf16-MFMA kernel.  Both give the same bits. */
ACE_GGML_API ace_ggml_status ace_mi_kernel_gemm_a8_mode(int32_t mode);
/* The kernel that runs f8c attention in this process: -1 = the environment (ACE_MI_ATTN_KH=0 / 1) / default policy
 * (the two-waves-per-SIMD kernel for blocks of >= 16 key tiles), 0 = the one-wave-per-SIMD kernel, 1 = the two-wave
 * kernel everywhere.  Same results within the f8c bound. */
ACE_GGML_API ace_ggml_status ace_mi_kernel_attn_kh(int32_t mode);
/* The whole attention launch policy of this process (csrc/attn_plan.h; ace_mi_kernel_attn_kh is its kh field alone):
 * fields = {ksplit_mode 0 auto / 1..4 as ACE_MI_ATTN_KSPLIT, tail 0 / 1, tail_min >= 2, xcd_order 0 / 1, kh 0 / 1,
 * n_cu >= 1 (the CU count the split rules plan for: a small one makes a small shape behave like an over-full chip)};
 * a field of -1 leaves the environment / the device in charge, six times -1 clears the override. */
ACE_GGML_API ace_ggml_status ace_mi_kernel_attn_policy(const int32_t fields[6]);
/* The attention launch plan (csrc/attn_plan.h), without a device.
 * ace_mi_attn_plan: shape = {B, Hq, Hkv, nq, nk, window, causal, a key-split workspace exists, split, pv_split, f8,
 * f32 output}, policy = the six fields above, all set (kh may be -1: the rule) -> plan = {ksplit, split_from, xcd_order,
 * logical blocks, main grid, kernel (0 attn2_kernel, 1 attn_kh_kernel), merge (0 none, 1 two parts, 2 four parts,
 * 3 tail), merge grid}.
 * ace_mi_attn_plan_block: launch index x of a plan -> out = {logical block, key-range part, the block's number of
 * parts, valid (0: an empty trailing workgroup)}.
 * ace_mi_attn_plan_tiles: the key tiles out = {first, count} that part `part` of `parts` streams for the queries
 * [q0, q0 + qpb). */
ACE_GGML_API ace_ggml_status ace_mi_attn_plan(const int32_t shape[12], const int32_t policy[6], int32_t plan[8]);
ACE_GGML_API ace_ggml_status ace_mi_attn_plan_block(int32_t ksplit, int32_t split_from, int32_t xcd_order,
                                                    int32_t n_blk, int32_t x, int32_t out[4]);
ACE_GGML_API ace_ggml_status ace_mi_attn_plan_tiles(int32_t nk, int32_t window, int32_t causal, int32_t q0,
                                                    int32_t qpb, int32_t part, int32_t parts, int32_t out[2]);
/* LoRA merge kernel (launch_lora_merge, csrc/kernels.h): n_jobs jobs in ONE launch on one matrix pair.  base
 * [total_rows][ld_base] (NULL = in place on out) and out [total_rows][ld_out] are raw 16-bit words of fmt (0 bf16,
 * 1 fp16); out holds its initial content on entry and the merged image on return, so a caller sees which words were
 * written.  A job covers the fused rows [row0, row0 + rows): module row o (A [r][cols], B [rows_mod][r] f32 host
 * arrays) lands at fused row row_off + o (map 0) or (o / 16) * 32 + half * 16 + o % 16 (map 1, the gate|up
 * interleave); rows of the range that belong to no module row are copied from base when copy_rest != 0; r = 0 (A, B
 * NULL) is a copy-only job.  out = rne16(f32(base) + eff * acc), acc the rank-ordered chain of separately rounded f32
 * multiplies and adds. */
typedef struct ace_mi_lora_job {
    int32_t row0, rows;
    int32_t r, rows_mod;
    const float* A;
    const float* B;
    float eff;
    int32_t map, row_off, half, copy_rest;
} ace_mi_lora_job;
ACE_GGML_API ace_ggml_status ace_mi_kernel_lora_merge(int32_t fmt, int32_t total_rows, int32_t cols, int32_t ld_base,
                                                      int32_t ld_out, const uint16_t* base, uint16_t* out,
                                                      const ace_mi_lora_job* jobs, int32_t n_jobs);
/* ---- LM decode kernels (csrc/kernels/lm_decode.hip through launch_lm_* of csrc/kernels.h; csrc/runtime/selftest_lm.cpp).
 * One launch_lm_* call each on host buffers; INVALID_ARG, before any allocation, for what the launch entry refuses or
 * what does not fit the host buffers.  16-bit words are raw bf16 (type / fmt 0) or fp16 (1).
 * Skinny product y[B][N] = x[B][K] . W[N][K]^T: x [B][ldx], W [N][K]; epi 0 store / 1 add into y_f32 [B][ldy]; epi 2
 * SwiGLU on the 16-row interleaved gate|up W into y_u16 [B][ldy] (N / 2 columns).  y_* holds its initial content on
 * entry and is copied back whole, padding columns included. */
ACE_GGML_API ace_ggml_status ace_mi_kernel_lm_skinny(int32_t act_type, int32_t epi, int32_t B, int32_t N, int32_t K,
                                                     int32_t ldx, int32_t ldy, const uint16_t* x, const uint16_t* W,
                                                     float* y_f32, uint16_t* y_u16);
/* Embedding rows: out [n][H] f32 = table [vocab][H] at ids [n] clamped into the table. */
ACE_GGML_API ace_ggml_status ace_mi_kernel_lm_embed(int32_t fmt, int32_t n, int32_t vocab, int32_t H,
                                                    const uint16_t* table, const int32_t* ids, float* out);
/* The same two on a weight in ggml block planes (csrc/kernels/lm_decode_q.hip).  qtype: ace_mi_quantize's
 * ids 1 Q8_0 / 2 Q4_K / 3 Q6_K; blocks: ggml block bytes [w_rows][row bytes] (w_rows >= N: rows past N are uploaded and must not be
 * read), re-laid out into the loader's planes here; x bf16.  *chain (may be NULL) receives the longest f32 addition
 * chain behind one output for this type and K, the c - 2 of the tests' bound. */
ACE_GGML_API ace_ggml_status ace_mi_kernel_lm_skinny_q(int32_t qtype, int32_t epi, int32_t B, int32_t N, int32_t w_rows,
                                                       int32_t K, int32_t ldx, int32_t ldy, const uint16_t* x,
                                                       const uint8_t* blocks, float* y_f32, uint16_t* y_u16,
                                                       int32_t* chain);
/* Embedding rows from the planes: out [n][H] f32 = the f32 dequant (ggml get_rows) of blocks [vocab][row bytes] at
 * ids [n] clamped into the table. */
ACE_GGML_API ace_ggml_status ace_mi_kernel_lm_embed_q(int32_t qtype, int32_t n, int32_t vocab, int32_t H,
                                                      const uint8_t* blocks, const int32_t* ids, float* out);
/* Decode step's q/k norm + RoPE + cache append at slot pos: qkv [B][ld] f32, q_norm / k_norm [128], rope_cos / rope_sin
 * [capacity][64], mask_new [B] or NULL; q_out [B][hq][128] f32; k_cache / v_cache [B][hkv][capacity][128] fp16 and
 * key_mask [B][capacity] (one layer) are in-out. */
ACE_GGML_API ace_ggml_status ace_mi_kernel_lm_qkv_post(int32_t B, int32_t hq, int32_t hkv, int32_t capacity, int32_t pos,
                                                       int32_t ld, float eps, const float* qkv, const float* q_norm,
                                                       const float* k_norm, const float* rope_cos,
                                                       const float* rope_sin, const int32_t* mask_new, float* q_out,
                                                       uint16_t* k_cache, uint16_t* v_cache, int32_t* key_mask);
/* Prefill cache fill of rows b * n + t of qkv [B * n][ld] (in-out: padding rows are zeroed) into slots t < n; mask
 * [B][n] or NULL; caches and key_mask as above. */
ACE_GGML_API ace_ggml_status ace_mi_kernel_lm_prefill_kv(int32_t B, int32_t hq, int32_t hkv, int32_t capacity, int32_t n,
                                                         int32_t ld, float eps, float* qkv, const float* k_norm,
                                                         const float* rope_cos, const float* rope_sin,
                                                         const int32_t* mask, uint16_t* k_cache, uint16_t* v_cache,
                                                         int32_t* key_mask);
/* Decode attention over keys 0 .. nk-1 of the cache: q [B][hq][128] f32, out_u16 [B][hq * 128] words of out_type; the
 * split workspace (lm_attn_part_floats) is allocated here. */
ACE_GGML_API ace_ggml_status ace_mi_kernel_lm_attention(int32_t out_type, int32_t B, int32_t hq, int32_t hkv,
                                                        int32_t capacity, int32_t nk, float scale, const float* q,
                                                        const uint16_t* k_cache, const uint16_t* v_cache,
                                                        const int32_t* key_mask, uint16_t* out_u16);
/* Token selection (kernels/lm_sample.hip; semantics: ace_mi_lm_select in acestep_mi355x.h) on host arrays with padded
 * leading dimensions: logits [B][ld_logits] (S = B, or B / 2 when cfg_scale > 1), allowed [n_allowed] or NULL, uniform
 * [S] or NULL, seen [S][ld_seen] bytes or NULL (in-out), tokens [S * token_stride] (in-out: word s * token_stride is
 * written), next_ids [B] or NULL (in-out), done [1 + S] or NULL (in-out: [0] = 1 + n_emitted at the first stop, [1 + s]
 * = sequence s has stopped), processed [S][ld_processed] or NULL (in-out: the logits after the top-p cut, -inf where
 * removed, columns < vocab only).  block_stop: the caller's n_emitted < min_tokens.  chains (int32 [3], may be NULL)
 * receives the longest f32 addition chains behind a top-p mass [0], behind the draw's total [1] and behind a cumulative
 * value of the draw [2]. */
typedef struct ace_mi_kernel_lm_select_args {
    int32_t B, vocab, ld_logits;
    float cfg_scale, pre_temperature, repetition_penalty;
    int32_t top_k;
    float top_p, temperature;
    int32_t n_allowed, stop_id, block_stop, force_stop, n_emitted;
    int32_t ld_seen, token_stride, ld_processed;
    const float* logits;
    const int32_t* allowed;
    const float* uniform;
    uint8_t* seen;
    int32_t* tokens;
    int32_t* next_ids;
    int32_t* done;
    float* processed;
    int32_t* chains;
} ace_mi_kernel_lm_select_args;
ACE_GGML_API ace_ggml_status ace_mi_kernel_lm_select(const ace_mi_kernel_lm_select_args* args);
/* Cache fan-out (kernels/lm_fanout.hip through launch_lm_cache_fanout) on host arrays: source k_src / v_src
 * [layers][G][hkv][cap_src][128] fp16 words and mask_src [G][cap_src]; destination k_dst / v_dst
 * [layers][G * S][hkv][cap_dst][128] and mask_dst [G * S][cap_dst].  Every array is in-out: uploaded, the launch copies
 * positions [0, n) of source sequence g to destination sequence g * S + s, and all six are read back (a source the
 * launch wrote to, or a destination word past n it touched, shows).  ACE_GGML_ERR_INVALID_ARG for what the launcher
 * refuses: G not 1 or 2, S < 1, G * S > 8, n < 1 or past either capacity. */
ACE_GGML_API ace_ggml_status ace_mi_kernel_lm_cache_fanout(int32_t layers, int32_t G, int32_t S, int32_t hkv,
                                                           int32_t cap_src, int32_t cap_dst, int32_t n, uint16_t* k_src,
                                                           uint16_t* v_src, int32_t* mask_src, uint16_t* k_dst,
                                                           uint16_t* v_dst, int32_t* mask_dst);
/* ---- VAE conv kernels (csrc/kernels/vae.hip through launch_conv_gemm / launch_conv_out / launch_pack_f16 /
 * launch_to_f16 of csrc/kernels.h).  One launch each on host buffers, on a stream, blocking.
 * conv_gemm: the integer fields are those of ConvGemmArgs.  S [items][T_in][Cin] and W [N][taps * Cin] fp16 words;
 * bias [N] (transposed conv, up > 1: [Cout]), snake_ea / snake_eb [Cout], W2 [Cout][Cout] fp16, bias2 [Cout], snake2_ea /
 * snake2_eb [N]: f32, any of them may be NULL.  X (f32) and S_out (fp16 words), either may be NULL, are host arrays of
 * guard + items * T_out * Cout + guard elements: the kernel gets the pointer to the payload behind the first guard, the
 * whole array is uploaded before and copied back after the launch, so a caller sees every word that was written.  guard
 * must be a multiple of 4 (the kernel's 16-byte accesses).  The zero row the kernel stages for rows outside [0, T_in) is
 * the 4096-byte zero buffer of VaeEngine.  ACE_MI_VAE_HALO is read by the launch.  INVALID_ARG: a dimension that no
 * buffer can be sized from; ERR: what launch_conv_gemm refuses (message on stderr); X and S_out are untouched in both
 * cases. */
typedef struct ace_mi_conv_gemm_args {
    int32_t T_in, Cin, taps, dil, pad, in_stride, M, N, Cout, up, crop, T_out, resid, store_x, items;
    int32_t guard;
    const uint16_t* S;
    const uint16_t* W;
    const float* bias;
    const float* snake_ea;
    const float* snake_eb;
    const uint16_t* W2;
    const float* bias2;
    const float* snake2_ea;
    const float* snake2_eb;
    float* X;
    uint16_t* S_out;
} ace_mi_conv_gemm_args;
ACE_GGML_API ace_ggml_status ace_mi_kernel_conv_gemm(const ace_mi_conv_gemm_args* args);
/* decoder.conv2: S [items][T][128] fp16 words, W [out_ch][7][128] fp16 words, out = guard + items * T * out_ch + guard
 * f32 (in-out, copied back whole). */
ACE_GGML_API ace_ggml_status ace_mi_kernel_conv_out(const uint16_t* S, int32_t T, int32_t items, const uint16_t* W,
                                                    int32_t out_ch, float* out, int32_t guard);
/* x [rows][C] f32 -> y [rows][Cpad] fp16 words (in-out), columns >= C zero: launch_pack_f16, or launch_to_f16 on the
 * rows * C values when C == Cpad. */
ACE_GGML_API ace_ggml_status ace_mi_kernel_pack_f16(const float* x, int64_t rows, int32_t C, int32_t Cpad, uint16_t* y);
/* Dequant-fused GEMM micro-benchmark: average ms per launch (HIP events). */
ACE_GGML_API ace_ggml_status ace_mi_bench_gemm_q(int32_t qtype, int32_t epi, int32_t variant, int32_t M, int32_t N,
                                                 int32_t K, int32_t iters, float* avg_ms);

/* The GEMM variant table and picker (csrc/gemm_variants.h), without a device.
 * ace_mi_gemm_resolve: the variant launch_gemm would launch for an M x N x K GEMM on weights of format wfmt (0 bf16,
 * 1 fp16, 2 Q8_0, 3 Q4_K, 4 Q6_K) with `forced` as the forced variant (-1 none) and `override_v` as the per-shape
 * override (-1 none); prep != 0: with the fused attention prep's sibling step.
 * ace_mi_gemm_variant_row: the row of base id `id` (INVALID_ARG: no such row): fields = dense kernel {family, BM, BN,
 * WM, WN, depth}, quantized kernel {the same six}, largest dense split-K factor, largest quantized one, prep sibling
 * id, needs N % 256 == 0; family 0 none, 1 gemm_kernel, 2 gemm8_kernel, 3 gemm_ws_kernel, 4 gemm_q_kernel,
 * 5 gemm_qr_kernel (WN = its waves), 6 gemm_wsq_kernel; the row's description into name (may be NULL).
 * ace_mi_gemm_variant_arg_ok: OK if ace_mi_gemm_variant (allow_unchecked = 0) or the self-test entries
 * (allow_unchecked = 1: the 0x10000 bit) accept `variant`. */
ACE_GGML_API ace_ggml_status ace_mi_gemm_resolve(int32_t forced, int32_t override_v, int32_t M, int32_t N, int32_t K,
                                                 int32_t wfmt, int32_t prep, int32_t* variant);
ACE_GGML_API ace_ggml_status ace_mi_gemm_variant_row(int32_t id, int32_t fields[16], char* name, size_t name_size);
ACE_GGML_API ace_ggml_status ace_mi_gemm_variant_arg_ok(int32_t variant, int32_t allow_unchecked);

/* The NEOX RoPE table every engine reads (csrc/runtime/devmem.h, RopeTable), built and copied back: cos_out and
 * sin_out [n][head_dim / 2] f32, positions 0..n-1.
 * ace_mi_rope_table_steps: `steps` ensure(n[i], head_dim[i], theta[i]) calls in a row on one table; rows[i] = the rows
 * the table holds after call i, and cos_out / sin_out receive the final table, rows[steps - 1] rows of
 * head_dim[steps - 1] / 2 values (the caller sizes them for that). */
ACE_GGML_API ace_ggml_status ace_mi_rope_table(int32_t n, int32_t head_dim, float theta, float* cos_out,
                                               float* sin_out);
ACE_GGML_API ace_ggml_status ace_mi_rope_table_steps(int32_t steps, const int32_t* n, const int32_t* head_dim,
                                                     const float* theta, int32_t* rows, float* cos_out,
                                                     float* sin_out);

#ifdef __cplusplus
}
#endif

#endif /* ACESTEP_MI355X_SELFTEST_H */
