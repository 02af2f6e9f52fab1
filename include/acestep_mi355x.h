/*
 * MI355X extensions of the ACE-Step DiT C-ABI (libacestep_mi355x.so).
 *
 * These add what the reference ABI cannot express (SURVEY §8b "What the
 * build adds"): a device-pointer, batched, stream-ordered forward that
 * removes the per-step host round trip and the serial per-item loop of
 * scripts/run_non_ggml_real_case.py:502-529, and a device-resident Euler
 * sampler equivalent to the C sampler loop acestep_ggml.cpp:2042-2086.
 * All pointers named d_* are HIP device pointers on the context's device;
 * `stream` is a hipStream_t (NULL = the context's own stream).  Calls are
 * asynchronous with respect to the host unless stated otherwise.
 */
#ifndef ACESTEP_MI355X_H
#define ACESTEP_MI355X_H

#include "acestep_ggml.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ace_mi_dit_info {
    int32_t hidden_size;
    int32_t intermediate_size;
    int32_t num_layers;
    int32_t num_heads;
    int32_t num_kv_heads;
    int32_t head_dim;
    int32_t patch_size;
    int32_t in_channels;
    int32_t audio_dim;
    int32_t sliding_window;
    int32_t act_type;       /* 0 = bf16, 1 = fp16 */
    int32_t device;
    int64_t weight_bytes;
} ace_mi_dit_info;

/* Like ace_ggml_create, bound to HIP device `device`. */
ACE_GGML_API ace_ggml_status ace_mi_create_on_device(const ace_ggml_init_params* params, int32_t device,
                                                     ace_ggml_context** out_ctx);

/* Model dimensions of the loaded DiT (ACE_GGML_ERR "dit not loaded" otherwise). */
ACE_GGML_API ace_ggml_status ace_mi_dit_get_info(ace_ggml_context* ctx, ace_mi_dit_info* out);

/* The device formats of the loaded DiT's 2-D weights as a NUL-terminated string (truncated to buf_size): "bf16", "f16",
 * "q8_0 planes" / "q4_K planes" / "q6_K planes" (online quantization, or a GGUF matrix purely of that type),
 * "f32 (fp16 x3)", "ggml raw blocks (<types>)" (GGUF matrices of any other block type, or fused from parts of
 * different block types: the file's bytes, expanded to bf16 by the staged-dequant scopes), comma-separated when mixed. */
ACE_GGML_API ace_ggml_status ace_mi_dit_weight_desc(ace_ggml_context* ctx, char* buf, size_t buf_size);

/* One denoising step for `batch` samples sharing (seq_len, enc_len).
 * d_hidden [B][T][audio], d_context [B][T][in-audio] (either may be NULL = zeros),
 * d_enc [B][L][hidden] (NULL only if enc_len == 0), d_mask [B][T] / d_enc_mask [B][L] int32
 * (NULL = all valid), d_timestep / d_timestep_r [B] f32, d_out [B][T][audio] f32.
 * Result equals `batch` calls of ace_ggml_dit_forward. */
ACE_GGML_API ace_ggml_status ace_mi_dit_forward_batched(ace_ggml_context* ctx, int32_t batch, const float* d_hidden,
                                                        const float* d_context, const float* d_enc,
                                                        const int32_t* d_mask, const int32_t* d_enc_mask,
                                                        int32_t seq_len, int32_t enc_len, const float* d_timestep,
                                                        const float* d_timestep_r, float* d_out, void* stream);

/* ace_mi_dit_forward_batched that also returns cross-attention probabilities (what the reference decoder returns
 * under output_attentions=True with a custom_layers_config; read by get_lyric_timestamp / get_lyric_score):
 * `layers` / `heads` are HOST arrays of n_pairs (layer, head) pairs, d_probs is DEVICE f32
 * [n_pairs][batch][ceil(seq_len / patch)][enc_len] in the caller's pair order, each map
 * softmax(q k^T / sqrt(head_dim) + encoder mask) over the encoder tokens at fp16 operand precision (a masked token is
 * exactly 0, an item whose tokens are all masked is all zeros).  Duplicate pairs are allowed.  early_exit != 0 stops
 * after the last listed layer: d_out is not written and may be NULL.  With early_exit == 0 d_out is bit-identical to
 * ace_mi_dit_forward_batched on the same inputs.  ACE_GGML_ERR_INVALID_ARG with a message naming the value for
 * n_pairs < 1, a layer outside [0, layers), a head outside [0, heads), a layer without a cross-attention block,
 * enc_len <= 0 and a NULL d_probs.  The call leaves no state behind. */
ACE_GGML_API ace_ggml_status ace_mi_dit_forward_capture(ace_ggml_context* ctx, int32_t batch, int32_t seq_len,
                                                        int32_t enc_len, const float* d_hidden,
                                                        const float* d_context, const float* d_enc,
                                                        const int32_t* d_mask, const int32_t* d_enc_mask,
                                                        const float* d_timestep, const float* d_timestep_r,
                                                        int32_t n_pairs, const int32_t* layers, const int32_t* heads,
                                                        int32_t early_exit, float* d_out, float* d_probs,
                                                        void* stream);

/* Euler ODE sampling on the device (acestep_ggml.cpp:2056-2086, mlx_dit/generate.py:154-197):
 * for i in steps: v = DiT(xt, t_i, r = t_i); xt -= v * (t_i - t_{i+1}); last step xt -= v * t_i.
 * d_xt [B][T][audio] holds the initial noise on entry and x0 on return.
 * `schedule` is a HOST array of n_steps timesteps. */
ACE_GGML_API ace_ggml_status ace_mi_dit_sample(ace_ggml_context* ctx, int32_t batch, float* d_xt,
                                               const float* d_context, const float* d_enc, const int32_t* d_mask,
                                               const int32_t* d_enc_mask, int32_t seq_len, int32_t enc_len,
                                               const float* schedule, int32_t n_steps, void* stream);
/* The Python/MLX generation loop (acestep/mlx_dit/generate.py:143-199) on the device: ODE (sde = 0)
 * or SDE (sde = 1: x0 = xt - v*t; xt = t_next*noise_i + (1 - t_next)*x0 with caller noise
 * d_noise [n_steps-1][batch][seq_len][audio]); when d_enc_nc is non-NULL, every step i >= cover_steps
 * runs on the non-cover conditions (generate.py:160): d_enc_nc replaces d_enc and d_context_nc (if
 * non-NULL) replaces d_context.  d_enc_nc = NULL or cover_steps >= n_steps: no switch; a negative
 * cover_steps switches at step 0.  cache_cross = 1 reuses the
 * encoder-side tensors (condition embedder + every layer's cross K/V) between steps with the same
 * conditions, as MLXCrossAttentionCache (use_cache=True) does.  Last step: x0 = xt - v*t. */
ACE_GGML_API ace_ggml_status ace_mi_dit_sample_ex(ace_ggml_context* ctx, int32_t batch, float* d_xt,
                                                  const float* d_context, const float* d_enc, const int32_t* d_mask,
                                                  const int32_t* d_enc_mask, int32_t seq_len, int32_t enc_len,
                                                  const float* schedule, int32_t n_steps, int32_t sde,
                                                  const float* d_noise, int32_t cover_steps,
                                                  const float* d_context_nc, const float* d_enc_nc,
                                                  int32_t cache_cross, void* stream);

/* Operand precision of the DiT's attention MFMAs for subsequent forwards (the ACE_MI_ATTN_PRECISION
 * default is read when the DiT is loaded): 0 = fp16 operands, 1 = `split` (hi/lo fp16 Q.K, fp16 P.V),
 * 2 = `f32` (hi/lo fp16 for both products), 3 = `f8c` (hi/lo for both products, the hi x hi product in fp16 and
 * the two correction products as block-scaled e4m3 MFMAs; the default when ACE_MI_ATTN_PRECISION is unset),
 * 4 = `pv8` (fp16 Q.K, P.V as in f8c).  All accumulate in f32. */
ACE_GGML_API ace_ggml_status ace_mi_dit_set_attn_precision(ace_ggml_context* ctx, int32_t mode);

/* ---- PEFT LoRA adapters on the DiT decoder (the reference handler's load_lora / set_lora_scale / unload_lora,
 * acestep/core/generation/handler/lora/lifecycle.py:30-98).  `adapter_dir` holds adapter_config.json and
 * adapter_model.safetensors as peft writes them: lora_A [r][in] / lora_B [out][r] (F32, BF16 or F16) for the q/k/v/o
 * projections of self_attn / cross_attn and the gate/up/down projections of mlp of decoder layers, r <= 128, per-module
 * ranks, lora_alpha / alpha_pattern / use_rslora honoured.  The engine builds an adapted 16-bit image
 * rne16(W + scale * alpha / r * B.A) of every weight matrix that holds a targeted module and runs its unchanged kernels
 * on the images, so an adapter costs nothing per step; the base weights are never modified.  Anything the engine cannot
 * apply is refused (nothing is skipped silently): ACE_GGML_ERR_IO for a missing file, ACE_GGML_ERR_UNSUPPORTED for
 * DoRA, bias != "none", modules_to_save, a non-LoRA peft_type, a tensor of a module the engine does not hold or the
 * quantized-activation mode (ACE_MI_QUANT_ACT=q8), ACE_GGML_ERR_INVALID_ARG for an unpaired, mis-shaped, rank > 128
 * or non-finite tensor; ace_ggml_last_error names the file or tensor.  A failed load leaves the previous state.
 * All three calls below are synchronous (the device is idle and the context stream drained on return), return
 * ACE_GGML_ERR "dit not loaded" without a model, and must not run concurrently with a forward of the context.
 * ace_ggml_load_dit and ace_ggml_destroy drop the adapter. */
typedef struct ace_mi_lora_info {
    int32_t loaded;          /* 1 while an adapter is resident (also at scale 0) */
    float scale;             /* current strength (0 = the base weights are used) */
    float lora_alpha;        /* adapter_config.json lora_alpha */
    int32_t min_rank;
    int32_t max_rank;
    int32_t num_modules;     /* adapted projections */
    int32_t num_images;      /* adapted weight matrices held as 16-bit images */
    int64_t image_bytes;     /* device memory of the images */
    double merge_ms;         /* host wall time of the last image build (launch to completion) */
} ace_mi_lora_info;
/* Load (replacing any previous adapter) at strength `scale`. */
ACE_GGML_API ace_ggml_status ace_mi_dit_load_lora(ace_ggml_context* ctx, const char* adapter_dir, float scale);
/* Rebuild the images from the base weights at a new strength; 0 routes every matrix back to its base weights and
 * keeps the adapter resident.  ACE_GGML_ERR "lora not loaded" without an adapter. */
ACE_GGML_API ace_ggml_status ace_mi_dit_set_lora_scale(ace_ggml_context* ctx, float scale);
/* Drop the adapter and its images (OK when nothing is loaded). */
ACE_GGML_API ace_ggml_status ace_mi_dit_unload_lora(ace_ggml_context* ctx);
ACE_GGML_API ace_ggml_status ace_mi_dit_lora_info(ace_ggml_context* ctx, ace_mi_lora_info* out);

/* Per-kernel-class timing with hipEvents on the launch stream (adds a sync per kernel).
 * ace_mi_profile_get copies up to `cap` entries: names (NUL-separated into `names`, `names_cap`
 * bytes), total milliseconds and launch counts.  Returns the number of classes in *n_out. */
ACE_GGML_API ace_ggml_status ace_mi_profile_enable(ace_ggml_context* ctx, int32_t on);
ACE_GGML_API ace_ggml_status ace_mi_profile_reset(ace_ggml_context* ctx);
ACE_GGML_API ace_ggml_status ace_mi_profile_get(ace_ggml_context* ctx, char* names, size_t names_cap, double* ms,
                                                int32_t* counts, int32_t cap, int32_t* n_out);

/* Launch `iters` copies of one DiT GEMM of layer 0 with M token rows on the context stream
 * (which: 0 = MLP gate|up, 1 = MLP down).  Used by bench.py for the roofline probe. */
ACE_GGML_API ace_ggml_status ace_mi_probe_gemm(ace_ggml_context* ctx, int32_t which, int32_t m_rows,
                                               int32_t iters);

/* Synchronise the context stream. */
ACE_GGML_API ace_ggml_status ace_mi_synchronize(ace_ggml_context* ctx);

/* Force the GEMM kernel variant of all later launches in this process (-1 = automatic; the ids of
 * csrc/gemm_variants.h: dense 0..16 and 18, quantized 0..5, 7 and 20..25, + 100 S for split-K over S = 2..4 blocks
 * per tile where the row allows it; a variant that does not handle a launch's shape or weights is ignored for that
 * launch; A/B measurements).  The kernel self-test and
 * micro-benchmark entries live in the separate test library (include/acestep_mi355x_selftest.h). */
ACE_GGML_API ace_ggml_status ace_mi_gemm_variant(int32_t variant);

/* VAE decode on device pointers, stream-ordered: latents [n_frames][latent_channels] f32 ->
 * out [out_len][audio_channels] f32 (out_len from ace_mi_vae_out_len: n_frames*hop for even strides). */
ACE_GGML_API ace_ggml_status ace_mi_vae_out_len(ace_ggml_context* ctx, int32_t n_frames, int64_t* out_len);
ACE_GGML_API ace_ggml_status ace_mi_vae_decode_device(ace_ggml_context* ctx, const float* d_latents,
                                                      int32_t n_frames, float* d_out, void* stream);
/* VAE encode on device pointers: audio [n_samples][audio_channels] -> latent mean [enc_out_len][latent]. */
ACE_GGML_API ace_ggml_status ace_mi_vae_enc_out_len(ace_ggml_context* ctx, int32_t n_samples, int64_t* out_len);
ACE_GGML_API ace_ggml_status ace_mi_vae_encode_device(ace_ggml_context* ctx, const float* d_audio,
                                                      int32_t n_samples, float* d_out, void* stream);

/* ggml block quantization (qtype 1 = Q8_0, 2 = Q4_K, 3 = Q6_K) with the encoders the loader uses for
 * ACE_GGML_DIT_WEIGHT_QTYPE (try_quantize_matrix, acestep_dit_model.cpp:156-192): rows x cols f32 ->
 * ggml block bytes.  Returns the byte count written, or -1 (bad type / cols % block / dst too small). */
ACE_GGML_API int64_t ace_mi_quantize(int32_t qtype, const float* src, int64_t rows, int64_t cols, uint8_t* dst,
                                     size_t dst_size);
/* ggml dequantize_row_* of block rows to f32: the three types above and the decode-only ones, 4 = Q4_0, 5 = Q4_1,
 * 6 = Q5_0, 7 = Q5_1, 8 = Q2_K, 9 = Q3_K, 10 = Q5_K, 11 = IQ4_NL (ace_mi_quantize keeps its three). */
ACE_GGML_API ace_ggml_status ace_mi_dequantize(int32_t qtype, const uint8_t* src, int64_t rows, int64_t cols,
                                               float* dst);
/* ---- condition encoders: the conditioning half of
 * ace_generate_audio_style_lyric_timbre_impl (acestep_ggml.cpp:2324-2556) on the GPU.  Host buffers,
 * blocking, like the reference's internal functions they expose. ---- */
typedef struct ace_mi_cond_info {
    int32_t hidden_size;         /* DiT hidden size = width of every condition state */
    int32_t lyric_in_dim;        /* lyric encoder input width (config text_hidden_dim, else 1024) */
    int32_t timbre_in_dim;       /* timbre encoder input width (timbre_hidden_dim, else audio dim, else 64) */
    int32_t text_projector_in;   /* encoder.text_projector in-features (0 = not loaded) */
    int32_t has_lyric_encoder;   /* lyric embed_tokens (or the text-projector fallback) loaded */
    int32_t lyric_layers;
    int32_t has_timbre_encoder;
    int32_t timbre_layers;
} ace_mi_cond_info;
ACE_GGML_API ace_ggml_status ace_mi_cond_get_info(ace_ggml_context* ctx, ace_mi_cond_info* out);

/* ace_project_tokens_linear with encoder.text_projector (acestep_ggml.cpp:1624-1678):
 * states [n_tokens][in_dim] -> out [n_tokens][hidden_size]. */
ACE_GGML_API ace_ggml_status ace_mi_text_project(ace_ggml_context* ctx, const float* states, int32_t n_tokens,
                                                 int32_t in_dim, float* out, size_t out_size);
/* ace_encode_lyric_condition / forward_lyric_encoder (acestep_ggml.cpp:1680-1727,
 * acestep_dit_model.cpp:1562-1651): lyric token embeddings [n_tokens][lyric_in_dim] ->
 * [n_tokens][hidden_size]; ACE_GGML_LYRIC_MAX_LAYERS honoured. */
ACE_GGML_API ace_ggml_status ace_mi_lyric_encode(ace_ggml_context* ctx, const float* lyric_embeds, int32_t n_tokens,
                                                 float* out, size_t out_size);
/* ace_encode_timbre_condition / forward_timbre_encoder (acestep_ggml.cpp:1803-1899,
 * acestep_dit_model.cpp:1653-1737): refer [n_refer][refer_len][timbre_in_dim] -> one token per
 * reference, out [n_refer][hidden_size]; a non-zero order_mask entry is ACE_GGML_ERR_UNSUPPORTED. */
ACE_GGML_API ace_ggml_status ace_mi_timbre_encode(ace_ggml_context* ctx, const float* refer,
                                                  const int32_t* order_mask, int32_t n_refer, int32_t refer_len,
                                                  float* out, size_t out_size);
/* The encoder_hidden_states assembly of ace_generate_audio_style_lyric_timbre_impl
 * (acestep_ggml.cpp:2414-2556): style states [n_style][text_hidden] (text-encoder output) through the
 * text projector, lyric embeddings [n_lyric][text_hidden] through the lyric encoder (copy fallback),
 * timbre references through the timbre encoder, packed lyric | timbre | style with
 * ace_pack_sequences_single_batch (:1729-1801).  Writes out_enc [len][hidden_size] f32,
 * out_mask [len] int32 and *out_len = len (sizes in bytes). */
ACE_GGML_API ace_ggml_status ace_mi_build_condition(ace_ggml_context* ctx, const float* style_states,
                                                    int32_t n_style, const float* lyric_embeds, int32_t n_lyric,
                                                    int32_t text_hidden, const float* refer,
                                                    const int32_t* refer_order_mask, int32_t n_refer,
                                                    int32_t refer_len, float* out_enc, size_t out_enc_size,
                                                    int32_t* out_mask, size_t out_mask_size, int32_t* out_len);

/* ---- the 5 Hz audio-code language model (acestep/llm_inference.py): a HF Qwen3ForCausalLM with a KV cache, driven
 * the way the reference's `pt` backend drives transformers: one prefill `model(input_ids, attention_mask,
 * use_cache=True)`, then single-token calls with `past_key_values` (llm_inference.py:345-367).  The engine supplies
 * the last position's logits; the constrained-decoding FSM stays with the caller, and so do CFG mixing and sampling
 * unless the caller uses ace_mi_lm_select / ace_mi_lm_generate below.
 * d_* are device pointers and the forward is stream-ordered like ace_mi_dit_forward_batched. ---- */
typedef struct ace_mi_lm_info {
    int32_t vocab_size;
    int32_t hidden_size;
    int32_t num_layers;
    int32_t num_heads;
    int32_t num_kv_heads;
    int32_t head_dim;
    int32_t max_positions;   /* max_position_embeddings */
    int32_t tied;            /* 1: the head is the embed_tokens table */
    int32_t act_type;        /* 0 = bf16, 1 = fp16 */
    int32_t batch;           /* of the last ace_mi_lm_begin (0 before it) */
    int32_t capacity;
    int32_t cache_len;       /* positions held per sequence */
    int64_t weight_bytes;
    int64_t cache_bytes;     /* device memory of the KV cache */
} ace_mi_lm_info;
/* Load a HF Qwen3ForCausalLM directory (config.json + model.safetensors, tensor names with or without the "model."
 * prefix; lm_head.weight when present, else the tied embed_tokens.weight, honouring tie_word_embeddings) into a slot
 * of its own: the text encoder of ace_ggml_load_text_encoder / ace_ggml_load_lm stays resident beside it.  16-bit
 * checkpoints only: ACE_GGML_QWEN_WEIGHT_QTYPE, a GGUF file or an F32 embed table are ACE_GGML_ERR_UNSUPPORTED.
 * Frees the KV cache of a previous LM. */
ACE_GGML_API ace_ggml_status ace_mi_load_lm(ace_ggml_context* ctx, const char* model_dir);
ACE_GGML_API ace_ggml_status ace_mi_lm_get_info(ace_ggml_context* ctx, ace_mi_lm_info* out);
/* Allocate (or reuse, when it fits) and reset the KV cache for `batch` sequences (1..8) of up to `capacity`
 * positions (1..max_positions); ACE_GGML_ERR_INVALID_ARG otherwise.  Synchronous. */
ACE_GGML_API ace_ggml_status ace_mi_lm_begin(ace_ggml_context* ctx, int32_t batch, int32_t capacity);
/* Append n tokens per sequence at positions len .. len+n-1 (slot indices, padding included, as transformers does
 * without position_ids) and write the logits of the last appended position: d_ids [batch][n] int32, d_mask [batch][n]
 * int32 or NULL (0 = a padding key no query ever attends to; remembered), d_logits [batch][vocab] f32.  n > 1 is the
 * prefill, allowed on an empty cache only (MFMA GEMMs + causal flash attention); n == 1 is the decode step
 * (kernels/lm_decode.hip), also on an empty cache.  Token ids outside [0, vocab) are clamped into it.
 * ACE_GGML_ERR_INVALID_ARG, with the cache unchanged, when len + n exceeds the capacity or n > 1 on a non-empty
 * cache; ACE_GGML_ERR "lm not loaded" before ace_mi_load_lm. */
ACE_GGML_API ace_ggml_status ace_mi_lm_forward(ace_ggml_context* ctx, const int32_t* d_ids, const int32_t* d_mask,
                                               int32_t n, float* d_logits, void* stream);
/* Cache length back to 0 (batch and capacity kept). */
ACE_GGML_API ace_ggml_status ace_mi_lm_reset(ace_ggml_context* ctx);

/* ---- token selection and the engine-side decode loop (kernels/lm_sample.hip): what the reference's loops do to the
 * logits between two forwards in the audio-code phase, on the GPU.  `batch` rows of logits give S sampled sequences:
 * cfg_scale > 1 mixes row s (conditional) with row s + S (unconditional), S = batch / 2; otherwise S = batch.
 * Per sequence, in this order, every arithmetic step one separately rounded f32 operation:
 *   1. z = u + cfg_scale * (c - u) (cfg_scale > 1), else z = logits
 *   2. candidates: the ids of d_allowed (ascending int32, device; NULL = the whole vocabulary), everything else
 *      -inf; stop_id >= 0 with n_emitted < min_tokens removes stop_id; force_stop leaves only stop_id; a NaN counts
 *      as -inf
 *   3. pre_temperature > 0: z = z / pre_temperature (the constrained processor's phase temperature)
 *   4. repetition_penalty != 1 and d_seen given (bytes [S][vocab], non-zero = seen): z < 0 ? z * p : z / p
 *   5. 0 < top_k < candidates: remove z < the k-th largest z (values equal to it stay)
 *   6. 0 < top_p < 1: with q = softmax(z) over the survivors, keep a value v iff the mass of the survivors strictly
 *      greater than v is <= top_p (equal values stay or go together; the maximum always stays)
 *   7. temperature > 0: p = softmax(z / temperature) over the kept ids; the token is the smallest kept id whose
 *      inclusive cumulative mass, ids ascending, exceeds u * sum(p) (the largest kept id if none does), u in [0, 1)
 *      one f32 per sequence.  temperature <= 0: the argmax, lowest id among equal maxima.
 *   8. the token goes to d_tokens; d_seen[s][token] = 1 where given.
 * If every candidate is -inf the first candidate id is returned. ---- */
typedef struct ace_mi_lm_sample_params {
    float cfg_scale;
    float pre_temperature;
    float repetition_penalty;
    int32_t top_k;
    float top_p;
    float temperature;
    const int32_t* d_allowed;   /* device, ascending, or NULL */
    int32_t n_allowed;
    int32_t stop_id;            /* < 0: none */
    int32_t min_tokens;
    uint64_t seed;              /* ace_mi_lm_generate with d_uniform == NULL */
} ace_mi_lm_sample_params;
/* One selection on the logits [batch][vocab] of the last forward, for callers that keep their own loop: d_uniform [S]
 * f32 (may be NULL when temperature <= 0), d_seen or NULL, n_emitted = tokens emitted so far (step 2), force_stop != 0
 * leaves only stop_id, d_tokens [S] int32.  Stream-ordered like ace_mi_lm_forward.  ACE_GGML_ERR_INVALID_ARG: see
 * ace_mi_lm_generate. */
ACE_GGML_API ace_ggml_status ace_mi_lm_select(ace_ggml_context* ctx, const ace_mi_lm_sample_params* params,
                                              const float* d_logits, const float* d_uniform, uint8_t* d_seen,
                                              int32_t n_emitted, int32_t force_stop, int32_t* d_tokens, void* stream);
/* The decode loop in the engine.  Precondition: the prompt is in the cache (ace_mi_lm_forward) and d_logits
 * [batch][vocab] holds the logits that forward wrote; the buffer is then scratch for the loop's own steps.  Token t <
 * n_max: select on d_logits with n_emitted = t, then (unless t is the last) one decode step that appends the token to
 * both rows of a pair, NULL mask, and writes d_logits again; all on `stream`, no host synchronisation per token.
 * d_tokens [S][n_max] int32.  d_uniform [n_max][S] f32 or NULL: the host then draws n_max * S values from
 * std::mt19937_64(params->seed), in that order, value = (x >> 40) * 2^-24 for each 64-bit output x, into a device
 * buffer before the loop.  A sequence that has emitted stop_id keeps emitting it.
 * stop_id >= 0 and min_tokens < n_max: after every 16th token the host reads a device word (pinned buffer, async
 * copy, event wait) and stops enqueuing once a sequence has emitted stop_id; *n_out = 1 + the index of the first token
 * at which any sequence emitted it (else n_max), entries of d_tokens past *n_out are unspecified, and the cache then
 * holds the prompt and the min(n_max, 16 * ceil(*n_out / 16)) - 1 tokens fed back.  Otherwise *n_out = n_max and the
 * cache grows by n_max - 1 (min_tokens == n_max with a stop_id is the duration-constrained case: the stop token is
 * never a candidate and nothing is polled; the caller appends EOS).  The call returns after a final read of that word.
 * ACE_GGML_ERR_INVALID_ARG, cache and cache_len unchanged: cache_len + n_max - 1 > capacity, n_max < 1, cfg_scale > 1
 * with an odd batch, n_allowed < 1 with a list, stop_id >= vocab, force_stop without a stop_id, or a candidate set
 * that step 2 empties (a one-id list, or a one-id vocabulary, that is the blocked stop_id).  ACE_GGML_ERR "lm not
 * loaded" before ace_mi_load_lm.  ACE_GGML_ERR from a failed launch or copy inside the loop: cache_len is back at its
 * value on entry, d_logits and d_tokens are unspecified, and the caller starts over from ace_mi_lm_begin or
 * ace_mi_lm_reset. */
ACE_GGML_API ace_ggml_status ace_mi_lm_generate(ace_ggml_context* ctx, const ace_mi_lm_sample_params* params,
                                                float* d_logits, int32_t n_max, const float* d_uniform,
                                                uint8_t* d_seen, int32_t* d_tokens, int32_t* n_out, void* stream);

/* ---- one decode loop for the items of a request that share a prompt (kernels/lm_fanout.hip).  Item s of the batched
 * loop gets, token for token, what a one-item run with the same uniforms gets: the prompt is prefilled once, exactly as
 * the one-item run prefills it (a prefill of more rows may pick other GEMM tiles and sum in another order), its cache
 * rows are copied bit for bit, and every kernel of the decode step treats a row independently of the batch.
 * Recommended call order, which keeps the peak at one small source cache plus the destination cache:
 *   1. ace_mi_lm_begin(G, n_prompt)                    G = 2 under CFG (conditional, unconditional), else 1
 *   2. ace_mi_lm_forward with the prompt
 *   3. ace_mi_lm_fanout(S, n_prompt + n_max, d_logits)
 *   4. ace_mi_lm_generate with d_uniform [n_max][S], column s = ace_mi_lm_uniforms(seed of item s, n_max)
 * Meant for the duration-constrained case (min_tokens == n_max, nothing polled), where every item emits the same
 * number of codes; ace_mi_lm_generate, ace_mi_lm_select and their stop semantics are unchanged. ---- */
/* After the prompt is in the cache of a batch of G = 1 or 2 sequences: re-lay the cache for G*copies sequences of up to
 * `capacity` positions; sequence g*copies + s is a bit copy of sequence g (K, V, key mask, cache_len).  d_logits, when
 * not NULL, holds [G][vocab] on entry and [G*copies][vocab] on return (row g*copies + s = row g).  Synchronous, like
 * ace_mi_lm_begin.  copies == 1 with capacity == the current one changes nothing.  The new cache is allocated beside
 * the old one, which is released once the copy has finished.
 * ACE_GGML_ERR_INVALID_ARG, with cache, batch, capacity and cache_len unchanged: copies < 1, G > 2 (or no
 * ace_mi_lm_begin), G*copies > 8, an empty cache, capacity < cache_len, capacity > max_positions.  ACE_GGML_ERR "lm
 * not loaded" before ace_mi_load_lm. */
ACE_GGML_API ace_ggml_status ace_mi_lm_fanout(ace_ggml_context* ctx, int32_t copies, int32_t capacity, float* d_logits,
                                              void* stream);
/* The engine's uniform stream, as ace_mi_lm_generate draws it with d_uniform == NULL and one sequence: n values of
 * std::mt19937_64(seed), (x >> 40) * 2^-24, into out (host).  Lets a caller give every item of a batch its own stream
 * through d_uniform [n_max][S], whatever the grouping. */
ACE_GGML_API ace_ggml_status ace_mi_lm_uniforms(uint64_t seed, int64_t n, float* out);

/* The x_T stream of the reference generator (std::mt19937(seed) + std::normal_distribution<float>,
 * acestep_ggml.cpp:2043-2048) as the generate entries draw it: n values into out (host). */
ACE_GGML_API ace_ggml_status ace_mi_reference_noise(int32_t seed, int64_t n, float* out);

#ifdef __cplusplus
}
#endif

#endif /* ACESTEP_MI355X_H */
