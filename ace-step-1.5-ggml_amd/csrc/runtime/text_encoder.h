// Qwen3 text encoder resident in HBM: ace_qwen::Model / Config
// (acestep_ggml/cpp/qwen_model.h, qwen_config.cpp:19-64), loaded like load_model_from_dir
// (qwen_model.cpp:340-478) and run like forward_text_encoder_layers (:528-677) — token-embedding
// gather, causal pre-norm blocks on the shared BlockRunner, optional final RMSNorm.
#pragma once

#include <string>
#include <vector>

#include "blocks.h"
#include "model.h"

namespace acemi {

struct TextConfig {
    int vocab = 0, hidden = 0, layers = 0, hq = 0, hkv = 0, intermediate = 0, head_dim = 0, max_pos = 0;
    float eps = 1e-6f, rope_theta = 1000000.0f;
    std::string dtype;
    int tie_word_embeddings = -1;  // config.json tie_word_embeddings: -1 absent, 0 false, 1 true
};

struct TextModel {
    TextConfig cfg;
    void* embed = nullptr;  // [vocab][hidden]: bf16 / fp16 bits as stored, or f32 values (F32 or quantized)
    int embed_fmt = 0;      // launch_embed_rows fmt: 0 bf16, 1 fp16, 2 f32; 3 (LM only): block planes in embed_q, embed null
    DevWeight embed_q;      // embed_fmt 3: the table in Q8_0 / Q4_K / Q6_K planes (the gather reads rows of the planes)
    float* norm = nullptr;  // [hidden]
    std::vector<DevLayer> layers;
    ActType act = ActType::BF16;
    int qtype = 0;
    // causal-LM head (TextLoadOptions::lm_head): [vocab][hidden], lm_head.weight or the tied embed table, in any form
    // Loader::finish gives a matrix (dense 16-bit, block planes, bf16 image); tied: the table's own allocation
    DevWeight head;
    bool tied = false;
    DevArena arena;  // every device allocation above
};

// What ace_mi_load_lm asks of the loader beyond the text encoder's behaviour (all off = ace_ggml_load_text_encoder /
// ace_ggml_load_lm exactly as before).
struct TextLoadOptions {
    bool model_prefix = false;   // also accept the HF causal-LM names "model.<tensor>"
    bool lm_head = false;        // resolve the head: lm_head.weight when the file has it, else the tied embed table
    // ace_mi_load_lm's checkpoint rules: a GGUF comes from the path, dir/model.gguf or ACE_GGML_LM_GGUF alone (the
    // text encoder's keys are not consulted) and keeps its types; a safetensors checkpoint must be 16-bit (no
    // ACE_GGML_QWEN_WEIGHT_QTYPE, no F32 embed table: Unsupported); a plane-typed table stays in planes
    bool lm_checkpoint = false;
};

// Throws std::runtime_error (the ABI reports ACE_GGML_ERR_IO like load_qwen_dir, acestep_ggml.cpp:238-244).
void load_text_model(const std::string& dir, TextModel& m, const TextLoadOptions& opt = TextLoadOptions());

class TextEncoderEngine {
   public:
    TextModel& model() { return model_; }
    BlockShape shape() const;
    // ids [n] (device) -> out [n][hidden] f32 token embeddings
    void embeddings(const int32_t* d_ids, int n, float* d_out, hipStream_t s);
    // forward_text_encoder_layers with causal = true: n_layers < 0 = all; the final norm only when
    // final_norm and every layer ran (:671-674); mask [n] int32 (device) or null
    void forward(const int32_t* d_ids, const int32_t* d_mask, int n, int n_layers, bool final_norm, float* d_out,
                 hipStream_t s);

   private:
    TextModel model_;
    BlockRunner blocks_;
};

}  // namespace acemi
