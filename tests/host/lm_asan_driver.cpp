// Stand-alone driver of the LM entries (ace_mi_load_lm / ace_mi_lm_*) over the host-emulated kernels, built with
// -fsanitize=address,undefined by tests/test_lm_cpu.py: config and tensor-name resolution, the "model." prefix, tied /
// untied head selection, the refusals, and the capacity / argument checks.  "Device" buffers are host allocations.
//   lm_asan_driver <tied> <untied> <no-prefix> <f32> <untied-config-without-head>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/acestep_mi355x.h"

static int failures = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                               \
        }                                                             \
    } while (0)

static bool finite(const std::vector<float>& v) {
    for (float x : v)
        if (!std::isfinite(x)) return false;
    return true;
}

int main(int argc, char** argv) {
    if (argc < 6) return 2;
    ace_ggml_init_params p{};
    ace_ggml_context* ctx = nullptr;
    EXPECT(ace_ggml_create(&p, &ctx) == ACE_GGML_OK);
    ace_mi_lm_info info{};
    std::vector<int32_t> ids{5, 6, 7, 8, 9, 0, 0, 11, 12, 13}, mask{1, 1, 1, 1, 1, 0, 0, 1, 1, 1};
    std::vector<float> logits(2 * 1000);

    EXPECT(ace_mi_lm_forward(ctx, ids.data(), nullptr, 1, logits.data(), nullptr) == ACE_GGML_ERR);
    EXPECT(std::strstr(ace_ggml_last_error(ctx), "lm not loaded") != nullptr);
    EXPECT(ace_mi_lm_begin(ctx, 1, 8) == ACE_GGML_ERR);
    EXPECT(ace_mi_lm_get_info(ctx, &info) == ACE_GGML_ERR);
    EXPECT(ace_mi_load_lm(ctx, nullptr) == ACE_GGML_ERR_INVALID_ARG);
    EXPECT(ace_mi_load_lm(ctx, "/nonexistent/lm") == ACE_GGML_ERR_IO);
    EXPECT(ace_mi_load_lm(ctx, argv[4]) == ACE_GGML_ERR_UNSUPPORTED);  // F32 checkpoint
    EXPECT(ace_mi_load_lm(ctx, argv[5]) == ACE_GGML_ERR_IO);           // tie_word_embeddings false, no lm_head
    EXPECT(std::strstr(ace_ggml_last_error(ctx), "lm_head.weight") != nullptr);
    setenv("ACE_GGML_QWEN_WEIGHT_QTYPE", "q8_0", 1);
    EXPECT(ace_mi_load_lm(ctx, argv[1]) == ACE_GGML_ERR_UNSUPPORTED);
    EXPECT(std::strstr(ace_ggml_last_error(ctx), "quantized LM weights are not supported") != nullptr);
    unsetenv("ACE_GGML_QWEN_WEIGHT_QTYPE");

    for (int which = 1; which <= 3; ++which) {  // tied, untied, names without "model."
        EXPECT(ace_mi_load_lm(ctx, argv[which]) == ACE_GGML_OK);
        EXPECT(ace_mi_lm_get_info(ctx, &info) == ACE_GGML_OK);
        EXPECT(info.tied == (which == 2 ? 0 : 1) && info.vocab_size == 1000 && info.batch == 0 && info.cache_len == 0);
        EXPECT(ace_mi_lm_forward(ctx, ids.data(), nullptr, 1, logits.data(), nullptr) == ACE_GGML_ERR_INVALID_ARG);  // no begin
        EXPECT(ace_mi_lm_begin(ctx, 0, 8) == ACE_GGML_ERR_INVALID_ARG);
        EXPECT(ace_mi_lm_begin(ctx, 9, 8) == ACE_GGML_ERR_INVALID_ARG);
        EXPECT(ace_mi_lm_begin(ctx, 1, 0) == ACE_GGML_ERR_INVALID_ARG);
        EXPECT(ace_mi_lm_begin(ctx, 1, info.max_positions + 1) == ACE_GGML_ERR_INVALID_ARG);
        EXPECT(ace_mi_lm_begin(ctx, 2, 7) == ACE_GGML_OK);
        EXPECT(ace_mi_lm_forward(ctx, nullptr, nullptr, 1, logits.data(), nullptr) == ACE_GGML_ERR_INVALID_ARG);
        EXPECT(ace_mi_lm_forward(ctx, ids.data(), nullptr, 0, logits.data(), nullptr) == ACE_GGML_ERR_INVALID_ARG);
        EXPECT(ace_mi_lm_forward(ctx, ids.data(), mask.data(), 8, logits.data(), nullptr) == ACE_GGML_ERR_INVALID_ARG);  // > capacity
        EXPECT(ace_mi_lm_forward(ctx, ids.data(), mask.data(), 5, logits.data(), nullptr) == ACE_GGML_OK);  // left-padded row 1
        EXPECT(finite(logits));
        EXPECT(ace_mi_lm_forward(ctx, ids.data(), nullptr, 2, logits.data(), nullptr) == ACE_GGML_ERR_INVALID_ARG);  // prefill, non-empty
        const int32_t tok[2] = {21, 21}, one[2] = {1, 1};
        EXPECT(ace_mi_lm_forward(ctx, tok, one, 1, logits.data(), nullptr) == ACE_GGML_OK);
        EXPECT(ace_mi_lm_forward(ctx, tok, nullptr, 1, logits.data(), nullptr) == ACE_GGML_OK);
        EXPECT(finite(logits));
        EXPECT(ace_mi_lm_forward(ctx, tok, nullptr, 1, logits.data(), nullptr) == ACE_GGML_ERR_INVALID_ARG);  // 8 > 7
        EXPECT(ace_mi_lm_get_info(ctx, &info) == ACE_GGML_OK && info.cache_len == 7 && info.capacity == 7 && info.batch == 2);
        EXPECT(ace_mi_lm_reset(ctx) == ACE_GGML_OK);
        const int32_t wild[2] = {-4, 1 << 30};  // ids nobody validated: clamped into the table
        EXPECT(ace_mi_lm_forward(ctx, wild, nullptr, 1, logits.data(), nullptr) == ACE_GGML_OK);  // n == 1 on an empty cache
        EXPECT(finite(logits));
        EXPECT(ace_mi_lm_begin(ctx, 1, 300) == ACE_GGML_OK);  // regrown; then past the split threshold of the decode attention
        std::vector<int32_t> many(258, 3);
        EXPECT(ace_mi_lm_forward(ctx, many.data(), nullptr, 258, logits.data(), nullptr) == ACE_GGML_OK);
        EXPECT(ace_mi_lm_forward(ctx, tok, nullptr, 1, logits.data(), nullptr) == ACE_GGML_OK);
        EXPECT(finite(std::vector<float>(logits.begin(), logits.begin() + 1000)));
        EXPECT(ace_mi_lm_begin(ctx, 2, 7) == ACE_GGML_OK);  // back to a small cache inside the regrown buffers
        EXPECT(ace_mi_lm_forward(ctx, ids.data(), mask.data(), 5, logits.data(), nullptr) == ACE_GGML_OK);
        EXPECT(ace_mi_lm_forward(ctx, tok, one, 1, logits.data(), nullptr) == ACE_GGML_OK);
        EXPECT(finite(logits));
    }
    ace_ggml_destroy(ctx);
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
