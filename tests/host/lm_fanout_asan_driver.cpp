// Stand-alone driver of the cache fan-out entries (ace_mi_lm_fanout / ace_mi_lm_uniforms) over the host-emulated
// kernels, built with -fsanitize=address,undefined by tests/test_lm_fanout_cpu.py: prefill -> fanout -> generate ->
// destroy, the refusals, the re-lay into a larger and a smaller capacity, and the equality of every item of the batched
// loop with its one-item run.  "Device" buffers are host allocations, so a copy past either cache, a logits row written
// past [G * copies][vocab] or a read of the released source cache is reported by the sanitizer.
//   lm_fanout_asan_driver <tied checkpoint>
#include <cstdio>
#include <cstring>
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

static bool same_state(const ace_mi_lm_info& a, const ace_mi_lm_info& b) {
    return a.batch == b.batch && a.capacity == b.capacity && a.cache_len == b.cache_len && a.cache_bytes == b.cache_bytes;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    ace_ggml_init_params ip{};
    ace_ggml_context* ctx = nullptr;
    EXPECT(ace_ggml_create(&ip, &ctx) == ACE_GGML_OK);
    const int V = 1000, n_prompt = 5, n_max = 8, S = 4;
    std::vector<int32_t> ids{5, 6, 7, 8, 9, 0, 0, 11, 12, 13}, mask{1, 1, 1, 1, 1, 0, 0, 1, 1, 1};
    std::vector<float> logits((size_t)2 * S * V);

    EXPECT(ace_mi_lm_fanout(ctx, 2, 16, logits.data(), nullptr) == ACE_GGML_ERR);
    EXPECT(std::strstr(ace_ggml_last_error(ctx), "lm not loaded") != nullptr);
    EXPECT(ace_mi_lm_fanout(nullptr, 2, 16, nullptr, nullptr) == ACE_GGML_ERR_INVALID_ARG);
    EXPECT(ace_mi_lm_uniforms(1, -1, logits.data()) == ACE_GGML_ERR_INVALID_ARG);
    EXPECT(ace_mi_lm_uniforms(1, 4, nullptr) == ACE_GGML_ERR_INVALID_ARG);
    EXPECT(ace_mi_lm_uniforms(1, 0, nullptr) == ACE_GGML_OK);
    EXPECT(ace_mi_load_lm(ctx, argv[1]) == ACE_GGML_OK);

    ace_mi_lm_info before{}, after{};
    EXPECT(ace_mi_lm_fanout(ctx, 2, 16, nullptr, nullptr) == ACE_GGML_ERR_INVALID_ARG);  // no ace_mi_lm_begin
    EXPECT(ace_mi_lm_begin(ctx, 2, n_prompt) == ACE_GGML_OK);
    EXPECT(ace_mi_lm_fanout(ctx, 2, 16, nullptr, nullptr) == ACE_GGML_ERR_INVALID_ARG);  // an empty cache
    EXPECT(ace_mi_lm_forward(ctx, ids.data(), mask.data(), n_prompt, logits.data(), nullptr) == ACE_GGML_OK);
    EXPECT(ace_mi_lm_get_info(ctx, &before) == ACE_GGML_OK);
    EXPECT(ace_mi_lm_fanout(ctx, 0, 16, logits.data(), nullptr) == ACE_GGML_ERR_INVALID_ARG);
    EXPECT(ace_mi_lm_fanout(ctx, 5, 16, logits.data(), nullptr) == ACE_GGML_ERR_INVALID_ARG);  // 10 rows
    EXPECT(ace_mi_lm_fanout(ctx, 2, n_prompt - 1, logits.data(), nullptr) == ACE_GGML_ERR_INVALID_ARG);
    EXPECT(ace_mi_lm_fanout(ctx, 2, before.max_positions + 1, logits.data(), nullptr) == ACE_GGML_ERR_INVALID_ARG);
    EXPECT(ace_mi_lm_get_info(ctx, &after) == ACE_GGML_OK && same_state(before, after));
    EXPECT(ace_mi_lm_fanout(ctx, 1, n_prompt, logits.data(), nullptr) == ACE_GGML_OK);  // changes nothing
    EXPECT(ace_mi_lm_get_info(ctx, &after) == ACE_GGML_OK && same_state(before, after));

    // the batched loop: 4 items under CFG, a candidate list, the duration-constrained stop
    std::vector<int32_t> allowed;
    for (int i = 100; i < 164; ++i) allowed.push_back(i);
    ace_mi_lm_sample_params p{};
    p.cfg_scale = 2.0f;
    p.pre_temperature = 0.85f;
    p.repetition_penalty = 1.1f;
    p.top_k = 8;
    p.top_p = 0.9f;
    p.temperature = 0.85f;
    p.d_allowed = allowed.data();
    p.n_allowed = (int32_t)allowed.size();
    p.stop_id = 7;
    p.min_tokens = n_max;
    const std::vector<float> prompt_logits(logits.begin(), logits.begin() + 2 * V);
    EXPECT(ace_mi_lm_fanout(ctx, S, n_prompt + n_max, logits.data(), nullptr) == ACE_GGML_OK);
    EXPECT(ace_mi_lm_get_info(ctx, &after) == ACE_GGML_OK && after.batch == 2 * S && after.capacity == n_prompt + n_max &&
           after.cache_len == n_prompt);
    for (int r = 0; r < 2 * S; ++r)
        EXPECT(std::memcmp(&logits[(size_t)r * V], &prompt_logits[(size_t)(r / S) * V], V * 4) == 0);
    std::vector<float> u((size_t)n_max * S), col(n_max);
    for (int s = 0; s < S; ++s) {
        EXPECT(ace_mi_lm_uniforms(1000 + s, n_max, col.data()) == ACE_GGML_OK);
        for (int t = 0; t < n_max; ++t) u[(size_t)t * S + s] = col[t];
    }
    std::vector<uint8_t> seen((size_t)S * V, 0);
    std::vector<int32_t> tokens((size_t)S * n_max, -1);
    int32_t n_out = 0;
    EXPECT(ace_mi_lm_generate(ctx, &p, logits.data(), n_max, u.data(), seen.data(), tokens.data(), &n_out, nullptr) ==
           ACE_GGML_OK);
    EXPECT(n_out == n_max);
    EXPECT(ace_mi_lm_get_info(ctx, &after) == ACE_GGML_OK && after.cache_len == n_prompt + n_max - 1);
    EXPECT(ace_mi_lm_fanout(ctx, 1, n_prompt + n_max, nullptr, nullptr) == ACE_GGML_ERR_INVALID_ARG);  // 8 sequences

    // every item against its one-item run
    for (int s = 0; s < S; ++s) {
        std::vector<float> lg((size_t)2 * V);
        std::vector<uint8_t> sn((size_t)V, 0);
        std::vector<int32_t> tk(n_max, -1);
        p.seed = 1000 + s;
        EXPECT(ace_mi_lm_begin(ctx, 2, n_prompt + n_max) == ACE_GGML_OK);
        EXPECT(ace_mi_lm_forward(ctx, ids.data(), mask.data(), n_prompt, lg.data(), nullptr) == ACE_GGML_OK);
        EXPECT(ace_mi_lm_generate(ctx, &p, lg.data(), n_max, nullptr, sn.data(), tk.data(), &n_out, nullptr) == ACE_GGML_OK);
        EXPECT(std::memcmp(tk.data(), &tokens[(size_t)s * n_max], n_max * 4) == 0);
    }

    // one sequence: re-laid into a larger cache, then into the smallest that holds it
    std::vector<int32_t> one{5, 6, 7, 8, 9};
    EXPECT(ace_mi_lm_begin(ctx, 1, n_prompt) == ACE_GGML_OK);
    EXPECT(ace_mi_lm_forward(ctx, one.data(), nullptr, n_prompt, logits.data(), nullptr) == ACE_GGML_OK);
    EXPECT(ace_mi_lm_fanout(ctx, 1, 300, logits.data(), nullptr) == ACE_GGML_OK);
    const int32_t tok[8] = {21, 21, 21, 21, 21, 21, 21, 21};
    EXPECT(ace_mi_lm_forward(ctx, tok, nullptr, 1, logits.data(), nullptr) == ACE_GGML_OK);
    EXPECT(ace_mi_lm_fanout(ctx, 8, n_prompt + 1, logits.data(), nullptr) == ACE_GGML_OK);
    EXPECT(ace_mi_lm_forward(ctx, tok, nullptr, 1, logits.data(), nullptr) == ACE_GGML_ERR_INVALID_ARG);  // full
    EXPECT(ace_mi_lm_get_info(ctx, &after) == ACE_GGML_OK && after.batch == 8 && after.capacity == n_prompt + 1 &&
           after.cache_len == n_prompt + 1);
    ace_ggml_destroy(ctx);
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
