// LyCORIS LoKr adapter reader: lokr_weights.safetensors as the reference trainer saves it
// (acestep/training/lokr_utils.py:184-204: header metadata algo = lokr, format = lycoris and, from the checkpoint
// path, lokr_config = the JSON of configs.py:42-75) -> the DiT decoder modules it adapts, each as the f32 factors of
// its Kronecker delta  dW = kron(w1 [a][b], W2 [c][d])  (kernels.h LokrMergeJob) and the per-module scale.
// Tensor names are "lycoris_" + the module path under the decoder with '.' replaced by '_', then one of the suffixes
// .lokr_w1 | .lokr_w1_a | .lokr_w1_b | .lokr_w2 | .lokr_w2_a | .lokr_w2_b | .alpha | .scalar; the names are built from
// the engine's own module list and looked up (underscores are never parsed back into a path).  a, b, c, d and the ranks
// come from the tensor shapes.  unit = 1 when w1 and W2 are both stored whole, else alpha / r (alpha / sqrt(r) with
// lokr_config.rs_lora), times .scalar when the file has one: eff = scale * unit.  As for LoRA nothing is skipped
// silently: Tucker (lokr_t2), DoRA (dora_scale, weight_decompose), a module the engine does not hold and shapes that
// do not factor the module are refused with a message that names the tensor.
#pragma once

#include <cmath>
#include <map>
#include <string>
#include <vector>

#include "lora.h"

namespace acemi {

struct LokrModule : AdapterModule {  // name: lycoris_layers_{i}_{self_attn|cross_attn|mlp}_{x}_proj
    int a = 0, b = 0, c = 0, d = 0, r1 = 0, r2 = 0;  // r1 / r2 = 0: w1 / W2 stored whole
    float scalar = 1.f;
    std::vector<float> f[6];  // w1, w1_a, w1_b, w2, w2_a, w2_b (empty: not stored)
    bool has_alpha = false;
};

struct LokrAdapter {
    bool rs_lora = false;
    int min_rank = 0, max_rank = 0;
    std::vector<LokrModule> modules;
};

// `dir`/lokr_weights.safetensors when `path` is a directory that holds it and no adapter_config.json, `path` itself
// when it names that file; "" otherwise (a PEFT LoRA directory, or nothing the LoKr reader takes)
inline std::string lokr_weights_file(const std::string& path) {
    static const std::string fn = "lokr_weights.safetensors";
    auto exists = [](const std::string& p) { return (bool)std::ifstream(p, std::ios::binary); };
    if (path.size() >= fn.size() && path.compare(path.size() - fn.size(), fn.size(), fn) == 0 &&
        (path.size() == fn.size() || path[path.size() - fn.size() - 1] == '/'))
        return path;
    if (exists(path + "/" + fn) && !exists(path + "/adapter_config.json")) return path + "/" + fn;
    return "";
}

// max_layers > 0: modules of layers >= max_layers are dropped (ACE_GGML_DIT_MAX_LAYERS: those layers never run)
inline LokrAdapter read_lokr_adapter(const std::string& file, const DitConfig& cfg, int max_layers) {
    StFile st;
    st.open(file);  // IoError names the path
    LokrAdapter ad;
    auto meta = [&](const char* k) {
        const auto it = st.metadata.find(k);
        return it == st.metadata.end() ? std::string() : it->second;
    };
    if (!meta("algo").empty() && meta("algo") != "lokr")
        throw Unsupported(file + ": algo " + meta("algo") + " is not supported (lokr only)");
    if (!meta("lokr_config").empty()) {
        try {
            const Json o = Json::parse(meta("lokr_config"));
            auto flag = [&](const char* k) { return o.kind == Json::Object && o.has(k) && o.at(k).kind != Json::Null && o.at(k).as_bool(); };
            if (flag("weight_decompose")) throw Unsupported(file + ": lokr_config.weight_decompose (DoRA) adapters are not supported");
            if (flag("use_tucker")) throw Unsupported(file + ": lokr_config.use_tucker adapters are not supported");
            ad.rs_lora = flag("rs_lora");
        } catch (const Unsupported&) {
            throw;
        } catch (const std::exception& e) {
            throw InvalidArg(file + ": lokr_config: " + e.what());
        }
    }

    // the engine's module list under the names LyCORIS gives them
    struct Known {
        int layer, block, proj;
    };
    std::map<std::string, Known> known;
    static const char* blocks[3] = {"self_attn", "cross_attn", "mlp"};
    static const char* projs[7] = {"q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"};
    for (int li = 0; li < cfg.layers; ++li)
        for (int bl = 0; bl < 3; ++bl)
            for (int p = (bl == LORA_MLP ? LORA_GATE : LORA_Q); p <= (bl == LORA_MLP ? LORA_DOWN : LORA_O); ++p)
                known["lycoris_layers_" + std::to_string(li) + "_" + blocks[bl] + "_" + projs[p]] = Known{li, bl, p};
    static const char* suffix[6] = {"lokr_w1", "lokr_w1_a", "lokr_w1_b", "lokr_w2", "lokr_w2_a", "lokr_w2_b"};

    std::map<std::string, LokrModule> mods;
    int64_t shp[6][2];
    std::map<std::string, std::vector<int64_t>> shapes;  // module -> 12 dims
    for (const auto& kv : st.tensors) {
        const std::string& key = kv.first;
        const size_t dot = key.find('.');
        const std::string mod = key.substr(0, dot), suf = dot == std::string::npos ? "" : key.substr(dot + 1);
        const auto kn = known.find(mod);
        if (kn == known.end())
            throw Unsupported("lokr tensor " + key + " adapts a module the DiT engine does not hold (" + file + ")");
        if (suf == "lokr_t2") throw Unsupported("lokr tensor " + key + ": Tucker-decomposed adapters are not supported");
        if (suf == "dora_scale") throw Unsupported("lokr tensor " + key + ": DoRA (weight-decomposed) adapters are not supported");
        if (max_layers > 0 && kn->second.layer >= max_layers) continue;  // the one permitted skip: layers that never run
        const StTensor& t = kv.second;
        if (t.dtype != "F32" && t.dtype != "BF16" && t.dtype != "F16")
            throw Unsupported("lokr tensor " + key + " has dtype " + t.dtype + " (F32/BF16/F16 supported)");
        LokrModule& m = mods[mod];
        if (m.name.empty()) {
            m.name = mod;
            m.layer = kn->second.layer;
            m.block = kn->second.block;
            m.proj = kn->second.proj;
            lora_module_dims(cfg, m.block, m.proj, m.in, m.out);
            shapes[mod].assign(12, 0);
        }
        std::vector<float> v = to_f32(t, st.read(t));
        for (float x : v)
            if (!std::isfinite(x)) throw InvalidArg("lokr tensor " + key + " holds a non-finite value");
        if (suf == "alpha" || suf == "scalar") {
            if (v.size() != 1) throw InvalidArg("lokr tensor " + key + " is not a scalar");
            (suf == "alpha" ? m.alpha : m.scalar) = v[0];
            if (suf == "alpha") m.has_alpha = true;
            continue;
        }
        int which = -1;
        for (int i = 0; i < 6; ++i)
            if (suf == suffix[i]) which = i;
        if (which < 0) throw Unsupported("lokr tensor " + key + " is not a tensor the LoKr merge applies");
        if (t.shape.size() != 2 || t.shape[0] < 1 || t.shape[1] < 1) throw InvalidArg("lokr tensor " + key + " is not 2-D");
        shapes[mod][2 * which] = t.shape[0];
        shapes[mod][2 * which + 1] = t.shape[1];
        m.f[which] = std::move(v);
    }

    for (auto& kv : mods) {
        LokrModule& m = kv.second;
        std::memcpy(shp, shapes[kv.first].data(), sizeof(shp));
        const std::string pre = "lokr tensor " + m.name + ".";
        // each factor: whole, or both halves of the product (never both forms, never half a product)
        int64_t dim[2][2], rk[2];
        for (int w = 0; w < 2; ++w) {
            const int full = 3 * w, fa = 3 * w + 1, fb = 3 * w + 2;
            const bool hf = !m.f[full].empty(), ha = !m.f[fa].empty(), hb = !m.f[fb].empty();
            if (hf && (ha || hb)) throw InvalidArg(pre + suffix[full] + " is stored next to its low-rank factors");
            if (!hf && !ha && !hb) throw InvalidArg(pre + suffix[full] + " is missing");
            if (!hf && !ha) throw InvalidArg(pre + suffix[fb] + " has no " + suffix[fa] + " partner");
            if (!hf && !hb) throw InvalidArg(pre + suffix[fa] + " has no " + suffix[fb] + " partner");
            if (hf) {
                dim[w][0] = shp[full][0], dim[w][1] = shp[full][1], rk[w] = 0;
            } else {
                if (shp[fa][1] != shp[fb][0]) throw InvalidArg(pre + suffix[fb] + " has a rank that differs from " + suffix[fa]);
                dim[w][0] = shp[fa][0], dim[w][1] = shp[fb][1], rk[w] = shp[fa][1];
                if (rk[w] > LOKR_MAX_RANK)
                    throw InvalidArg(pre + suffix[fa] + " has rank " + std::to_string(rk[w]) + " (1.." + std::to_string(LOKR_MAX_RANK) + " supported)");
            }
        }
        if (dim[0][0] * dim[1][0] != m.out || dim[0][1] * dim[1][1] != m.in)
            throw Unsupported(pre + "lokr_w1 / lokr_w2: kron([" + std::to_string(dim[0][0]) + ", " + std::to_string(dim[0][1]) + "], [" +
                              std::to_string(dim[1][0]) + ", " + std::to_string(dim[1][1]) + "]) does not factor the module's [" +
                              std::to_string(m.out) + ", " + std::to_string(m.in) + "] weight");
        m.a = (int)dim[0][0], m.b = (int)dim[0][1], m.c = (int)dim[1][0], m.d = (int)dim[1][1];
        m.r1 = (int)rk[0], m.r2 = (int)rk[1];
        if (m.r1 > 0 && m.r2 > 0 && m.r1 != m.r2) throw InvalidArg(pre + "lokr_w1_a and lokr_w2_a have different ranks");
        const int r = m.r2 > 0 ? m.r2 : m.r1;
        if (r == 0) {
            m.unit = 1.f;  // LyCORIS sets alpha = rank when both factors are whole
        } else {
            if (!m.has_alpha) throw InvalidArg(pre + "alpha is missing");
            m.unit = ad.rs_lora ? (float)((double)m.alpha / std::sqrt((double)r)) : (float)((double)m.alpha / (double)r);
        }
        m.unit = m.unit * m.scalar;
        ad.min_rank = ad.modules.empty() ? r : std::min(ad.min_rank, r);
        ad.max_rank = std::max(ad.max_rank, r);
        ad.modules.push_back(std::move(m));
    }
    if (ad.modules.empty()) throw InvalidArg(file + ": no lokr tensors");
    return ad;
}

}  // namespace acemi
