// PEFT LoRA adapter reader: adapter_config.json + adapter_model.safetensors of one directory -> the DiT decoder
// modules they adapt, as f32 A [r][in] / B [out][r] and the per-module scale alpha / r (alpha / sqrt(r) with
// use_rslora).  The files are those peft's save_pretrained writes for the reference trainer
// (acestep/training/lora_utils.py, configs.py:12-38) and its handler loads (acestep/core/generation/handler/lora/
// lifecycle.py:30-98).  Nothing is skipped silently: whatever the engine cannot apply is refused with a message that
// names the file or tensor (IoError -> ACE_GGML_ERR_IO, Unsupported -> _UNSUPPORTED, InvalidArg -> _INVALID_ARG).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "json.h"
#include "model.h"
#include "safetensors.h"

namespace acemi {

struct InvalidArg : std::runtime_error {
    using std::runtime_error::runtime_error;
};

enum LoraBlock : int { LORA_SELF = 0, LORA_CROSS = 1, LORA_MLP = 2 };
enum LoraProj : int { LORA_Q = 0, LORA_K = 1, LORA_V = 2, LORA_O = 3, LORA_GATE = 4, LORA_UP = 5, LORA_DOWN = 6 };

struct LoraModule {
    std::string name;  // layers.{i}.{self_attn|cross_attn|mlp}.{x}_proj
    int layer = 0, block = 0, proj = 0;
    int r = 0, in = 0, out = 0;
    float alpha = 0.f;
    float unit = 0.f;  // alpha / r or alpha / sqrt(r): eff = scale * unit
    std::vector<float> A, B;
    std::string a_key, b_key;
};

struct LoraAdapter {
    float lora_alpha = 0.f;
    bool rslora = false;
    int min_rank = 0, max_rank = 0;
    std::vector<LoraModule> modules;
};

namespace lora_detail {

inline bool take_prefix(std::string& s, const std::string& p) {
    if (s.compare(0, p.size(), p) != 0) return false;
    s.erase(0, p.size());
    return true;
}

inline std::vector<std::string> split_dots(const std::string& s) {
    std::vector<std::string> out;
    size_t i = 0;
    while (true) {
        const size_t j = s.find('.', i);
        out.push_back(s.substr(i, j == std::string::npos ? j : j - i));
        if (j == std::string::npos) break;
        i = j + 1;
    }
    return out;
}

// "…layers.{i}.{block}.{proj}.lora_{A|B}[.{adapter}].weight" -> module name, layer, block, proj, which (0 A, 1 B);
// false when the key is not a LoRA tensor of a DiT decoder layer
inline bool parse_key(const std::string& key, std::string& name, int& layer, int& block, int& proj, int& which) {
    std::string s = key;
    if (!take_prefix(s, "base_model.model.")) return false;
    take_prefix(s, "decoder.");
    const auto p = split_dots(s);
    if (p.size() != 6 && p.size() != 7) return false;
    if (p[0] != "layers" || p.back() != "weight") return false;
    if (p[1].empty() || p[1].size() > 6 || p[1].find_first_not_of("0123456789") != std::string::npos) return false;
    layer = std::atoi(p[1].c_str());
    if (p[2] == "self_attn")
        block = LORA_SELF;
    else if (p[2] == "cross_attn")
        block = LORA_CROSS;
    else if (p[2] == "mlp")
        block = LORA_MLP;
    else
        return false;
    static const char* names[7] = {"q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"};
    proj = -1;
    for (int i = 0; i < 7; ++i)
        if (p[3] == names[i]) proj = i;
    if (proj < 0 || (block == LORA_MLP) != (proj >= LORA_GATE)) return false;
    if (p[4] == "lora_A")
        which = 0;
    else if (p[4] == "lora_B")
        which = 1;
    else
        return false;
    if (p.size() == 7 && p[5].empty()) return false;  // the adapter-name segment
    name = p[0] + "." + p[1] + "." + p[2] + "." + p[3];
    return true;
}

// peft matches a pattern key against the end of the module name (whole dotted segments)
inline bool pattern_matches(const std::string& module, const std::string& pat) {
    if (pat.empty() || pat.size() > module.size()) return false;
    if (module.compare(module.size() - pat.size(), pat.size(), pat) != 0) return false;
    return pat.size() == module.size() || module[module.size() - pat.size() - 1] == '.';
}

}  // namespace lora_detail

// (in, out) of a decoder module of the loaded model
inline void lora_module_dims(const DitConfig& c, int block, int proj, int& in, int& out) {
    const int H = c.hidden, qd = c.hq * c.head_dim, kd = c.hkv * c.head_dim, I = c.intermediate;
    switch (proj) {
        case LORA_Q: in = H, out = qd; break;
        case LORA_K:
        case LORA_V: in = H, out = kd; break;
        case LORA_O: in = qd, out = H; break;
        case LORA_GATE:
        case LORA_UP: in = H, out = I; break;
        default: in = I, out = H; break;
    }
    (void)block;
}

// max_layers > 0: tensors of layers >= max_layers are dropped (ACE_GGML_DIT_MAX_LAYERS: those layers never run)
inline LoraAdapter read_lora_adapter(const std::string& dir, const DitConfig& cfg, int max_layers) {
    using namespace lora_detail;
    const std::string cfg_path = dir + "/adapter_config.json";
    const std::string st_path = dir + "/adapter_model.safetensors";
    LoraAdapter ad;
    Json o;
    {
        const std::string text = read_file(cfg_path);  // IoError names the path
        try {
            o = Json::parse(text);
        } catch (const std::exception& e) {
            throw IoError(cfg_path + ": " + e.what());
        }
        if (o.kind != Json::Object) throw IoError(cfg_path + ": not a JSON object");
    }
    std::map<std::string, double> alpha_pattern;
    double lora_alpha = 0.0;
    try {
        if (o.has("peft_type") && o.at("peft_type").kind == Json::String && o.at("peft_type").as_str() != "LORA")
            throw Unsupported(cfg_path + ": peft_type " + o.at("peft_type").as_str() + " is not supported (LORA only)");
        if (o.has("use_dora") && o.at("use_dora").kind != Json::Null && o.at("use_dora").as_bool())
            throw Unsupported(cfg_path + ": use_dora adapters are not supported");
        if (o.has("bias") && o.at("bias").kind == Json::String && o.at("bias").as_str() != "none")
            throw Unsupported(cfg_path + ": bias \"" + o.at("bias").as_str() + "\" is not supported (none only)");
        if (o.has("modules_to_save") && o.at("modules_to_save").kind == Json::Array && !o.at("modules_to_save").arr.empty())
            throw Unsupported(cfg_path + ": modules_to_save is not supported");
        if (!o.has("lora_alpha") || o.at("lora_alpha").kind != Json::Number)
            throw InvalidArg(cfg_path + ": lora_alpha missing");
        lora_alpha = o.at("lora_alpha").as_num();
        ad.lora_alpha = (float)lora_alpha;
        ad.rslora = o.has("use_rslora") && o.at("use_rslora").kind != Json::Null && o.at("use_rslora").as_bool();
        if (o.has("alpha_pattern") && o.at("alpha_pattern").kind == Json::Object)
            for (const auto& kv : o.at("alpha_pattern").obj) alpha_pattern[kv.first] = kv.second.as_num();
    } catch (const Unsupported&) {
        throw;
    } catch (const InvalidArg&) {
        throw;
    } catch (const std::exception& e) {
        throw InvalidArg(cfg_path + ": " + e.what());
    }

    StFile st;
    st.open(st_path);  // IoError names the path
    std::map<std::string, LoraModule> mods;
    for (const auto& kv : st.tensors) {
        const std::string& key = kv.first;
        std::string name;
        int layer, block, proj, which;
        if (!parse_key(key, name, layer, block, proj, which))
            throw Unsupported("lora tensor " + key + " adapts a module the DiT engine does not hold (" + st_path + ")");
        if (max_layers > 0 && layer >= max_layers) continue;  // the one permitted skip: layers that never run
        if (layer >= cfg.layers)
            throw Unsupported("lora tensor " + key + " adapts a layer the loaded model does not have");
        const StTensor& t = kv.second;
        if (t.dtype != "F32" && t.dtype != "BF16" && t.dtype != "F16")
            throw Unsupported("lora tensor " + key + " has dtype " + t.dtype + " (F32/BF16/F16 supported)");
        if (t.shape.size() != 2) throw InvalidArg("lora tensor " + key + " is not 2-D");
        LoraModule& m = mods[name];
        m.name = name;
        m.layer = layer;
        m.block = block;
        m.proj = proj;
        lora_module_dims(cfg, block, proj, m.in, m.out);
        const int64_t d0 = t.shape[0], d1 = t.shape[1];
        const int64_t rank = which == 0 ? d0 : d1;
        if ((which == 0 ? d1 : d0) != (which == 0 ? m.in : m.out))
            throw InvalidArg("lora tensor " + key + " has shape [" + std::to_string(d0) + ", " + std::to_string(d1) +
                             "], which does not match the loaded model");
        if (rank < 1 || rank > LORA_MAX_RANK)
            throw InvalidArg("lora tensor " + key + " has rank " + std::to_string(rank) + " (1.." +
                             std::to_string(LORA_MAX_RANK) + " supported)");
        std::string& seen = which == 0 ? m.a_key : m.b_key;
        if (!seen.empty()) throw InvalidArg("lora tensor " + key + " duplicates " + seen);
        seen = key;
        std::vector<float> v = to_f32(t, st.read(t));
        for (float x : v)
            if (!std::isfinite(x)) throw InvalidArg("lora tensor " + key + " holds a non-finite value");
        (which == 0 ? m.A : m.B) = std::move(v);
        if (which == 0) m.r = (int)rank;
    }
    for (auto& kv : mods) {
        LoraModule& m = kv.second;
        if (m.a_key.empty()) throw InvalidArg("lora tensor " + m.b_key + " has no lora_A partner");
        if (m.b_key.empty()) throw InvalidArg("lora tensor " + m.a_key + " has no lora_B partner");
        if ((int64_t)m.B.size() != (int64_t)m.out * m.r)
            throw InvalidArg("lora tensor " + m.b_key + " has a rank that differs from " + m.a_key);
        double alpha = lora_alpha;
        for (const auto& ap : alpha_pattern)
            if (pattern_matches(m.name, ap.first)) alpha = ap.second;
        m.alpha = (float)alpha;
        m.unit = ad.rslora ? (float)(alpha / std::sqrt((double)m.r)) : (float)(alpha / (double)m.r);
        ad.min_rank = ad.modules.empty() ? m.r : std::min(ad.min_rank, m.r);
        ad.max_rank = std::max(ad.max_rank, m.r);
        ad.modules.push_back(std::move(m));
    }
    if (ad.modules.empty()) throw InvalidArg(st_path + ": no lora tensors");
    return ad;
}

}  // namespace acemi
