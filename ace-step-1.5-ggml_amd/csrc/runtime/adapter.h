// The adapter a DitEngine holds: a PEFT LoRA (runtime/lora.h) or a LyCORIS LoKr (runtime/lokr.h) read from a path,
// its factors in one device buffer, and the merge jobs of its kind.  The engine says which rows of which image a
// module lands on (a MergeTarget, kernels.h); what the delta of those rows is stays in here.  Header-only, included by
// runtime/engine.cpp alone: the host test library links a fixed list of runtime sources, which this adds nothing to.
#pragma once

#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "../kernels.h"
#include "devmem.h"
#include "engine.h"
#include "lokr.h"
#include "lora.h"

namespace acemi {

class DitAdapter {
   public:
    // Reads and uploads (blocking; nothing of the engine is touched).  `path`: a PEFT directory, or what
    // lokr_weights_file() takes for LoKr.  Throws what the readers throw.
    DitAdapter(const std::string& path, const DitConfig& cfg, int max_layers);

    float scale = 0.f;      // of the images the engine builds from this adapter
    double merge_ms = 0.0;  // of the last rebuild
    // LoRA: lora_alpha and the ranks of the modules; LoKr: the first module's alpha and the ranks of the low-rank
    // factors (0: every factor stored whole)
    float alpha = 0.f;
    int min_rank = 0, max_rank = 0;
    // loaded / scale / lora_alpha / ranks / modules / merge_ms of the engine's report (images are the engine's)
    void info(DitEngine::LoraInfo& i) const;

    // index of the module that adapts (layer, block, proj) (LoraBlock / LoraProj), or -1
    int find(int layer, int block, int proj) const;
    // One job of the next launch(): module `module` merged into the rows of t at `scale`, or with module -1 the
    // copy-through rows of t alone.  rows_mod: the rows the engine's slot has for the module, checked against its shape.
    void add_job(const MergeTarget& t, int rows_mod, int module);
    void clear_jobs();
    void launch(hipStream_t s);

   private:
    // every non-empty host vector into factors_ (256-byte aligned parts, one blocking copy) and its device address
    // into the slot; an empty vector leaves its slot null.  The vectors are released.
    void upload(const std::vector<std::pair<std::vector<float>*, const float**>>& parts);

    bool lokr_ = false;  // the kind: which reader ran, which jobs are built and launched, the messages' prefix
    std::vector<AdapterModule> mods_;
    std::map<std::tuple<int, int, int>, int> index_;
    // per module, the job of its kind with the operands filled and no target yet; then the jobs of the next launch
    std::vector<LoraMergeJob> lora_mods_, lora_jobs_;
    std::vector<LokrMergeJob> lokr_mods_, lokr_jobs_;
    DevBuf factors_;
    DevBuf ws_;  // LoKr: the f32 workspaces of the modules' product factors
};

inline DitAdapter::DitAdapter(const std::string& path, const DitConfig& cfg, int max_layers) {
    std::vector<std::pair<std::vector<float>*, const float**>> parts;
    const std::string lokr_file = lokr_weights_file(path);
    // the readers' results live until upload() has taken the factors
    LoraAdapter lora;
    LokrAdapter lokr;
    if (lokr_file.empty()) {
        lora = read_lora_adapter(path, cfg, max_layers);
        alpha = lora.lora_alpha, min_rank = lora.min_rank, max_rank = lora.max_rank;
        lora_mods_.resize(lora.modules.size());
        for (size_t i = 0; i < lora.modules.size(); ++i) {
            LoraModule& m = lora.modules[i];
            mods_.push_back(m);
            lora_mods_[i].r = m.r;
            lora_mods_[i].rows_mod = m.out;
            parts.emplace_back(&m.A, &lora_mods_[i].A);
            parts.emplace_back(&m.B, &lora_mods_[i].B);
        }
    } else {
        lokr_ = true;
        lokr = read_lokr_adapter(lokr_file, cfg, max_layers);
        alpha = lokr.modules[0].alpha, min_rank = lokr.min_rank, max_rank = lokr.max_rank;
        lokr_mods_.resize(lokr.modules.size());
        for (size_t i = 0; i < lokr.modules.size(); ++i) {
            LokrModule& m = lokr.modules[i];
            LokrMergeJob& j = lokr_mods_[i];
            mods_.push_back(m);
            j.a = m.a, j.b = m.b, j.c = m.c, j.d = m.d, j.r1 = m.r1, j.r2 = m.r2;
            const float** slot[6] = {&j.w1, &j.w1a, &j.w1b, &j.w2, &j.w2a, &j.w2b};
            for (int k = 0; k < 6; ++k) parts.emplace_back(&m.f[k], slot[k]);
        }
    }
    upload(parts);
    size_t ws = 0;  // (the workspace layout is the job's: it depends on which factors upload() found stored)
    for (const LokrMergeJob& j : lokr_mods_) ws += (lokr_ws_floats(j) + 63) & ~size_t(63);
    if (lokr_) ws_.ensure(ws * 4);
    ws = 0;
    for (LokrMergeJob& j : lokr_mods_) {
        j.ws = ws_.as<float>() + ws;
        ws += (lokr_ws_floats(j) + 63) & ~size_t(63);
    }
    for (size_t i = 0; i < mods_.size(); ++i) index_[std::make_tuple(mods_[i].layer, mods_[i].block, mods_[i].proj)] = (int)i;
}

inline void DitAdapter::upload(const std::vector<std::pair<std::vector<float>*, const float**>>& parts) {
    auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
    size_t total = 0;
    for (const auto& p : parts) total += al(p.first->size() * 4);
    std::vector<char> host(total);
    factors_.ensure(total);
    size_t off = 0;
    for (const auto& p : parts) {
        if (p.first->empty()) continue;
        std::memcpy(&host[off], p.first->data(), p.first->size() * 4);
        *p.second = reinterpret_cast<const float*>(factors_.as<char>() + off);
        off += al(p.first->size() * 4);
        *p.first = std::vector<float>();
    }
    ACEMI_HIP(hipMemcpy(factors_.p, host.data(), total, hipMemcpyHostToDevice));
    ACEMI_HIP(hipDeviceSynchronize());  // null-stream copy: done before any stream reads it
}

inline int DitAdapter::find(int layer, int block, int proj) const {
    const auto it = index_.find(std::make_tuple(layer, block, proj));
    return it == index_.end() ? -1 : it->second;
}

inline void DitAdapter::clear_jobs() {
    lora_jobs_.clear();
    lokr_jobs_.clear();
}

inline void DitAdapter::add_job(const MergeTarget& t, int rows_mod, int module) {
    if (module >= 0) {
        const AdapterModule& m = mods_[module];
        ACEMI_CHECK(m.in == t.cols && m.out == rows_mod, std::string(lokr_ ? "lokr" : "lora") + ": module shape does not match the weight");
    }
    const float eff = module >= 0 ? scale * mods_[module].unit : 0.f;
    if (!lokr_) {
        lora_jobs_.push_back(module >= 0 ? lora_mods_[module] : LoraMergeJob{});
        lora_jobs_.back().t = t;
        lora_jobs_.back().eff = eff;
    } else {
        lokr_jobs_.push_back(module >= 0 ? lokr_mods_[module] : LokrMergeJob{});
        lokr_jobs_.back().t = t;
        lokr_jobs_.back().eff = eff;
    }
}

inline void DitAdapter::launch(hipStream_t s) {
    if (lokr_)
        launch_lokr_merge(lokr_jobs_.data(), (int)lokr_jobs_.size(), s);
    else
        launch_lora_merge(lora_jobs_.data(), (int)lora_jobs_.size(), s);
}

inline void DitAdapter::info(DitEngine::LoraInfo& i) const {
    i.loaded = true;
    i.scale = scale;
    i.lora_alpha = alpha;
    i.min_rank = min_rank;
    i.max_rank = max_rank;
    i.modules = (int)mods_.size();
    i.merge_ms = merge_ms;
}

}  // namespace acemi
