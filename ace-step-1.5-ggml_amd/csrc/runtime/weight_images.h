// Which bytes a DiT GEMM reads for a weight: the resident weights or a 16-bit image of them.  One owner for the images,
// their storage and the policy of when they are written, kept and dropped.  resolve() picks in one fixed order:
//   adapted: rne16(W + eff * B.A) of a matrix a loaded LoRA adapter targets (a quantized matrix reads as WF_BF16, a
//            dense one keeps its format); the resident weights are never written;
//   staged   (ACE_MI_QUANT_STAGED, default on; 0 = the dequant-fused GEMMs): the bf16 images of a layer's quantized
//            block matrices, expanded right before the layer, in stream order, back to back into the layer's arena
//            slot (an adapted matrix's part is not written); bit-identical to the dequant-fused GEMM's LDS tiles.  (A
//            side-stream ring gained nothing and, for Q4_K only, changed the concurrent layer's results: not used.)
//   kept:    the bf16 image of a quantized matrix outside the layer loop, expanded at its first use;
//   resident otherwise.  A raw ggml block matrix always gets an image, in every scope and with ACE_MI_QUANT_STAGED=0.
// ACE_MI_QUANT_STAGE_SCOPE: `model` (default, and any unknown value) = one slot per layer, expanded at the first
// forward and kept while the weights are loaded (an adapter change invalidates); `call` = one slot per layer, kept for
// one sampling call (ForwardIO::reuse_stage); both cost a bf16 image of the block weights (2.8 GB for the 24-layer
// DiT); `layer` = one shared 117 MB slot, expanded before every layer of every forward (low memory), and plane-format
// matrices outside the layer loop stay on the dequant-fused GEMM.
#pragma once

#include <array>
#include <cstdlib>
#include <cstring>
#include <map>

#include "../kernels.h"
#include "devmem.h"
#include "model.h"

namespace acemi {

enum class StageScope { Model, Call, Layer };
using LayerViews = std::array<WeightView, N_BLOCK_WEIGHTS>;  // indexed by BlockWeight

class WeightImages {
   public:
    explicit WeightImages(const DitModel& m) : model_(m) {
        const char* q = std::getenv("ACE_MI_QUANT_STAGED");
        staged_quant_ = !(q && q[0] == '0');
        const char* h = std::getenv("ACE_MI_QUANT_STAGE_SCOPE");
        if (h && std::strcmp(h, "call") == 0) scope_ = StageScope::Call;
        if (h && std::strcmp(h, "layer") == 0) scope_ = StageScope::Layer;
    }
    ~WeightImages() {
        if (ev_) (void)hipEventDestroy(ev_);
    }

    // A forward of the first n_layers layers (0: stages nothing) on s: waits for the images an earlier forward wrote
    // (possibly on another stream), decides whether this one expands its layers, sizes the arena.
    void begin_forward(int n_layers, bool reuse_stage, hipStream_t s) {
        if (ev_) ACEMI_HIP(hipStreamWaitEvent(s, ev_, 0));
        wrote_ = false;
        // whether the layer loop reads arena slots at all: layer 0's gate|up speaks for the plane formats, and a
        // raw-block matrix anywhere is staged whatever ACE_MI_QUANT_STAGED says
        bool any_raw = false;
        for (int li = 0; li < n_layers; ++li)
            for (const DevWeight* w : model_.layers[li].block_weights()) any_raw = any_raw || w->fmt == WF_GGML_RAW;
        arena_on_ = n_layers > 0 && ((staged_quant_ && weight_quantized(model_.layers[0].w_gu.fmt)) || any_raw);
        expand_ = false;
        if (!arena_on_) return;
        slot_bytes_ = 0;
        for (const DevWeight* w : model_.layers[0].block_weights()) slot_bytes_ += wbytes(*w);
        const bool slot_per_layer = scope_ != StageScope::Layer;
        ensure(arena_, slot_bytes_ * (slot_per_layer ? n_layers : 1));
        // model scope: the slots stay valid across calls; call scope: across the steps of one sampling call (its
        // step 0 and any forward outside a sampling call expand); layer scope: never
        const bool keeps = scope_ == StageScope::Model || (scope_ == StageScope::Call && reuse_stage);
        expand_ = !(keeps && kept_layers_ >= n_layers);
        kept_layers_ = slot_per_layer ? n_layers : 0;
    }
    // Records the event the next begin_forward waits on, if this forward wrote an image.
    void end_forward(hipStream_t s) {
        if (!wrote_) return;
        if (!ev_) ACEMI_HIP(hipEventCreateWithFlags(&ev_, hipEventDisableTiming));
        ACEMI_HIP(hipEventRecord(ev_, s));
    }
    bool expanding() const { return expand_; }  // this forward's layer() calls expand (the engine times them)

    // The six block matrices of layer li; expands the layer first when this forward expands.
    LayerViews layer(int li, hipStream_t s) {
        if (expand_) {
            Expander ex;
            char* slot = slot_of(li);
            for (const DevWeight* w : model_.layers[li].block_weights()) {
                if (w->q && resolve(*w, true, slot).image) ex.add(*w, reinterpret_cast<uint16_t*>(slot), s);
                slot += wbytes(*w);
            }
            ex.flush(s);
            wrote_ = true;
        }
        return views(li);
    }
    // The same views without expanding anything (the prefetch sweep of the next layer).
    LayerViews views(int li) const {
        LayerViews v;
        char* slot = slot_of(li);
        int i = 0;
        for (const DevWeight* w : model_.layers[li].block_weights()) {
            v[i++] = resolve(*w, true, slot).v;
            if (slot) slot += wbytes(*w);
        }
        return v;
    }
    // A matrix outside the layer loop; expands its kept image at the first use.
    WeightView matrix(const DevWeight& w, hipStream_t s) {
        Pick r = resolve(w, false, nullptr);
        if (!r.image) return r.v;
        DevBuf& b = kept_[w.q];
        if (!b.p) {
            ensure(b, wbytes(w));
            expand(w, static_cast<uint16_t*>(b.p), s);
            wrote_ = true;
        }
        r.v.q = b.p;
        return r.v;
    }
    // The staged images no longer match what layer() would hand out: the next forward expands again.
    void invalidate() { kept_layers_ = 0; }

    // Adapted images, keyed by the resident weight pointer: the LoRA code allocates (ensure) and writes them, and
    // resolve() reads them while adapter_on.  expand: the bf16 image of a quantized w, the base of its merge.
    std::map<const void*, DevBuf> adapted;
    bool adapter_on = false;
    static void expand(const DevWeight& w, uint16_t* out, hipStream_t s) {
        Expander e;
        e.add(w, out, s);
        e.flush(s);
    }
    static size_t wbytes(const DevWeight& w) { return (size_t)w.rows * w.cols * 2; }

   private:
    // The bf16 images of quantized matrices: plane formats through launch_dequant_bf16_batch (one launch per format),
    // raw-block matrices through launch_dequant_blocks (one job per row segment, one launch per ggml type).
    struct Expander {
        DequantJob planes[8];
        int n_planes = 0;
        std::vector<DequantBlocksJob> blocks;
        void add(const DevWeight& w, uint16_t* out, hipStream_t s) {
            const WeightView v = w.view();
            if (v.fmt == WF_GGML_RAW) {
                for (int i = 0; i < v.n_segs; ++i) blocks.push_back(DequantBlocksJob{v.segs[i], w.cols, w.cols, out});
                return;
            }
            if (n_planes == 8 || (n_planes > 0 && v.fmt != planes[0].w.fmt)) flush_planes(s);
            planes[n_planes++] = DequantJob{v, w.rows, w.cols, out};
        }
        void flush_planes(hipStream_t s) {
            if (n_planes > 0) launch_dequant_bf16_batch(planes, n_planes, s);
            n_planes = 0;
        }
        void flush(hipStream_t s) {
            flush_planes(s);
            if (!blocks.empty()) launch_dequant_blocks(blocks.data(), (int)blocks.size(), s);
        }
    };
    struct Pick {
        WeightView v;
        bool image;  // v reads the staged / kept image at `image`
    };
    // The one place that picks a weight's source, adapted -> image -> resident.  An image is due in the layer loop
    // when this forward reads arena slots and the format is staged; outside it for every raw-block matrix, and for a
    // plane format unless the scope is `layer` or ACE_MI_QUANT_STAGED=0.
    Pick resolve(const DevWeight& w, bool in_layer_loop, const void* image) const {
        Pick r{w.view(), false};
        int fmt = WF_BF16;
        const auto it = adapter_on && w.q ? adapted.find(w.q) : adapted.end();
        if (it != adapted.end() && it->second.p) {
            image = it->second.p;
            if (!weight_quantized(w.fmt)) fmt = w.fmt;
        } else {
            const bool planes_kept = staged_quant_ && scope_ != StageScope::Layer && weight_planes(w.fmt);
            r.image = in_layer_loop ? arena_on_ && stages(w.fmt) : w.q && (w.fmt == WF_GGML_RAW || planes_kept);
            if (!r.image) return r;
        }
        r.v.fmt = fmt;
        r.v.q = image;
        r.v.s = nullptr;
        r.v.ld = w.cols;
        return r;
    }
    bool stages(int fmt) const { return staged_quant_ ? weight_quantized(fmt) : fmt == WF_GGML_RAW; }
    char* slot_of(int li) const {  // layer li's slot; null when this forward reads no slots
        if (!arena_on_) return nullptr;
        return static_cast<char*>(arena_.p) + (scope_ == StageScope::Layer ? 0 : (size_t)li * slot_bytes_);
    }

    const DitModel& model_;
    StageScope scope_ = StageScope::Model;
    bool staged_quant_ = true;
    // this forward (begin_forward): the layer loop reads arena slots / expands them first; an image was written
    bool arena_on_ = false, expand_ = false, wrote_ = false;
    DevBuf arena_;  // one slot per layer, or the one shared slot of the layer scope; allocated once something is staged
    size_t slot_bytes_ = 0;
    int kept_layers_ = 0;                  // layers whose slots hold their images (model / call scope)
    std::map<const void*, DevBuf> kept_;   // keyed by the resident weight pointer
    hipEvent_t ev_ = nullptr;              // created and recorded after a forward that wrote images
};

}  // namespace acemi
