// Operand blocks of the transformer-layer walks (DitEngine::walk, BlockRunner::run): every kind of PrepArgs,
// AttnArgs and GemmEpilogue the walks launch with is filled in here and nowhere else.
#pragma once

#include <cmath>

#include "../kernels.h"

namespace acemi {

// Which attention operands carry a second (lo) plane: AttnArgs::split / pv_split / f8.  A prep writes a lo plane
// only where the attention reads one, so the plane offsets are zeroed from the same three flags.
struct AttnPlanes {
    bool split, pv_split, f8;
};

// The query side of one attention call: B items of n tokens (padded to n_pad), the head counts and width.
struct AttnDims {
    int B, hq, hkv, D, n, n_pad;
    float eps;  // of the q / k RMSNorms
    int qd() const { return hq * D; }
    int kd() const { return hkv * D; }
    int64_t q_plane() const { return (int64_t)B * hq * n_pad * D; }   // lo plane offsets (elements)
    int64_t k_plane() const { return (int64_t)B * hkv * n_pad * D; }  // self-attention keys / values
};

// Self-attention [q | k | v] rows -> QK-RMSNorm, RoPE, attention layouts.  src / ld: the f32 rows attn_prep reads
// (null / 0 when the prep runs in the GEMM's epilogue, EPI_QKV_PREP).
inline PrepArgs self_prep(const AttnDims& d, AttnPlanes p, const float* src, int ld, const float* q_norm,
                          const float* k_norm, const float* rope_cos, const float* rope_sin, uint16_t* qh,
                          uint16_t* kh, uint16_t* vt) {
    PrepArgs pa{};
    pa.src = src;
    pa.ld = ld;
    pa.q_col = 0;
    pa.k_col = d.qd();
    pa.v_col = d.qd() + d.kd();
    pa.hq = d.hq;
    pa.hkv = d.hkv;
    pa.n_tok = d.n;
    pa.n_pad = d.n_pad;
    pa.B = d.B;
    pa.q_norm = q_norm;
    pa.k_norm = k_norm;
    pa.rope_cos = rope_cos;
    pa.rope_sin = rope_sin;
    pa.eps = d.eps;
    pa.qh = qh;
    pa.kh = kh;
    pa.vt = vt;
    pa.q_plane = p.split ? d.q_plane() : 0;
    pa.k_plane = p.split ? d.k_plane() : 0;
    pa.v_plane = p.pv_split ? d.k_plane() : 0;
    pa.f8 = p.f8 ? 1 : 0;
    return pa;
}

// Cross-attention queries: q section only, no RoPE.
inline PrepArgs cross_q_prep(const AttnDims& d, AttnPlanes p, const float* q_norm, uint16_t* qh) {
    PrepArgs pa{};
    pa.q_col = 0;
    pa.k_col = -1;
    pa.v_col = -1;
    pa.hq = d.hq;
    pa.hkv = d.hkv;
    pa.n_tok = d.n;
    pa.n_pad = d.n_pad;
    pa.B = d.B;
    pa.q_norm = q_norm;
    pa.eps = d.eps;
    pa.qh = qh;
    pa.q_plane = p.split ? d.q_plane() : 0;
    pa.f8 = p.f8 ? 1 : 0;
    return pa;
}

// Cross-attention keys / values of one layer from its [k | v] rows src (L tokens per item, padded to Lpad), into
// that layer's kh / vt; lo_plane: where the lo planes of the all-layers kh / vt buffers start.  With k_norm_layers
// (a device table of every layer's k-norm weights) one launch covers `layers` consecutive layers, starting at
// this one (PrepArgs::layers).
inline PrepArgs cross_kv_prep(const AttnDims& d, AttnPlanes p, int L, int Lpad, const float* src, int ld,
                              const float* k_norm, uint16_t* kh, uint16_t* vt, int64_t lo_plane, int layers = 1,
                              const float* const* k_norm_layers = nullptr) {
    PrepArgs pa{};
    pa.src = src;
    pa.ld = ld;
    pa.q_col = -1;
    pa.k_col = 0;
    pa.v_col = d.kd();
    pa.hq = d.hq;
    pa.hkv = d.hkv;
    pa.n_tok = L;
    pa.n_pad = Lpad;
    pa.B = d.B;
    pa.k_norm = k_norm;
    pa.eps = d.eps;
    pa.kh = kh;
    pa.vt = vt;
    pa.k_plane = p.split ? lo_plane : 0;
    pa.v_plane = p.pv_split ? lo_plane : 0;
    pa.f8 = p.f8 ? 1 : 0;
    if (k_norm_layers) {
        pa.layers = layers;
        pa.src_layer = 2 * d.kd();
        pa.kh_layer = (int64_t)d.B * d.hkv * Lpad * d.D;
        pa.vt_layer = (int64_t)d.B * d.hkv * d.D * Lpad;
        pa.k_norm_layers = k_norm_layers;
    }
    return pa;
}

// One attention call of d's queries (q) over nk keys (padded to nk_pad) in k / vt, whose lo planes start kv_plane
// elements in.  out_f32 set: f32 rows instead of `out`.
inline AttnArgs attn_args(const AttnDims& d, AttnPlanes p, const uint16_t* q, const uint16_t* k, const uint16_t* vt,
                          const float* kbias, int nk, int nk_pad, int64_t kv_plane, int window, bool causal,
                          float* part, uint16_t* out, float* out_f32 = nullptr) {
    AttnArgs aa{};
    aa.q = q;
    aa.k = k;
    aa.vt = vt;
    aa.kbias = kbias;
    aa.part = part;
    aa.out = out;
    aa.out_f32 = out_f32;
    aa.B = d.B;
    aa.Hq = d.hq;
    aa.Hkv = d.hkv;
    aa.nq = d.n;
    aa.nq_pad = d.n_pad;
    aa.nk = nk;
    aa.nk_pad = nk_pad;
    aa.window = window;
    aa.causal = causal;
    aa.scale = 1.0f / std::sqrt((float)d.D);
    aa.split = p.split;
    aa.pv_split = p.pv_split;
    aa.f8 = p.f8;
    aa.q_plane = d.q_plane();
    aa.k_plane = kv_plane;
    aa.v_plane = kv_plane;
    return aa;
}

// The probabilities of n_heads listed heads of d's queries (q) over nk keys in k (launch_attn_probs: the hi planes
// only), head i into map slots[i] of out.
inline AttnProbArgs attn_prob_args(const AttnDims& d, const uint16_t* q, const uint16_t* k, const float* kbias, int nk,
                                   int nk_pad, int n_heads, const int* heads, const int* slots, float* out) {
    AttnProbArgs pa{};
    pa.q = q;
    pa.k = k;
    pa.kbias = kbias;
    pa.B = d.B;
    pa.Hq = d.hq;
    pa.Hkv = d.hkv;
    pa.nq = d.n;
    pa.nq_pad = d.n_pad;
    pa.nk = nk;
    pa.nk_pad = nk_pad;
    pa.scale = 1.0f / std::sqrt((float)d.D);
    pa.n_heads = n_heads;
    pa.heads = heads;
    pa.slots = slots;
    pa.out = out;
    return pa;
}

// ---- the GEMM epilogues of the walks (GemmEpiKind)
inline GemmEpilogue epi_store_f32(float* c, int ldc, const float* bias = nullptr) {
    GemmEpilogue e;
    e.kind = EPI_STORE_F32;
    e.bias = bias;
    e.c_f32 = c;
    e.ldc = ldc;
    return e;
}
inline GemmEpilogue epi_store_act(uint16_t* c, int ldc, const float* bias) {
    GemmEpilogue e;
    e.kind = EPI_STORE_ACT;
    e.bias = bias;
    e.c_act = c;
    e.ldc = ldc;
    return e;
}
inline GemmEpilogue epi_resid(float* c, int ldc) {
    GemmEpilogue e;
    e.kind = EPI_RESID;
    e.c_f32 = c;
    e.ldc = ldc;
    return e;
}
inline GemmEpilogue epi_resid_gated(float* c, int ldc, const float* gate, int64_t gate_stride, int rows_per_item) {
    GemmEpilogue e;
    e.kind = EPI_RESID_GATED;
    e.c_f32 = c;
    e.ldc = ldc;
    e.gate = gate;
    e.gate_stride = gate_stride;
    e.rows_per_item = rows_per_item;
    return e;
}
inline GemmEpilogue epi_swiglu(uint16_t* c, int ldc) {
    GemmEpilogue e;
    e.kind = EPI_SWIGLU;
    e.c_act = c;
    e.ldc = ldc;
    return e;
}
inline GemmEpilogue epi_swiglu(float* c, int ldc) {  // the quantized-activation GEMM only
    GemmEpilogue e;
    e.kind = EPI_SWIGLU_F32;
    e.c_f32 = c;
    e.ldc = ldc;
    return e;
}
inline GemmEpilogue epi_proj_out(float* out, const float* bias, int rows_per_item, int T, int out_ch, int patch) {
    GemmEpilogue e;
    e.kind = EPI_PROJ_OUT;
    e.bias = bias;
    e.c_f32 = out;
    e.rows_per_item = rows_per_item;
    e.out_T = T;
    e.out_ch = out_ch;
    e.patch = patch;
    return e;
}
inline GemmEpilogue epi_qkv_prep(const PrepArgs& pa) {
    GemmEpilogue e;
    e.kind = EPI_QKV_PREP;
    e.prep = pa;
    return e;
}

}  // namespace acemi
