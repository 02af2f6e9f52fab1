"""The launch sequence of one DiT forward, pinned per mode: the kernel classes the engine's profile records
(name, launches), in first-launch order.  The product forward and the quantized-activation parity mode
(ACE_MI_QUANT_ACT=q8) are one walk of the graph with a narrow seam (DitEngine::walk); this test keeps the two
from drifting apart unnoticed, and keeps a restructuring of the walk from adding, dropping or reordering a launch.

The lists are written out from the graph, not recorded: the tiny checkpoint has 2 layers (sliding, then full), both
with a cross-attention block, and fused cross-k|v weights, so one forward with L > 0 runs
  pack + proj_in, the timestep rows, the key masks, the condition embedder, ONE cross-k|v GEMM for both layers,
  then per layer 3 norms (self, cross, MLP), qkv, self attention, o, cross q, cross attention, cross o, gate|up,
  down, and the head's norm + proj_out:  rmsnorm_mod = 3 * 2 + 1 = 7.
What differs per mode is stated at each list."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T, L = 50, 8  # Np = 25 tokens (odd), 8 condition tokens

LAYERS = [("rmsnorm_mod", 7), ("gemm_qkv", 2), ("attn_self_sliding", 1), ("gemm_o", 2), ("gemm_cross_q", 2),
          ("attn_cross", 2), ("gemm_cross_o", 2), ("gemm_gate_up", 2), ("gemm_down", 2), ("attn_self_full", 1),
          ("gemm_proj_out", 1)]
PRODUCT_HEAD = [("pack_input", 1), ("gemm_proj_in", 1), ("timestep", 1), ("key_bias", 1), ("gemm_condition", 1),
                ("gemm_cross_kv", 1)]
# (env, expected): (a) bf16 weights, defaults: the fused cross-k|v GEMM is followed by one all-layers attn_prep; the
# qkv / cross-q projections prep their attention operands in the GEMM epilogue
MODES = {
    "a_bf16": ({}, PRODUCT_HEAD + [("attn_prep", 1)] + LAYERS),
    # (b) every qkv (2) and cross-q (2) projection stores f32 and runs its own attn_prep: 1 + 4
    "b_unfused_prep": ({"ACE_MI_UNFUSED_PREP": "1"}, PRODUCT_HEAD + [("attn_prep", 5)] + LAYERS),
    # (c) Q8_0 weights through the dequant-fused GEMMs: the same launches as (a), no dequant_stage
    "c_q8_0_unstaged": ({"ACE_GGML_DIT_WEIGHT_QTYPE": "q8_0", "ACE_MI_QUANT_STAGED": "0"},
                        PRODUCT_HEAD + [("attn_prep", 1)] + LAYERS),
    # (d) parity mode: the timestep MLP's six linears (two embedders x l1, l2, proj) time themselves and replace the
    # `timestep` bracket, the key masks are not bracketed, and the cross K/V prep runs once per layer
    "d_quant_act_q8": ({"ACE_GGML_DIT_WEIGHT_QTYPE": "q8_0", "ACE_MI_QUANT_ACT": "q8"},
                       [("pack_input", 1), ("gemm_proj_in", 1), ("timestep_l1", 2), ("timestep_l2", 2),
                        ("timestep_proj", 2), ("gemm_condition", 1), ("gemm_cross_kv", 1), ("attn_prep", 2)] + LAYERS),
    # (e) Q8_0 weights, defaults (staged dequant, model scope): the launches of (a) plus one expansion per layer, the
    # first of them right before layer 0's first norm (WeightImages::layer at the top of the layer loop)
    "e_q8_0_staged": ({"ACE_GGML_DIT_WEIGHT_QTYPE": "q8_0"},
                      PRODUCT_HEAD + [("attn_prep", 1), ("dequant_stage", 2)] + LAYERS),
}


def inputs():
    rng = np.random.default_rng(50)
    h = rng.standard_normal((T, 64)).astype(np.float32)
    c = rng.standard_normal((T, 128)).astype(np.float32)
    e = rng.standard_normal((L, 256)).astype(np.float32)
    mask = np.ones(T, np.int32)
    mask[45:] = 0
    emask = np.ones(L, np.int32)
    emask[6:] = 0
    return h, c, e, mask, emask


def profile(br):
    return [(name, count) for name, _, count in br.profile_get()]


@pytest.mark.parametrize("mode", list(MODES))
def test_forward_launch_sequence(tiny_ckpt, monkeypatch, mode):
    from acestep_mi355x.capi import GGMLCAPIBridge
    env, expected = MODES[mode]
    for k in ("ACE_MI_UNFUSED_PREP", "ACE_GGML_DIT_WEIGHT_QTYPE", "ACE_MI_QUANT_STAGED", "ACE_MI_QUANT_ACT",
              "ACE_MI_QUANT_STAGE_SCOPE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    br = GGMLCAPIBridge()
    try:
        br.load_dit(tiny_ckpt)
        br.profile_enable(True)
        h, c, e, mask, emask = inputs()
        out = br.dit_forward_tfirst(h, c, e, mask, emask, 0.7, 0.4)
        got = profile(br)
    finally:
        br.close()
    assert np.isfinite(out).all()
    assert got == expected


def test_reused_cross_kv_skips_the_condition_side(tiny_ckpt, monkeypatch):
    """Two steps of one sampling call with the cross-attention cache (ForwardIO::reuse_cross, the same enc): the
    second forward launches no gemm_condition, gemm_cross_kv or attn_prep, so those stay at one launch while every
    other class doubles; the call's timestep rows are precomputed once up front."""
    import torch
    from acestep_mi355x.capi import GGMLCAPIBridge
    for k in ("ACE_MI_UNFUSED_PREP", "ACE_GGML_DIT_WEIGHT_QTYPE", "ACE_MI_QUANT_STAGED", "ACE_MI_QUANT_ACT"):
        monkeypatch.delenv(k, raising=False)
    h, c, e, mask, emask = inputs()
    dev = torch.device("cuda:0")
    xt, tc, te, tm, tem = (torch.from_numpy(a[None]).to(dev) for a in (h, c, e, mask, emask))
    torch.cuda.synchronize()
    br = GGMLCAPIBridge()
    try:
        br.load_dit(tiny_ckpt)
        br.profile_enable(True)
        br.dit_sample_ex_device(1, T, L, xt.data_ptr(), tc.data_ptr(), te.data_ptr(), tm.data_ptr(), tem.data_ptr(),
                                [1.0, 0.5], cache_cross=True)
        br.synchronize()
        got = profile(br)
    finally:
        br.close()
    once = {"gemm_condition", "gemm_cross_kv", "attn_prep"}
    expected = [("timestep_precompute", 1)] + [(n, k if n in once else 2 * k) for n, k in MODES["a_bf16"][1]]
    assert torch.isfinite(xt).all()
    assert got == expected
