"""When the 16-bit images of quantized weights are expanded, kept and dropped (runtime/weight_images.h), pinned by
launch counts on the CPU: the cumulative number of `dequant_stage` brackets in the engine's profile, one per layer
expansion, read after each forward of a fixed sequence on the host-emulation library (its profiling events are stubs).
Output bits cannot show a redundant re-expansion (same bits, slower) or a stale image that happens to come from the
same weights; the counts can.

Every list is written out from the policy, for the tiny 2-layer checkpoint:
  model scope: a layer is expanded once and kept while the weights are loaded; a change of the adapter drops the
               images, so the next forward expands both layers again;
  call scope:  kept for one sampling call (expanded at its step 0); a forward outside a sampling call expands;
  layer scope: one shared slot, expanded before every layer of every forward;
  ACE_MI_QUANT_STAGED=0: plane formats run the dequant-fused GEMMs and nothing is expanded; raw ggml blocks, which no
               GEMM reads, are still expanded under the scope's rules."""
import os

import numpy as np
import pytest

from hostlib import CLANG, build_host_lib
from test_ggml_blocks_cpu import gguf_pair
from test_lora_cpu import adapter, base_ckpt, bridge, fwd, inputs, target_sets

ENV = ("ACE_GGML_DIT_WEIGHT_QTYPE", "ACE_MI_QUANT_STAGED", "ACE_MI_QUANT_STAGE_SCOPE", "ACE_MI_QUANT_ACT",
       "ACE_GGML_DIT_MAX_LAYERS", "ACE_MI_WEIGHT_PREFETCH")


@pytest.fixture(scope="module")
def host_lib():
    if not os.path.exists(CLANG):
        pytest.skip("host clang++ not available")
    return build_host_lib()


@pytest.fixture()
def env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def profiled(lib, ckpt):
    br = bridge(lib, ckpt)
    br.profile_enable(True)
    return br


def stages(br):
    """cumulative launches of the per-layer expansion bracket (0: never recorded)"""
    return dict((name, count) for name, _, count in br.profile_get()).get("dequant_stage", 0)


# forward, forward, load_lora (all targets, scale 1), forward, forward, unload_lora, forward
SEQUENCE = {
    ("model", "1"): [2, 2, 4, 4, 6],
    ("call", "1"): [2, 4, 6, 8, 10],
    ("layer", "1"): [2, 4, 6, 8, 10],
    ("model", "0"): [0, 0, 0, 0, 0],
}


@pytest.mark.parametrize("scope,staged", list(SEQUENCE))
def test_expansions_over_forwards_and_adapter_changes(host_lib, env, scope, staged):
    env.setenv("ACE_GGML_DIT_WEIGHT_QTYPE", "q8_0")
    env.setenv("ACE_MI_QUANT_STAGE_SCOPE", scope)
    env.setenv("ACE_MI_QUANT_STAGED", staged)
    x = inputs()
    br = profiled(host_lib, base_ckpt())
    got = []
    try:
        for step in ("fwd", "fwd", "load", "fwd", "fwd", "unload", "fwd"):
            if step == "load":
                br.load_lora(adapter(targets=target_sets()["all"]), 1.0)
            elif step == "unload":
                br.unload_lora()
            else:
                assert np.isfinite(fwd(br, x)).all()
                got.append(stages(br))
    finally:
        br.close()
    assert got == SEQUENCE[(scope, staged)]


def test_call_scope_expands_once_per_sampling_call(host_lib, env):
    """4 steps of one ace_mi_dit_sample_ex call: step 0 expands both layers, steps 1..3 reuse the images"""
    env.setenv("ACE_GGML_DIT_WEIGHT_QTYPE", "q8_0")
    env.setenv("ACE_MI_QUANT_STAGE_SCOPE", "call")
    h, c, e = inputs(T=16, L=4)
    p = lambda a: a.ctypes.data
    br = profiled(host_lib, base_ckpt())
    got = []
    try:
        for _ in range(2):
            xt, cc, ee = h[None].copy(), c[None].copy(), e[None].copy()
            br.dit_sample_ex_device(1, h.shape[0], e.shape[0], p(xt), p(cc), p(ee), 0, 0, [1.0, 0.75, 0.5, 0.25])
            br.synchronize()
            assert np.isfinite(xt).all()
            got.append(stages(br))
    finally:
        br.close()
    assert got == [2, 4]


def test_model_scope_expands_the_layers_a_shorter_forward_left_out(host_lib, env):
    """ACE_GGML_DIT_MAX_LAYERS=1 first (layer 0 expanded, a one-slot arena), then both layers: the kept images do not
    cover layer 1, and the grown arena is a new allocation, so that forward expands both; the next one expands none"""
    env.setenv("ACE_GGML_DIT_WEIGHT_QTYPE", "q8_0")
    x = inputs()
    br = profiled(host_lib, base_ckpt())
    got = []
    try:
        env.setenv("ACE_GGML_DIT_MAX_LAYERS", "1")
        fwd(br, x)
        got.append(stages(br))
        env.delenv("ACE_GGML_DIT_MAX_LAYERS")
        for _ in range(2):
            fwd(br, x)
            got.append(stages(br))
    finally:
        br.close()
    assert got == [1, 3, 3]


def test_unstaged_mode_still_expands_raw_blocks(host_lib, env):
    """ACE_MI_QUANT_STAGED=0 on the mixed GGUF (q|k|v fuses Q4_K and Q6_K parts = raw blocks; o, gate|up, down are
    Q4_K planes): the layers are expanded for the raw qkv alone, under the model scope's rules"""
    env.setenv("ACE_MI_LIB", host_lib)  # the GGUF writer quantizes through capi's default library
    da, _ = gguf_pair("q4k_q6k_qkv")
    env.setenv("ACE_MI_QUANT_STAGED", "0")
    x = inputs(seed=5)
    br = profiled(host_lib, da)
    got = []
    try:
        for _ in range(2):
            fwd(br, x)
            got.append(stages(br))
    finally:
        br.close()
    assert got == [2, 2]
