"""Raw ggml block weights on the GPU: the expansion kernel (kernels/dequant_blocks.hip) against the numpy restatement of
ggml's CPU dequantize_row_* (tests/ggml_blocks_np.py), bit for bit, and GGUF checkpoints of the decode-only and mixed
block types through the engine's three stage scopes against a BF16 GGUF of the dequantized weights: both sides run the
same dense bf16 GEMMs on equal images, so the forwards are compared bit for bit.  Helpers: tests/test_ggml_blocks_cpu.py."""
import os
import shutil
import tempfile

import numpy as np
import pytest

import ggml_blocks_np as gnp
from test_ggml_blocks_cpu import S, blocks, gguf_pair
from test_lora_cpu import bridge, fwd, inputs

pytestmark = pytest.mark.gpu

ALL_TYPES = gnp.NEW_TYPES + ("q8_0", "q4_k", "q6_k")


@pytest.mark.parametrize("K", [512, 768])
@pytest.mark.parametrize("qtype", ALL_TYPES)
def test_kernel_equals_numpy(qtype, K):
    """N = 5 rows: more than one block per row, 3 K-blocks of 256 at K = 768, an odd row count, a partial tile"""
    from acestep_mi355x import capi
    b = blocks(qtype, 5, K, seed=K + len(qtype))
    got = capi.kernel_dequant_blocks(b, qtype)
    want = gnp.bf16_bits(gnp.dequant(b, qtype))
    if qtype in gnp.NEW_TYPES:
        np.testing.assert_array_equal(got, want)
    else:
        # the three shared types reproduce the plane kernel (test_shared_types_equal_the_planes_kernel), whose zeros are
        # +0 where ggml's d * q is -0 under a negative scale (tests/test_gpu_quant.py): equal but for the sign of zero
        bad = np.argwhere((got != want) & ~(((got | want) & 0x7FFF) == 0))
        assert len(bad) == 0, (len(bad), bad[:8].tolist())


def test_kernel_more_than_one_tile():
    """40 x 768 = 3.75 tiles of 8192 values: tiles that start mid-row and at a block that is not 16-byte aligned"""
    from acestep_mi355x import capi
    for qtype in ("q5_0", "q3_k", "q8_0"):
        b = blocks(qtype, 40, 768, seed=9)
        want = capi.kernel_dequant(b, qtype) if qtype == "q8_0" else gnp.bf16_bits(gnp.dequant(b, qtype))
        np.testing.assert_array_equal(capi.kernel_dequant_blocks(b, qtype), want)


def test_kernel_segments():
    from acestep_mi355x import capi
    K = 512
    q5k, q6k, q40, q80 = blocks("q5_k", 4, K, 1), blocks("q6_k", 2, K, 2), blocks("q4_0", 3, K, 3), blocks("q8_0", 3, K, 4)
    out0 = np.full((13, K), 0xABCD, np.uint16)  # 12 rows + a guard row
    segs = [dict(qtype="q5_k", blocks=q5k, row0=0), dict(qtype="q6_k", blocks=q6k, row0=4),
            dict(qtype="q4_0", blocks=q40, row0=6, step=2), dict(qtype="q8_0", blocks=q80, row0=7, step=2)]
    got = capi.kernel_dequant_segments(out0, segs)
    ref = out0.copy()
    ref[0:4] = gnp.bf16_bits(gnp.dequant(q5k, "q5_k"))
    ref[4:6] = capi.kernel_dequant(q6k, "q6_k")   # (shared types: the plane kernel's bits, zeros +0)
    ref[6:12:2] = gnp.bf16_bits(gnp.dequant(q40, "q4_0"))
    ref[7:12:2] = capi.kernel_dequant(q80, "q8_0")
    np.testing.assert_array_equal(got, ref)
    assert np.all(got[12] == 0xABCD)


def test_kernel_interleaved_groups():
    """the gate | up row map of w_gu: step 2 over 16-row groups, row0 = 0 / 16"""
    from acestep_mi355x import capi
    K = 256
    g, u = blocks("q5_k", 48, K, 5), blocks("q6_k", 48, K, 6)
    got = capi.kernel_dequant_segments(np.zeros((96, K), np.uint16),
                                       [dict(qtype="q5_k", blocks=g, row0=0, step=2, group=16),
                                        dict(qtype="q6_k", blocks=u, row0=16, step=2, group=16)])
    ref = np.zeros((96, K), np.uint16)
    o = np.arange(48)
    ref[(o // 16) * 32 + o % 16] = gnp.bf16_bits(gnp.dequant(g, "q5_k"))
    ref[(o // 16) * 32 + 16 + o % 16] = capi.kernel_dequant(u, "q6_k")
    np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize("qtype", ["q8_0", "q4_k", "q6_k"])
def test_shared_types_equal_the_planes_kernel(qtype):
    from acestep_mi355x import capi
    b = blocks(qtype, 5, 768, seed=7)
    np.testing.assert_array_equal(capi.kernel_dequant_blocks(b, qtype), capi.kernel_dequant(b, qtype))


MODES = {"default": {}, "layer": {"ACE_MI_QUANT_STAGE_SCOPE": "layer"}, "unstaged": {"ACE_MI_QUANT_STAGED": "0"}}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind", ["q5_k_m", "iq4_nl"])
def test_forward_equals_the_bf16_twin(monkeypatch, kind, mode):
    da, db = gguf_pair(kind)
    x = inputs(seed=8, T=40, L=7)
    bb = bridge(None, db)
    ref = fwd(bb, x)
    bb.close()
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    ba = bridge(None, da)
    assert "ggml raw blocks" in ba.dit_weight_desc()
    got = [fwd(ba, x), fwd(ba, x)]
    ba.close()
    assert np.all(np.isfinite(ref)) and float(np.abs(ref).max()) > 0
    for g in got:
        np.testing.assert_array_equal(g.view(np.uint32), ref.view(np.uint32))


def test_q4_0_and_mixed_plane_types_load_and_run():
    for kind in ("q4_0", "q4k_q6k_qkv"):
        da, db = gguf_pair(kind)
        x = inputs(seed=9, T=40, L=7)
        ba, bb = bridge(None, da), bridge(None, db)
        np.testing.assert_array_equal(fwd(ba, x).view(np.uint32), fwd(bb, x).view(np.uint32))
        ba.close()
        bb.close()


def test_text_encoder_q4_1_equals_the_bf16_twin():
    from acestep_mi355x.capi import GGMLCAPIBridge
    s = S()
    base = tempfile.mkdtemp(prefix="acemi_blk_text_")
    s.write_checkpoint(base, s.TEXT_TINY_CONFIG, seed=6, dtype="BF16", specs=s.text_tensor_specs(s.TEXT_TINY_CONFIG))
    da, db = gguf_pair("text_q4_1", base=base, types=lambda n, sh: "Q4_1")
    ids = np.random.default_rng(3).integers(0, s.TEXT_TINY_CONFIG["vocab_size"], size=37).astype(np.int32)
    outs = []
    for d in (da, db):
        br = GGMLCAPIBridge()
        br.load_text_encoder(d)
        outs.append(br.text_encoder_forward(ids))
        br.close()
    assert np.all(np.isfinite(outs[1])) and float(np.abs(outs[1]).max()) > 0
    np.testing.assert_array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
