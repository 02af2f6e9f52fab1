"""GGUF checkpoints in every common ggml block type, mixed or not, on the CPU: the reader's type table, the host
dequantize against an independent numpy restatement (tests/ggml_blocks_np.py), layout cross-checks that do not rest on
one reading of the structs, and the loader / engine bookkeeping of raw-block matrices in the host-emulation library.
A raw-block checkpoint and a BF16 GGUF holding rne_bf16(numpy dequant) of the same matrices put identical bf16 images
in front of the same dense GEMMs, so their forwards are compared bit for bit.  The gfx950 kernel and the HIP path are
in tests/test_gpu_ggml_blocks.py, which borrows this module's helpers."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import ggml_blocks_np as gnp
from hostlib import CLANG, CSRC, build_host_lib
from test_lora_cpu import adapter, base_ckpt, bridge, fwd, inputs

UNSUPPORTED = 4
GGML_NAME = {"q4_0": "Q4_0", "q4_1": "Q4_1", "q5_0": "Q5_0", "q5_1": "Q5_1", "q8_0": "Q8_0", "q2_k": "Q2_K",
             "q3_k": "Q3_K", "q4_k": "Q4_K", "q5_k": "Q5_K", "q6_k": "Q6_K", "iq4_nl": "IQ4_NL"}


@pytest.fixture(scope="module")
def host_lib():
    if not os.path.exists(CLANG):
        pytest.skip("host clang++ not available")
    return build_host_lib()


def S():
    from acestep_mi355x import synthetic
    return synthetic


def blocks(qtype, rows, cols, seed=0):
    return S().random_blocks(GGML_NAME[qtype], rows, cols, np.random.default_rng(seed))


# ------------------------------------------------------------------ checkpoints
def mixed_qkv_types(name, shape):
    """Q4_K everywhere, Q6_K for k_proj: q|k|v (and cross k|v) fuse parts of two plane types"""
    return "Q6_K" if "k_proj" in name else "Q4_K"


FILES = {"q5_k_m": lambda: S().q5_k_m_types, "q4_0": lambda: (lambda n, s: "Q4_0"), "iq4_nl": lambda: (lambda n, s: "IQ4_NL"),
         "q4k_q6k_qkv": lambda: mixed_qkv_types}
_PAIRS = {}


def is_matmul_weight(name, shape):
    return len(shape) == 2 and "embed_tokens" not in name and "scale_shift_table" not in name


def gguf_pair(kind, base=None, types=None):
    """(dir of the typed GGUF checkpoint, dir of its BF16 twin): the twin stores rne_bf16(numpy dequant) for every
    block-quantized matmul weight and the typed file's own bytes for everything else.  Built once, never modified."""
    if kind in _PAIRS:
        return _PAIRS[kind]
    s = S()
    base = base or base_ckpt()
    src = os.path.join(base, "model.safetensors")
    da, db = tempfile.mkdtemp(prefix=f"acemi_blk_{kind}_"), tempfile.mkdtemp(prefix=f"acemi_blk_{kind}_bf16_")
    for d in (da, db):
        shutil.copy(os.path.join(base, "config.json"), d)
    entries = s.write_gguf_typed(src, os.path.join(da, "model.gguf"), types or FILES[kind](), seed=11)
    twin = {}
    for name, (shape, t, data) in entries.items():
        q = t.lower()
        if q in gnp.BLOCK and is_matmul_weight(name, shape):
            raw = np.frombuffer(data, np.uint8).reshape(shape[0], shape[1] // gnp.BLOCK[q][0], gnp.BLOCK[q][1])
            twin[name] = (shape, "BF16", gnp.bf16_bits(gnp.dequant(raw, q)).astype("<u2").tobytes())
        else:
            twin[name] = (shape, t, data)
    s.write_gguf_tensors(os.path.join(db, "model.gguf"), twin)
    _PAIRS[kind] = (da, db)
    return _PAIRS[kind]


# ------------------------------------------------------------------ host dequantize against numpy
@pytest.mark.parametrize("qtype", gnp.NEW_TYPES)
def test_host_dequantize_equals_numpy(host_lib, qtype):
    from acestep_mi355x import capi
    capi.load_library(host_lib)
    b = blocks(qtype, 64, 512, seed=1)
    got = capi.dequantize(b, qtype)
    ref = gnp.dequant(b, qtype)
    assert np.all(np.isfinite(ref)) and 0.005 < float(ref.std()) < 0.08, float(ref.std())
    np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("qtype", ["q8_0", "q4_k", "q6_k"])
def test_numpy_restatement_of_the_pinned_types(host_lib, qtype):
    """the twin files use the numpy decoder for Q8_0 / Q4_K / Q6_K too: it equals the library's (pinned) decoders"""
    from acestep_mi355x import capi
    capi.load_library(host_lib)
    b = blocks(qtype, 16, 512, seed=2)
    np.testing.assert_array_equal(capi.dequantize(b, qtype).view(np.uint32), gnp.dequant(b, qtype).view(np.uint32))


def test_fma_contraction_cannot_change_a_value():
    """every product of the formulas is exact in f32 (an fp16 scale times a small integer), so a value rounds at most
    once: evaluated with exact (float64) products, each type gives the float32 result of the numpy restatement"""
    for qtype in gnp.NEW_TYPES:
        b = blocks(qtype, 8, 512, seed=3)
        ref = gnp.dequant(b, qtype)
        F, saved = gnp.F, gnp.F
        try:
            gnp.F = np.float64  # the same formulas with no intermediate rounding at all
            exact = gnp.dequant(b, qtype)
        finally:
            gnp.F = saved
        np.testing.assert_array_equal(exact.astype(np.float32).view(np.uint32), ref.view(np.uint32), err_msg=qtype)


# ------------------------------------------------------------------ layout cross-checks
def test_q5_k_without_high_bits_is_q4_k(host_lib):
    from acestep_mi355x import capi
    capi.load_library(host_lib)
    q5 = blocks("q5_k", 16, 512, seed=4)
    q5[..., 16:48] = 0                                             # qh
    q4 = np.concatenate([q5[..., :16], q5[..., 48:]], axis=-1)     # d, dmin, scales | qs
    np.testing.assert_array_equal(capi.dequantize(q5, "q5_k").view(np.uint32), capi.dequantize(q4, "q4_k").view(np.uint32))


def test_q5_0_q5_1_without_high_bits_are_q4_shifted(host_lib):
    from acestep_mi355x import capi
    capi.load_library(host_lib)
    q5 = blocks("q5_0", 16, 512, seed=5)
    q5[..., 2:6] = 0
    q4 = np.concatenate([q5[..., :2], q5[..., 6:]], axis=-1)
    d = np.repeat(np.ascontiguousarray(q4[..., :2]).view("<f2").astype(np.float32), 32, axis=-1).reshape(16, 512)
    # (q - 16) d = (q - 8) d - 8 d, both products exact and the difference of multiples of d exact at these magnitudes
    np.testing.assert_array_equal(capi.dequantize(q5, "q5_0"), capi.dequantize(q4, "q4_0") - np.float32(8) * d)
    q5 = blocks("q5_1", 16, 512, seed=6)
    q5[..., 4:8] = 0
    q4 = np.concatenate([q5[..., :4], q5[..., 8:]], axis=-1)
    np.testing.assert_array_equal(capi.dequantize(q5, "q5_1").view(np.uint32), capi.dequantize(q4, "q4_1").view(np.uint32))


@pytest.mark.parametrize("qtype", ["q4_0", "q4_1", "q5_0", "q5_1", "iq4_nl"])
def test_encode_decode_reproduces_a_ramp(host_lib, qtype):
    """ggml's short encoders in numpy, then the library's decoder: a ramp comes back within half a quantization step
    per element (the widest table gap for IQ4_NL).  A swapped nibble or high-bit position moves values by many steps."""
    from acestep_mi355x import capi
    capi.load_library(host_lib)
    x = np.stack([np.linspace(-1.0, 0.7, 32), np.linspace(0.9, -0.4, 32), np.linspace(0.05, 1.3, 32),
                  np.linspace(-0.2, -1.1, 32)]).astype(np.float32).reshape(2, 64)
    b = gnp.quantize(x, qtype)
    y = capi.dequantize(b, qtype)
    d = np.abs(np.ascontiguousarray(b[..., 0:2]).view("<f2").astype(np.float32))   # [rows][nb][1]
    gap = 24.0 if qtype == "iq4_nl" else 1.0                       # widest gap of kvalues_iq4nl: 89 -> 113
    tol = np.repeat(0.5 * gap * d * (1 + 2.0 ** -9), 32, axis=-1).reshape(x.shape)
    assert np.all(np.abs(y - x) <= tol + 1e-7), float(np.max(np.abs(y - x) - tol))
    assert float(np.abs(y - x).max()) > 0 and len(np.unique(y)) > 16


# ------------------------------------------------------------------ reader
READER_DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include "runtime/gguf.h"
int main(int argc, char** argv) {
    using namespace acemi;
    if (argc == 1) {
        const int types[] = {2, 3, 6, 7, 8, 10, 11, 12, 13, 14, 20, 16};
        for (int t : types)
            std::printf("%d %s %llu %llu\n", t, ggml_type_name(t).c_str(), (unsigned long long)ggml_row_bytes(t, 512),
                        (unsigned long long)ggml_row_bytes(t, 480));
        return 0;
    }
    try {
        GgufFile g;
        g.open(argv[1]);
        (void)g.read(g.get(argv[2]));
        std::printf("read ok\n");
    } catch (const std::exception& e) {
        std::printf("error: %s\n", e.what());
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def reader():
    if not os.path.exists(CLANG):
        pytest.skip("host clang++ not available")
    d = tempfile.mkdtemp(prefix="acemi_gguf_reader_")
    src = os.path.join(d, "reader.cpp")
    with open(src, "w") as f:
        f.write(READER_DRIVER)
    exe = os.path.join(d, "reader")
    subprocess.run([CLANG, "-std=c++17", "-O1", "-I" + CSRC, src, os.path.join(CSRC, "runtime", "gguf.cpp"), "-o", exe],
                   check=True)
    return exe


def test_reader_row_bytes_and_names(reader):
    out = subprocess.run([reader], check=True, capture_output=True, text=True).stdout.split("\n")
    rows = {int(l.split()[0]): l.split()[1:] for l in out if l.strip()}
    table = {2: ("q4_0", 32, 18), 3: ("q4_1", 32, 20), 6: ("q5_0", 32, 22), 7: ("q5_1", 32, 24), 8: ("q8_0", 32, 34),
             10: ("q2_K", 256, 84), 11: ("q3_K", 256, 110), 12: ("q4_K", 256, 144), 13: ("q5_K", 256, 176),
             14: ("q6_K", 256, 210), 20: ("iq4_nl", 32, 18)}
    for t, (name, bv, bb) in table.items():
        assert rows[t][0] == name
        assert int(rows[t][1]) == 512 // bv * bb
        assert int(rows[t][2]) == (480 // bv * bb if 480 % bv == 0 else 0)
    assert rows[16][0] == "type" and rows[16][1] == "16" and rows[16][2:] == ["0", "0"]


def test_reader_refuses_partial_blocks_and_unknown_types(reader):
    s = S()
    d = tempfile.mkdtemp(prefix="acemi_gguf_bad_")
    p = os.path.join(d, "bad.gguf")
    s.write_gguf_tensors(p, {"ok.weight": ((4, 64), "Q4_0", bytes(4 * 2 * 18)),
                             "short.weight": ((4, 48), "Q4_0", bytes(4 * 18))})
    run = lambda name: subprocess.run([reader, p, name], check=True, capture_output=True, text=True).stdout
    assert "read ok" in run("ok.weight")
    msg = run("short.weight")
    assert "error" in msg and "short.weight" in msg and "48" in msg and "q4_0" in msg
    s.GGML_TYPES["IQ2_XXS"] = 16                 # a type the table lacks
    try:
        s.write_gguf_tensors(p, {"odd.weight": ((4, 256), "IQ2_XXS", bytes(4 * 66))})
    finally:
        del s.GGML_TYPES["IQ2_XXS"]
    msg = run("odd.weight")
    assert "error" in msg and "16" in msg and "odd.weight" in msg and "unsupported" in msg


# ------------------------------------------------------------------ loader + engine (host emulation)
@pytest.mark.parametrize("kind", ["q5_k_m", "q4_0", "q4k_q6k_qkv"])
def test_forward_equals_the_bf16_twin(host_lib, kind):
    da, db = gguf_pair(kind)
    x = inputs()
    ba = bridge(host_lib, da)
    desc = ba.dit_weight_desc()
    got = fwd(ba, x)
    ba.close()
    bb = bridge(host_lib, db)
    assert bb.dit_weight_desc().startswith("bf16")
    ref = fwd(bb, x)
    bb.close()
    assert "ggml raw blocks" in desc, desc
    assert {"q5_k_m": "q5_K, q6_K", "q4_0": "q4_0", "q4k_q6k_qkv": "q4_K, q6_K"}[kind] in desc, desc
    if kind == "q4k_q6k_qkv":
        assert "q4_K planes" in desc, desc  # o_proj, gate|up, down: purely Q4_K, planes as before
    assert np.all(np.isfinite(ref)) and float(np.abs(ref).max()) > 0
    np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("scope", ["call", "layer"])
def test_forward_in_the_other_stage_scopes(host_lib, monkeypatch, scope):
    da, db = gguf_pair("q5_k_m")
    x = inputs(seed=4)
    bb = bridge(host_lib, db)
    ref = fwd(bb, x)
    bb.close()
    monkeypatch.setenv("ACE_MI_QUANT_STAGE_SCOPE", scope)
    ba = bridge(host_lib, da)
    got = [fwd(ba, x), fwd(ba, x)]
    ba.close()
    for g in got:
        np.testing.assert_array_equal(g.view(np.uint32), ref.view(np.uint32))


def test_unstaged_mode_stages_raw_blocks(host_lib, monkeypatch):
    """ACE_MI_QUANT_STAGED=0: plane matrices run the dequant-fused GEMM, raw-block matrices are staged per layer"""
    da, db = gguf_pair("q4k_q6k_qkv")
    x = inputs(seed=5)
    bb = bridge(host_lib, db)
    ref = fwd(bb, x)
    bb.close()
    monkeypatch.setenv("ACE_MI_QUANT_STAGED", "0")
    ba = bridge(host_lib, da)
    got = fwd(ba, x)
    ba.close()
    np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_lora_round_trip_on_a_mixed_file(host_lib):
    da, db = gguf_pair("q5_k_m")
    s = S()
    ad = adapter(targets=s.LORA_ALL_TARGETS, seed=2)
    x = inputs(seed=6)
    ba, bb = bridge(host_lib, da), bridge(host_lib, db)
    base = fwd(ba, x)
    np.testing.assert_array_equal(base.view(np.uint32), fwd(bb, x).view(np.uint32))
    for scale in (1.0, 0.5):
        if scale == 1.0:
            ba.load_lora(ad, scale)
            bb.load_lora(ad, scale)
        else:
            ba.set_lora_scale(scale)
            bb.set_lora_scale(scale)
        got, ref = fwd(ba, x), fwd(bb, x)
        assert not np.array_equal(got, base)
        # the merge base of a raw-block matrix is its expanded image = the twin's bf16 weights
        np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32))
    ba.unload_lora()
    np.testing.assert_array_equal(fwd(ba, x).view(np.uint32), base.view(np.uint32))
    ba.close()
    bb.close()


def test_q8_activation_mode_is_refused(host_lib, monkeypatch):
    da, _ = gguf_pair("q5_k_m")
    monkeypatch.setenv("ACE_MI_QUANT_ACT", "q8")
    br = bridge(host_lib)
    st = br.lib.ace_ggml_load_dit(br.ctx, da.encode())
    msg = br._last_error()
    br.close()
    assert st == UNSUPPORTED, (st, msg)
    assert "ACE_MI_QUANT_ACT=q8" in msg and "decoder." in msg and ".weight" in msg, msg
    assert "(q5_K)" in msg or "(q6_K)" in msg, msg
