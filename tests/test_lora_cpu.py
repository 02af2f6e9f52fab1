"""PEFT LoRA adapters in the DiT engine, on the CPU: the product's runtime (adapter reader, image bookkeeping, view
routing, the host build of launch_lora_merge) in the host-emulation library, against merged checkpoints written with
the same arithmetic in numpy (acestep_mi355x/synthetic.py lora_acc / lora_merge_bits).  An engine that loaded
base + adapter and an engine that loaded the merged checkpoint hold identical weight bits and run the same code, so
their forwards are compared bit for bit.  The gfx950 kernel and the HIP path are in tests/test_gpu_lora.py, which
borrows this module's helpers."""
import ctypes
import json
import os
import shutil
import tempfile
import types

import numpy as np
import pytest

from hostlib import CLANG, build_host_lib

OK, ERR, INVALID_ARG, IO, UNSUPPORTED = 0, 1, 2, 3, 4


@pytest.fixture(scope="module")
def host_lib():
    if not os.path.exists(CLANG):
        pytest.skip("host clang++ not available")
    return build_host_lib()


def S():
    from acestep_mi355x import synthetic
    return synthetic


def target_sets():
    s = S()
    return {
        "self_qkvo": tuple(f"self_attn.{p}" for p in s.LORA_ATTN_TARGETS),
        "all": s.LORA_ALL_TARGETS,
        # v_proj and up_proj left out: copy-through rows inside w_qkv, w_ckv_all and w_gu
        "no_v_up": tuple(t for t in s.LORA_ALL_TARGETS if not t.endswith(("v_proj", "up_proj"))),
    }


_CKPT = {}


def base_ckpt(dtype="BF16", cfg=None, seed=0):
    """One synthetic base checkpoint per (config, dtype), shared and never modified."""
    s = S()
    cfg = cfg or s.TINY_CONFIG
    key = (json.dumps(cfg, sort_keys=True), dtype, seed)
    if key not in _CKPT:
        d = tempfile.mkdtemp(prefix="acemi_lora_base_")
        s.write_checkpoint(d, cfg, seed=seed, dtype=dtype)
        _CKPT[key] = d
    return _CKPT[key]


def bridge(lib, ckpt=None):
    from acestep_mi355x.capi import GGMLCAPIBridge
    br = GGMLCAPIBridge(lib_path=lib)
    if ckpt is not None:
        br.load_dit(ckpt)
    return br


def inputs(seed=3, T=24, L=5, H=256):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((T, 64)).astype(np.float32), rng.standard_normal((T, 128)).astype(np.float32),
            rng.standard_normal((L, H)).astype(np.float32))


def fwd(br, x, t=0.7, r=0.4):
    return br.dit_forward_tfirst(x[0], x[1], x[2], None, None, t, r)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def adapter(cfg=None, **kw):
    d = tempfile.mkdtemp(prefix="acemi_lora_ad_")
    return S().write_lora_adapter(d, cfg or S().TINY_CONFIG, **kw)


def merged(base, ad, scale):
    return S().merged_checkpoint(base, ad, scale, tempfile.mkdtemp(prefix="acemi_lora_m_"))


def forward_pair(lib, base, ad, scale, x):
    """(forward of base + adapter at `scale`, forward of the merged checkpoint), each on its own engine."""
    br = bridge(lib, base)
    br.load_lora(ad, scale)
    got = fwd(br, x)
    br.close()
    bm = bridge(lib, merged(base, ad, scale))
    ref = fwd(bm, x)
    bm.close()
    return got, ref


def sample(br, x, cache_cross=True):
    """A 3-step sampling run (ace_mi_dit_sample_ex) on host pointers; returns x0."""
    h, c, e = x
    xt = h[None].copy()
    cc, ee = c[None].copy(), e[None].copy()
    p = lambda a: a.ctypes.data
    br.dit_sample_ex_device(1, h.shape[0], e.shape[0], p(xt), p(cc), p(ee), 0, 0, [1.0, 0.6, 0.3], cache_cross=cache_cross)
    br.synchronize()
    return xt[0]


# ------------------------------------------------------------------ the host launcher against numpy
def numpy_merge(base, out0, cols, jobs, fmt):
    """launch_lora_merge restated on numpy arrays of 16-bit words (the reference of the kernel tests)."""
    s = S()
    out = out0.copy()
    src = out0 if base is None else base
    F = {"bf16": "BF16", "fp16": "F16"}[fmt]
    for j in jobs:
        rows = np.arange(j["row0"], j["row0"] + j["rows"])
        A, B = j.get("A"), j.get("B")
        hit = np.zeros(len(rows), bool)
        if A is not None:
            o = np.arange(B.shape[0])
            if j.get("map", 0) == 1:
                fr = (o // 16) * 32 + j.get("half", 0) * 16 + o % 16
            else:
                fr = j.get("row_off", 0) + o
            ok = (fr >= rows[0]) & (fr <= rows[-1])
            acc = s.lora_acc(A, B)
            out[fr[ok], :cols] = s.lora_merge_bits(src[fr[ok], :cols], acc[ok], j["eff"], F)
            hit[fr[ok] - rows[0]] = True
        if j.get("copy_rest") and base is not None:
            out[rows[~hit], :cols] = base[rows[~hit], :cols]
    return out


def words(rng, shape, fmt):
    v = rng.standard_normal(shape).astype(np.float32) * np.float32(0.05)
    return S()._bf16_bits(v) if fmt == "bf16" else v.astype("<f2").view("<u2")


def merge_cases(rows, cols, r, fmt, seed):
    """The row maps of the issue on one [rows][cols] matrix with ld > cols on both sides: (name, base, out0, jobs)."""
    rng = np.random.default_rng(seed)
    ldb, ldo = cols + 8, cols + 16
    base = words(rng, (rows, ldb), fmt)
    out0 = words(rng, (rows, ldo), fmt)
    f = lambda *sh: (rng.standard_normal(sh).astype(np.float32) * np.float32(0.1))
    cases = []
    for eff in (0.0, 0.37):
        cases.append((f"plain eff={eff}", base, out0,
                      [dict(row0=0, rows=rows, A=f(r, cols), B=f(rows, r), eff=eff, copy_rest=False)]))
    # a module in the middle of a concatenation: copy-through rows above and below, and rows outside the job
    lo, n = max(1, rows // 4), max(1, rows // 3)
    cases.append(("offset", base, out0, [dict(row0=1 if rows > 4 else 0, rows=rows - 2 if rows > 4 else rows, A=f(r, cols), B=f(n, r),
                                              eff=0.37, row_off=lo + 1, copy_rest=True)]))
    if rows % 32 == 0:  # the gate|up interleave with only the gate half adapted
        cases.append(("interleave gate", base, out0,
                      [dict(row0=0, rows=rows, A=f(r, cols), B=f(rows // 2, r), eff=0.37, map=1, half=0, copy_rest=True)]))
        cases.append(("interleave both", base, out0,
                      [dict(row0=0, rows=rows, A=f(r, cols), B=f(rows // 2, r), eff=0.37, map=1, half=h) for h in (0, 1)]))
    # several jobs in one launch: q | k | copy-only v, like w_qkv with v_proj untargeted
    a, b = rows // 2, rows // 4
    if b > 0:
        cases.append(("several", base, out0, [
            dict(row0=0, rows=a, A=f(r, cols), B=f(a, r), eff=0.37, row_off=0),
            dict(row0=a, rows=b, A=f(max(1, r // 2), cols), B=f(b, max(1, r // 2)), eff=-1.5, row_off=a),
            dict(row0=a + b, rows=rows - a - b - (1 if rows - a - b > 1 else 0), A=None, B=None, copy_rest=True)]))
        cases.append(("in place", None, out0, [dict(row0=0, rows=a, A=f(r, cols), B=f(a, r), eff=0.37, copy_rest=True)]))
    return cases


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("rows,cols,r", [(17, 40, 1), (48, 256, 13), (64, 264, 33)])
def test_host_launcher_matches_numpy(host_lib, rows, cols, r, fmt):
    from acestep_mi355x import capi
    lib = ctypes.CDLL(host_lib)
    for name, base, out0, jobs in merge_cases(rows, cols, r, fmt, seed=rows + r):
        got = capi.kernel_lora_merge(base, out0, cols, jobs, fmt=fmt, lib=lib)
        np.testing.assert_array_equal(got, numpy_merge(base, out0, cols, jobs, fmt), err_msg=name)


# ------------------------------------------------------------------ 1. reader errors
def rewrite_tensors(ad, fn, dtype="F32"):
    """Rewrite adapter_model.safetensors of `ad` with fn applied to its {name: f32 array} dict."""
    s = S()
    path = os.path.join(ad, "adapter_model.safetensors")
    t = fn(dict(s._read_safetensors_f32(path)))
    s.write_safetensors(path, list(t.items()), dtype)
    return ad


def load_status(br, ad, scale=1.0):
    st = br.lib.ace_mi_dit_load_lora(br.ctx, str(ad).encode(), ctypes.c_float(scale))
    return st, br._last_error()


@pytest.fixture()
def loaded(host_lib):
    br = bridge(host_lib, base_ckpt())
    yield br
    br.close()


def test_calls_without_model_or_adapter(host_lib):
    br = bridge(host_lib)
    ad = adapter()
    assert load_status(br, ad) == (ERR, "dit not loaded")
    assert br.lib.ace_mi_dit_set_lora_scale(br.ctx, ctypes.c_float(0.5)) == ERR and br._last_error() == "dit not loaded"
    assert br.lib.ace_mi_dit_unload_lora(br.ctx) == ERR and br._last_error() == "dit not loaded"
    br.load_dit(base_ckpt())
    assert br.lib.ace_mi_dit_set_lora_scale(br.ctx, ctypes.c_float(0.5)) == ERR and br._last_error() == "lora not loaded"
    assert br.lib.ace_mi_dit_unload_lora(br.ctx) == OK  # nothing loaded: still OK
    assert br.lora_info()["loaded"] is False
    br.close()


def test_missing_files_are_io_errors(loaded):
    d = tempfile.mkdtemp(prefix="acemi_lora_empty_")
    st, msg = load_status(loaded, d)
    assert st == IO and "adapter_config.json" in msg
    ad = adapter()
    os.remove(os.path.join(ad, "adapter_model.safetensors"))
    st, msg = load_status(loaded, ad)
    assert st == IO and "adapter_model.safetensors" in msg


@pytest.mark.parametrize("extra", [dict(use_dora=True), dict(bias="all"), dict(modules_to_save=["proj_out"]),
                                   dict(peft_type="LOKR")])
def test_unsupported_adapter_configs(loaded, extra):
    st, msg = load_status(loaded, adapter(extra_config=extra))
    assert st == UNSUPPORTED and "adapter_config.json" in msg and list(extra)[0] in msg
    assert loaded.lora_info()["loaded"] is False


def test_unpaired_tensor(loaded):
    key = "base_model.model.layers.1.self_attn.k_proj.lora_B.weight"
    ad = rewrite_tensors(adapter(), lambda t: {k: v for k, v in t.items() if k != key})
    st, msg = load_status(loaded, ad)
    assert st == INVALID_ARG and key.replace("lora_B", "lora_A") in msg


def test_shape_mismatch(loaded):
    key = "base_model.model.layers.0.self_attn.o_proj.lora_A.weight"

    def f(t):
        t[key] = np.zeros((8, 384), np.float32)  # o_proj's input is hq * D = 512 in the tiny model
        return t
    st, msg = load_status(loaded, rewrite_tensors(adapter(), f))
    assert st == INVALID_ARG and key in msg
    # a layer the model does not have is a module the engine does not hold
    cfg3 = dict(S().TINY_CONFIG, num_hidden_layers=3)
    st, msg = load_status(loaded, adapter(cfg=cfg3))
    assert st == UNSUPPORTED and "layers.2." in msg


def test_rank_above_128(loaded):
    st, msg = load_status(loaded, adapter(r=129, targets=("self_attn.q_proj",)))
    assert st == INVALID_ARG and "lora_" in msg and "129" in msg
    loaded.load_lora(adapter(r=128, targets=("self_attn.q_proj",)))  # the largest supported rank
    assert loaded.lora_info()["max_rank"] == 128


def test_non_finite_value(loaded):
    key = "base_model.model.layers.0.cross_attn.v_proj.lora_B.weight"

    def f(t):
        t[key] = t[key].copy()
        t[key][3, 2] = np.inf
        return t
    st, msg = load_status(loaded, rewrite_tensors(adapter(), f))
    assert st == INVALID_ARG and key in msg


def test_module_the_engine_does_not_hold(loaded):
    key = "base_model.model.encoder.lyric_encoder.layers.0.self_attn.q_proj.lora_A.weight"

    def f(t):
        t[key] = np.zeros((8, 256), np.float32)
        t[key.replace("lora_A", "lora_B")] = np.zeros((512, 8), np.float32)
        return t
    st, msg = load_status(loaded, rewrite_tensors(adapter(), f))
    assert st == UNSUPPORTED and key in msg


def test_failed_load_keeps_the_previous_adapter(loaded):
    x = inputs()
    loaded.load_lora(adapter(seed=1))
    before = fwd(loaded, x)
    st, _ = load_status(loaded, adapter(extra_config=dict(use_dora=True)))
    assert st == UNSUPPORTED and loaded.lora_info()["loaded"]
    np.testing.assert_array_equal(fwd(loaded, x), before)


def test_layers_beyond_the_layer_cap_are_dropped(host_lib, monkeypatch):
    monkeypatch.setenv("ACE_GGML_DIT_MAX_LAYERS", "1")
    br = bridge(host_lib, base_ckpt())
    br.load_lora(adapter(cfg=dict(S().TINY_CONFIG, num_hidden_layers=5), targets=("self_attn.q_proj",)))
    assert br.lora_info()["num_modules"] == 1
    br.close()


def test_key_forms_and_info(host_lib):
    """The decoder. prefix and the adapter-name segment name the same modules; lora_info reports the adapter."""
    x = inputs()
    outs = []
    for kw in (dict(), dict(key_prefix="base_model.model.decoder."), dict(adapter_name="default"),
               dict(dtype="BF16"), dict(dtype="F16")):
        br = bridge(host_lib, base_ckpt())
        br.load_lora(adapter(seed=5, r=4, alpha=8.0, **kw), 0.5)
        info = br.lora_info()
        assert info["loaded"] and info["scale"] == 0.5 and info["lora_alpha"] == 8.0
        assert (info["min_rank"], info["max_rank"], info["num_modules"]) == (4, 4, 2 * 2 * 4)
        # tiny model, q/k/v/o on self and cross: w_qkv, w_o, w_cq, w_co per layer + the fused cross k|v matrix
        assert info["num_images"] == 2 * 4 + 1 and info["image_bytes"] > 0
        outs.append(fwd(br, x))
        br.close()
    for o in outs[1:3]:
        np.testing.assert_array_equal(o, outs[0])
    assert rel(outs[3], outs[0]) < 1e-2 and rel(outs[4], outs[0]) < 1e-2  # 16-bit A / B: rounded values, same modules


# ------------------------------------------------------------------ 2. merged-checkpoint identity
@pytest.mark.parametrize("dtype", ["BF16", "F16"])
@pytest.mark.parametrize("scale", [1.0, 0.37])
@pytest.mark.parametrize("r", [1, 8, 13])
@pytest.mark.parametrize("targets", ["self_qkvo", "all", "no_v_up"])
def test_adapter_equals_merged_checkpoint(host_lib, targets, r, scale, dtype):
    base = base_ckpt(dtype)
    ad = adapter(r=r, targets=target_sets()[targets], seed=r)
    x = inputs()
    got, ref = forward_pair(host_lib, base, ad, scale, x)
    np.testing.assert_array_equal(got, ref)


def test_adapter_changes_the_forward(host_lib):
    """The defect this feature fixes: an adapter that loads and is ignored."""
    x = inputs()
    br = bridge(host_lib, base_ckpt())
    plain = fwd(br, x)
    br.load_lora(adapter(targets=target_sets()["all"]))
    assert rel(fwd(br, x), plain) > 1e-4
    br.close()


def test_rslora_and_alpha_pattern_and_rank_pattern(host_lib):
    base = base_ckpt()
    x = inputs()
    got, ref = forward_pair(host_lib, base, adapter(r=13, rslora=True, targets=target_sets()["all"]), 0.37, x)
    np.testing.assert_array_equal(got, ref)
    ad = adapter(r={"q_proj": 3, "layers.1.mlp.down_proj": 21}, alpha=16.0, targets=target_sets()["all"],
                 alpha_pattern={"k_proj": 4.0, "layers.0.self_attn.o_proj": 40.0})
    got, ref = forward_pair(host_lib, base, ad, 1.0, x)
    np.testing.assert_array_equal(got, ref)
    # the pattern is not ignored: the same tensors under the plain lora_alpha give another forward
    plain = tempfile.mkdtemp(prefix="acemi_lora_ap_")
    shutil.copytree(ad, plain, dirs_exist_ok=True)
    conf = json.load(open(os.path.join(plain, "adapter_config.json")))
    conf["alpha_pattern"] = {}
    json.dump(conf, open(os.path.join(plain, "adapter_config.json"), "w"))
    br = bridge(host_lib, base)
    br.load_lora(plain)
    assert rel(fwd(br, x), got) > 1e-5
    assert (br.lora_info()["min_rank"], br.lora_info()["max_rank"]) == (3, 21)
    br.close()


# ------------------------------------------------------------------ 3. state
def test_scale_zero_disable_and_unload_restore_the_base(host_lib):
    from acestep_mi355x import hook
    x = inputs()
    br = bridge(host_lib, base_ckpt())
    plain = fwd(br, x)
    ad = adapter(targets=target_sets()["all"], seed=2)
    br.load_lora(ad, 0.0)
    assert br.lora_info()["loaded"]
    np.testing.assert_array_equal(fwd(br, x), plain)
    br.set_lora_scale(0.8)
    adapted = fwd(br, x)
    assert rel(adapted, plain) > 1e-4
    br.set_lora_scale(0.0)
    np.testing.assert_array_equal(fwd(br, x), plain)
    # the handler's switch: off = base, on = the remembered scale
    h = types.SimpleNamespace(model=types.SimpleNamespace(decoder=types.SimpleNamespace()), lora_scale=0.8)
    hook.install_lora_backend(h, br)
    assert h.load_lora(ad).startswith("✅")
    np.testing.assert_array_equal(fwd(br, x), adapted)
    assert h.set_use_lora(False).startswith("✅") and br.lora_info()["scale"] == 0.0 and h.lora_scale == 0.8
    np.testing.assert_array_equal(fwd(br, x), plain)
    assert h.set_use_lora(True).startswith("✅")
    np.testing.assert_array_equal(fwd(br, x), adapted)
    assert h.unload_lora().startswith("✅") and not br.lora_info()["loaded"]
    np.testing.assert_array_equal(fwd(br, x), plain)
    br.close()


def test_second_load_and_rescale_equal_fresh_loads(host_lib):
    x = inputs()
    X = adapter(targets=target_sets()["all"], seed=7, r=5)
    Y = adapter(targets=target_sets()["self_qkvo"], seed=8, r=8)
    fresh = bridge(host_lib, base_ckpt())
    fresh.load_lora(Y, 0.6)
    want = fwd(fresh, x)
    fresh.close()
    br = bridge(host_lib, base_ckpt())
    br.load_lora(X, 1.0)
    br.load_lora(Y, 0.6)  # replaces X (its mlp / cross images must be gone)
    np.testing.assert_array_equal(fwd(br, x), want)
    br.load_lora(Y, 0.9)
    br.set_lora_scale(0.2)
    br.set_lora_scale(0.6)  # rebuilt from the base, not from the 0.2 images
    np.testing.assert_array_equal(fwd(br, x), want)
    br.close()


def test_cross_cache_is_invalidated(host_lib):
    x = inputs(T=16, L=4)
    br = bridge(host_lib, base_ckpt())
    first = sample(br, x)
    np.testing.assert_array_equal(sample(br, x), first)
    br.load_lora(adapter(targets=("cross_attn.k_proj", "cross_attn.v_proj"), seed=4, std=0.1))
    with_lora = sample(br, x)
    assert rel(with_lora, first) > 1e-4, "cached cross K/V of the base weights were reused"
    fresh = bridge(host_lib, base_ckpt())
    fresh.load_lora(adapter(targets=("cross_attn.k_proj", "cross_attn.v_proj"), seed=4, std=0.1))
    np.testing.assert_array_equal(with_lora, sample(fresh, x))
    fresh.close()
    br.unload_lora()
    np.testing.assert_array_equal(sample(br, x), first)
    br.close()


# ------------------------------------------------------------------ 4. quantized base
def dequantized_checkpoint(base, qtype="q8_0"):
    """D: a dense BF16 checkpoint holding bf16(dequant(quantize(W))) for every matrix the loader would quantize
    in its file layout (2-D, in-dim % 32 == 0)."""
    from acestep_mi355x import capi
    s = S()
    d = tempfile.mkdtemp(prefix="acemi_lora_dq_")
    shutil.copy(os.path.join(base, "config.json"), d)
    t = s._read_safetensors_f32(os.path.join(base, "model.safetensors"))
    out = []
    for name, v in t.items():
        if v.ndim == 2 and v.shape[1] % 32 == 0:
            v = capi.dequantize(capi.quantize(np.ascontiguousarray(v, np.float32), qtype), qtype)
        out.append((name, np.asarray(v, np.float32)))
    s.write_safetensors(os.path.join(d, "model.safetensors"), out, "BF16")
    return d


def quantized_pair_errors(lib, monkeypatch, env=()):
    """(e0, e1): relL2 of the Q8_0 engine against the dense engine on D without an adapter, and with the adapter
    against D merged with it."""
    base = base_ckpt()
    D = dequantized_checkpoint(base)
    ad = adapter(targets=target_sets()["no_v_up"], r=8, seed=9)
    Dp = merged(D, ad, 0.8)
    x = inputs()
    dense = bridge(lib, D)
    ref0 = fwd(dense, x)
    dense.close()
    dense = bridge(lib, Dp)
    ref1 = fwd(dense, x)
    dense.close()
    monkeypatch.setenv("ACE_GGML_DIT_WEIGHT_QTYPE", "q8_0")
    for k, v in env:
        monkeypatch.setenv(k, v)
    q = bridge(lib, base)
    e0 = rel(fwd(q, x), ref0)
    q.load_lora(ad, 0.8)
    got = fwd(q, x)
    e1 = rel(got, ref1)
    assert rel(got, ref0) > 1e-4  # the adapter is applied
    q.unload_lora()
    assert rel(fwd(q, x), ref0) == e0
    q.close()
    return e0, e1


@pytest.mark.parametrize("staged", ["1", "0"])
def test_quantized_base(host_lib, monkeypatch, staged):
    e0, e1 = quantized_pair_errors(host_lib, monkeypatch, env=(("ACE_MI_QUANT_STAGED", staged),))
    print(f"quantized base (host emulation, ACE_MI_QUANT_STAGED={staged}): e0 = {e0:.3e}, with adapter = {e1:.3e}")
    assert e1 == 0.0 if e0 == 0.0 else e1 <= 2.0 * e0, (e0, e1)


@pytest.mark.parametrize("scope", ["call", "layer"])
def test_quantized_base_stage_scopes(host_lib, monkeypatch, scope):
    e0, e1 = quantized_pair_errors(host_lib, monkeypatch, env=(("ACE_MI_QUANT_STAGE_SCOPE", scope),))
    assert e1 == 0.0 if e0 == 0.0 else e1 <= 2.0 * e0, (e0, e1)


# ------------------------------------------------------------------ 5. refusal
def test_quantized_activation_mode_refuses(host_lib, monkeypatch):
    monkeypatch.setenv("ACE_GGML_DIT_WEIGHT_QTYPE", "q8_0")
    monkeypatch.setenv("ACE_MI_QUANT_ACT", "q8")
    br = bridge(host_lib, base_ckpt())
    st, msg = load_status(br, adapter())
    assert st == UNSUPPORTED and "ACE_MI_QUANT_ACT" in msg
    br.close()


# ------------------------------------------------------------------ 6. hook
class FakeLoraBridge:
    def __init__(self):
        self.calls = []
        self.fail = False

    def load_lora(self, path, scale=1.0):
        if self.fail:
            raise RuntimeError("ace_mi_dit_load_lora failed: boom (status=4)")
        self.calls.append(("load", path, scale))

    def set_lora_scale(self, scale):
        self.calls.append(("scale", scale))

    def unload_lora(self):
        self.calls.append(("unload",))


def test_hook_drives_the_bridge_and_the_flags():
    from acestep_mi355x import hook
    dec = types.SimpleNamespace(forward=lambda **kw: ("original", kw))
    h = types.SimpleNamespace(model=types.SimpleNamespace(decoder=dec))
    br = FakeLoraBridge()
    hook.install_dit_backend(h, br)  # installs the LoRA controls too
    assert h._ggml_lora_backend == "mi355x-capi"
    assert (h.lora_loaded, h.use_lora, h.lora_scale) == (False, False, 1.0)
    assert h.set_lora_scale(0.5).startswith("⚠️") and h.set_use_lora(True).startswith("❌")
    assert h.unload_lora().startswith("⚠️") and br.calls == []
    assert h.load_lora("").startswith("❌") and h.load_lora("/nonexistent/adapter").startswith("❌ LoRA path not found")
    empty = tempfile.mkdtemp(prefix="acemi_lora_hook_")
    assert "adapter_config.json not found" in h.load_lora(empty) and br.calls == []
    ad = adapter()
    br.fail = True
    assert h.load_lora(ad).startswith("❌ Failed to load LoRA: ") and "boom" in h.load_lora(ad) and not h.lora_loaded
    br.fail = False
    assert h.load_lora(f"  {ad} ") == f"✅ LoRA loaded from {ad}"
    assert br.calls == [("load", ad, 1.0)] and (h.lora_loaded, h.use_lora, h.lora_scale) == (True, True, 1.0)
    assert h.set_lora_scale(0.37) == "✅ LoRA scale: 0.37" and br.calls[-1] == ("scale", 0.37)
    assert h.set_lora_scale(7).endswith("1.00") and br.calls[-1] == ("scale", 1.0)  # clamped to 0..1 as the reference
    assert h.set_lora_scale("x").startswith("❌") and h.set_lora_scale(float("nan")).startswith("❌")
    h.set_lora_scale(0.37)
    n = len(br.calls)
    assert h.set_use_lora(False) == "✅ LoRA disabled" and br.calls[n:] == [("scale", 0.0)]
    assert (h.use_lora, h.lora_scale) == (False, 0.37)
    assert h.set_lora_scale(0.6) == "✅ LoRA scale: 0.60 (LoRA disabled)" and len(br.calls) == n + 1  # remembered only
    assert h.set_use_lora(True) == "✅ LoRA enabled" and br.calls[-1] == ("scale", 0.6) and h.use_lora
    assert h.unload_lora() == "✅ LoRA unloaded, using base model" and br.calls[-1] == ("unload",)
    assert (h.lora_loaded, h.use_lora, h.lora_scale) == (False, False, 1.0)
    assert h.model.decoder is dec  # never wrapped or copied
