"""LyCORIS LoKr adapters in the DiT engine, on the CPU: the reader (runtime/lokr.h), the engine's bookkeeping and the
host build of launch_lokr_merge in the host-emulation library, against numpy's restatement of the fixed chain
(acestep_mi355x/synthetic.py lokr_delta / lora_merge_bits).  The kernel cases and their numpy reference are shared
with tests/test_gpu_lokr.py, which runs them on the gfx950 kernels."""
import ctypes
import os
import tempfile

import numpy as np
import pytest

from hostlib import CLANG, build_host_lib
from test_lora_cpu import UNSUPPORTED, S, base_ckpt, bridge, fwd, inputs, load_status, rel, words


@pytest.fixture(scope="module")
def host_lib():
    if not os.path.exists(CLANG):
        pytest.skip("host clang++ not available")
    return build_host_lib()


def lokr_adapter(**kw):
    return S().write_lokr_adapter(tempfile.mkdtemp(prefix="acemi_lokr_ad_"), S().TINY_CONFIG, **kw)


# ------------------------------------------------------------------ the merge entry against numpy
# (a, b, c, d, r, form, map, fmt, in place): module rows a*c, columns b*d
KERNEL_CASES = {
    "full": (3, 4, 4, 8, 0, "full", "plain", "bf16", False),
    "w2 r=3, d=12 straddles j, c=5 crosses i, partial tile": (9, 2, 5, 12, 3, "w2_lowrank", "plain", "bf16", False),
    "both low-rank, r=33 (one past the rank chunk)": (4, 4, 8, 8, 33, "both_lowrank", "plain", "fp16", False),
    "c > tile rows, d > tile columns, several column tiles": (2, 2, 40, 264, 5, "w2_lowrank", "plain", "bf16", False),
    "qkv: q and v adapted, k copied through": (5, 2, 4, 12, 3, "w2_lowrank", "qkv", "bf16", False),
    "gate|up interleave, gate adapted": (4, 4, 8, 6, 3, "both_lowrank", "gate", "fp16", False),
    "in place": (9, 2, 5, 12, 3, "w2_lowrank", "plain", "fp16", True),
}


def kernel_case(name):
    """(base or None, out0, cols, jobs, fmt) of a KERNEL_CASES entry, ld > cols on both sides."""
    a, b, c, d, r, form, rowmap, fmt, in_place = KERNEL_CASES[name]
    rng = np.random.default_rng(len(name))
    rows_mod, cols = a * c, b * d
    f = lambda *sh: rng.standard_normal(sh).astype(np.float32) * np.float32(0.3)
    w1 = lambda: (f(a, r), f(r, b)) if form == "both_lowrank" else f(a, b)
    w2 = lambda: f(c, d) if form == "full" else (f(c, r), f(r, d))
    job = lambda **kw: dict(w1=w1(), w2=w2(), eff=0.37, r=r, **kw)
    if rowmap == "qkv":  # q | k | v stacked, k half as tall and without an adapter; one row outside every job
        k = rows_mod // 2
        rows = 2 * rows_mod + k + 1
        jobs = [job(row0=0, rows=rows_mod, row_off=0), dict(row0=rows_mod, rows=k, copy_rest=True),
                job(row0=rows_mod + k, rows=rows_mod, row_off=rows_mod + k)]
    elif rowmap == "gate":
        rows = 2 * rows_mod
        jobs = [job(row0=0, rows=rows, map=1, half=0, copy_rest=True)]
    else:
        rows = rows_mod + 2
        jobs = [job(row0=1, rows=rows_mod, row_off=1)]
    out0 = words(rng, (rows, cols + 16), fmt)
    return (None if in_place else words(rng, (rows, cols + 8), fmt)), out0, cols, jobs, fmt


def f64_bound(j, base_bits, got_bits, fmt):
    """|got - ref| <= bound, ref = base + eff * kron(w1, W2) in float64.  bound = half an ulp of the 16-bit output at
    the larger of |got|, |ref|, plus the f32 chain's own bound (r + 3) * 2^-24 * sum|terms|: r multiply-adds of the
    rank chain, the multiply w1 * W2, the multiply by eff and the add to the base, each within 2^-24 relative of
    sum|terms| = |base| + |eff| * kron(|L1| . |R1|, |L2| . |R2|).  Derived, not measured."""
    wide = (lambda v: v.view("<f2").astype(np.float64)) if fmt == "fp16" else \
        (lambda v: (v.astype(np.uint32) << 16).view(np.float32).astype(np.float64))
    prod = lambda f, g=np.asarray: g(f[0], np.float64) @ g(f[1], np.float64) if isinstance(f, tuple) else g(f, np.float64)
    ab = lambda x, dt: np.abs(np.asarray(x, dt))
    base, got = wide(np.ascontiguousarray(base_bits)), wide(np.ascontiguousarray(got_bits))
    ref = base + j["eff"] * np.kron(prod(j["w1"]), prod(j["w2"]))
    terms = np.abs(base) + abs(j["eff"]) * np.kron(prod(j["w1"], ab), prod(j["w2"], ab))
    mant, emin = (10, -14) if fmt == "fp16" else (7, -126)
    e = np.maximum(np.floor(np.log2(np.maximum(np.maximum(np.abs(ref), np.abs(got)), 2.0 ** emin))), emin)
    return np.abs(got - ref), 0.5 * 2.0 ** (e - mant) + (j["r"] + 3) * 2.0 ** -24 * terms


def check_kernel_case(name, lib=None):
    """Bit-equality with the numpy restatement everywhere (so the words beyond cols, the rows outside the jobs and the
    copy-through rows are right too), and the float64 bound on the adapted rows."""
    from acestep_mi355x import capi
    s = S()
    base, out0, cols, jobs, fmt = kernel_case(name)
    got = capi.kernel_lokr_merge(base, out0, cols, jobs, fmt=fmt, lib=lib)
    src = out0 if base is None else base
    want = out0.copy()
    for j in jobs:
        rows = np.arange(j["row0"], j["row0"] + j["rows"])
        hit = np.zeros(len(rows), bool)
        if "w1" in j:
            delta = s.lokr_delta(j["w1"], j["w2"])
            o = np.arange(delta.shape[0])
            fr = (o // 16) * 32 + j.get("half", 0) * 16 + o % 16 if j.get("map") else j["row_off"] + o
            want[fr, :cols] = s.lora_merge_bits(src[fr, :cols], delta, j["eff"], {"bf16": "BF16", "fp16": "F16"}[fmt])
            hit[fr - rows[0]] = True
            err, bound = f64_bound(j, src[fr, :cols], got[fr, :cols], fmt)
            assert (err <= bound).all(), (name, float((err / bound).max()))
            assert (got[fr, :cols] != src[fr, :cols]).mean() > 0.5  # the delta is applied
        if j.get("copy_rest") and base is not None:
            want[rows[~hit], :cols] = base[rows[~hit], :cols]
    np.testing.assert_array_equal(got, want, err_msg=name)


@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_host_launcher_matches_numpy(host_lib, name):
    check_kernel_case(name, ctypes.CDLL(host_lib))


# ------------------------------------------------------------------ engine
def forward_triple(lib, ad, scale, x, dtype="BF16", as_file=False):
    """(base forward, forward with the adapter at `scale`, forward after set-scale and unload; forward of the numpy-merged
    checkpoint)."""
    base = base_ckpt(dtype)
    br = bridge(lib, base)
    plain = fwd(br, x)
    br.load_lora(os.path.join(ad, "lokr_weights.safetensors") if as_file else ad, scale)
    info = br.lora_info()
    got = fwd(br, x)
    br.set_lora_scale(0.25)
    br.unload_lora()
    after = fwd(br, x)
    br.close()
    bm = bridge(lib, S().merged_lokr_checkpoint(base, ad, scale, tempfile.mkdtemp(prefix="acemi_lokr_m_")))
    ref = fwd(bm, x)
    bm.close()
    return plain, got, after, ref, info


@pytest.mark.parametrize("kw,scale,dtype,as_file", [
    (dict(form="w2_lowrank", r=4), 1.0, "BF16", False),
    (dict(form="both_lowrank", r=3, rs_lora=True, scalar=0.5, targets=("q_proj", "v_proj", "gate_proj", "down_proj")), 0.37, "F16", False),
    (dict(form="full", factor=4, targets=S().LORA_ALL_TARGETS, config=False, dtype="BF16"), 0.8, "BF16", True),
])
def test_lokr_equals_merged_checkpoint_and_unload_restores(host_lib, kw, scale, dtype, as_file):
    plain, got, after, ref, info = forward_triple(host_lib, lokr_adapter(seed=3, **kw), scale, inputs(), dtype, as_file)
    np.testing.assert_array_equal(got, ref)
    assert rel(got, plain) > 1e-4  # the adapter is not ignored
    np.testing.assert_array_equal(after, plain)
    assert info["loaded"] and info["num_modules"] > 0 and info["max_rank"] == (0 if kw["form"] == "full" else kw["r"])


def edited(fn=None, **kw):
    """A LoKr adapter whose tensor dict went through fn (the header metadata is kept)."""
    s = S()
    ad = lokr_adapter(**kw)
    path = os.path.join(ad, "lokr_weights.safetensors")
    t = dict(s._read_safetensors_f32(path))
    fn(t)
    s.write_safetensors(path, list(t.items()), "F32")
    s.set_safetensors_metadata(path, {"algo": "lokr", "format": "lycoris"})
    return ad


Q = "lycoris_layers_0_self_attn_q_proj"
REFUSALS = {
    "tucker": (lambda: edited(lambda t: t.update({Q + ".lokr_t2": np.zeros((2, 2, 1, 1), np.float32)})), Q + ".lokr_t2", ()),
    "dora tensor": (lambda: edited(lambda t: t.update({Q + ".dora_scale": np.ones((1, 256), np.float32)})), Q + ".dora_scale", ()),
    "dora header": (lambda: lokr_adapter(extra_config=dict(weight_decompose=True)), "weight_decompose", ()),
    "module not held": (lambda: edited(lambda t: t.update({"lycoris_lyric_encoder_layers_0_self_attn_q_proj.lokr_w1":
                                                          np.zeros((4, 4), np.float32)})), "lycoris_lyric_encoder_layers_0", ()),
    "not a factorization": (lambda: edited(lambda t: t.update({Q + ".lokr_w1": np.zeros((3, 16), np.float32)}), form="full"), Q, ()),
    "q8 activations": (lokr_adapter, "ACE_MI_QUANT_ACT", (("ACE_GGML_DIT_WEIGHT_QTYPE", "q8_0"), ("ACE_MI_QUANT_ACT", "q8"))),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refused_adapters(host_lib, monkeypatch, case):
    make, needle, env = REFUSALS[case]
    for k, v in env:
        monkeypatch.setenv(k, v)
    br = bridge(host_lib, base_ckpt())
    st, msg = load_status(br, make())
    assert st == UNSUPPORTED and needle in msg, (st, msg)
    assert br.lora_info()["loaded"] is False
    br.close()
