"""Shared by tests/test_gpu_lm_gguf.py (the product library on the GPU) and tests/test_lm_gguf_cpu.py (the host
emulation): the causal LM on GGUF checkpoints (acestep_mi355x.synthetic.LM_GGUF_VARIANTS) against
tests/golden/lm_qwen3_gguf.npz -- float64 Qwen3ForCausalLM logits with weights equal to the exact f32 dequant of each
GGUF's blocks (tests/golden/make_lm_gguf_fixture.py), on the ids / masks of cases a, b and e of lm_qwen3.npz.

The bound is tests/lm_cases.py's rule: per call and row, rel-L2 over the vocabulary <= 1.5 x the larger of
  * the error of the engine's full-sequence prefill path on the same tokens (BlockRunner's quantized GEMMs: code that
    the text encoder has run on such files all along), and
  * the error of oracle/text_oracle.py on the same GGUF, the oracle reading the file's types (ggml's quantized mul_mat),
    for rows without padding.  The oracle reads F32 / F16 / BF16 / Q8_0 / Q4_K / Q6_K files only: `mixed` has a Q5_K
    tensor, so its bound is the first number alone (np.fmax keeps the number that exists; never the wider choice)."""
import hashlib
import os
import struct
import tempfile

import numpy as np

import lm_cases as lc

SEED = 7
VARIANTS = ("q8_0", "q4_k", "q6_k", "mixed")
ORACLE_VARIANTS = ("q8_0", "q4_k", "q6_k")
_CACHE = {}


def fixture():
    if "z" not in _CACHE:
        _CACHE["z"] = np.load(os.path.join(lc.GOLDEN, "lm_qwen3_gguf.npz"))
    return _CACHE["z"]


def case(variant, name):
    """(ids, mask, prompt, float64-model logits [calls][B][vocab])"""
    b = lc.fixture()
    return (b[f"tied/{name}/ids"], b[f"tied/{name}/mask"], int(b[f"tied/{name}/prompt"]),
            fixture()[f"{variant}/{name}/logits"])


def spec(variant):
    from acestep_mi355x.synthetic import LM_GGUF_VARIANTS
    return LM_GGUF_VARIANTS[variant]


def checkpoint(variant, model_prefix=True, **kw):
    """directory holding config.json + model.gguf of the variant"""
    from acestep_mi355x.synthetic import write_lm_gguf
    key = (variant, model_prefix, tuple(sorted(kw.items())))
    if key not in _CACHE:
        d = tempfile.mkdtemp(prefix=f"acemi_lm_gguf_{variant}_")
        s = spec(variant)
        write_lm_gguf(d, s["types"], tied=s["tied"], seed=SEED, model_prefix=model_prefix, **kw)
        _CACHE[key] = d
    return _CACHE[key]


def sha256(d):
    with open(os.path.join(d, "model.gguf"), "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


# ggml type id -> (values per block, bytes per block)
_TYPE_BYTES = {0: (1, 4), 1: (1, 2), 30: (1, 2), 2: (32, 18), 3: (32, 20), 6: (32, 22), 7: (32, 24), 8: (32, 34),
               10: (256, 84), 11: (256, 110), 12: (256, 144), 13: (256, 176), 14: (256, 210), 20: (32, 18)}


def read_gguf_dir(path):
    """GGUF v3 tensor directory: name -> (ggml type id, numpy shape, raw bytes); sizes from the next offset."""
    data = open(path, "rb").read()
    pos = [4]

    def rd(fmt):
        v = struct.unpack_from("<" + fmt, data, pos[0])
        pos[0] += struct.calcsize("<" + fmt)
        return v[0] if len(v) == 1 else v

    def rstr():
        n = rd("Q")
        s = data[pos[0]:pos[0] + n].decode()
        pos[0] += n
        return s

    assert data[:4] == b"GGUF"
    version, n_tensors, n_kv = rd("IQQ")
    assert version == 3
    for _ in range(n_kv):
        rstr()
        t = rd("I")
        if t == 8:
            rstr()
        else:
            pos[0] += {0: 1, 1: 1, 2: 2, 3: 2, 4: 4, 5: 4, 6: 4, 7: 1, 10: 8, 11: 8, 12: 8}[t]
    infos = []
    for _ in range(n_tensors):
        name = rstr()
        nd = rd("I")
        ne = [rd("Q") for _ in range(nd)]
        gt, off = rd("IQ")
        infos.append((name, gt, ne, off))
    start = (pos[0] + 31) // 32 * 32
    ends = sorted(o for _, _, _, o in infos)[1:] + [len(data) - start]
    by_off = dict(zip(sorted(o for _, _, _, o in infos), ends))
    out = {}
    for name, gt, ne, off in infos:
        n = int(np.prod(ne))
        bv, bb = _TYPE_BYTES[gt]
        assert n % bv == 0 and n // bv * bb <= by_off[off] - off, name
        out[name] = (gt, tuple(reversed(ne)), data[start + off:start + off + n // bv * bb])
    return out


def resident_bytes(path):
    """What ace_mi_load_lm keeps in HBM for the file, from the tensor shapes and types alone: planes for Q8_0 / Q4_K /
    Q6_K matrices (1.125 / 0.75 / 1.25 bytes per weight), a bf16 image for every other block type and for a fused QKV
    or gate|up whose parts differ in type, 16-bit words for dense matrices, f32 for 1-D tensors; the embed table once
    (planes shared by the gather and a tied head)."""
    plane = {8: 1.125, 12: 0.75, 14: 1.25}
    dense = {1: 2, 30: 2}
    t = {n[6:] if n.startswith("model.") else n: v for n, v in read_gguf_dir(path).items()}
    total = 0

    def matrix(names):
        types = {t[n][0] for n in names}
        weights = sum(int(np.prod(t[n][1])) for n in names)
        gt = types.pop() if len(types) == 1 else None
        if gt in plane:
            return int(weights * plane[gt])
        return weights * 2 if gt is None or gt not in dense else weights * dense[gt]

    for name, (gt, shape, _) in t.items():
        if len(shape) == 1:
            total += 4 * shape[0]
    layers = 1 + max(int(n.split(".")[1]) for n in t if n.startswith("layers."))
    for i in range(layers):
        p = f"layers.{i}."
        total += matrix([p + f"self_attn.{x}_proj.weight" for x in "qkv"]) + matrix([p + "self_attn.o_proj.weight"])
        total += matrix([p + "mlp.gate_proj.weight", p + "mlp.up_proj.weight"]) + matrix([p + "mlp.down_proj.weight"])
    total += matrix(["embed_tokens.weight"])
    if "lm_head.weight" in t:
        total += matrix(["lm_head.weight"])
    return total


def oracle_logits(variant, ids_row, prompt):
    """oracle/text_oracle.py on the variant's GGUF (names without "model."; the same bytes), the file's types kept: logits
    at the position of every call of one unpadded row.  The head product is ggml's too (mul_mat on the file's type)."""
    from oracle import text_oracle as to
    from oracle.dit_oracle import mul_mat
    key = ("W", variant)
    if key not in _CACHE:
        d = checkpoint(variant, model_prefix=False)
        g = os.path.join(d, "model.gguf")
        W = to.TextWeights(d, gguf=g)
        _CACHE[key] = (W, _head(g, spec(variant)["tied"]))
    W, head = _CACHE[key]
    hidden = to.forward_text_encoder_layers(W, np.asarray(ids_row, np.int32))
    return mul_mat(head, hidden[prompt - 1:].astype(np.float32)).astype(np.float64)


def _head(gguf, tied):
    from oracle.dit_oracle import read_gguf, _gguf_values
    from oracle.ggml_numerics import GgmlWeight
    from oracle.text_oracle import _GGUF_QT
    gt, ne, raw = read_gguf(gguf)["embed_tokens.weight" if tied else "lm_head.weight"]
    return GgmlWeight(_gguf_values(gt, ne, raw).reshape(ne[1], ne[0]), _GGUF_QT[gt])


def measure(bridge, variant, name, device, label):
    """lm_cases.measure on a GGUF variant: (got, err, bound), err / bound [calls][B]; prints every figure."""
    ids, mask, prompt, ref = case(variant, name)
    got = lc.drive(bridge, ids, mask, prompt, device)
    err = lc.rel_l2(got, ref)
    full = lc.rel_l2(lc.full_sequence(bridge, ids, mask, prompt, device), ref)
    ora = np.full_like(err, np.nan)
    if variant in ORACLE_VARIANTS:
        for b in range(ids.shape[0]):
            if mask[b].all():
                ora[:, b] = lc.rel_l2(oracle_logits(variant, ids[b], prompt), ref[:, b])
    bound = np.fmax(1.5 * full, 1.5 * ora)
    key = f"{variant}/{name}"
    for i in range(err.shape[0]):
        print(f"{label} {key} call {i}: rel_l2 step path {np.array2string(err[i], precision=3)} full-sequence path "
              f"{np.array2string(full[i], precision=3)} oracle {np.array2string(ora[i], precision=3)} "
              f"bound {np.array2string(bound[i], precision=3)}")
    print(f"{label} {key}: max rel_l2 {err.max():.3e}, max err/bound {np.nanmax(err / bound):.3f}")
    return got, err, bound


# ---------------------------------------------------------------------------------------------- the tests themselves
def iq2_checkpoint():
    """the q8_0 variant with one projection declared as IQ2_XXS (ggml type 16: no decoder here)"""
    from acestep_mi355x import synthetic as s
    if "iq2" not in _CACHE:
        names = {v: k for k, v in s.GGML_TYPES.items()}
        d = tempfile.mkdtemp(prefix="acemi_lm_gguf_iq2_")
        src = checkpoint("q8_0")
        tensors = {n: (sh, names[gt], raw) for n, (gt, sh, raw) in read_gguf_dir(os.path.join(src, "model.gguf")).items()}
        sh = tensors["model.layers.1.self_attn.o_proj.weight"][0]
        tensors["model.layers.1.self_attn.o_proj.weight"] = (sh, "IQ2_XXS", bytes(sh[0] * sh[1] // 256 * 66))
        s.GGML_TYPES["IQ2_XXS"] = 16
        try:
            s.write_gguf_tensors(os.path.join(d, "model.gguf"), tensors)
        finally:
            del s.GGML_TYPES["IQ2_XXS"]
        with open(os.path.join(src, "config.json"), "rb") as f, open(os.path.join(d, "config.json"), "wb") as g:
            g.write(f.read())
        _CACHE["iq2"] = d
    return _CACHE["iq2"]


class LmGgufChecks:
    """A test file subclasses this as Test..., sets DEVICE, LABEL and CASES ((variant, case) pairs to run) and provides
    the module fixtures `new_bridge` (() -> a fresh bridge) and `loaded` (variant -> a bridge with the variant loaded)."""
    DEVICE = None
    LABEL = None
    CASES = ()
    _results = {}

    @classmethod
    def result(cls, loaded, variant, name):
        key = (cls.__name__, variant, name)
        if key not in cls._results:
            cls._results[key] = measure(loaded(variant), variant, name, cls.DEVICE, cls.LABEL)
        return cls._results[key]

    def test_writer_matches_fixture_sha(self):
        for v in VARIANTS:
            assert sha256(checkpoint(v)) == str(fixture()[f"{v}/sha256"]), v

    def test_every_variant_loads(self, loaded):
        for v in VARIANTS:
            info = loaded(v).lm_info()
            assert info["tied"] == int(spec(v)["tied"]) and info["vocab_size"] == 1000 and info["act_type"] == 0, (v, info)

    def test_resident_size(self, loaded):
        """weight_bytes = the plane / image / 1-D bytes of the shapes: one copy of a tied table, no f32 or bf16 twin"""
        for v in VARIANTS:
            want = resident_bytes(os.path.join(checkpoint(v), "model.gguf"))
            assert loaded(v).lm_info()["weight_bytes"] == want, (v, loaded(v).lm_info()["weight_bytes"], want)
        # the tied Q4_K model by hand: 2 layers x (qkv 1024 + o 512 + gate|up 1024 + down 512 rows-by-256-equivalents)
        c = 256
        mats = 2 * ((512 + 256 + 256) * c + c * 512 + 2 * 512 * c + c * 512) + 1000 * c
        norms = (c + 2 * (2 * c + 2 * 128)) * 4
        assert resident_bytes(os.path.join(checkpoint("q4_k"), "model.gguf")) == mats * 3 // 4 + norms

    def test_logits_within_bound(self, loaded):
        for v, name in self.CASES:
            got, err, bound = self.result(loaded, v, name)
            assert np.isfinite(got).all()
            assert np.all(err <= bound), (v, name, float(np.nanmax(err / bound)))

    def test_step_matches_prefill_of_same_tokens(self, loaded):
        for v, name in self.CASES:
            ids, mask, prompt, _ = case(v, name)
            got, _, bound = self.result(loaded, v, name)
            full = lc.full_sequence(loaded(v), ids, mask, prompt, self.DEVICE)
            d = lc.rel_l2(got, full)
            print(f"{self.LABEL} {v}/{name}: step vs prefill of the same tokens rel_l2 max {d[1:].max():.3e} "
                  f"(bound min {bound.min():.3e})")
            np.testing.assert_array_equal(got[0], full[0])       # the prefill call is the same computation
            assert np.all(d[1:] <= bound[1:]), (v, name, float((d[1:] / bound[1:]).max()))

    def test_padding_keys_have_no_effect(self, loaded):
        """Case b row 1 (8 padding slots, then the prompt) against the same engine's run of that row unpadded at B = 1
        (RoPE is relative and padding keys are masked: equal in exact arithmetic), under row 1's bound."""
        for v in sorted({v for v, name in self.CASES if name == "b"}):
            ids, mask, prompt, _ = case(v, "b")
            got, _, bound = self.result(loaded, v, "b")
            pad = int((mask[1] == 0).sum())
            assert pad == 8
            alone = lc.drive(loaded(v), ids[1:, pad:], mask[1:, pad:], prompt - pad, self.DEVICE)
            d = lc.rel_l2(got[:, 1], alone[:, 0])
            print(f"{self.LABEL} {v}/b row 1 vs its unpadded run: rel_l2 max {d.max():.3e}")
            assert np.all(d <= bound[:, 1]), (v, float((d / bound[:, 1]).max()))

    def test_two_runs_identical(self, loaded):
        for v, name in self.CASES:
            if name == "a":
                continue
            ids, mask, prompt, _ = case(v, name)
            a = lc.drive(loaded(v), ids, mask, prompt, self.DEVICE)
            b = lc.drive(loaded(v), ids, mask, prompt, self.DEVICE)
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))

    def test_environment_keys(self, new_bridge, loaded, monkeypatch):
        """ACE_GGML_LM_GGUF selects the file; the text encoder's key alone does not: the directory's safetensors load."""
        gguf = os.path.join(checkpoint("q4_k"), "model.gguf")
        plain = lc.checkpoint("tied")
        want_q = loaded("q4_k").lm_info()["weight_bytes"]
        br = new_bridge()
        try:
            br.load_lm(plain)
            want_plain = br.lm_info()["weight_bytes"]
            assert want_plain != want_q
            monkeypatch.setenv("ACE_GGML_TEXT_ENCODER_GGUF", gguf)
            monkeypatch.setenv("ACE_GGML_QWEN_GGUF", gguf)
            br.load_lm(plain)
            assert br.lm_info()["weight_bytes"] == want_plain
            monkeypatch.setenv("ACE_GGML_LM_GGUF", gguf)
            br.load_lm(plain)                              # config.json of `plain` (the same tiny shape), tensors of the GGUF
            assert br.lm_info()["weight_bytes"] == want_q
            monkeypatch.delenv("ACE_GGML_LM_GGUF")
            monkeypatch.delenv("ACE_GGML_TEXT_ENCODER_GGUF")
            monkeypatch.delenv("ACE_GGML_QWEN_GGUF")
            br.load_lm(gguf)                               # a path ending in .gguf, config.json beside it
            assert br.lm_info()["weight_bytes"] == want_q
            monkeypatch.setenv("ACE_GGML_QWEN_WEIGHT_QTYPE", "q8_0")
            br.load_lm(gguf)                               # ignored with a GGUF: the file's types hold
            assert br.lm_info()["weight_bytes"] == want_q
        finally:
            br.close()

    def test_remaining_refusals(self, new_bridge, monkeypatch):
        import pytest
        br = new_bridge()
        try:
            with pytest.raises(RuntimeError, match=r"(?s)16.*o_proj.*status=4"):
                br.load_lm(iq2_checkpoint())
            monkeypatch.setenv("ACE_GGML_QWEN_WEIGHT_QTYPE", "q8_0")
            with pytest.raises(RuntimeError, match=r"quantized LM weights are not supported.*status=4"):
                br.load_lm(lc.checkpoint("tied"))
            monkeypatch.delenv("ACE_GGML_QWEN_WEIGHT_QTYPE")
            with pytest.raises(RuntimeError, match=r"16-bit.*status=4"):
                br.load_lm(lc.checkpoint("tied", dtype="F32"))
        finally:
            br.close()
