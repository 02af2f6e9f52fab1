"""Shared by tests/test_gpu_lm_raw_blocks.py (the product library) and tests/test_lm_raw_blocks_cpu.py (the host
emulation): the causal LM with ACE_MI_LM_RAW_BLOCKS=1 (runtime/lm.cpp) against the default mode on the same GGUF -- the
`mixed` variant of tests/lm_gguf_cases.py (a fused QKV of Q4_K | Q6_K parts and a Q5_K o_proj stay raw blocks; the Q4_K
gate|up, Q6_K down and Q6_K table keep their planes) and `q5_k`, written here: every matrix and the tied table Q5_K, so
the gather and the tied head run on raw blocks too."""
import os
import tempfile

import numpy as np
import pytest

import lm_cases as lc
import lm_gguf_cases as lg

VARIANTS = ("mixed", "q5_k")
_DIRS = {}


def checkpoint(variant):
    if variant == "mixed":
        return lg.checkpoint("mixed")
    if variant not in _DIRS:
        from acestep_mi355x.synthetic import write_lm_gguf
        _DIRS[variant] = tempfile.mkdtemp(prefix="acemi_lm_raw_q5_k_")
        write_lm_gguf(_DIRS[variant], "Q5_K", tied=True, seed=lg.SEED)
    return _DIRS[variant]


def raw_mode_bytes(path):
    """lm_gguf_cases.resident_bytes with the file's block bytes where that counts a bf16 image"""
    plane = {8: 1.125, 12: 0.75, 14: 1.25}
    t = {n[6:] if n.startswith("model.") else n: v for n, v in lg.read_gguf_dir(path).items()}

    def matrix(names):
        types = {t[n][0] for n in names}
        if len(types) == 1 and next(iter(types)) in plane:
            return int(sum(int(np.prod(t[n][1])) for n in names) * plane[next(iter(types))])
        assert all(t[n][0] not in (0, 1, 30) for n in names)
        return sum(len(t[n][2]) for n in names)

    total = sum(4 * shape[0] for _, shape, _ in t.values() if len(shape) == 1)
    for i in range(1 + max(int(n.split(".")[1]) for n in t if n.startswith("layers."))):
        p = f"layers.{i}."
        total += matrix([p + f"self_attn.{x}_proj.weight" for x in "qkv"]) + matrix([p + "self_attn.o_proj.weight"])
        total += matrix([p + "mlp.gate_proj.weight", p + "mlp.up_proj.weight"]) + matrix([p + "mlp.down_proj.weight"])
    return total + matrix(["embed_tokens.weight"])


def load_pair(new_bridge, variant):
    """(default-mode bridge, raw-mode bridge) on the variant's file; the variable is read by ace_mi_load_lm"""
    plain, raw = new_bridge(), new_bridge()
    plain.load_lm(checkpoint(variant))
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("ACE_MI_LM_RAW_BLOCKS", "1")
        raw.load_lm(checkpoint(variant))
    return plain, raw


class LmRawBlocksChecks:
    """A test file subclasses this as Test..., sets DEVICE and LABEL and provides the module fixture `pairs`
    (variant -> load_pair's bridges)."""
    DEVICE = None
    LABEL = None

    @pytest.mark.parametrize("variant", VARIANTS)
    def test_weight_bytes_are_the_files_blocks(self, pairs, variant):
        plain, raw = pairs(variant)
        want = raw_mode_bytes(os.path.join(checkpoint(variant), "model.gguf"))
        got = raw.lm_info()["weight_bytes"]
        print(f"{self.LABEL} {variant}: weight_bytes raw mode {got}, default {plain.lm_info()['weight_bytes']}")
        assert got == want and got < plain.lm_info()["weight_bytes"]

    @pytest.mark.parametrize("variant", VARIANTS)
    def test_prefill_identical_and_steps_within_the_default_paths_own_gap(self, pairs, variant):
        """The prefill call: the default mode's bits.  The decode calls against the default mode's: within the default
        path's own distance between a step and the prefill of the same tokens (the measure of
        lm_gguf_cases.test_step_matches_prefill_of_same_tokens), per call and row."""
        plain, raw = pairs(variant)
        ids, mask, prompt, _ = lg.case("mixed", "a")
        a, b = lc.drive(plain, ids, mask, prompt, self.DEVICE), lc.drive(raw, ids, mask, prompt, self.DEVICE)
        np.testing.assert_array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
        gap = lc.rel_l2(a, lc.full_sequence(plain, ids, mask, prompt, self.DEVICE))[1:]
        d = lc.rel_l2(b, a)[1:]
        print(f"{self.LABEL} {variant}: raw-mode steps vs default steps rel_l2 max {d.max():.3e}, default step vs prefill "
              f"min {gap.min():.3e}")
        assert np.all(d <= gap), (variant, float((d / gap).max()))

    def test_mixed_steps_within_the_fixture_bound(self, pairs):
        got, err, bound = lg.measure(pairs("mixed")[1], "mixed", "a", self.DEVICE, self.LABEL + " raw")
        assert np.isfinite(got).all() and np.all(err <= bound), float(np.nanmax(err / bound))

    def test_generate_yields_the_default_modes_tokens(self, pairs):
        import torch
        ids, mask, prompt, _ = lg.case("mixed", "a")
        toks = []
        for br in pairs("mixed"):
            br.lm_begin(ids.shape[0], prompt + 12)
            logits = br.lm_forward(torch.from_numpy(ids[:, :prompt].copy()).to(self.DEVICE),
                                   torch.from_numpy(mask[:, :prompt].copy()).to(self.DEVICE))
            t, n_out = br.lm_generate(logits, 12, temperature=1.0, top_k=50, seed=11)
            assert n_out == 12
            toks.append(t.cpu().numpy())
        np.testing.assert_array_equal(toks[0], toks[1])
