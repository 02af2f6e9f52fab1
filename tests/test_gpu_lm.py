"""GPU tests of the causal LM on the engine (ace_mi_load_lm / ace_mi_lm_*, kernels/lm_decode.hip, hook.install_lm_backend)
against tests/golden/lm_qwen3.npz (transformers' Qwen3ForCausalLM in float64, tests/golden/make_lm_fixture.py).

Measured on MI355X (rel-L2 over the vocabulary, worst call and row of each case; bound = tests/lm_cases.py): see
DESIGN.md §5."""
import os

import numpy as np
import pytest

import lm_cases as lc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def bridges():
    from acestep_mi355x.capi import GGMLCAPIBridge
    made = {}

    def get(variant):
        if variant not in made:
            assert lc.sha256(lc.checkpoint(variant)) == str(lc.fixture()[f"{variant}/sha256"])
            br = GGMLCAPIBridge()
            br.load_lm(lc.checkpoint(variant))
            made[variant] = br
        return made[variant]
    yield get
    for br in made.values():
        br.close()


@pytest.fixture(scope="module")
def results(bridges):
    """Every case once per variant: (got, err, bound), shared by the tests below and never modified."""
    done = {}

    def get(variant, case):
        if (variant, case) not in done:
            done[(variant, case)] = lc.measure(bridges(variant), variant, case, DEV, "gpu")
        return done[(variant, case)]
    return get


@pytest.mark.parametrize("case", ["a", "b", "c", "d", "e"])
@pytest.mark.parametrize("variant", ["tied", "untied"])
def test_lm_logits_vs_transformers(results, variant, case):
    """Every call of every case: prefill logits, then every decode step's, per row."""
    got, err, bound = results(variant, case)
    assert np.isfinite(got).all()
    assert np.all(err <= bound), (variant, case, float(np.nanmax(err / bound)))


@pytest.mark.parametrize("variant,case", [("tied", "a"), ("untied", "e")])
def test_lm_step_matches_prefill_of_same_tokens(bridges, results, variant, case):
    """No fixture: the step logits at cache length L against the prefill logits of the same L + 1 tokens, under the
    case's bound (the distance of two engine paths that each sit within it of the float64 model)."""
    z = lc.fixture()
    key = f"{variant}/{case}"
    ids, mask, prompt = z[key + "/ids"], z[key + "/mask"], int(z[key + "/prompt"])
    got, _, bound = results(variant, case)
    full = lc.full_sequence(bridges(variant), ids, mask, prompt, DEV)
    d = lc.rel_l2(got, full)
    print(f"gpu {key}: step vs prefill of the same tokens rel_l2 max {d.max():.3e} (bound min {bound.min():.3e})")
    np.testing.assert_array_equal(got[0], full[0])       # the prefill call is the same computation
    assert np.all(d[1:] <= bound[1:]), float((d[1:] / bound[1:]).max())


@pytest.mark.parametrize("variant", ["tied", "untied"])
def test_lm_padding_keys_have_no_effect(results, variant):
    """Case (b) row 1 (8 padding slots, then the prompt) against the float64 model's run of the same prompt unpadded at
    B = 1 (fixture b1u; RoPE is relative, so the 8-position offset changes nothing in exact arithmetic)."""
    z = lc.fixture()
    got, _, bound = results(variant, "b")
    d = lc.rel_l2(got[:, 1], z[f"{variant}/b1u/logits"][:, 0])
    print(f"gpu {variant}/b row 1 vs unpadded float64 run: rel_l2 max {d.max():.3e}")
    assert np.all(d <= bound[:, 1]), float((d / bound[:, 1]).max())


def test_lm_determinism(bridges):
    z = lc.fixture()
    ids, mask, prompt = z["tied/b/ids"], z["tied/b/mask"], int(z["tied/b/prompt"])
    a = lc.drive(bridges("tied"), ids, mask, prompt, DEV)
    b = lc.drive(bridges("tied"), ids, mask, prompt, DEV)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    ids, mask, prompt = z["tied/e/ids"], z["tied/e/mask"], int(z["tied/e/prompt"])   # the split-and-merge path
    a = lc.drive(bridges("tied"), ids, mask, prompt, DEV)
    b = lc.drive(bridges("tied"), ids, mask, prompt, DEV)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def test_lm_state_handling(bridges, results):
    import torch
    br = bridges("tied")
    z = lc.fixture()
    got, _, _ = results("tied", "a")
    ids = torch.from_numpy(z["tied/a/ids"]).to(DEV)
    ones = torch.ones((1, 37), dtype=torch.int32, device=DEV)   # as the case ran: the prefill's key-mask path
    info = br.lm_info()
    assert info["tied"] == 1 and info["vocab_size"] == 1000 and info["num_layers"] == 2 and info["head_dim"] == 128
    br.lm_begin(1, 39)
    first = br.lm_forward(ids[:, :37], ones).cpu().numpy()
    np.testing.assert_array_equal(first, got[0])
    info = br.lm_info()
    assert (info["batch"], info["capacity"], info["cache_len"]) == (1, 39, 37)
    assert info["cache_bytes"] >= 39 * 2 * 2 * 2 * 128 * 2
    with pytest.raises(RuntimeError, match="empty cache.*status=2"):
        br.lm_forward(ids[:, :2])                              # n > 1 on a non-empty cache (it would fit)
    br.lm_forward(ids[:, 37:38])
    br.lm_forward(ids[:, 38:39])
    with pytest.raises(RuntimeError, match="capacity.*status=2"):
        br.lm_forward(ids[:, 39:40])                           # 40 > capacity 39; the cache stays as it was
    assert br.lm_info()["cache_len"] == 39
    br.lm_begin(1, 64)                                         # begin after use resets the cache
    assert br.lm_info()["cache_len"] == 0
    seq = [br.lm_forward(ids[:, :37], ones)] + [br.lm_forward(ids[:, i:i + 1]) for i in range(37, 40)]
    np.testing.assert_array_equal(torch.stack(seq).cpu().numpy(), got[:4])
    br.lm_begin(1, 39)                                         # refused forward, then the next legal step still matches
    br.lm_forward(ids[:, :37], ones)
    br.lm_forward(ids[:, 37:38])
    with pytest.raises(RuntimeError, match="status=2"):
        br.lm_forward(ids[:, :5])
    np.testing.assert_array_equal(br.lm_forward(ids[:, 38:39]).cpu().numpy(), got[2])
    br.lm_reset()
    assert br.lm_info()["cache_len"] == 0
    for bad in ((0, 8), (9, 8), (1, 0), (1, info["max_positions"] + 1)):
        with pytest.raises(RuntimeError, match="status=2"):
            br.lm_begin(*bad)


def test_lm_not_loaded_and_quantized_refused(monkeypatch):
    import torch
    from acestep_mi355x.capi import GGMLCAPIBridge
    br = GGMLCAPIBridge()
    try:
        with pytest.raises(RuntimeError, match="lm not loaded"):
            br.lm_begin(1, 8)
        ids = torch.zeros((1, 1), dtype=torch.int32, device=DEV)
        out = torch.zeros((1, 1000), device=DEV)
        with pytest.raises(RuntimeError, match="lm not loaded"):
            br.lm_forward_device(ids.data_ptr(), 0, 1, out.data_ptr())
        monkeypatch.setenv("ACE_GGML_QWEN_WEIGHT_QTYPE", "q8_0")
        with pytest.raises(RuntimeError, match=r"quantized LM weights are not supported.*status=4"):
            br.load_lm(lc.checkpoint("tied"))
        monkeypatch.delenv("ACE_GGML_QWEN_WEIGHT_QTYPE")
        with pytest.raises(RuntimeError, match=r"16-bit.*status=4"):
            br.load_lm(lc.checkpoint("tied", dtype="F32"))
        br.load_lm(lc.checkpoint("tied", model_prefix=False))   # names without the "model." prefix
        assert br.lm_info()["tied"] == 1
    finally:
        br.close()


def test_text_encoder_unchanged_beside_resident_lm():
    """ace_ggml_load_text_encoder / ace_ggml_load_lm keep their slot and their bits with an LM resident."""
    import tempfile
    from acestep_mi355x.capi import GGMLCAPIBridge
    from acestep_mi355x.synthetic import TEXT_TINY_CONFIG, text_tensor_specs, write_checkpoint
    d = tempfile.mkdtemp(prefix="acemi_lmte_")
    write_checkpoint(d, TEXT_TINY_CONFIG, seed=6, dtype="BF16", specs=text_tensor_specs(TEXT_TINY_CONFIG))
    ids = np.random.default_rng(5).integers(0, 1000, 70).astype(np.int32)
    z = lc.fixture()
    br = GGMLCAPIBridge()
    try:
        br.load_text_encoder(d)
        before = br.text_encoder_forward(ids)
        br.load_lm(lc.checkpoint("untied"))
        lm = lc.drive(br, z["untied/c/ids"], z["untied/c/mask"], int(z["untied/c/prompt"]), DEV)
        assert np.isfinite(lm).all()
        np.testing.assert_array_equal(br.text_encoder_forward(ids).view(np.uint32), before.view(np.uint32))
        br._ensure_ok(br.lib.ace_ggml_load_lm(br.ctx, d.encode()), "ace_ggml_load_lm")   # still the text-encoder slot
        np.testing.assert_array_equal(br.text_encoder_forward(ids).view(np.uint32), before.view(np.uint32))
        again = lc.drive(br, z["untied/c/ids"], z["untied/c/mask"], int(z["untied/c/prompt"]), DEV)
        np.testing.assert_array_equal(again.view(np.uint32), lm.view(np.uint32))
    finally:
        br.close()


def test_hook_reproduces_case_b(bridges, results):
    """install_lm_backend + a hand-written copy of the reference loop's calling pattern (prefill, then
    input_ids[:, -1:] with past_key_values and the grown mask)."""
    import torch
    from acestep_mi355x.hook import install_lm_backend

    class Handler:
        llm = None
        llm_backend = None
        device = DEV

    h = Handler()
    install_lm_backend(h, bridges("tied"), max_new_tokens=32)
    assert h.llm_backend == "pt"
    z = lc.fixture()
    got, _, _ = results("tied", "b")
    ids = torch.from_numpy(z["tied/b/ids"].astype(np.int64)).to(DEV)
    mask = torch.from_numpy(z["tied/b/mask"].astype(np.int64)).to(DEV)
    P = int(z["tied/b/prompt"])
    model = h.llm
    generated, attn = ids[:, :P], mask[:, :P]
    out = model(input_ids=generated, attention_mask=attn, past_key_values=None, use_cache=True)
    logits = [out.logits[:, -1, :]]
    past = out.past_key_values
    stale = past
    for i in range(P, ids.shape[1]):
        generated = torch.cat([generated, ids[:, i:i + 1]], dim=1)
        attn = torch.cat([attn, torch.ones((2, 1), dtype=attn.dtype, device=DEV)], dim=1)
        out = model(input_ids=generated[:, -1:], attention_mask=attn, past_key_values=past, use_cache=True)
        past = out.past_key_values
        logits.append(out.logits[:, -1, :])
    assert out.logits.shape == (2, 1, 1000)
    np.testing.assert_array_equal(torch.stack(logits).cpu().numpy(), got)
    model(input_ids=ids[:, :P], attention_mask=mask[:, :P])          # a new prefill: the old handle dies
    with pytest.raises(ValueError, match="stale"):
        model(input_ids=ids[:, -1:], attention_mask=attn, past_key_values=stale)
