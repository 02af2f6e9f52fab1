"""Generates tests/golden/lm_qwen3.npz: the causal LM's reference-side pin.

transformers' Qwen3ForCausalLM in float64 with eager attention on the synthetic tiny LM checkpoint
(acestep_mi355x.synthetic.write_lm_checkpoint, seed 7, BF16 weights: exactly representable), tied and untied, driven
the way the reference's `pt` backend drives it (acestep/llm_inference.py:345-367): one
`model(input_ids, attention_mask, use_cache=True)` prefill, then single-token calls with `past_key_values` and a growing
mask, no position_ids (positions are slot indices, padding included).  The fixture holds no weights: it records the
sha256 of each checkpoint's safetensors bytes, the ids, the masks and the last-position logits of every call.

Cases (per variant `tied` / `untied`):
  a      B = 1, prompt 37, 24 steps
  b      B = 2, prompts 37 and 29 left-padded to 37, 24 steps, the same appended token in both rows
  b1u    row 1 of b unpadded at B = 1 (what the padded row must equal: RoPE is relative, padding keys are masked)
  c      B = 1, prompt 60, 8 steps (crosses the 64-key tile edge)
  d      B = 1, prompt 1 (the engine feeds it through its n == 1 path on an empty cache), 4 steps
  e      B = 2, prompts 256 and 251 left-padded to 256, 4 steps: the first step attends 257 keys, one more than the
         decode attention's LM_SPLIT_KEYS = 256, so every step takes the split-and-merge path

Run from the repo root: python tests/golden/make_lm_fixture.py"""
import hashlib
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ace-step-1.5-ggml_amd"))

from acestep_mi355x.synthetic import TEXT_TINY_CONFIG, write_lm_checkpoint  # noqa: E402
from oracle.dit_oracle import read_safetensors  # noqa: E402

SEED = 7
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lm_qwen3.npz")
# name: (prompt lengths per row, steps)
CASES = {"a": ((37,), 24), "b": ((37, 29), 24), "c": ((60,), 8), "d": ((1,), 4), "e": ((256, 251), 4)}


def hf_model(st_path, tied):
    from transformers import Qwen3Config, Qwen3ForCausalLM
    c = TEXT_TINY_CONFIG
    cfg = Qwen3Config(vocab_size=c["vocab_size"], hidden_size=c["hidden_size"], intermediate_size=c["intermediate_size"],
                      num_hidden_layers=c["num_hidden_layers"], num_attention_heads=c["num_attention_heads"],
                      num_key_value_heads=c["num_key_value_heads"], head_dim=c["head_dim"],
                      max_position_embeddings=c["max_position_embeddings"], rms_norm_eps=c["rms_norm_eps"],
                      rope_theta=c["rope_theta"], attention_bias=False, tie_word_embeddings=tied)
    cfg._attn_implementation = "eager"
    model = Qwen3ForCausalLM(cfg).double().eval()
    sd = {k: torch.from_numpy(v[2].astype(np.float64)) for k, v in read_safetensors(st_path).items()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all("rotary" in m or (tied and m == "lm_head.weight") for m in missing), (missing, unexpected)
    if tied:
        model.tie_weights()
        assert model.lm_head.weight.data_ptr() == model.model.embed_tokens.weight.data_ptr()
    return model


def additive_mask(mask, q0, q1):
    """The [B, 1, q, kv] additive form of attention_mask [B, q1] for queries q0..q1-1 over keys 0..q1-1: what
    transformers builds from the 2-D mask (causal and padding keys masked), with -1e30 instead of finfo(float64).min.
    In float64 `score + finfo.min` overflows to -inf for a negative score, the all-masked rows of left-padding queries
    turn into NaN and 0 * NaN then poisons every later query of the sequence; in the float32 / bfloat16 runs of the
    reference that sum is finite.  A 4-D mask is passed through unchanged."""
    kv = torch.arange(q1)
    allow = (kv[None, :] <= torch.arange(q0, q1)[:, None])[None] & (torch.from_numpy(mask[:, :q1]) != 0)[:, None, :]
    return torch.where(allow, 0.0, -1e30).double()[:, None]


def drive(model, ids, mask, prompt):
    """The reference loop's calls: prefill, then ids[:, -1:] with past_key_values and the grown mask."""
    t_ids = torch.from_numpy(ids.astype(np.int64))
    out = model(input_ids=t_ids[:, :prompt], attention_mask=additive_mask(mask, 0, prompt), use_cache=True)
    logits = [out.logits[:, -1, :].numpy()]
    past = out.past_key_values
    for i in range(prompt, ids.shape[1]):
        out = model(input_ids=t_ids[:, i:i + 1], attention_mask=additive_mask(mask, i, i + 1), past_key_values=past,
                    use_cache=True)
        past = out.past_key_values
        logits.append(out.logits[:, -1, :].numpy())
    out = np.stack(logits)   # [calls][B][vocab]
    assert np.isfinite(out).all()
    return out.astype(np.float32)


def main():
    res = {"seed": np.array(SEED)}
    vocab = TEXT_TINY_CONFIG["vocab_size"]
    for variant in ("tied", "untied"):
        d = tempfile.mkdtemp(prefix="acemi_lm_fix_")
        write_lm_checkpoint(d, seed=SEED, tied=variant == "tied")
        st = os.path.join(d, "model.safetensors")
        with open(st, "rb") as f:
            res[f"{variant}/sha256"] = np.array(hashlib.sha256(f.read()).hexdigest())
        model = hf_model(st, variant == "tied")
        rng = np.random.default_rng(2027)
        with torch.no_grad():
            for name, (prompts, steps) in CASES.items():
                P, B = max(prompts), len(prompts)
                ids = np.zeros((B, P + steps), np.int32)
                mask = np.ones((B, P + steps), np.int32)
                new = rng.integers(1, vocab, steps)
                for b, p in enumerate(prompts):
                    ids[b, P - p:P] = rng.integers(1, vocab, p)
                    mask[b, :P - p] = 0
                    ids[b, P:] = new
                key = f"{variant}/{name}"
                res[key + "/ids"], res[key + "/mask"], res[key + "/prompt"] = ids, mask, np.array(P)
                res[key + "/logits"] = drive(model, ids, mask, P)
                if name == "b":
                    pad = P - prompts[1]
                    u = f"{variant}/b1u"
                    res[u + "/ids"], res[u + "/mask"] = ids[1:, pad:], mask[1:, pad:]
                    res[u + "/prompt"] = np.array(prompts[1])
                    res[u + "/logits"] = drive(model, ids[1:, pad:], mask[1:, pad:], prompts[1])
    np.savez_compressed(OUT, **res)
    print(OUT, os.path.getsize(OUT), sorted(res))


if __name__ == "__main__":
    main()
