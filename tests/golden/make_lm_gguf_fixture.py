"""Generates tests/golden/lm_qwen3_gguf.npz: the reference-side pin of the causal LM on GGUF checkpoints.

For each variant of acestep_mi355x.synthetic.LM_GGUF_VARIANTS (write_lm_gguf, seed 7): transformers' Qwen3ForCausalLM
in float64 whose weights are the exact f32 dequant of the GGUF's blocks (tests/ggml_blocks_np.py, ggml's CPU
dequantize_row_*; F32 norms as stored), driven like tests/golden/make_lm_fixture.py drives the 16-bit model, on the ids
and masks of that fixture's cases a, b and, for `mixed`, e.  The fixture holds the
sha256 of each GGUF and the last-position logits of every call; the ids and masks stay in lm_qwen3.npz (its `tied/...`
keys: the tokens do not depend on the variant).

Logits are stored as float32 with the low 9 mantissa bits cleared after rounding (a relative step of 2^-15, error
<= 2^-16 = 1.5e-5 per element, a hundred times below the bf16-arithmetic errors the tests bound): that is what keeps
the compressed file below lm_qwen3.npz's size.

Run from the repo root: python tests/golden/make_lm_gguf_fixture.py"""
import hashlib
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ace-step-1.5-ggml_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import ggml_blocks_np as gb  # noqa: E402
from acestep_mi355x.synthetic import GGML_TYPES, LM_GGUF_VARIANTS, TEXT_TINY_CONFIG, write_lm_gguf  # noqa: E402
from make_lm_fixture import drive  # noqa: E402
from lm_gguf_cases import read_gguf_dir  # noqa: E402

SEED = 7
OUT = os.path.join(HERE, "lm_qwen3_gguf.npz")
CASES = {"q8_0": ("a", "b"), "q4_k": ("a", "b"), "q6_k": ("a", "b"), "mixed": ("a", "b", "e")}
_NAMES = {v: k for k, v in GGML_TYPES.items()}


def gguf_values(path):
    """name -> float64 array (numpy shape) of the f32 values ggml reads from the file"""
    out = {}
    for name, (gt, shape, raw) in read_gguf_dir(path).items():
        t = _NAMES[gt]
        if t == "F32":
            v = np.frombuffer(raw, "<f4").astype(np.float32)
        elif t == "F16":
            v = np.frombuffer(raw, "<f2").astype(np.float32)
        elif t == "BF16":
            v = (np.frombuffer(raw, "<u2").astype(np.uint32) << 16).view(np.float32)
        else:
            bv, bb = gb.BLOCK[t.lower()]
            v = gb.dequant(np.frombuffer(raw, np.uint8).reshape(-1, shape[-1] // bv, bb), t.lower())
        out[name] = v.reshape(shape).astype(np.float64)
    return out


def hf_model(values, tied):
    from transformers import Qwen3Config, Qwen3ForCausalLM
    c = TEXT_TINY_CONFIG
    cfg = Qwen3Config(vocab_size=c["vocab_size"], hidden_size=c["hidden_size"], intermediate_size=c["intermediate_size"],
                      num_hidden_layers=c["num_hidden_layers"], num_attention_heads=c["num_attention_heads"],
                      num_key_value_heads=c["num_key_value_heads"], head_dim=c["head_dim"],
                      max_position_embeddings=c["max_position_embeddings"], rms_norm_eps=c["rms_norm_eps"],
                      rope_theta=c["rope_theta"], attention_bias=False, tie_word_embeddings=tied)
    cfg._attn_implementation = "eager"
    model = Qwen3ForCausalLM(cfg).double().eval()
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in values.items()}, strict=False)
    assert not unexpected and all("rotary" in m or (tied and m == "lm_head.weight") for m in missing), (missing, unexpected)
    if tied:
        model.tie_weights()
    return model


def trim(x):
    """float32, rounded (to nearest even) to 14 explicit mantissa bits (see the module docstring)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0xFF + ((u >> 9) & 1)) >> 9) << 9).astype(np.uint32).view(np.float32)


def main():
    base = np.load(os.path.join(HERE, "lm_qwen3.npz"))
    res = {"seed": np.array(SEED)}
    for variant, cases in CASES.items():
        spec = LM_GGUF_VARIANTS[variant]
        path = write_lm_gguf(tempfile.mkdtemp(prefix="acemi_lm_gguf_fix_"), spec["types"], tied=spec["tied"], seed=SEED)
        with open(path, "rb") as f:
            res[f"{variant}/sha256"] = np.array(hashlib.sha256(f.read()).hexdigest())
        model = hf_model(gguf_values(path), spec["tied"])
        with torch.no_grad():
            for case in cases:
                ids, mask, prompt = (base[f"tied/{case}/{k}"] for k in ("ids", "mask", "prompt"))
                for other in ("ids", "mask"):
                    assert np.array_equal(base[f"untied/{case}/{other}"], base[f"tied/{case}/{other}"])
                res[f"{variant}/{case}/logits"] = trim(drive(model, ids, mask, int(prompt)))
    np.savez_compressed(OUT, **res)
    print(OUT, os.path.getsize(OUT), "limit", os.path.getsize(os.path.join(HERE, "lm_qwen3.npz")), sorted(res))


if __name__ == "__main__":
    main()
