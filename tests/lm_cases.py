"""Shared by tests/test_gpu_lm.py (the product library on the GPU) and tests/test_lm_cpu.py (the host emulation): drive a
bridge's LM through the cases of tests/golden/lm_qwen3.npz and measure it against the fixture.

The bound on rel-L2 over the vocabulary, per call and row, is the larger of
  * 1.5 x the distance of oracle/text_oracle.py's BF16-arithmetic restatement from the float64 model on the same
    tokens -- the bound tests/test_gpu_text_encoder.py applies to this model family against its transformers fixture
    (taken for rows without padding: the restatement has no left-padding mode; padded rows get the second number only,
    which is never the wider choice), and
  * 1.5 x the error the engine's full-sequence path makes on the same tokens against the same fixture: one prefill over
    prompt + generated tokens per call, last position's logits (the 1.5 x floor convention of tests/test_gpu_forward.py)."""
import hashlib
import os
import tempfile

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED = 7
_CACHE = {}


def fixture():
    if "z" not in _CACHE:
        _CACHE["z"] = np.load(os.path.join(GOLDEN, "lm_qwen3.npz"))
    return _CACHE["z"]


def checkpoint(variant: str, **kw) -> str:
    from acestep_mi355x.synthetic import write_lm_checkpoint
    key = (variant, tuple(sorted(kw.items())))
    if key not in _CACHE:
        d = tempfile.mkdtemp(prefix=f"acemi_lm_{variant}_")
        write_lm_checkpoint(d, seed=SEED, tied=variant == "tied", **kw)
        _CACHE[key] = d
    return _CACHE[key]


def sha256(d: str) -> str:
    with open(os.path.join(d, "model.safetensors"), "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def rel_l2(got, ref):
    """[.., vocab] -> rel-L2 over the vocabulary"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.linalg.norm(got - ref, axis=-1) / np.linalg.norm(ref, axis=-1)


def drive(bridge, ids, mask, prompt, device, capacity=None):
    """The reference loop's calls: lm_begin, prefill (n == 1 for a one-token prompt), then one token per call.
    Returns logits [calls][B][vocab]."""
    import torch
    t_ids = torch.from_numpy(np.ascontiguousarray(ids)).to(device)
    t_mask = torch.from_numpy(np.ascontiguousarray(mask)).to(device)
    bridge.lm_begin(ids.shape[0], capacity or ids.shape[1])
    out = [bridge.lm_forward(t_ids[:, :prompt], t_mask[:, :prompt])]
    for i in range(prompt, ids.shape[1]):
        out.append(bridge.lm_forward(t_ids[:, i:i + 1], t_mask[:, i:i + 1]))
    return torch.stack(out).cpu().numpy()


def full_sequence(bridge, ids, mask, prompt, device):
    """The engine's existing full-sequence path on the same tokens: for each call, one prefill over every token up to
    it; the last position's logits."""
    import torch
    t_ids = torch.from_numpy(np.ascontiguousarray(ids)).to(device)
    t_mask = torch.from_numpy(np.ascontiguousarray(mask)).to(device)
    out = []
    for L in range(prompt, ids.shape[1] + 1):
        bridge.lm_begin(ids.shape[0], ids.shape[1])
        if L == 1:  # n == 1 is the decode step by definition; the full-sequence path of one token is a 2-row prefill
            out.append(None)
            continue
        out.append(bridge.lm_forward(t_ids[:, :L], t_mask[:, :L]))
    ref = next(o for o in out if o is not None)
    return torch.stack([o if o is not None else torch.full_like(ref, float("nan")) for o in out]).cpu().numpy()


def oracle_logits(variant: str, ids_row, prompt):
    """oracle/text_oracle.py's BF16-arithmetic restatement on one unpadded row: logits at the position of every call."""
    from oracle import text_oracle as to
    from oracle.dit_oracle import read_safetensors
    d = checkpoint(variant, model_prefix=False)
    key = ("W", variant)
    if key not in _CACHE:
        st = read_safetensors(os.path.join(d, "model.safetensors"))
        head = st["lm_head.weight" if variant == "untied" else "embed_tokens.weight"][2].astype(np.float64)
        _CACHE[key] = (to.TextWeights(d), head)
    W, head = _CACHE[key]
    hidden = to.forward_text_encoder_layers(W, np.asarray(ids_row, np.int32))
    from acestep_mi355x.synthetic import _bf16_bits
    hb = (_bf16_bits(hidden[prompt - 1:]).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return hb @ head.T


def measure(bridge, variant: str, case: str, device, label: str):
    """Runs `case`; returns (got, err, bound) with err / bound [calls][B]; prints every figure."""
    z = fixture()
    key = f"{variant}/{case}"
    ids, mask, prompt, ref = z[key + "/ids"], z[key + "/mask"], int(z[key + "/prompt"]), z[key + "/logits"]
    got = drive(bridge, ids, mask, prompt, device)
    err = rel_l2(got, ref)
    full = rel_l2(full_sequence(bridge, ids, mask, prompt, device), ref)
    bound = 1.5 * full
    ora = np.full_like(err, np.nan)
    for b in range(ids.shape[0]):
        if mask[b].all():
            ora[:, b] = rel_l2(oracle_logits(variant, ids[b], prompt), ref[:, b])
    bound = np.fmax(bound, 1.5 * ora)   # fmax: the number that exists when the other is NaN
    for i in range(err.shape[0]):
        print(f"{label} {key} call {i}: rel_l2 step path {np.array2string(err[i], precision=3)} full-sequence path "
              f"{np.array2string(full[i], precision=3)} oracle {np.array2string(ora[i], precision=3)} "
              f"bound {np.array2string(bound[i], precision=3)}")
    print(f"{label} {key}: max rel_l2 {err.max():.3e}, max err/bound {np.nanmax(err / bound):.3f}")
    return got, err, bound
