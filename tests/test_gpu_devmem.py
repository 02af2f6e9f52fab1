"""Workspaces that grow and are reused at a smaller size change no result (csrc/runtime/devmem.h: DevBuf, RopeTable).

Each engine runs small, large, small on one instance; every output must equal, bit for bit, the output of a fresh
engine that only ever saw that size.  The launches are identical (the project asserts run-to-run identity elsewhere), so
any difference comes from what this sequence exercises: a buffer regrown while holding live content, the RoPE table
kept as a longer prefix for the shorter request, and the zero-fill of regrown padding."""
import tempfile

import numpy as np
import pytest

import lm_cases as lc

pytestmark = pytest.mark.gpu
DEV = "cuda"


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


def sequence_equals_fresh(make, run, sizes):
    """run(engine, size) on one engine over `sizes`, against a fresh engine per distinct size."""
    fresh = {}
    for size in sorted(set(sizes)):
        br = make()
        try:
            fresh[size] = run(br, size)
        finally:
            br.close()
    br = make()
    try:
        got = [run(br, size) for size in sizes]
    finally:
        br.close()
    for size, out in zip(sizes, got):
        for a, b in zip(out, fresh[size]):
            assert np.isfinite(np.asarray(a, np.float64)).all()
            np.testing.assert_array_equal(bits(a), bits(b), err_msg=f"size {size} of {sizes}")


def test_dit_forward_grows_and_shrinks(tiny_ckpt):
    """T = 50, 114, 50 on the 2-layer checkpoint: Np = 25 and 57, both odd, on two sides of a 32-row tile edge."""
    from acestep_mi355x.capi import GGMLCAPIBridge
    L = 8

    def make():
        br = GGMLCAPIBridge()
        br.load_dit(tiny_ckpt)
        return br

    def run(br, T):
        rng = np.random.default_rng(T)
        h = rng.standard_normal((T, 64)).astype(np.float32)
        c = rng.standard_normal((T, 128)).astype(np.float32)
        e = rng.standard_normal((L, 256)).astype(np.float32)
        mask = np.ones(T, np.int32)
        mask[T - 5:] = 0
        emask = np.ones(L, np.int32)
        emask[6:] = 0
        return (br.dit_forward_tfirst(h, c, e, mask, emask, 0.7, 0.4),)

    sequence_equals_fresh(make, run, [50, 114, 50])


def test_text_encoder_grows_and_shrinks():
    from acestep_mi355x.capi import GGMLCAPIBridge
    from acestep_mi355x.synthetic import TEXT_TINY_CONFIG, text_tensor_specs, write_checkpoint
    d = tempfile.mkdtemp(prefix="acemi_dm_text_")
    write_checkpoint(d, TEXT_TINY_CONFIG, seed=6, dtype="BF16", specs=text_tensor_specs(TEXT_TINY_CONFIG))

    def make():
        br = GGMLCAPIBridge()
        br.load_text_encoder(d)
        return br

    def run(br, n):
        ids = np.random.default_rng(n).integers(0, 1000, n).astype(np.int32)
        return (br.text_encoder_forward(ids),)

    sequence_equals_fresh(make, run, [8, 40, 8])


def test_lm_capacity_grows_and_shrinks():
    """begin at capacity 64, 256, 64: an 8-token prefill and four greedy decode steps at each; the tokens and the last
    step's logits."""
    import torch
    from acestep_mi355x.capi import GGMLCAPIBridge
    ckpt = lc.checkpoint("tied")
    B, prompt, steps = 2, 8, 4

    def make():
        br = GGMLCAPIBridge()
        br.load_lm(ckpt)
        return br

    def run(br, capacity):
        ids = torch.from_numpy(np.random.default_rng(3).integers(0, 1000, (B, prompt)).astype(np.int32)).to(DEV)
        br.lm_begin(B, capacity)
        logits = br.lm_forward(ids, torch.ones_like(ids))
        tokens = []
        for _ in range(steps):
            nxt = logits.argmax(dim=-1).to(torch.int32).reshape(B, 1)
            tokens.append(nxt)
            logits = br.lm_forward(nxt)
        return torch.cat(tokens, dim=1).cpu().numpy(), logits.cpu().numpy()

    sequence_equals_fresh(make, run, [64, 256, 64])


def test_vae_decode_grows_and_shrinks():
    from acestep_mi355x.capi import GGMLCAPIBridge
    from acestep_mi355x.synthetic import VAE_TINY_CONFIG, write_vae_checkpoint
    d = tempfile.mkdtemp(prefix="acemi_dm_vae_")
    write_vae_checkpoint(d, VAE_TINY_CONFIG, seed=0)

    def make():
        br = GGMLCAPIBridge()
        br.load_vae(d)
        return br

    def run(br, frames):
        lat = np.random.default_rng(frames).standard_normal((frames, 64)).astype(np.float32)
        return (br.vae_decode_tfirst(lat)[:br.vae_out_len(frames)],)

    sequence_equals_fresh(make, run, [4, 12, 4])
