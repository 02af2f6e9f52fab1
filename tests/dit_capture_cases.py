"""Shared by tests/test_gpu_dit_capture.py (the gfx950 library, cuda tensors) and tests/test_dit_capture_cpu.py (the host
library, whose "device" pointers are host pointers): ace_mi_dit_forward_capture and the decoder.forward hook's
output_attentions path on the tiny synthetic checkpoint (2 layers, 4 heads, 2 KV heads).

Reference of the probabilities: oracle.dit_oracle.attention is wrapped (monkeypatch) to record (w, xq, xkv, key_mask) of
the cross-attention calls (rope is None), and the selected heads' softmax(q k^T / sqrt(D) + mask) is recomputed in
float64 with the oracle's own mul_mat, rms_norm and build_key_bias.

Tolerance: the engine rounds activations to bf16 upstream, so its distance to that reference cannot be derived; it is
held against a yardstick taken from the reference alone.  floor = the rel-L2 distance between the float64
probabilities and the same probabilities with the recorded q and k rounded to bf16 before the product (the precision
of the reference's own eager bf16 attention); the engine's rel-L2 per pair must be <= 2 x floor, the 2 x being the
stated allowance for the engine's two extra bf16 roundings (the norm output and the projection input)."""
import math
import types

import numpy as np
import pytest

SEQ = (10, 33)        # Np = 5 and 17; 33 is odd against the patch size
ENC = (7, 70)         # inside one 64-key tile; a second, ragged tile
B = 2
ALL_PAIRS = [(l, h) for l in range(2) for h in range(4)]
INVALID_ARG = 2


def bf16(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def inputs(T, L, seed=5):
    rng = np.random.default_rng(seed * 1000 + T * 10 + L)
    h = rng.standard_normal((B, T, 64)).astype(np.float32)
    c = rng.standard_normal((B, T, 128)).astype(np.float32)
    e = rng.standard_normal((B, L, 256)).astype(np.float32)
    em = np.ones((B, L), np.int32)
    em[0, L - 2:] = 0          # different encoder masks per item
    em[1, L // 2] = 0
    t = np.array([0.8, 0.35], np.float32)
    r = np.array([0.8, 0.1], np.float32)
    return h, c, e, em, t, r


def oracle_probs(monkeypatch, ckpt, T, L, pairs):
    """(ref, floor_ref): float64 [n_pairs][B][Np][L] probabilities of the oracle's cross-attention, and the same with q
    and k rounded to bf16 before the product"""
    from oracle import dit_oracle as do
    h, c, e, em, t, r = inputs(T, L)
    W = do.DitWeights(ckpt)
    cfg = W.cfg
    D, rep = cfg.head_dim, cfg.num_attention_heads // cfg.num_key_value_heads
    Np = (T + cfg.patch_size - 1) // cfg.patch_size
    ref = np.zeros((len(pairs), B, Np, L))
    low = np.zeros_like(ref)
    orig = do.attention
    for b in range(B):
        rec = []

        def spy(cfg_, w, xq, xkv, key_mask, sliding, window, rope, causal=False):
            if rope is None:
                rec.append((w, np.array(xq), np.array(xkv), key_mask))
            return orig(cfg_, w, xq, xkv, key_mask, sliding, window, rope, causal)

        with monkeypatch.context() as mp:
            mp.setattr(do, "attention", spy)
            do.forward_dit(W, h[b], c[b], e[b], None, em[b], T, L, float(t[b]), float(r[b]))
        assert len(rec) == cfg.num_hidden_layers
        for j, (layer, head) in enumerate(pairs):
            w, xq, xkv, key_mask = rec[layer]
            q = do.rms_norm(do.mul_mat(w["q"], xq).reshape(Np, -1, D), w["q_norm"], cfg.rms_norm_eps)[:, head]
            k = do.rms_norm(do.mul_mat(w["k"], xkv).reshape(L, -1, D), w["k_norm"], cfg.rms_norm_eps)[:, head // rep]
            bias = do.build_key_bias(Np, L, key_mask, False, 0)
            for dst, qq, kk in ((ref, q.astype(np.float64), k.astype(np.float64)), (low, bf16(q), bf16(k))):
                s = (qq @ kk.T) / math.sqrt(D) + (0.0 if bias is None else bias.astype(np.float64))
                ex = np.exp(s - s.max(axis=1, keepdims=True))
                dst[j, b] = ex / ex.sum(axis=1, keepdims=True)
    return ref, low


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


class HostMem:
    """arrays the host library reads through "device" pointers"""

    def dev(self, a):
        return None if a is None else np.ascontiguousarray(a)

    def empty(self, shape):
        return np.full(shape, np.nan, np.float32)

    def ptr(self, a):
        return 0 if a is None else a.ctypes.data

    def host(self, a):
        return np.array(a)

    def sync(self):
        pass


class CudaMem:
    def dev(self, a):
        import torch
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def empty(self, shape):
        import torch
        return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")

    def ptr(self, a):
        return 0 if a is None else a.data_ptr()

    def host(self, a):
        import torch
        torch.cuda.synchronize()
        return a.cpu().numpy()

    def sync(self):  # torch's fills run on its own stream, the library on the context's
        import torch
        torch.cuda.synchronize()


def run_capture(br, mem, T, L, pairs, early_exit, with_out=True):
    h, c, e, em, t, r = inputs(T, L)
    Np = (T + 1) // 2
    d = [mem.dev(a) for a in (h, c, e, em, t, r)]
    out = mem.empty((B, T, 64)) if with_out else None
    probs = mem.empty((len(pairs), B, Np, L))
    mem.sync()
    br.dit_forward_capture_device(B, T, L, mem.ptr(d[0]), mem.ptr(d[1]), mem.ptr(d[2]), 0, mem.ptr(d[3]), mem.ptr(d[4]),
                                  mem.ptr(d[5]), pairs, early_exit, mem.ptr(out), mem.ptr(probs))
    br.synchronize()
    return (mem.host(out) if with_out else None), mem.host(probs)


def run_forward(br, mem, T, L):
    h, c, e, em, t, r = inputs(T, L)
    d = [mem.dev(a) for a in (h, c, e, em, t, r)]
    out = mem.empty((B, T, 64))
    mem.sync()
    br.dit_forward_batched_device(B, T, L, mem.ptr(d[0]), mem.ptr(d[1]), mem.ptr(d[2]), 0, mem.ptr(d[3]), mem.ptr(d[4]),
                                  mem.ptr(d[5]), mem.ptr(out))
    br.synchronize()
    return mem.host(out)


def same_bits(a, b):
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) == np.ascontiguousarray(b, np.float32).view(np.uint32)).all()


def make_handler():
    dec = types.SimpleNamespace()
    dec.forward = lambda **kw: ("original", kw)
    return types.SimpleNamespace(model=types.SimpleNamespace(decoder=dec))


class DitCaptureChecks:
    """fixtures of the subclass' module: env = (bridge with the tiny checkpoint loaded, mem, torch device name),
    tiny_ckpt"""

    @pytest.mark.parametrize("T", SEQ)
    @pytest.mark.parametrize("L", ENC)
    def test_probs_within_twice_the_reference_floor_and_out_unchanged(self, env, tiny_ckpt, monkeypatch, T, L):
        br, mem, _ = env
        before = run_forward(br, mem, T, L)
        out, probs = run_capture(br, mem, T, L, ALL_PAIRS, False)
        assert same_bits(out, before), "early_exit = 0: out differs from ace_mi_dit_forward_batched"
        assert same_bits(run_forward(br, mem, T, L), before), "a forward after the capture call differs"
        ref, low = oracle_probs(monkeypatch, tiny_ckpt, T, L, ALL_PAIRS)
        _, _, _, em, _, _ = inputs(T, L)
        assert (probs.transpose(0, 2, 1, 3)[:, :, em == 0] == 0).all(), "a masked encoder token is not exactly 0"
        np.testing.assert_allclose(probs.sum(axis=-1), 1.0, atol=1e-5)
        worst = 0.0
        for j, pair in enumerate(ALL_PAIRS):
            err, floor = rel_l2(probs[j], ref[j]), rel_l2(low[j], ref[j])
            print(f"dit capture T={T} L={L} pair {pair}: rel-L2 {err:.3e}, floor {floor:.3e}, ratio {err / floor:.3f}")
            worst = max(worst, err / floor)
        print(f"dit capture T={T} L={L}: worst ratio {worst:.3f}")
        assert worst <= 2.0, worst

    @pytest.mark.parametrize("T,L", [(33, 70), (10, 7)])
    def test_early_exit_order_and_duplicates(self, env, T, L):
        br, mem, _ = env
        _, full = run_capture(br, mem, T, L, ALL_PAIRS, False)
        # pairs on layer 0 only, early exit, no output buffer
        pairs = [(0, 2), (0, 1)]
        out, probs = run_capture(br, mem, T, L, pairs, True, with_out=False)
        for j, p in enumerate(pairs):
            assert same_bits(probs[j], full[ALL_PAIRS.index(p)]), p
        # both layers, out of order, one duplicate: the caller's order; early exit leaves `out` alone
        pairs = [(1, 3), (0, 1), (1, 0), (0, 1)]
        for early in (False, True):
            out, probs = run_capture(br, mem, T, L, pairs, early)
            for j, p in enumerate(pairs):
                assert same_bits(probs[j], full[ALL_PAIRS.index(p)]), (early, p)
            assert np.isnan(out).all() == early

    def test_invalid_arguments(self, env):
        br, mem, _ = env
        T, L = 10, 7
        h, c, e, em, t, r = inputs(T, L)
        d = [mem.dev(a) for a in (h, c, e, em, t, r)]
        out, probs = mem.empty((B, T, 64)), mem.empty((4, B, 5, L))
        mem.sync()

        def call(pairs, enc_len=L, p_probs=None, p_out=None, early=False):
            layers = np.array([p[0] for p in pairs], np.int32)
            heads = np.array([p[1] for p in pairs], np.int32)
            import ctypes
            ip = ctypes.POINTER(ctypes.c_int32)
            st = br.lib.ace_mi_dit_forward_capture(
                br.ctx, B, T, enc_len, mem.ptr(d[0]), mem.ptr(d[1]), mem.ptr(d[2]), None, mem.ptr(d[3]), mem.ptr(d[4]),
                mem.ptr(d[5]), len(pairs), layers.ctypes.data_as(ip), heads.ctypes.data_as(ip), 1 if early else 0,
                (mem.ptr(out) if p_out is None else p_out) or None,
                (mem.ptr(probs) if p_probs is None else p_probs) or None, None)
            return st, br._last_error()

        for kw, word in ((dict(pairs=[]), "n_pairs = 0"), (dict(pairs=[(2, 0)]), "layer 2"),
                         (dict(pairs=[(-1, 0)]), "layer -1"), (dict(pairs=[(0, 4)]), "head 4"),
                         (dict(pairs=[(1, -1)]), "head -1"), (dict(pairs=[(0, 0)], enc_len=0), "enc_len = 0"),
                         (dict(pairs=[(0, 0)], enc_len=-3), "enc_len = -3"),
                         (dict(pairs=[(0, 0)], p_probs=0), "probs is null"),
                         (dict(pairs=[(0, 0)], p_out=0), "out is null")):
            st, msg = call(**kw)
            assert st == INVALID_ARG and word in msg, (kw, st, msg)
        st, msg = call(pairs=[(0, 0)], p_out=0, early=True)   # out = NULL is accepted with early_exit
        assert st == 0, msg
        br.synchronize()

    def test_quantized_activation_walk_captures_too(self, tiny_ckpt, monkeypatch, env):
        """ACE_MI_QUANT_ACT=q8 (the parity walk) supports capture: the same launch on its own operand planes"""
        _, mem, _ = env
        monkeypatch.setenv("ACE_GGML_DIT_WEIGHT_QTYPE", "q8_0")
        monkeypatch.setenv("ACE_MI_QUANT_ACT", "q8")
        br = self.bridge()
        br.load_dit(tiny_ckpt)
        T, L = 33, 70
        out, probs = run_capture(br, mem, T, L, ALL_PAIRS, False)
        assert same_bits(out, run_forward(br, mem, T, L))
        _, early = run_capture(br, mem, T, L, [(0, 3)], True, with_out=False)
        assert same_bits(early[0], probs[3])
        _, _, _, em, _, _ = inputs(T, L)
        assert (probs.transpose(0, 2, 1, 3)[:, :, em == 0] == 0).all() and np.isfinite(probs).all()
        np.testing.assert_allclose(probs.sum(axis=-1), 1.0, atol=1e-5)
        br.close()

    # ---- the decoder.forward hook
    def hook_call(self, env, bsz, cfg, early=True, T=33, L=70):
        import torch
        from acestep_mi355x import hook
        br, _, dev = env
        g = torch.Generator().manual_seed(bsz)
        hs = torch.randn(bsz, T, 64, generator=g).to(torch.bfloat16).to(dev)
        ctx = torch.randn(bsz, T, 128, generator=g).to(dev)
        enc = torch.randn(bsz, L, 256, generator=g).to(dev)
        eam = torch.ones(bsz, L, dtype=torch.long)
        eam[0, L - 3:] = 0
        t = torch.linspace(0.9, 0.2, bsz)
        h = make_handler()
        hook.install_dit_backend(h, br)
        out = h.model.decoder.forward(hidden_states=hs, timestep=t.to(dev), timestep_r=t.to(dev), attention_mask=None,
                                      encoder_hidden_states=enc, encoder_attention_mask=eam.to(dev),
                                      context_latents=ctx, past_key_values="pkv", output_attentions=True,
                                      custom_layers_config=cfg, enable_early_exit=early)
        return h, out, (hs, ctx, enc, eam, t)

    @pytest.mark.parametrize("bsz", [1, 2])
    def test_hook_returns_the_tuple_the_handler_reads(self, env, bsz):
        import torch
        br, mem, dev = env
        cfg = {0: [1], 1: [0, 3]}
        T, L, Np = 33, 70, 17
        h, (pred, pkv, attn), (hs, ctx, enc, eam, t) = self.hook_call(env, bsz, cfg)
        assert pkv == "pkv" and pred.shape == hs.shape and pred.dtype == hs.dtype and not pred.any()
        assert isinstance(attn, tuple) and len(attn) == 2 and all(a is not None for a in attn)
        for a in attn:
            assert a.shape == (bsz, 4, Np, L) and a.dtype == hs.dtype and a.device == hs.device
        assert not attn[0][:, [0, 2, 3]].any() and not attn[1][:, [1, 2]].any()
        # the engine's maps of the same inputs, straight from the capture entry
        pairs = [(0, 1), (1, 0), (1, 3)]
        d = [mem.dev(a) for a in (hs.float().cpu().numpy(), ctx.cpu().numpy(), enc.cpu().numpy(),
                                  eam.numpy().astype(np.int32), t.numpy(), t.numpy())]
        probs = mem.empty((3, bsz, Np, L))
        mem.sync()
        br.dit_forward_capture_device(bsz, T, L, mem.ptr(d[0]), mem.ptr(d[1]), mem.ptr(d[2]), 0, mem.ptr(d[3]),
                                      mem.ptr(d[4]), mem.ptr(d[5]), pairs, True, 0, mem.ptr(probs))
        br.synchronize()
        maps = torch.from_numpy(mem.host(probs)).to(hs.dtype)
        # the handler's own lines (acestep/handler.py get_lyric_timestamp): drop None, [:bsz], transpose, stack, squeeze
        filtered = [a for a in attn if a is not None]
        stacked = torch.stack([a[:bsz].transpose(-1, -2) for a in filtered])
        if bsz == 1:
            stacked = stacked.squeeze(1)
        for j, (layer_idx, head_idx) in enumerate(pairs):
            m = stacked[layer_idx, head_idx] if bsz == 1 else stacked[layer_idx, :, head_idx]
            want = maps[j].transpose(-1, -2)
            assert torch.equal(m.cpu(), want[0] if bsz == 1 else want), (layer_idx, head_idx)

    def test_hook_unselected_layer_is_a_stride_0_view(self, env):
        _, (pred, pkv, attn), _ = self.hook_call(env, 1, {1: [2]}, early=False)
        assert len(attn) == 2 and attn[0].stride() == (0, 0, 0, 0) and not attn[0].any()
        assert attn[1][:, 2].any() and pred.any()      # no early exit: the velocity is returned too

    def test_hook_chunks_a_batch_larger_than_one_call(self, env):
        from acestep_mi355x import hook
        bsz = hook.MAX_BATCH_PER_CALL + 1
        _, (pred, pkv, attn), _ = self.hook_call(env, bsz, {0: [1]}, T=10, L=7)
        _, (_, _, last), _ = self.hook_call(env, bsz, {0: [1]}, T=10, L=7)
        assert attn[0].shape == (bsz, 4, 5, 7)
        s = attn[0][:, 1].float().sum(dim=-1)
        assert (s - 1).abs().max() < 2e-2 and (attn[0][-1] == last[0][-1]).all()   # (bf16 maps) the second call's item

    def test_hook_without_a_config_keeps_todays_result(self, env):
        for cfg in (None, {}):
            _, out, _ = self.hook_call(env, 2, cfg, T=10, L=7)
            assert len(out) == 3 and out[2] is None and out[1] == "pkv"
