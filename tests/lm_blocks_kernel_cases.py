"""Shared by tests/test_gpu_lm_blocks_kernels.py (kernels/lm_decode_blocks.hip through the self-test library) and
tests/test_lm_blocks_kernels_cpu.py (the plain C++ restatement, kernels/lm_decode_blocks_host.h, through the LM host
library): the decode step's skinny product and embedding gather on raw ggml blocks of all eleven block types.

Blocks: ggml_blocks_np.quantize on N(0, 0.02) rows for the five types it encodes (Q4_0, Q4_1, Q5_0, Q5_1, IQ4_NL);
it has no encoder for Q8_0 and the K-quants, which get acestep_mi355x.synthetic.random_blocks (every code byte random,
finite fp16 fields).  The weight the product multiplies is rne_bf16 of ggml_blocks_np.dequant; references are float64.
Bound (lm_q_kernel_cases.check_random's rule): |got - ref| <= c 2^-24 sum_k |x_k w_k|, c = the longest f32 addition
chain + 2: the kernel's lm_skinny_blocks_chain (13 at K <= 256, else 8 ceil(K / 512) + 6), K for the restatement."""
import numpy as np
import pytest

import ggml_blocks_np as gb
import lm_kernel_cases as lk
from lm_kernel_cases import RESID, STORE, SWIGLU, U, Y_PAD

TYPES = tuple(gb.BLOCK)
KS = (256, 512, 2560)       # one K-quant block in the two-units-per-wave mapping; one trip of 64 lanes; a partial 2nd trip
KERNEL = dict(name="kernel", chain=lambda K: 13 if K <= 256 else 8 * (-(-K // 512)) + 6)
EMULATION = dict(name="emulation", chain=lambda K: K)
_ENCODED = ("q4_0", "q4_1", "q5_0", "q5_1", "iq4_nl")


def blocks_of(qtype, rows, K, rng):
    from acestep_mi355x.synthetic import random_blocks
    if qtype in _ENCODED:
        return gb.quantize(rng.standard_normal((rows, K)).astype(np.float32) * np.float32(0.02), qtype)
    return random_blocks(qtype.upper(), rows, K, rng)


def guarded(blocks, qtype):
    """one block row before and one after whose fp16 fields are NaN: every value of them decodes to NaN"""
    from acestep_mi355x.synthetic import GGML_BLOCKS
    nan = np.full((1,) + blocks.shape[1:], 0x11, np.uint8)
    for off in GGML_BLOCKS[qtype.upper()][2]:
        nan[..., off:off + 2] = np.array([0x7E00], "<u2").view(np.uint8)
    assert np.isnan(gb.dequant(nan, qtype)).all()
    return np.concatenate([nan, blocks, nan], axis=0)


def weights(blocks, qtype):
    return lk.bf16_bits_to_f32(gb.bf16_bits(gb.dequant(blocks, qtype))).astype(np.float64)


def seg(blocks, qtype, **place):
    return dict(qtype=qtype, blocks=guarded(blocks, qtype), **place)


def _x(rng, B, K):
    xb = lk.bits(rng.standard_normal((B, K)), 0)
    return lk._padded_x(xb, 0), lk.vals(xb, 0)


def check_product(run, segs, wv, x, xv, epi, c, rng, what):
    """STORE / RESID of x [B] against the fused float64 weights wv [N][K]; runs twice: identical bits."""
    B, N = x.shape[0], wv.shape[0]
    dot, mag = xv @ wv.T, np.abs(xv) @ np.abs(wv).T
    y0 = lk._f32_sentinel((B, N + Y_PAD))
    if epi == RESID:
        y0[:, :N] = (rng.uniform(-1, 1, (B, N)) * mag.min()).astype(np.float32)
    got = run(x, segs, y0, epi=epi, n_rows=N, guard_rows=1)
    assert lk._same_bits(got, run(x, segs, y0, epi=epi, n_rows=N, guard_rows=1)).all(), what
    assert lk._same_bits(got[:, N:], y0[:, N:]).all(), what
    ref = dot + (y0[:, :N].astype(np.float64) if epi == RESID else 0.0)
    err, bound = np.abs(got[:, :N].astype(np.float64) - ref), c * U * mag
    print(f"lm_skinny_blocks {what}: c {c}, worst err/bound {float(np.max(err / bound)):.3f}")
    assert np.all(err <= bound), (what, float(np.max(err / bound)))


def check_swiglu(run, gtype, utype, K, I, c, what):
    """gate rows of gtype, up rows of utype in the group 16 / step 2 placement, B = 1..8 (lm_kernel_cases._check_swiglu:
    the f32 bounds of both products through silu(g) u plus half an ulp of the bf16 output)"""
    rng = np.random.default_rng(7000 + K + TYPES.index(gtype) + 20 * TYPES.index(utype))
    g, u = blocks_of(gtype, I, K, rng), blocks_of(utype, I, K, rng)
    segs = [seg(g, gtype, row0=0, step=2, group=16), seg(u, utype, row0=16, step=2, group=16)]
    x, xv = _x(rng, 8, K)
    gw, uw = weights(g, gtype), weights(u, utype)
    eg, eu = c * U * (np.abs(xv) @ np.abs(gw).T), c * U * (np.abs(xv) @ np.abs(uw).T)
    run1 = lambda xx, ww, y0, epi, act_type: run(xx, segs, y0, epi=epi, n_rows=2 * I, guard_rows=1)     # noqa: E731
    worst = lk._check_swiglu(run1, 0, x, None, xv @ gw.T, xv @ uw.T, eg, eu, what)
    print(f"lm_skinny_blocks {what}: c {c}, worst err/bound {worst:.3f}")
    y0 = np.zeros((8, I), np.uint16)
    assert np.array_equal(run1(x, None, y0, SWIGLU, 0), run1(x, None, y0, SWIGLU, 0)), what


def check_onehot(run, qtype, K):
    """x[b] = e_k for k at both ends of the row and on either side of a block (K = 2560: trip) boundary: STORE returns
    the bf16 image value exactly (a -0 weight gives +0: the sum starts at +0)."""
    rng = np.random.default_rng(900 + K + TYPES.index(qtype))
    bv = gb.BLOCK[qtype][0]
    ks = (0, bv - 1, bv, K - 1) if K <= 512 else (0, 2047, 2048, K - 1)
    blocks = blocks_of(qtype, 5, K, rng)
    xv = np.zeros((4, K), np.float32)
    xv[np.arange(4), ks] = 1.0
    y0 = lk._f32_sentinel((4, 5 + Y_PAD))
    want = y0.copy()
    want[:, :5] = weights(blocks, qtype)[:, ks].T.astype(np.float32) + np.float32(0.0)
    got = run(lk._padded_x(lk.bits(xv, 0), 0), [seg(blocks, qtype)], y0, epi=STORE, n_rows=5, guard_rows=1)
    ok = lk._same_bits(got, want)
    assert ok.all(), (qtype, K, np.argwhere(~ok)[:4].tolist())


def check_embed(run, qtype, H):
    rng = np.random.default_rng(17 + H + TYPES.index(qtype))
    vocab = 11
    blocks = blocks_of(qtype, vocab, H, rng)
    ids = np.array([-1, 0, vocab - 1, vocab, 4, -1000, vocab + 1000, 7], np.int32)
    ok = lk._same_bits(run(blocks, qtype, ids), gb.dequant(blocks, qtype)[np.clip(ids, 0, vocab - 1)])
    assert ok.all(), (qtype, H, np.argwhere(~ok)[:4].tolist())


def runners(lib=None):
    import functools
    import types
    from acestep_mi355x import capi
    return types.SimpleNamespace(skinny=functools.partial(capi.kernel_lm_skinny_blocks, lib=lib),
                                 embed=functools.partial(capi.kernel_lm_embed_blocks, lib=lib))


class LmBlocksKernelChecks:
    """The test functions; a test file subclasses this as Test..., sets IMPL and provides the module fixture `k`."""
    IMPL = None

    @pytest.mark.parametrize("epi", (STORE, RESID))
    @pytest.mark.parametrize("B", (1, 3, 8))
    @pytest.mark.parametrize("K", KS)
    @pytest.mark.parametrize("qtype", TYPES)
    def test_skinny_blocks_random(self, k, qtype, K, B, epi):
        rng = np.random.default_rng(1000 * K + 10 * B + 3 * epi + TYPES.index(qtype))
        blocks = blocks_of(qtype, 5, K, rng)
        x, xv = _x(rng, B, K)
        check_product(k.skinny, [seg(blocks, qtype)], weights(blocks, qtype), x, xv, epi, self.IMPL["chain"](K) + 2, rng,
                      (self.IMPL["name"], qtype, K, B, epi))

    @pytest.mark.parametrize("K", KS)
    @pytest.mark.parametrize("qtype", TYPES)
    def test_skinny_blocks_swiglu(self, k, qtype, K):
        check_swiglu(k.skinny, qtype, qtype, K, 16, self.IMPL["chain"](K) + 2, (self.IMPL["name"], qtype, K, "swiglu"))

    def test_skinny_blocks_swiglu_of_two_types(self, k):
        check_swiglu(k.skinny, "q4_k", "q5_0", 512, 32, self.IMPL["chain"](512) + 2, (self.IMPL["name"], "q4_k|q5_0"))

    def test_skinny_blocks_two_segments(self, k):
        """Q4_K rows 0..2, then Q6_K rows 3..6 of one matrix"""
        rng = np.random.default_rng(41)
        a, b = blocks_of("q4_k", 3, 512, rng), blocks_of("q6_k", 4, 512, rng)
        x, xv = _x(rng, 3, 512)
        check_product(k.skinny, [seg(a, "q4_k", row0=0), seg(b, "q6_k", row0=3)],
                      np.concatenate([weights(a, "q4_k"), weights(b, "q6_k")]), x, xv, STORE, self.IMPL["chain"](512) + 2,
                      rng, (self.IMPL["name"], "q4_k+q6_k"))

    @pytest.mark.parametrize("K", (512, 2560))
    @pytest.mark.parametrize("qtype", TYPES)
    def test_skinny_blocks_onehot(self, k, qtype, K):
        check_onehot(k.skinny, qtype, K)

    @pytest.mark.parametrize("K", KS)
    def test_skinny_blocks_reports_its_chain(self, k, K):
        blocks = blocks_of("q4_0", 1, K, np.random.default_rng(1))
        _, chain = k.skinny(np.zeros((1, K), np.uint16), [dict(qtype="q4_0", blocks=blocks)], np.zeros((1, 1), np.float32),
                            with_chain=True)
        assert chain == self.IMPL["chain"](K)

    @pytest.mark.parametrize("H", (256, 2560))
    @pytest.mark.parametrize("qtype", TYPES)
    def test_embed_blocks(self, k, qtype, H):
        check_embed(k.embed, qtype, H)
