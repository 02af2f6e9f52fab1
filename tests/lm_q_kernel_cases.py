"""Shared by tests/test_gpu_lm_q_kernels.py (kernels/lm_decode_q.hip through the self-test library) and
tests/test_lm_q_kernels_cpu.py (the plain C++ restatement, kernels/lm_decode_q_host.h, through the LM host library): the
decode step's skinny product and embedding gather on weights in ggml block planes (Q8_0 / Q4_K / Q6_K).

Blocks are built here as ggml block bytes (packers below, proven against tests/ggml_blocks_np.py's dequant by the CPU
file) and handed to the entries, which re-lay them out with quant::to_planes as the loader does.  The weight value the
product multiplies is rne_bf16 of ggml's f32 dequant; references are float64 on those rounded values.

Lane mapping of the kernel (its file header): a lane holds VPL = 16 values per trip (Q8_0, Q6_K) or 32 (Q4_K);
K <= 32 VPL: 32 lanes per row, one trip; larger K: 64 lanes per row, ceil(K / (64 VPL)) trips.  The longest f32 addition
chain behind one output is VPL trips + log2(lanes per row); the restatement sums K terms in order."""
import numpy as np
import pytest

import ggml_blocks_np as gb
import lm_kernel_cases as lk
from lm_kernel_cases import RESID, STORE, SWIGLU, U, X_PAD, Y_PAD

TYPES = ("q8_0", "q4_k", "q6_k")
VPL = {"q8_0": 16, "q4_k": 32, "q6_k": 16}
F16_NAN = 0x7E00


def kernel_chain(qtype, K):
    v = VPL[qtype]
    return v + 5 if K <= 32 * v else v * (-(-K // (64 * v))) + 6


KERNEL = dict(name="kernel", chain=kernel_chain)
EMULATION = dict(name="emulation", chain=lambda qtype, K: K)


# ---------------------------------------------------------------------------------------------- block builders
def _put16(blk, off, v):
    blk[..., off:off + 2] = np.asarray(v, np.float32).astype("<f2").view(np.uint8).reshape(blk.shape[:-1] + (2,))


def pack_q8_0(d, q):
    """d [rows][nb] (fp16-representable), q [rows][nb][32] in -128..127 -> uint8 [rows][nb][34]"""
    blk = np.zeros(q.shape[:2] + (34,), np.uint8)
    _put16(blk, 0, d)
    blk[..., 2:] = q.astype(np.int8).view(np.uint8)
    return blk


def pack_q4_k(d, dmin, sc, mn, q):
    """d, dmin [rows][nb]; sc, mn [rows][nb][8] in 0..63; q [rows][nb][256] in 0..15 -> uint8 [rows][nb][144]
    (block_q4_K: d, dmin, scales[12] as get_scale_min_k4 reads them, qs[128]: sub-block 2g low nibbles, 2g + 1 high)"""
    blk = np.zeros(q.shape[:2] + (144,), np.uint8)
    _put16(blk, 0, d)
    _put16(blk, 2, dmin)
    sc, mn = sc.astype(np.int32), mn.astype(np.int32)
    s = np.zeros(q.shape[:2] + (12,), np.int32)
    for j in range(4):
        s[..., j] = (sc[..., j] & 63) | ((sc[..., j + 4] >> 4) << 6)
        s[..., j + 4] = (mn[..., j] & 63) | ((mn[..., j + 4] >> 4) << 6)
        s[..., j + 8] = (sc[..., j + 4] & 0xF) | ((mn[..., j + 4] & 0xF) << 4)
    blk[..., 4:16] = s.astype(np.uint8)
    v = q.reshape(q.shape[:2] + (4, 2, 32)).astype(np.int32)
    blk[..., 16:] = (v[..., 0, :] | (v[..., 1, :] << 4)).reshape(q.shape[:2] + (128,)).astype(np.uint8)
    return blk


def pack_q6_k(d, sc, q):
    """d [rows][nb]; sc [rows][nb][16] int8; q [rows][nb][256] in -32..31 -> uint8 [rows][nb][210]
    (block_q6_K: ql[128], qh[64], scales[16], d; value 128 n + 32 j + l: low 4 bits in ql[64 n + 32 (j & 1) + l]'s
    nibble j >> 1, high 2 bits in qh[32 n + l] at bit 2 j)"""
    blk = np.zeros(q.shape[:2] + (210,), np.uint8)
    v = (q.astype(np.int32) + 32).reshape(q.shape[:2] + (2, 4, 32))
    lo, hi = v & 0xF, v >> 4
    ql = np.stack([lo[..., 0, :] | (lo[..., 2, :] << 4), lo[..., 1, :] | (lo[..., 3, :] << 4)], axis=-2)
    blk[..., 0:128] = ql.reshape(q.shape[:2] + (128,)).astype(np.uint8)
    qh = hi[..., 0, :] | (hi[..., 1, :] << 2) | (hi[..., 2, :] << 4) | (hi[..., 3, :] << 6)
    blk[..., 128:192] = qh.reshape(q.shape[:2] + (64,)).astype(np.uint8)
    blk[..., 192:208] = sc.astype(np.int8).view(np.uint8)
    _put16(blk, 208, d)
    return blk


def unit_blocks(qtype, wi):
    """Blocks whose dequant is exactly the integers wi [rows][K]: Q8_0 d = 1 (wi in -128..127); Q4_K d = sc = dmin = 1,
    m = 8 (wi in -8..7); Q6_K d = sc = 1 (wi in -32..31)."""
    rows, K = wi.shape
    bv = gb.BLOCK[qtype][0]
    q = wi.reshape(rows, K // bv, bv)
    one = np.ones((rows, K // bv), np.float32)
    if qtype == "q8_0":
        return pack_q8_0(one, q)
    if qtype == "q4_k":
        e = np.ones((rows, K // bv, 8), np.int32)
        return pack_q4_k(one, one, e, 8 * e, q + 8)
    return pack_q6_k(one, np.ones((rows, K // bv, 16), np.int32), q)


UNIT_RANGE = {"q8_0": (-128, 128), "q4_k": (-8, 8), "q6_k": (-32, 32)}
_FIELDS = {"q8_0": (0,), "q4_k": (0, 2), "q6_k": (208,)}
# (scale, min as a multiple of it): the smallest fp16-normal sizes, 0.5 x scale >= 2^-14 (weights of std 0.02 .. 0.2)
_SCALE = {"q8_0": (0.00027, 0.0), "q4_k": (0.00016, 7.5), "q6_k": (0.00016, 0.0)}


def random_blocks(qtype, rows, K, rng):
    """Uniformly random block bytes (every code, every 6-bit scale / min, every int8 scale), the fp16 fields overwritten
    by small normal values (either sign where the type has no min)."""
    bv, bb = gb.BLOCK[qtype]
    nb = K // bv
    blk = rng.integers(0, 256, size=(rows, nb, bb), dtype=np.uint8)
    scale, min_mult = _SCALE[qtype]
    d = (scale * (0.5 + rng.random((rows, nb)))).astype(np.float32)
    if min_mult == 0.0:
        d = d * np.where(rng.random((rows, nb)) < 0.5, -1.0, 1.0).astype(np.float32)
    vals = [d] + ([d * np.float32(min_mult)] if len(_FIELDS[qtype]) > 1 else [])
    for off, v in zip(_FIELDS[qtype], vals):
        h = v.astype("<f2")
        assert np.all(np.isfinite(h.astype(np.float32))) and np.all(np.abs(h.astype(np.float32)) >= 2.0 ** -14)
        _put16(blk, off, h.astype(np.float32))
    return blk


def nan_row(qtype, K):
    """One row of blocks whose fp16 scale fields are NaN: every value of it dequantizes to NaN."""
    bv, bb = gb.BLOCK[qtype]
    blk = np.full((1, K // bv, bb), 0x11, np.uint8)
    for off in _FIELDS[qtype]:
        blk[..., off:off + 2] = np.array([F16_NAN], "<u2").view(np.uint8)
    return blk


def rounded_weights(blocks, qtype):
    """the product's weight values: rne_bf16(ggml dequant), float32"""
    return lk.bf16_bits_to_f32(gb.bf16_bits(gb.dequant(blocks, qtype)))


def with_guard(blocks, qtype):
    K = blocks.shape[1] * gb.BLOCK[qtype][0]
    return np.concatenate([blocks, nan_row(qtype, K)], axis=0)


# ---------------------------------------------------------------------------------------------- the product
# smallest K; both sides of the 32 -> 64 lanes-per-row switch and of every trip boundary up to 2560; idle lanes in the
# last trip (Q8_0 544, 1056, 2080, 2560; Q6_K 1280, 2304, 2560; Q4_K 1280, 2304, 2560)
EXACT_K = {"q8_0": (32, 512, 544, 1024, 1056, 2048, 2080, 2560),
           "q6_k": (256, 512, 768, 1024, 1280, 2048, 2304, 2560),
           "q4_k": (256, 1024, 1280, 2048, 2304, 2560)}
EXACT_N = lk.SKINNY_EXACT_N


def check_exact(run, qtype, K):
    """Unit-scale blocks and x integers in [-8, 8]: every product and partial sum is exact in f32 (|sum| <= 8 * 128 *
    2560 < 2^24), so STORE and RESID equal the integer result bit for bit.  x is NaN past K, y keeps its sentinel past
    N, and the blocks carry one more row, of NaN scales, past N."""
    rng = np.random.default_rng(300 + 2 * K + TYPES.index(qtype))
    xi = rng.integers(-8, 9, (8, K))
    x = lk._padded_x(lk.bits(xi, 0), 0)
    lo, hi = UNIT_RANGE[qtype]
    for N in EXACT_N:
        wi = rng.integers(lo, hi, (N, K))
        blocks = unit_blocks(qtype, wi)
        assert np.array_equal(gb.dequant(blocks, qtype), wi.astype(np.float32))
        w = with_guard(blocks, qtype)
        ref = (xi @ wi.T).astype(np.float32)
        yi = rng.integers(-1000, 1001, (8, N)).astype(np.float32)
        for B in range(1, 9):
            for epi in (STORE, RESID):
                y0 = lk._f32_sentinel((B, N + Y_PAD))
                y0[:, :N] = yi[:B] if epi == RESID else lk._f32_sentinel((B, N), 0x7FC0BEEF)
                want = y0.copy()
                want[:, :N] = ref[:B] + (yi[:B] if epi == RESID else 0)
                got = run(x[:B], w, qtype, y0, epi=epi, n_rows=N)
                ok = lk._same_bits(got, want)
                assert ok.all(), (qtype, K, N, B, epi, np.argwhere(~ok)[:4].tolist())


# (K, first k): every k of one whole super-block (Q8_0: block) that is not the row's first -- at a K of the 32-lane
# mapping and at one of the 64-lane mapping (there the last block of a row whose last trip leaves lanes idle)
ONEHOT = {"q8_0": ((64, 32), (1056, 1024)), "q4_k": ((512, 256), (2304, 2048)), "q6_k": ((512, 256), (1280, 1024))}


def check_onehot(run, qtype, K, k0):
    """Random blocks, x[b] = e_k: STORE returns f32(rne_bf16(dequant(W)[n][k])) exactly (a -0 weight gives +0: the sum
    starts at +0).  Eight k per call over the whole block: the nibble / high-bit / scale index maps."""
    rng = np.random.default_rng(900 + K + TYPES.index(qtype))
    N = 5
    blocks = random_blocks(qtype, N, K, rng)
    wv = rounded_weights(blocks, qtype)
    w = with_guard(blocks, qtype)
    count = gb.BLOCK[qtype][0]
    for k in range(k0, k0 + count, 8):
        xv = np.zeros((8, K), np.float32)
        xv[np.arange(8), np.arange(k, k + 8)] = 1.0
        y0 = lk._f32_sentinel((8, N + Y_PAD))
        want = y0.copy()
        want[:, :N] = wv[:, k:k + 8].T + np.float32(0.0)
        got = run(lk._padded_x(lk.bits(xv, 0), 0), w, qtype, y0, epi=STORE, n_rows=N)
        ok = lk._same_bits(got, want)
        assert ok.all(), (qtype, K, k, np.argwhere(~ok)[:4].tolist())


RANDOM_K = {"q8_0": (512, 1056), "q4_k": (1024, 2304), "q6_k": (512, 1280)}


def check_random(run, qtype, epi, K, N, impl):
    """x ~ N(0, 1) in bf16, random blocks, against the float64 product on the rounded weights
    under lm_kernel_cases.check_skinny_random's bound with c = the implementation's longest addition chain + 2.  RESID's
    y is drawn inside +- min sum |x||w|, so the rounding of the last add sits inside the + 2, as there."""
    rng = np.random.default_rng(1000 * K + 10 * N + 3 * epi + TYPES.index(qtype))
    xb = lk.bits(rng.standard_normal((8, K)), 0)
    x = lk._padded_x(xb, 0)
    xv = lk.vals(xb, 0)
    c = impl["chain"](qtype, K) + 2
    worst = 0.0
    if epi != SWIGLU:
        blocks = random_blocks(qtype, N, K, rng)
        wv = rounded_weights(blocks, qtype).astype(np.float64)
        w = with_guard(blocks, qtype)
        dot, mag = xv @ wv.T, np.abs(xv) @ np.abs(wv).T
        yi = (rng.uniform(-1, 1, (8, N)) * mag.min()).astype(np.float32)
        assert np.all(np.abs(yi) <= mag)
        for B in range(1, 9):
            y0 = lk._f32_sentinel((B, N + Y_PAD))
            if epi == RESID:
                y0[:, :N] = yi[:B]
            got = run(x[:B], w, qtype, y0, epi=epi, n_rows=N)
            assert lk._same_bits(got[:, N:], y0[:, N:]).all(), (qtype, epi, K, N, B)
            ref = dot[:B] + (yi[:B].astype(np.float64) if epi == RESID else 0.0)
            err, bound = np.abs(got[:, :N].astype(np.float64) - ref), c * U * mag[:B]
            worst = max(worst, float(np.max(err / bound)))
            assert np.all(err <= bound), (qtype, epi, K, N, B, float(np.max(err / bound)))
    else:
        I = N // 2
        g, u = random_blocks(qtype, I, K, rng), random_blocks(qtype, I, K, rng)
        w = with_guard(lk.interleave_gate_up(g, u), qtype)
        gw, uw = rounded_weights(g, qtype).astype(np.float64), rounded_weights(u, qtype).astype(np.float64)
        gv, uv = xv @ gw.T, xv @ uw.T
        eg, eu = c * U * (np.abs(xv) @ np.abs(gw).T), c * U * (np.abs(xv) @ np.abs(uw).T)
        worst = lk._check_swiglu(lambda xx, ww, y0, epi, act_type: run(xx, ww, qtype, y0, epi=epi, n_rows=N), 0, x, w, gv,
                                 uv, eg, eu, (qtype, K, N))
    print(f"lm_skinny_q {impl['name']} {qtype} epi {epi} K {K} N {N}: c {c}, worst err/bound {worst:.3f}")
    return worst


def check_deterministic(run, qtype, K):
    rng = np.random.default_rng(55 + K)
    x = lk.bits(rng.standard_normal((8, K)), 0)
    for epi, N in ((STORE, 37), (SWIGLU, 64)):
        w = random_blocks(qtype, N, K, rng)
        y0 = np.zeros((8, N), np.uint16 if epi == SWIGLU else np.float32)
        a, b = run(x, w, qtype, y0, epi=epi), run(x, w, qtype, y0, epi=epi)
        assert lk._same_bits(a, b).all(), (qtype, K, epi)


# ---------------------------------------------------------------------------------------------- the gather
EMBED_H = {"q8_0": (32, 544, 1056), "q4_k": (256, 1280), "q6_k": (256, 1280)}


def check_embed(run, qtype, H):
    """Gathered rows equal ggml's f32 dequant of the clamped ids' rows bit for bit (not rounded to bf16)."""
    rng = np.random.default_rng(17 + H + TYPES.index(qtype))
    vocab = 11
    blocks = random_blocks(qtype, vocab, H, rng)
    ids = np.array([-1, 0, vocab - 1, vocab, 4, -1000, vocab + 1000, 7], np.int32)
    got = run(blocks, qtype, ids)
    want = gb.dequant(blocks, qtype)[np.clip(ids, 0, vocab - 1)]
    assert np.isfinite(want).all() and not np.array_equal(want, lk.bf16_bits_to_f32(gb.bf16_bits(want)))
    ok = lk._same_bits(got, want)
    assert ok.all(), (qtype, H, np.argwhere(~ok)[:4].tolist())


# ---------------------------------------------------------------------------------------------- the tests themselves
def runners(lib=None):
    import functools
    import types
    from acestep_mi355x import capi
    return types.SimpleNamespace(skinny=functools.partial(capi.kernel_lm_skinny_q, lib=lib),
                                 embed=functools.partial(capi.kernel_lm_embed_q, lib=lib))


def _cases(table):
    return [(t, v) for t in TYPES for v in table[t]]


class LmQKernelChecks:
    """The test functions; a test file subclasses this as Test..., sets IMPL and provides the module fixture `k`."""
    IMPL = None

    @pytest.mark.parametrize("qtype,K", _cases(EXACT_K))
    def test_skinny_q_exact_integers(self, k, qtype, K):
        check_exact(k.skinny, qtype, K)

    @pytest.mark.parametrize("qtype,at", _cases(ONEHOT))
    def test_skinny_q_onehot(self, k, qtype, at):
        check_onehot(k.skinny, qtype, *at)

    @pytest.mark.parametrize("epi,N", [(STORE, 37), (RESID, 37), (SWIGLU, 32), (SWIGLU, 96)])
    @pytest.mark.parametrize("qtype,K", _cases(RANDOM_K))
    def test_skinny_q_random(self, k, qtype, K, epi, N):
        check_random(k.skinny, qtype, epi, K, N, self.IMPL)

    @pytest.mark.parametrize("qtype,K", _cases(RANDOM_K))
    def test_skinny_q_two_runs_identical(self, k, qtype, K):
        check_deterministic(k.skinny, qtype, K)

    @pytest.mark.parametrize("qtype,K", _cases(RANDOM_K))
    def test_skinny_q_reports_its_chain(self, k, qtype, K):
        """the entry's chain (kernels.h lm_skinny_q_chain) is the one the bound above is computed from"""
        x = np.zeros((1, K), np.uint16)
        w = unit_blocks(qtype, np.zeros((1, K), np.int64))
        _, chain = k.skinny(x, w, qtype, np.zeros((1, 1), np.float32), with_chain=True)
        assert chain == self.IMPL["chain"](qtype, K)

    @pytest.mark.parametrize("qtype,H", _cases(EMBED_H))
    def test_embed_q(self, k, qtype, H):
        check_embed(k.embed, qtype, H)

    def test_q_entries_refuse_bad_arguments(self, k):
        z16, zf = (lambda *s: np.zeros(s, np.uint16)), (lambda *s: np.zeros(s, np.float32))
        q8 = lambda rows, K: np.zeros((rows, K // 32, 34), np.uint8)     # noqa: E731
        bad = [
            lambda: k.skinny(z16(9, 64), q8(4, 64), "q8_0", zf(9, 4)),                         # B = 9
            lambda: k.skinny(z16(1, 68), q8(4, 64), "q8_0", zf(1, 4)),                         # ldx % 8
            lambda: k.skinny(z16(1, 32), q8(4, 64), "q8_0", zf(1, 4)),                         # ldx < K
            lambda: k.skinny(z16(1, 64), q8(48, 64), "q8_0", z16(1, 24), epi=SWIGLU),          # N % 32
            lambda: k.skinny(z16(1, 64), q8(4, 64), "q8_0", zf(1, 4), epi=3),                  # no such epilogue
            lambda: k.skinny(z16(1, 64), q8(4, 64), "q8_0", zf(1, 4), n_rows=5),               # N > rows given
            lambda: k.skinny(z16(1, 64), q8(4, 64), "q8_0", zf(1, 3)),                         # ldy < N
            lambda: k.embed(q8(4, 64), "q8_0", np.zeros(0, np.int32)),                         # n = 0
        ]
        for i, f in enumerate(bad):
            with pytest.raises(RuntimeError, match="status=2"):
                f()
                pytest.fail(f"bad call {i} was accepted")
