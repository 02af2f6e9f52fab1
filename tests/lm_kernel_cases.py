"""Shared by tests/test_gpu_lm_kernels.py (kernels/lm_decode.hip through the self-test library) and
tests/test_lm_kernels_cpu.py (tests/host/lm_emul.cpp through the LM host library): input builders, float64 numpy
references written from each operation's definition on the already-rounded 16-bit inputs, the bounds, and one check_*
function per property.  Every check takes the callable that runs the kernel (the capi.kernel_lm_* wrapper bound to a
library) and, where a bound depends on the summation order of the implementation under test, its IMPL description.

u = 2^-24 is the unit roundoff of f32 (half an ulp, relative).  A toleranced check prints its worst err / bound."""
import math

import numpy as np
import pytest

from oracle.ggml_numerics import bf16_bits_to_f32, f32_to_bf16_bits

U = 2.0 ** -24
STORE, RESID, SWIGLU = 0, 1, 2
D = 128

# What a bound needs to know about the implementation under test: its longest f32 addition chains.
#   skinny_c(K)   c of the skinny bound.  Kernel: a lane makes ceil(K / 512) trips of 8 fmas, then 6 butterfly adds.
#   norm_adds     additions behind the sum of squares of one head row (kernel: a*a + b*b, then 6 butterfly adds)
#   attn_c(nk)    c_sum of the attention bound = 16 (exp, the l chain, the divide, the merge weights) + the P.V
#                 chain: kernel 4 tree adds behind the per-thread fmas + one fma per range; emulation one fma per key.
KERNEL = dict(name="kernel", skinny_c=lambda K: 8 * (-(-K // 512)) + 6, norm_adds=7,
              attn_c=lambda nk: 16 + 4 + (-(-nk // 256)))
EMULATION = dict(name="emulation", skinny_c=lambda K: K, norm_adds=127, attn_c=lambda nk: 16 + nk)


def bits(x, act):
    if act == 0:
        return f32_to_bf16_bits(np.asarray(x, np.float32))
    return np.asarray(x, np.float32).astype(np.float16).view(np.uint16)


def vals(b, act):
    """16-bit words -> float64"""
    b = np.ascontiguousarray(b, dtype=np.uint16)
    if act == 0:
        return bf16_bits_to_f32(b).astype(np.float64)
    return b.view(np.float16).astype(np.float64)


def half_ulp(v, act):
    """Half an ulp of the 16-bit type at |v| (fp16: the subnormal spacing below 2^-14)."""
    v = np.abs(np.asarray(v, np.float64))
    e = np.frexp(np.maximum(v, 2.0 ** -140))[1] - 1          # floor(log2 v)
    if act == 0:
        return np.ldexp(1.0, e - 8)
    return np.ldexp(1.0, np.maximum(e, -14) - 11)


def _f32_sentinel(shape, word=0x7FC12345):
    return np.full(shape, word, np.uint32).view(np.float32)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    u = {2: np.uint16, 4: np.uint32}[a.dtype.itemsize]
    return a.view(u) == b.view(u)


# ---------------------------------------------------------------------------------------------- skinny product
X_PAD, Y_PAD = 8, 3
SKINNY_EXACT_K = (8, 256, 512, 520, 1024, 1536, 2560)
SKINNY_EXACT_N = (1, 3, 4, 5, 37)
X_NAN = {0: 0x7FC1, 1: 0x7E01}      # a NaN of the type beyond column K of x: any read of it poisons the sum


def _padded_x(xb, act):
    x = np.full((xb.shape[0], xb.shape[1] + X_PAD), X_NAN[act], np.uint16)
    x[:, :xb.shape[1]] = xb
    return x


def check_skinny_exact(run, act, K):
    """Integers in [-8, 8]: every product and partial sum is exact in f32 (|sum| <= 64 K < 2^24), so STORE and RESID
    equal the integer result bit for bit in any summation order.  ldx = K + 8, ldy = N + 3; the padding of y keeps its
    sentinel, the padding of x is NaN (read = poisoned result; x is a const input of the entry, so it cannot change)."""
    rng = np.random.default_rng(100 + 2 * K + act)
    xi = rng.integers(-8, 9, (8, K))
    x = _padded_x(bits(xi, act), act)
    for N in SKINNY_EXACT_N:
        wi = rng.integers(-8, 9, (N, K))
        w = bits(wi, act)
        ref = (xi @ wi.T).astype(np.float32)
        yi = rng.integers(-1000, 1001, (8, N)).astype(np.float32)
        for B in range(1, 9):
            for epi in (STORE, RESID):
                y0 = _f32_sentinel((B, N + Y_PAD))
                y0[:, :N] = yi[:B] if epi == RESID else _f32_sentinel((B, N), 0x7FC0BEEF)
                want = y0.copy()
                want[:, :N] = ref[:B] + (yi[:B] if epi == RESID else 0)
                got = run(x[:B], w, y0, epi=epi, act_type=act)
                ok = _same_bits(got, want)
                assert ok.all(), (act, K, N, B, epi, np.argwhere(~ok)[:4].tolist())


ONEHOT_COLS = {520: (0, 7, 8, 255, 511, 512, 513, 519), 1536: (0, 7, 511, 512, 513, 1024, 1031, 1535)}


def check_skinny_onehot(run, act, K):
    """x[b] = e_{k_b} (k_b = K - 1 and k_b just past a 512 boundary among them), W[n][k] pairwise distinct normal values
    of the type: STORE returns W[n][k_b] exactly.  Any row, column or batch mix-up returns another word."""
    N = 5
    cols = ONEHOT_COLS[K]
    n_i, k_i = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    w = (0x2000 + n_i * K + k_i + 0x8000 * ((n_i + k_i) & 1)).astype(np.uint16)     # 0x2000 .. 0x3e00, both signs
    assert len(np.unique(w)) == N * K
    xv = np.zeros((8, K), np.float32)
    xv[np.arange(8), cols] = 1.0
    x = _padded_x(bits(xv, act), act)
    for B in range(1, 9):
        y0 = _f32_sentinel((B, N + Y_PAD))
        want = y0.copy()
        want[:, :N] = vals(w[:, list(cols[:B])].T, act).astype(np.float32)
        got = run(x[:B], w, y0, epi=STORE, act_type=act)
        ok = _same_bits(got, want)
        assert ok.all(), (act, K, B, np.argwhere(~ok)[:4].tolist())


def interleave_gate_up(g, u):
    """the 16-row gate|up interleave [g0..15, u0..15, g16..31, ...] (runtime/model.cpp)"""
    I = g.shape[0]
    wi = np.empty((2 * I,) + g.shape[1:], g.dtype)
    for r in range(2 * I):
        grp, w16 = divmod(r, 32)
        wi[r] = (g if w16 < 16 else u)[grp * 16 + (w16 % 16)]
    return wi


def check_skinny_random(run, act, epi, K, N, impl):
    """x ~ N(0, 1), W ~ N(0, 0.05), rounded to the type, against the float64 product.
    STORE / RESID: |got - ref| <= c u sum_k |x_k||w_k|, c = the implementation's longest addition chain + 2
    (impl.skinny_c).  RESID's y is drawn with |y| <= sum |x||w| (asserted), so the rounding of the last add, u |y + acc|
    <= 2 u sum |x||w|, sits inside the + 2.
    SWIGLU: silu(g) u in float64; bound = half an ulp of the output type + the f32 bounds e_g, e_u of the two products
    through d/dg and d/du (second-order terms with |silu'| <= 1.1, |silu''| <= 0.5 added) + 4 u |ref| for exp, add,
    divide and multiply.  The half ulp is taken at |ref| + the f32 error, the value the kernel rounds."""
    rng = np.random.default_rng(1000 * K + 10 * N + 3 * epi + act)
    xb = bits(rng.standard_normal((8, K)), act)
    x = _padded_x(xb, act)
    xv = vals(xb, act)
    c = impl["skinny_c"](K)
    worst = 0.0
    if epi != SWIGLU:
        w = bits(rng.standard_normal((N, K)) * 0.05, act)
        wv = vals(w, act)
        dot, mag = xv @ wv.T, np.abs(xv) @ np.abs(wv).T
        yi = np.clip(rng.standard_normal((8, N)), -4, 4).astype(np.float32)
        assert np.all(np.abs(yi) <= mag)
        for B in range(1, 9):
            y0 = _f32_sentinel((B, N + Y_PAD))
            if epi == RESID:
                y0[:, :N] = yi[:B]
            got = run(x[:B], w, y0, epi=epi, act_type=act)
            assert _same_bits(got[:, N:], y0[:, N:]).all(), (act, epi, K, N, B)
            ref = dot[:B] + (yi[:B].astype(np.float64) if epi == RESID else 0.0)
            err, bound = np.abs(got[:, :N].astype(np.float64) - ref), c * U * mag[:B]
            worst = max(worst, float(np.max(err / bound)))
            assert np.all(err <= bound), (act, epi, K, N, B, float(np.max(err / bound)))
    else:
        I = N // 2
        g = bits(rng.standard_normal((I, K)) * 0.05, act)
        u = bits(rng.standard_normal((I, K)) * 0.05, act)
        w = interleave_gate_up(g, u)
        gv, uv = xv @ vals(g, act).T, xv @ vals(u, act).T
        eg, eu = c * U * (np.abs(xv) @ np.abs(vals(g, act)).T), c * U * (np.abs(xv) @ np.abs(vals(u, act)).T)
        worst = _check_swiglu(run, act, x, w, gv, uv, eg, eu, (act, K, N))
    print(f"lm_skinny {impl['name']} act {act} epi {epi} K {K} N {N}: worst err/bound {worst:.3f}")
    return worst


def _check_swiglu(run, act, x, w, gv, uv, eg, eu, what):
    I = gv.shape[1]
    sig = 1.0 / (1.0 + np.exp(-gv))
    silu, dsilu = gv * sig, sig * (1.0 + gv * (1.0 - sig))
    ref = silu * uv
    e32 = np.abs(dsilu * uv) * eg + np.abs(silu) * eu + 1.1 * eg * eu + 0.25 * np.abs(uv) * eg * eg + 4 * U * np.abs(ref)
    bound = e32 + half_ulp(np.abs(ref) + e32, act)
    worst = 0.0
    for B in range(1, 9):
        y0 = np.full((B, I + Y_PAD), 0x7FFF, np.uint16)
        got = run(x[:B], w, y0, epi=SWIGLU, act_type=act)
        assert (got[:, I:] == 0x7FFF).all(), (what, B)
        err = np.abs(vals(got[:, :I], act) - ref[:B])
        worst = max(worst, float(np.max(err / bound[:B])))
        assert np.all(err <= bound[:B]), (what, B, float(np.max(err / bound[:B])))
    return worst


def check_skinny_swiglu_integer(run, act):
    """Exact-integer inputs (K = 8, 64 rows = two interleave groups): g and u are exact, so the bound is the half ulp of
    the output plus 4 u |ref| alone, and silu(g) u of another row pair, or of the pair swapped, lies far outside it."""
    rng = np.random.default_rng(77 + act)
    K, I = 8, 32
    xi = rng.integers(-2, 3, (8, K))
    gi, ui = rng.integers(-2, 3, (I, K)), rng.integers(-2, 3, (I, K))
    x = _padded_x(bits(xi, act), act)
    w = interleave_gate_up(bits(gi, act), bits(ui, act))
    gv, uv = (xi @ gi.T).astype(np.float64), (xi @ ui.T).astype(np.float64)
    zero = np.zeros_like(gv)
    worst = _check_swiglu(run, act, x, w, gv, uv, zero, zero, ("integer", act))
    print(f"lm_skinny swiglu integer act {act}: worst err/bound {worst:.3f}")
    return worst


# ---------------------------------------------------------------------------------------------- embedding
def check_embed(run, fmt, H):
    """ids below, inside and above the table: the output rows are bit-equal to the widened rows of the clamped ids.
    Table words: every finite pattern class of the type (normal, subnormal, zero of both signs)."""
    rng = np.random.default_rng(5 + H + fmt)
    vocab = 11
    t = rng.integers(0, 1 << 16, (vocab, H)).astype(np.uint16)
    exp_mask = 0x7F80 if fmt == 0 else 0x7C00
    t = np.where((t & exp_mask) == exp_mask, t & 0xBFFF, t).astype(np.uint16)      # no inf / NaN: top exponent bit off
    t[0, :4] = (0x0000, 0x8000, 0x0001, 0x83FF)
    ids = np.array([-5, 0, vocab - 1, vocab + 7], np.int32)
    got = run(t, ids, fmt=fmt)
    want = vals(t[np.clip(ids, 0, vocab - 1)], fmt).astype(np.float32)
    assert np.isfinite(want).all()
    ok = _same_bits(got, want)
    assert ok.all(), (fmt, H, np.argwhere(~ok)[:4].tolist())


# ---------------------------------------------------------------------------------------------- q/k norm + RoPE, append
CAPACITY = 7
EPS = np.float32(1e-6)
CACHE_SENTINEL, MASK_SENTINEL = 0x5A5A, -7
LD_PAD = 24


def rope_tables(capacity, theta=1.0e6):
    """LmEngine::begin: theta_p,i by ggml's f32 recurrence, cos / sin in double, rounded to f32."""
    scale = np.float32(np.power(np.float32(theta), np.float32(-2.0 / D)))
    cs, sn = np.empty((capacity, 64), np.float32), np.empty((capacity, 64), np.float32)
    for p in range(capacity):
        th = np.float32(p)
        for i in range(64):
            cs[p, i], sn[p, i] = np.float32(math.cos(float(th))), np.float32(math.sin(float(th)))
            th = np.float32(th * scale)
    return cs, sn


def norm_rope_c(impl):
    """The f32 chain of one output of RMSNorm + NEOX RoPE, in u, relative to |a'| + |b'| (a', b' the normalised,
    weighted pair): squares 1 + the sum's adds, + eps 1 -> halved by the square root, + sqrt 1, + reciprocal 1, + two
    multiplies 2, + the rotation's multiply 1 and add 1.  Kernel: (2 + 7 + 1) / 2 + 6 = 11 (below the 16 the first count
    allowed for)."""
    return math.ceil((2 + impl["norm_adds"] + 1) / 2 + 6)


def norm_rope_ref(x, w, cs, sn):
    """x [.., 128] float64 -> (rotated [.., 128], |a'| + |b'| [.., 128]) in float64; cs, sn [.., 64] broadcastable"""
    y = x / np.sqrt(np.mean(x * x, axis=-1, keepdims=True) + float(EPS)) * w
    a, b = y[..., :64], y[..., 64:]
    mag = np.abs(a) + np.abs(b)
    return np.concatenate([a * cs - b * sn, a * sn + b * cs], -1), np.concatenate([mag, mag], -1)


# V inputs that the cache must hold as round-to-nearest-even fp16 of the value clamped to +-65504
V_SPECIALS = np.array([1e6, -1e6, np.inf, -np.inf, 65504.0, 65520.0, -65519.996, 3e-6, -2.5 * 2.0 ** -24, 2.0 ** -25,
                       2.0 ** -25 * (1 + 2.0 ** -20), 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2.0 ** -14 - 2.0 ** -25,
                       -(2.0 ** -14 - 2.0 ** -24), 0.0, -0.0, 2049.0, 2051.0, 6.0e-8], np.float32)


def f16_sat_bits(v):
    return np.clip(np.asarray(v, np.float32), np.float32(-65504), np.float32(65504)).astype(np.float16).view(np.uint16)


def _qkv_rows(rng, rows, hq, hkv):
    """[rows][ld] f32: heads at scales from 0.01 to 30 (the norm removes them), V heads with V_SPECIALS, NaN padding"""
    H = hq + 2 * hkv
    x = rng.standard_normal((rows, H, D)) * np.exp(rng.uniform(np.log(0.01), np.log(30.0), (rows, H, 1)))
    x = x.astype(np.float32)
    for r in range(rows):
        for h in range(hq + hkv, H):
            at = rng.permutation(D)[:len(V_SPECIALS)]
            x[r, h, at] = V_SPECIALS
    out = _f32_sentinel((rows, H * D + LD_PAD))
    out[:, :H * D] = x.reshape(rows, H * D)
    return out


def _norm_weights(rng):
    return (1 + 0.3 * rng.standard_normal(D)).astype(np.float32)


def _sentinel_cache(B, hkv):
    return (np.full((B, hkv, CAPACITY, D), CACHE_SENTINEL, np.uint16), np.full((B, hkv, CAPACITY, D), CACHE_SENTINEL, np.uint16),
            np.full((B, CAPACITY), MASK_SENTINEL, np.int32))


def _check_k_slot(got_bits, ref, mag, c):
    """fp16 K against the float64 value: the f32 bound c u (|a'| + |b'|), then half an fp16 ulp of the rounded value"""
    e32 = c * U * mag
    bound = e32 + half_ulp(np.abs(ref) + e32, 1)
    err = np.abs(vals(got_bits, 1) - ref)
    return err, bound


def check_qkv_post(run, hq, hkv, B, impl):
    """Every pos in {0, 3, 6} of a 7-slot cache, mask_new NULL or with a zero in one row; ld > row.
    q_out: |got - ref| <= c u (|a'| + |b'|) per element, c = norm_rope_c.  K slot: the same plus half an fp16 ulp.
    V slot: bit-equal to rne fp16 of the clamped input.  Nothing but slot pos of each (b, kv head) and key_mask[b][pos]
    changes; key_mask[b][pos] = 1, or mask_new[b] != 0."""
    rng = np.random.default_rng(31 * hq + 7 * hkv + B)
    cs, sn = rope_tables(CAPACITY)
    c = norm_rope_c(impl)
    worst_q = worst_k = 0.0
    for pos in (0, 3, 6):
        for masked in (False, True):
            qkv = _qkv_rows(rng, B, hq, hkv)
            qn, kn = _norm_weights(rng), _norm_weights(rng)
            mask_new = None
            if masked:
                mask_new = np.array([1, 5, -2, 1, 1, 9, 1, 1][:B], np.int32)
                mask_new[B // 2] = 0
            kc0, vc0, km0 = _sentinel_cache(B, hkv)
            q, kc, vc, km = run(qkv, hq, hkv, pos, float(EPS), qn, kn, cs, sn, mask_new, kc0, vc0, km0)
            heads = qkv[:, :(hq + 2 * hkv) * D].reshape(B, hq + 2 * hkv, D).astype(np.float64)
            what = (hq, hkv, B, pos, masked)
            ref, mag = norm_rope_ref(heads[:, :hq], qn.astype(np.float64), cs[pos].astype(np.float64), sn[pos].astype(np.float64))
            err, bound = np.abs(q.astype(np.float64) - ref), c * U * mag
            worst_q = max(worst_q, float(np.max(err / bound)))
            assert np.all(err <= bound), ("q_out", what, float(np.max(err / bound)))
            ref, mag = norm_rope_ref(heads[:, hq:hq + hkv], kn.astype(np.float64), cs[pos].astype(np.float64), sn[pos].astype(np.float64))
            err, bound = _check_k_slot(kc[:, :, pos], ref, mag, c)
            worst_k = max(worst_k, float(np.max(err / bound)))
            assert np.all(err <= bound), ("k slot", what, float(np.max(err / bound)))
            want_v = f16_sat_bits(heads[:, hq + hkv:].astype(np.float32))
            ok = vc[:, :, pos] == want_v
            assert ok.all(), ("v slot", what, np.argwhere(~ok)[:4].tolist())
            others = np.arange(CAPACITY) != pos
            assert (kc[:, :, others] == CACHE_SENTINEL).all() and (vc[:, :, others] == CACHE_SENTINEL).all(), what
            want_m = km0.copy()
            want_m[:, pos] = 1 if mask_new is None else (mask_new != 0)
            assert (km == want_m).all(), ("key_mask", what, km.tolist())
    print(f"lm_qkv_post {impl['name']} hq {hq} hkv {hkv} B {B}: worst err/bound q_out {worst_q:.3f} k slot {worst_k:.3f}")
    return worst_q, worst_k


def check_prefill_kv(run, hq, hkv, B, n, impl):
    """Rows b n + t -> slots t < n of a 7-slot cache; mask NULL, or left padding of min(2, n) in one row (n = 1: that
    row is padding only).  Valid rows: K normed and rotated at slot t (the qkv_post bound), V rne fp16 of the clamped
    input, their q|k|v columns bit-identical afterwards.  Padding rows: q|k|v zeroed in place (+0), cache slots 0x0000,
    key_mask 0.  Slots >= n, the row padding of qkv and key_mask beyond n keep their sentinels."""
    rng = np.random.default_rng(500 + 31 * hq + 7 * hkv + 3 * B + n)
    cs, sn = rope_tables(CAPACITY)
    c = norm_rope_c(impl)
    H = hq + 2 * hkv
    worst = 0.0
    for padded in (False, True):
        qkv0 = _qkv_rows(rng, B * n, hq, hkv)
        kn = _norm_weights(rng)
        mask = None
        if padded:
            mask = np.ones((B, n), np.int32)
            mask[B // 2, :min(2, n)] = 0
        kc0, vc0, km0 = _sentinel_cache(B, hkv)
        qkv, kc, vc, km = run(qkv0, n, hq, hkv, float(EPS), kn, cs, sn, mask, kc0, vc0, km0)
        what = (hq, hkv, B, n, padded)
        valid = np.ones((B, n), bool) if mask is None else mask != 0
        want_x = qkv0.copy()
        want_x[~valid.reshape(-1), :H * D] = 0.0
        ok = _same_bits(qkv, want_x)
        assert ok.all(), ("qkv", what, np.argwhere(~ok)[:4].tolist())
        heads = qkv0[:, :H * D].reshape(B, n, H, D).astype(np.float64)
        kin = heads[:, :, hq:hq + hkv].transpose(0, 2, 1, 3)                        # [B][hkv][n][128]
        ref, mag = norm_rope_ref(kin, kn.astype(np.float64), cs[:n].astype(np.float64), sn[:n].astype(np.float64))
        err, bound = _check_k_slot(kc[:, :, :n], ref, mag, c)
        vsel = np.broadcast_to(valid[:, None, :, None], err.shape)
        r = float(np.max((err / bound)[vsel], initial=0.0))
        worst = max(worst, r)
        assert np.all((err <= bound)[vsel]), ("k slots", what, r)
        assert (kc[:, :, :n][~vsel] == 0).all() and (vc[:, :, :n][~vsel] == 0).all(), ("padding slots", what)
        want_v = f16_sat_bits(heads[:, :, hq + hkv:].transpose(0, 2, 1, 3).astype(np.float32))
        assert (vc[:, :, :n] == want_v)[vsel].all(), ("v slots", what)
        assert (kc[:, :, n:] == CACHE_SENTINEL).all() and (vc[:, :, n:] == CACHE_SENTINEL).all(), ("slots >= n", what)
        want_m = km0.copy()
        want_m[:, :n] = valid
        assert (km == want_m).all(), ("key_mask", what, km.tolist())
    print(f"lm_prefill_kv {impl['name']} hq {hq} hkv {hkv} B {B} n {n}: worst err/bound k slots {worst:.3f}")
    return worst


# ---------------------------------------------------------------------------------------------- decode attention
ATTN_CONFIGS = ((1, 1), (2, 2), (4, 2), (4, 1), (8, 2))            # (hq, hkv): REP 1, 1, 2, 4, 4
ATTN_SMALL_NK = (1, 15, 16, 17)
ATTN_LARGE = ((255, (1, 1)), (256, (2, 2)), (257, (4, 2)), (512, (4, 1)), (513, (8, 2)), (700, (4, 2)))
ATTN_SCALE = np.float32(1.0 / math.sqrt(D))
F16_NAN = 0x7E00
BIG = 6.0e4


def attn_inputs(rng, B, hq, hkv, nk, mask, score_sd=4.0):
    """q ~ N(0, score_sd) so that scale q.k has that standard deviation (a peaked softmax); K, V ~ N(0, 1) in fp16;
    capacity = nk + 5.  mask: 'none', 'pad3' / 'pad260' (left padding in the last row), 'all' (every key of row 0
    masked).  Masked slots inside nk hold +-6e4 in K and V, slots >= nk fp16 NaN (with key_mask 1: reading one shows)."""
    cap = nk + 5
    q = (rng.standard_normal((B, hq, D)) * score_sd).astype(np.float32)
    kc = rng.standard_normal((B, hkv, cap, D)).astype(np.float16).view(np.uint16)
    vc = rng.standard_normal((B, hkv, cap, D)).astype(np.float16).view(np.uint16)
    km = np.ones((B, cap), np.int32)
    if mask.startswith("pad"):
        km[B - 1, :int(mask[3:])] = 0
    elif mask == "all":
        km[0, :nk] = 0
    assert mask == "all" or km[:, :nk].any(axis=1).all()
    big = np.where(rng.integers(0, 2, (B, hkv, cap, D)) == 1, BIG, -BIG).astype(np.float16).view(np.uint16)
    off = np.broadcast_to((km == 0)[:, None, :, None], kc.shape)
    kc, vc = np.where(off, big, kc), np.where(off, big[..., ::-1], vc)
    kc[:, :, nk:], vc[:, :, nk:] = F16_NAN, F16_NAN
    return q, np.ascontiguousarray(kc), np.ascontiguousarray(vc), km


def attn_ref(q, kc, vc, km, nk, scale):
    """float64 softmax(scale q.k) . V on the fp16 cache values: (ref, sum_j p_j |v_jd|, delta_s, scores), each
    [B][hq][..]; a row with every key masked gives 0."""
    B, hq, _ = q.shape
    rep = hq // kc.shape[1]
    k, v = vals(kc[:, :, :nk], 1), vals(vc[:, :, :nk], 1)
    ref, pv = np.zeros((B, hq, D)), np.zeros((B, hq, D))
    delta, scores = np.zeros((B, hq, 1)), np.full((B, hq, nk), -np.inf)
    for b in range(B):
        on = km[b, :nk] != 0
        if not on.any():
            continue
        for h in range(hq):
            qv = q[b, h].astype(np.float64)
            s = float(scale) * (k[b, h // rep, on] @ qv)
            p = np.exp(s - s.max())
            p /= p.sum()
            ref[b, h], pv[b, h] = p @ v[b, h // rep, on], p @ np.abs(v[b, h // rep, on])
            delta[b, h] = 16 * U * float(scale) * np.max(np.abs(k[b, h // rep, on]) @ np.abs(qv))
            scores[b, h, on] = s
    return ref, pv, delta, scores


def check_attention(run, out_type, q, kc, vc, km, nk, impl, what):
    """|got - ref| <= half an ulp of the output type (at |ref| + e) + e, e = (c_sum u + 2 delta_s) sum_j p_j |v_jd|:
    delta_s = 16 u scale max_j sum_i |q_i k_ji| is the score error, which exp turns into a relative error of p (twice:
    numerator and denominator); c_sum = impl.attn_c(nk).  Every output is finite; a row with every key masked is +0."""
    got = run(q, kc, vc, km, nk, float(ATTN_SCALE), out_type=out_type)
    ref, pv, delta, _ = attn_ref(q, kc, vc, km, nk, ATTN_SCALE)
    gv = vals(got, out_type)
    assert np.isfinite(gv).all(), (what, "non-finite output")
    dead = ~(km[:, :nk] != 0).any(axis=1)
    assert (got[dead] == 0).all(), (what, "a fully masked row is not +0")
    e = (impl["attn_c"](nk) * U + 2 * delta) * pv
    bound = e + half_ulp(np.abs(ref) + e, out_type)
    err = np.abs(gv - ref)
    live = ~dead
    r = float(np.max((err / bound)[live])) if live.any() else 0.0
    assert np.all((err <= bound)[live]), (what, r)
    return r


def check_attention_shapes(run, out_type, hq, hkv, B, nks, masks, impl):
    worst = 0.0
    for nk in nks:
        for mask in masks:
            if mask.startswith("pad") and int(mask[3:]) >= nk:
                continue
            rng = np.random.default_rng(9000 + 64 * nk + 8 * hq + hkv + B + len(mask))
            q, kc, vc, km = attn_inputs(rng, B, hq, hkv, nk, mask)
            worst = max(worst, check_attention(run, out_type, q, kc, vc, km, nk, impl, (out_type, hq, hkv, B, nk, mask)))
    print(f"lm_attention {impl['name']} out {out_type} hq {hq} hkv {hkv} B {B} nk {list(nks)}: worst err/bound {worst:.3f}")
    return worst


def check_attention_large_scores(run, out_type, hq, hkv, B, impl):
    """nk = 700, three ranges: K is built along the first query of each kv head so that its scores spread over
    [-150, 140], with 150 at key 690 (last range) and 149 at key 5 (first range).  Without the max subtraction exp
    overflows; with a wrong merge weight the two keys that carry the result get the wrong shares."""
    nk, rep = 700, hq // hkv
    rng = np.random.default_rng(4242 + hq + B + out_type)
    q, kc, vc, km = attn_inputs(rng, B, hq, hkv, nk, "none")
    target = rng.uniform(-150.0, 140.0, (B, hkv, nk))
    target[:, :, 690], target[:, :, 5] = 150.0, 149.0
    q0 = q[:, ::rep].astype(np.float64)                                        # [B][hkv][128]
    k = target[..., None] * (q0 / (float(ATTN_SCALE) * np.sum(q0 * q0, -1, keepdims=True)))[:, :, None, :]
    kc[:, :, :nk] = k.astype(np.float16).view(np.uint16)
    _, _, _, s = attn_ref(q, kc, vc, km, nk, ATTN_SCALE)
    order = np.argsort(s[:, ::rep], axis=-1)
    assert (order[..., -1] == 690).all() and (order[..., -2] == 5).all() and s.max() > 149.5 and s.min() < -100
    r = check_attention(run, out_type, q, kc, vc, km, nk, impl, ("large scores", out_type, hq, hkv, B))
    print(f"lm_attention {impl['name']} large scores out {out_type} hq {hq} hkv {hkv} B {B}: worst err/bound {r:.3f}")
    return r


ONEHOT_NK = 300
ONEHOT_KEYS = (0, 15, 16, 255, 256, ONEHOT_NK - 1)


def check_attention_onehot(run, out_type, hq, hkv, B):
    """nk = 300 (two ranges).  Key j* = sign pattern of its kv head's queries, every query = that pattern times 12 .. 16,
    every other key ~ N(0, 0.1): the score of j* beats every other by more than 110 (asserted on the float64 scores), so
    every other p and the other range's merge weight are exactly 0 in f32 and the output row is V[j*]: exactly in F16,
    rne bf16 of it in BF16, for every head."""
    nk, rep = ONEHOT_NK, hq // hkv
    for jstar in ONEHOT_KEYS:
        rng = np.random.default_rng(777 + jstar + hq + B)
        _, kc, vc, km = attn_inputs(rng, B, hq, hkv, nk, "none")
        sign = np.where(rng.integers(0, 2, (B, hkv, D)) == 1, 1.0, -1.0)
        gain = 12.0 + rng.integers(0, 5, (B, hq, 1))
        q = (np.repeat(sign, rep, axis=1) * gain).astype(np.float32)
        kc[:, :, :nk] = (rng.standard_normal((B, hkv, nk, D)) * 0.1).astype(np.float16).view(np.uint16)
        kc[:, :, jstar] = sign.astype(np.float16).view(np.uint16)
        _, _, _, s = attn_ref(q, kc, vc, km, nk, ATTN_SCALE)
        rest = np.delete(s, jstar, axis=-1)
        assert (s[..., jstar] - rest.max(axis=-1) > 110).all()
        got = run(q, kc, vc, km, nk, float(ATTN_SCALE), out_type=out_type)
        want = np.repeat(vc[:, :, jstar], rep, axis=1)                          # [B][hq][128] fp16 words
        if out_type == 0:
            want = f32_to_bf16_bits(want.view(np.float16).astype(np.float32))
        ok = got == want
        assert ok.all(), (out_type, hq, hkv, B, jstar, np.argwhere(~ok)[:4].tolist())


# ---------------------------------------------------------------------------------------------- the tests themselves
def runners(lib=None):
    """The five capi.kernel_lm_* wrappers bound to `lib` (None: the GPU self-test library)."""
    import functools
    import types
    from acestep_mi355x import capi
    return types.SimpleNamespace(**{n: functools.partial(getattr(capi, "kernel_lm_" + n), lib=lib)
                                    for n in ("skinny", "embed", "qkv_post", "prefill_kv", "attention")})



class LmKernelChecks:
    """The test functions; a test file subclasses this as Test..., sets IMPL and provides the module fixture `k`
    (runners(lib))."""
    IMPL = None

    @pytest.mark.parametrize("act", [0, 1])
    @pytest.mark.parametrize("K", SKINNY_EXACT_K)
    def test_skinny_exact_integers(self, k, act, K):
        check_skinny_exact(k.skinny, act, K)

    @pytest.mark.parametrize("act", [0, 1])
    @pytest.mark.parametrize("K", sorted(ONEHOT_COLS))
    def test_skinny_onehot(self, k, act, K):
        check_skinny_onehot(k.skinny, act, K)

    @pytest.mark.parametrize("act", [0, 1])
    @pytest.mark.parametrize("epi,N", [(STORE, 37), (RESID, 37), (SWIGLU, 32), (SWIGLU, 96)])
    @pytest.mark.parametrize("K", [520, 1536])
    def test_skinny_random(self, k, act, epi, N, K):
        check_skinny_random(k.skinny, act, epi, K, N, self.IMPL)

    @pytest.mark.parametrize("act", [0, 1])
    def test_skinny_swiglu_integer_pairing(self, k, act):
        check_skinny_swiglu_integer(k.skinny, act)

    @pytest.mark.parametrize("fmt", [0, 1])
    @pytest.mark.parametrize("H", [8, 256, 2056])
    def test_embed(self, k, fmt, H):
        check_embed(k.embed, fmt, H)

    @pytest.mark.parametrize("hq,hkv", [(1, 1), (4, 2), (4, 1)])
    @pytest.mark.parametrize("B", [1, 3, 8])
    def test_qkv_post(self, k, hq, hkv, B):
        check_qkv_post(k.qkv_post, hq, hkv, B, self.IMPL)

    @pytest.mark.parametrize("hq,hkv", [(1, 1), (4, 2)])
    @pytest.mark.parametrize("B", [1, 3])
    @pytest.mark.parametrize("n", [1, 5])
    def test_prefill_kv(self, k, hq, hkv, B, n):
        check_prefill_kv(k.prefill_kv, hq, hkv, B, n, self.IMPL)

    @pytest.mark.parametrize("out_type", [0, 1])
    @pytest.mark.parametrize("hq,hkv", ATTN_CONFIGS)
    @pytest.mark.parametrize("B", [1, 3])
    def test_attention_small(self, k, out_type, hq, hkv, B):
        check_attention_shapes(k.attention, out_type, hq, hkv, B, ATTN_SMALL_NK, ("none", "pad3", "all"), self.IMPL)

    @pytest.mark.parametrize("out_type", [0, 1])
    @pytest.mark.parametrize("nk,cfg", ATTN_LARGE)
    @pytest.mark.parametrize("B", [1, 3])
    def test_attention_large(self, k, out_type, nk, cfg, B):
        masks = ("none", "pad3") + (("pad260", "all") if nk == 513 else ())
        check_attention_shapes(k.attention, out_type, cfg[0], cfg[1], B, (nk,), masks, self.IMPL)

    @pytest.mark.parametrize("out_type", [0, 1])
    @pytest.mark.parametrize("hq,hkv,B", [(2, 2, 1), (4, 2, 3), (4, 1, 2)])
    def test_attention_large_scores(self, k, out_type, hq, hkv, B):
        check_attention_large_scores(k.attention, out_type, hq, hkv, B, self.IMPL)

    @pytest.mark.parametrize("out_type", [0, 1])
    @pytest.mark.parametrize("hq,hkv,B", [(1, 1, 1), (4, 2, 3), (8, 2, 2)])
    def test_attention_onehot(self, k, out_type, hq, hkv, B):
        check_attention_onehot(k.attention, out_type, hq, hkv, B)

    def test_entries_refuse_bad_arguments(self, k):
        """INVALID_ARG (status 2) for what launch_lm_* refuses, before anything is launched."""
        z16, zf = (lambda *s: np.zeros(s, np.uint16)), (lambda *s: np.zeros(s, np.float32))
        cs, sn = rope_tables(CAPACITY)
        kc, vc, km = _sentinel_cache(1, 1)
        bad = [
            lambda: k.skinny(z16(9, 16), z16(4, 16), zf(9, 4)),                           # B = 9
            lambda: k.skinny(z16(1, 16), z16(4, 12), zf(1, 4)),                           # K % 8
            lambda: k.skinny(z16(1, 20), z16(4, 16), zf(1, 4)),                           # ldx % 8
            lambda: k.skinny(z16(1, 16), z16(48, 16), z16(1, 24), epi=SWIGLU),            # N % 32
            lambda: k.skinny(z16(1, 16), z16(4, 16), zf(1, 4), epi=3),                    # no such epilogue
            lambda: k.embed(z16(4, 12), np.zeros(2, np.int32)),                           # H % 8
            lambda: k.embed(z16(4, 8), np.zeros(2, np.int32), fmt=2),
            lambda: k.qkv_post(zf(1, 3 * D), 1, 1, CAPACITY, 1e-6, zf(D), zf(D), cs, sn, None, kc, vc, km),   # pos
            lambda: k.qkv_post(zf(1, 3 * D), 1, 1, -1, 1e-6, zf(D), zf(D), cs, sn, None, kc, vc, km),
            lambda: k.prefill_kv(zf(8, 3 * D), 8, 1, 1, 1e-6, zf(D), cs, sn, None, kc, vc, km),               # n > capacity
            lambda: k.attention(zf(1, 3, D), kc, vc, km, 1, 1.0),                         # GQA ratio 3
            lambda: k.attention(zf(1, 1, D), kc, vc, km, CAPACITY + 1, 1.0),              # nk > capacity
            lambda: k.attention(zf(1, 1, D), kc, vc, km, 0, 1.0),
        ]
        for i, f in enumerate(bad):
            with pytest.raises(RuntimeError, match="status=2"):
                f()
                pytest.fail(f"bad call {i} was accepted")
