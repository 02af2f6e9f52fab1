"""Shared by tests/test_gpu_vae_kernels.py (kernels/vae.hip through the self-test library) and
tests/test_vae_kernels_cpu.py (tests/host/kernel_emul.cpp through the host library): shapes, input builders, float64
numpy references written from the definition of each operation in csrc/kernels.h on the already-rounded fp16 inputs,
the bounds, and one check_* function per property.  Every check takes the callable that runs the kernel (a
capi.kernel_* wrapper bound to a library) and, where a bound depends on the implementation's sine, its IMPL description.

The operation (ConvGemmArgs): the A row (m, tap) of item i is S[i][ml * in_stride + tap * dil - pad] (ml = m mod M / items),
or zero outside [0, T_in); acc[m][n] = sum_k A[m][k] W[n][k]; up == 1: (m, n) -> (u = ml, co = n); up > 1: n = r * Cout + co
-> u = ml * up + r - crop; outputs with u outside [0, T_out) are dropped.  v = acc + bias[co]; resid: v = X[u][co] + v;
store_x: X[u][co] = v; S_out[u][co] = f16(v + sin^2(ea v) / eb) or f16(v).  With W2: y = f16(Snake2(acc + bias)) and
acc is replaced by y . W2^T, bias by bias2.

u = 2^-24 is the unit roundoff of f32.  A toleranced check prints its worst err / bound."""
import math

import numpy as np
import pytest

U = 2.0 ** -24
G = 64                                   # guard elements before and after the payload of X / S_out
X_SENT, S_SENT = 0x7FC12345, 0x7E5A      # NaN sentinels (f32 word, fp16 word)

# What a bound needs to know about the implementation under test: e_sin(|x|), the absolute error of sin^2(x) as the
# Snake of that implementation computes it (x = ea v), including the rounding of the argument, of the square, of the
# division by eb (relative to the term) and the term's share of the final addition.
#   Emulation (libm sinf, true division, every step rounded to f32): the argument fl(ea v) is off by |x| u, which moves
#   sin^2 by |sin 2x| |x| u <= |x| u; sinf is within 1 ulp = 2 u relative, so sin^2 moves by <= 4 u sin^2 <= 4 u; the
#   square, the division and the term's share of the last addition (u sin^2 / eb each, relative to the term) add 3 u.
#   e_sin = (|x| + 7) u, at most 39 u for |x| <= 32.
#   Kernel (__sinf, multiply by the hardware reciprocal): measured, see E_SIN_KERNEL.
#   E_SIN_KERNEL = 4 x the measured maximum, and must stay below 2^-14 (an eighth of fp16's half spacing at 1.0), or the
#   kernel header's "far below the fp16 rounding" no longer holds (asserted in test_sine_term).
E_SIN_MEASURED = 2.954e-6
E_SIN_KERNEL = 4 * E_SIN_MEASURED
EMULATION = dict(name="emulation", e_sin=lambda ax: (ax + 7.0) * U)
KERNEL = dict(name="kernel", e_sin=lambda ax: np.full_like(ax, E_SIN_KERNEL),
              e_sin_measured=E_SIN_MEASURED, e_sin_const=E_SIN_KERNEL,
              e_sin_from="2026-10-20, MI355X (gfx950), check_sin_term: max |s_got - s_ref| |eb| = 2.954e-06 = 49.6 u over "
                         "296888 elements, at rep 2, ea = 3.7960265, v = 7.6912742 (|x| = 29.2), eb = -0.082545914")


# ---------------------------------------------------------------------------------------------- small helpers
def f16bits(x):
    return np.asarray(x, np.float32).astype(np.float16).view(np.uint16)


def f16vals(b):
    return np.ascontiguousarray(b, dtype=np.uint16).view(np.float16).astype(np.float64)


def f16round(x):
    """float64 -> the nearest fp16 value (rne), as float64"""
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def spacing16(v):
    """the fp16 spacing above |v| (the subnormal spacing 2^-24 below 2^-14)"""
    v = np.abs(np.asarray(v, np.float64))
    e = np.frexp(np.maximum(v, 2.0 ** -140))[1] - 1
    return np.ldexp(1.0, np.maximum(e, -14) - 10)


def x_sentinel(n):
    return np.full(n, X_SENT, np.uint32).view(np.float32)


def s_sentinel(n):
    return np.full(n, S_SENT, np.uint16)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    w = {2: np.uint16, 4: np.uint32}[a.dtype.itemsize]
    return a.view(w) == b.view(w)


def assert_same_bits(got, want, what):
    ok = same_bits(got, want)
    assert ok.all(), (what, int((~ok).sum()), np.argwhere(~ok)[:4].tolist())


# ---------------------------------------------------------------------------------------------- shapes
def conv_shape(taps, dil, pad, Cin, N, Mi, items):
    return dict(T_in=Mi, Cin=Cin, taps=taps, dil=dil, pad=pad, in_stride=1, M=Mi * items, N=N, Cout=N, up=1, crop=0,
                T_out=Mi, items=items)


def convt_shape(up, Cout, crop, T_in, items, Cin=64):
    """transposed conv, kernel 2 up, stride up, as VaeEngine::run_conv sets it (crop = 0: the uncropped length)"""
    return dict(T_in=T_in, Cin=Cin, taps=2, dil=-1, pad=0, in_stride=1, M=(T_in + 1) * items, N=up * Cout, Cout=Cout,
                up=up, crop=crop, T_out=(T_in + 1) * up - 2 * crop, items=items)


def strided_shape(s, Cin, N, T_in, items):
    """encoder conv: kernel 2 s, stride s, pad ceil(s / 2); T_out = ggml_conv_1d's length"""
    taps, pad = 2 * s, (s + 1) // 2
    T_out = (T_in + 2 * pad - (taps - 1) - 1) // s + 1
    return dict(T_in=T_in, Cin=Cin, taps=taps, dil=1, pad=pad, in_stride=s, M=T_out * items, N=N, Cout=N, up=1, crop=0,
                T_out=T_out, items=items)


PLAIN = ((7, 1, 3, 64, 128), (1, 1, 0, 128, 128), (7, 3, 9, 256, 256), (7, 9, 27, 192, 384))
PLAIN_MI = (1, 5, 127, 128, 129, 150)        # 150 x 3 items: tile 1 holds the end of item 0 and the start of item 1
HALO_MI = (1, 5, 53, 54, 55, 128, 129, 150, 300)
FUSE2_GENERIC = ((1, 1, 0, 64), (7, 2, 6, 128))          # (taps, dil, pad, Cin): shapes the halo predicate rejects
FUSE2_GENERIC_MI = (5, 129, 150)
CONVT = ((2, 128, 1), (3, 128, 2), (4, 256, 2), (6, 64, 3), (10, 64, 5), (2, 192, 1), (4, 128, 0))   # (up, Cout, crop)
CONVT_TIN = (1, 2, 37, 128)
STRIDED = ((2, 64, 128), (3, 128, 256), (4, 64, 256), (6, 128, 128), (10, 64, 128))                  # (s, Cin, N)
ITEMS = (1, 3)


def plain_shapes(p):
    return [conv_shape(*p, Mi, it) for Mi in PLAIN_MI for it in ITEMS]


def big_shape():
    """11 M-tiles + 7 rows, two N-tiles: more than GM = 8 M-tiles and a ragged last M-group"""
    return conv_shape(7, 1, 3, 64, 256, 128 * 11 + 7, 1)


def halo_shapes(hd):
    return [conv_shape(7, hd, 3 * hd, 128, 128, Mi, it) for Mi in HALO_MI for it in ITEMS]


def fuse2_generic_shapes(p):
    taps, dil, pad, Cin = p
    return [conv_shape(taps, dil, pad, Cin, 128, Mi, it) for Mi in FUSE2_GENERIC_MI for it in ITEMS]


def convt_shapes(p):
    return [convt_shape(*p, T_in, it, Cin=128 if p[0] == 2 else 64) for T_in in CONVT_TIN for it in ITEMS]


def strided_shapes(p):
    s, Cin, N = p
    return [strided_shape(s, Cin, N, T_in, it) for T_in in (2 * s, 20 * s + 1, 20 * s + s - 1) for it in ITEMS]


def is_halo(c):
    """launch_conv_gemm's predicate for the halo-staged kernel (with ACE_MI_VAE_HALO unset)"""
    return (c["taps"] == 7 and c["Cin"] == 128 and c["N"] == 128 and c["Cout"] == 128 and c["up"] <= 1 and
            c["in_stride"] == 1 and c["T_in"] * c["items"] == c["M"] and c["pad"] == 3 * c["dil"] and c["dil"] in (1, 3, 9))


# ---------------------------------------------------------------------------------------------- the reference
def a_rows(c, Sv):
    """The implicit GEMM's A [M][taps * Cin] from Sv [items][T_in][Cin] (float64), zero rows outside [0, T_in)"""
    Mi = c["M"] // c["items"]
    t = np.arange(Mi)[:, None] * c["in_stride"] + np.arange(c["taps"])[None, :] * c["dil"] - c["pad"]     # [Mi][taps]
    ok = (t >= 0) & (t < c["T_in"])
    A = Sv[:, np.clip(t, 0, c["T_in"] - 1), :] * ok[None, :, :, None]                 # [items][Mi][taps][Cin]
    return A.reshape(c["M"], c["taps"] * c["Cin"]) + 0.0                               # + 0.0: no -0 rows


def out_index(c):
    """(flat payload index [M][N] or -1 where the output is dropped, channel co [N])"""
    Mi = c["M"] // c["items"]
    m, n = np.arange(c["M"])[:, None], np.arange(c["N"])[None, :]
    item, ml = m // Mi, m % Mi
    if c["up"] > 1:
        r, co = n // c["Cout"], n % c["Cout"]
        u = ml * c["up"] + r - c["crop"]
    else:
        co, u = n + 0 * m, ml + 0 * n
    ok = (u >= 0) & (u < c["T_out"])
    o = (item * c["T_out"] + u) * c["Cout"] + co
    return np.where(ok, o, -1), (np.arange(c["N"]) % c["Cout"])


def payload(c):
    return c["items"] * c["T_out"] * c["Cout"]


def buffers(c, o, x_old=None):
    """X0 / S_out0 with guards: NaN sentinels everywhere but x_old ([M][N], by output) at the defined payload words"""
    X0, S0 = x_sentinel(2 * G + payload(c)), s_sentinel(2 * G + payload(c))
    if x_old is not None:
        X0[G + o[o >= 0]] = np.asarray(x_old, np.float32)[o >= 0]
    return X0, S0


def scatter(base, o, vals):
    out = base.copy()
    out[G + o[o >= 0]] = np.asarray(vals)[o >= 0]
    return out


def snake64(v, ea, eb):
    return v + np.sin(ea * v) ** 2 / eb


def run_conv(run, c, S, W, halo=True, **kw):
    return run(S, W, M=c["M"], Cout=c["Cout"], T_out=c["T_out"], taps=c["taps"], dil=c["dil"], pad=c["pad"],
               in_stride=c["in_stride"], up=c["up"], crop=c["crop"], guard=G, halo=halo, **kw)


def sparse_rows(rng, N, taps, Cin, nnz, draw):
    """W [N][taps * Cin] with nnz non-zeros per row: row n's j-th non-zero sits in tap (n + j) mod taps and 8-channel
    chunk (n * nnz + j) mod (Cin / 8), at a random channel of the chunk, so that the rows together touch every tap and
    every chunk of every tap (asserted)."""
    W = np.zeros((N, taps, Cin))
    chunks = Cin // 8
    for n in range(N):
        for j in range(nnz):
            tap, ch = (n + j) % taps, (n * nnz + j + (n // chunks)) % chunks
            W[n, tap, ch * 8 + rng.integers(0, 8)] = draw()
    hit = (W != 0).reshape(N, taps, chunks, 8).any(axis=(0, 3))
    assert hit.all() or N * nnz < taps * chunks, "sparse rows miss a (tap, chunk)"
    return W.reshape(N, taps * Cin)


# ---------------------------------------------------------------------------------------------- (a) exact integers
def _nonzero_int(rng, lim):
    return lambda: float(rng.choice([-1, 1]) * rng.integers(1, lim + 1))


def check_exact(run, c, variant, fused=False, halo=True):
    """Small integers (|S| <= 4, |W| <= 2, bias, old X): every partial sum is an integer below 2^24, so the result equals
    the integer result bit for bit in any summation order, and (asserted on the reference: |result| <= 2048) its fp16
    copy in S_out is exact too.  fused: the first conv's rows are sparse (8 non-zeros of +-1, |S| <= 2), Snake2 is the
    identity in f32 (ea = 1, eb = 2^60: v + sin^2 / eb rounds to v), so y = acc + bias (|y| <= 2048 asserted) and the
    fused result is exact.
    variant 0: resid, store_x and S_out; 1: neither resid nor store_x: X comes back unchanged, S_out = f16(acc + bias);
    2: S_out null: only X changes.  Guards and payload words the operation does not define keep their NaN sentinel."""
    rng = np.random.default_rng(1000 + 7 * c["M"] + 3 * c["N"] + c["taps"] + variant + 100 * c["up"] + c["in_stride"])
    K = c["taps"] * c["Cin"]
    Si = rng.integers(-2, 3, (c["items"], c["T_in"], c["Cin"])) if fused else rng.integers(-4, 5, (c["items"], c["T_in"], c["Cin"]))
    if fused:
        Wi = sparse_rows(rng, c["N"], c["taps"], c["Cin"], 8, _nonzero_int(rng, 1))
    else:
        Wi = rng.integers(-2, 3, (c["N"], K)).astype(np.float64)
    o, co = out_index(c)
    nb = c["N"] if c["up"] <= 1 else c["Cout"]
    bias = rng.integers(-8 if fused else -64, (8 if fused else 64) + 1, nb).astype(np.float64)
    acc = a_rows(c, Si.astype(np.float64)) @ Wi.T
    kw = {}
    if fused:
        y = acc + bias[None, :]
        assert np.abs(y).max() <= 2048
        W2i = rng.integers(-2, 3, (128, 128)).astype(np.float64)
        bias2 = rng.integers(-64, 65, 128).astype(np.float64)
        v = y @ W2i.T + bias2[None, :]
        kw = dict(W2_bits=f16bits(W2i), bias2=bias2, snake2=(np.ones(128), np.full(128, 2.0 ** 60)))
    else:
        v = acc + bias[co][None, :]
    x_old = rng.integers(-512, 513, (c["M"], c["N"])).astype(np.float64)
    if variant != 1:
        v = x_old + v
    assert np.abs(v).max() <= 2048 and np.abs(acc).max() < 2 ** 20
    X0, S0 = buffers(c, o, x_old)
    X, So = run_conv(run, c, f16bits(Si), f16bits(Wi), halo=halo, bias=bias, X0=X0, S_out0=None if variant == 2 else S0,
                     resid=variant != 1, store_x=variant != 1, **kw)
    what = (c, variant, fused, halo)
    assert_same_bits(X, X0 if variant == 1 else scatter(X0, o, v.astype(np.float32)), ("X",) + what)
    if variant != 2:
        assert_same_bits(So, scatter(S0, o, f16bits(v)), ("S_out",) + what)
    return X, So


# ---------------------------------------------------------------------------------------------- (b) index-coded one-hot
def onehot_inputs(c):
    """S words: pairwise distinct normal fp16 words of both signs by linear index (distinct within any 61440 consecutive
    elements = 480 rows of 128 channels, which no row, tap, chunk, item or tile mix-up spans); W row n is one-hot at
    (tap_n, c_n) = (n mod taps, clist[(n / taps) mod len]) with clist = 0, 7, 8, 63, 64, Cin - 1 and a spread."""
    idx = np.arange(c["items"] * c["T_in"] * c["Cin"]) % 61440
    S = ((0x0400 + (idx >> 1)) | ((idx & 1) << 15)).astype(np.uint16).reshape(c["items"], c["T_in"], c["Cin"])
    Cin = c["Cin"]
    clist = [0, 7, 8, 63, 64 % Cin, Cin - 1] + [(37 * j + 5) % Cin for j in range(13)]
    n = np.arange(c["N"])
    tap_n, c_n = n % c["taps"], np.array(clist)[(n // c["taps"]) % len(clist)]
    W = np.zeros((c["N"], c["taps"] * Cin), np.float32)
    W[n, tap_n * Cin + c_n] = 1.0
    return S, f16bits(W), tap_n * Cin + c_n


def check_onehot(run, c):
    """X (store, no bias, no residual) is the f32 value and S_out the very word of S[i][t + tap_n dil - pad][c_n], +0 at
    the sequence edges.  For a halo shape the run is repeated with the generic staging and must give the same arrays."""
    S, W, col = onehot_inputs(c)
    o, _ = out_index(c)
    want = a_rows(c, f16vals(S))[:, col]
    outs = []
    for halo in ((True, False) if is_halo(c) else (True,)):
        X0, S0 = buffers(c, o)
        X, So = run_conv(run, c, S, W, halo=halo, X0=X0, S_out0=S0, store_x=True)
        assert_same_bits(X, scatter(X0, o, want.astype(np.float32)), ("X", c, halo))
        assert_same_bits(So, scatter(S0, o, f16bits(want)), ("S_out", c, halo))
        outs.append((X, So))
    if len(outs) == 2:
        np.testing.assert_array_equal(outs[0][0].view(np.uint32), outs[1][0].view(np.uint32))
        np.testing.assert_array_equal(outs[0][1], outs[1][1])


# ---------------------------------------------------------------------------------------------- (c) random, (d) Snake
def chain_c(Wv):
    """c of the f32 bound per output column: non-zero products of the row + 3.  Any order of correctly rounded f32
    additions of the K exact products rounds at most (non-zero products - 1) times (adding an exact zero does not round),
    then once for the bias and once for the residual: c = K + 3 for a dense row leaves two roundings spare (the Snake's
    last addition uses one)."""
    return (Wv != 0).sum(axis=1) + 3.0


def random_inputs(c, seed, w_sd=0.05):
    rng = np.random.default_rng(seed)
    S = f16bits(rng.standard_normal((c["items"], c["T_in"], c["Cin"])))
    W = f16bits(rng.standard_normal((c["N"], c["taps"] * c["Cin"])) * w_sd)
    nb = c["N"] if c["up"] <= 1 else c["Cout"]
    bias = (rng.standard_normal(nb) * 0.5).astype(np.float32)
    x_old = rng.standard_normal((c["M"], c["N"])).astype(np.float32)
    return rng, S, W, bias, x_old


def check_random(run, c, impl):
    """S ~ N(0, 1), W ~ N(0, 0.05) in fp16, bias, residual and store against float64:
    |X - ref| <= c u (sum |s||w| + |bias| + |x_old|), c = K + 3 (chain_c).  S_out (no Snake) is the fp16 word of the X
    that was stored.  A halo shape also runs with the generic staging: same bits."""
    _, S, W, bias, x_old = random_inputs(c, 2000 + 7 * c["M"] + 3 * c["N"] + c["taps"] + 100 * c["up"] + c["in_stride"])
    o, co = out_index(c)
    A, Wv = a_rows(c, f16vals(S)), f16vals(W)
    b64, x64 = bias.astype(np.float64)[co][None, :], x_old.astype(np.float64)
    ref = x64 + (A @ Wv.T + b64)
    bound = chain_c(Wv)[None, :] * U * (np.abs(A) @ np.abs(Wv).T + np.abs(b64) + np.abs(x64))
    X0, S0 = buffers(c, o, x_old)
    outs, worst = [], 0.0
    for halo in ((True, False) if is_halo(c) else (True,)):
        X, So = run_conv(run, c, S, W, halo=halo, bias=bias, X0=X0, S_out0=S0, resid=True, store_x=True)
        keep = np.ones(X.size, bool)
        keep[G + o[o >= 0]] = False
        assert same_bits(X[keep], X0[keep]).all() and (So[keep] == S0[keep]).all(), ("sentinels", c, halo)
        got = X[G + o[o >= 0]].astype(np.float64)
        ratio = np.abs(got - ref[o >= 0]) / bound[o >= 0]
        worst = max(worst, float(ratio.max()))
        assert ratio.max() <= 1.0, ("X", c, halo, float(ratio.max()))
        assert (So[G + o[o >= 0]] == f16bits(X[G + o[o >= 0]])).all(), ("S_out is not f16(X)", c, halo)
        outs.append((X, So))
    if len(outs) == 2:
        np.testing.assert_array_equal(outs[0][0].view(np.uint32), outs[1][0].view(np.uint32))
        np.testing.assert_array_equal(outs[0][1], outs[1][1])
    return worst


def snake_params(rng, n, ea=(0.5, 4.0), eb=(0.25, 4.0)):
    """ea = exp(alpha), eb = exp(beta), log-uniform in the given ranges (f32, as the loader's expf gives them)"""
    return (np.exp(rng.uniform(math.log(ea[0]), math.log(ea[1]), n)).astype(np.float32),
            np.exp(rng.uniform(math.log(eb[0]), math.log(eb[1]), n)).astype(np.float32))


def snake_bound(v, e_v, ea, eb, impl):
    """(y = v + sin^2(ea v) / eb in float64, bound on |S_out - y|) of a Snake output whose v carries the f32 error e_v:
    |d snake / dv| = |1 + ea sin(2 ea v) / eb| <= 1 + ea / eb everywhere, so the value the implementation rounds is off
    by at most e = e_v (1 + ea / eb) + e_sin / eb, and its fp16 rounding adds half a spacing at that value.  The fp16
    output is compared with the unrounded y: two fp16 words that straddle a rounding boundary differ by a whole
    spacing however small e is, so f16(y) itself cannot be the reference of a half-spacing bound."""
    y = snake64(v, ea, eb)
    e = e_v * (1 + ea / eb) + impl["e_sin"](np.abs(ea * v)) / eb
    return y, e + 0.5 * spacing16(np.abs(y) + e)


def check_snake(run, c, impl):
    """S_out with the Snake epilogue, ea in [0.5, 4], eb in [0.25, 4], |v| <= 8 (asserted; W ~ N(0, 0.03) keeps it there),
    with bias, residual and store, against v64 + sin^2(ea v64) / eb: snake_bound with e_v the bound of check_random."""
    rng, S, W, bias, x_old = random_inputs(c, 3000 + 7 * c["M"] + 3 * c["N"] + c["taps"] + 100 * c["up"] + c["in_stride"], 0.03)
    ea, eb = snake_params(rng, c["Cout"])
    o, co = out_index(c)
    A, Wv = a_rows(c, f16vals(S)), f16vals(W)
    b64, x64 = bias.astype(np.float64)[co][None, :], x_old.astype(np.float64)
    v = x64 + (A @ Wv.T + b64)
    assert np.abs(v).max() <= 8
    e_v = chain_c(Wv)[None, :] * U * (np.abs(A) @ np.abs(Wv).T + np.abs(b64) + np.abs(x64))
    ref, bound = snake_bound(v, e_v, ea.astype(np.float64)[co][None, :], eb.astype(np.float64)[co][None, :], impl)
    X0, S0 = buffers(c, o, x_old)
    worst = 0.0
    outs = []
    for halo in ((True, False) if is_halo(c) else (True,)):
        X, So = run_conv(run, c, S, W, halo=halo, bias=bias, snake=(ea, eb), X0=X0, S_out0=S0, resid=True, store_x=True)
        ratio = np.abs(f16vals(So[G + o[o >= 0]]) - ref[o >= 0]) / bound[o >= 0]
        worst = max(worst, float(ratio.max()))
        assert ratio.max() <= 1.0, ("S_out", c, halo, float(ratio.max()))
        outs.append(So)
    if len(outs) == 2:
        np.testing.assert_array_equal(outs[0], outs[1])
    return worst


def check_snake_exact_v(run, c, impl):
    """The same with v exact (integer S, sparse +-1 rows, bias and old X multiples of 1/8, |v| <= 8): e_v = 0, so the bound
    is half an fp16 spacing + e_sin / eb alone, and the Snake of a neighbouring channel's (ea, eb) lies outside it."""
    rng = np.random.default_rng(3500 + c["M"] + c["taps"])
    Si = rng.integers(-1, 2, (c["items"], c["T_in"], c["Cin"]))
    Wi = sparse_rows(rng, c["N"], c["taps"], c["Cin"], 4, _nonzero_int(rng, 1))
    o, co = out_index(c)
    nb = c["N"] if c["up"] <= 1 else c["Cout"]
    bias = rng.integers(-8, 9, nb) / 8.0
    x_old = rng.integers(-24, 25, (c["M"], c["N"])) / 8.0
    v = x_old + (a_rows(c, Si.astype(np.float64)) @ Wi.T + bias[co][None, :])
    assert np.abs(v).max() <= 8
    ea, eb = snake_params(rng, c["Cout"])
    ref, bound = snake_bound(v, 0.0, ea.astype(np.float64)[co][None, :], eb.astype(np.float64)[co][None, :], impl)
    X0, S0 = buffers(c, o, x_old)
    X, So = run_conv(run, c, f16bits(Si), f16bits(Wi), bias=bias, snake=(ea, eb), X0=X0, S_out0=S0, resid=True, store_x=True)
    assert_same_bits(X, scatter(X0, o, v.astype(np.float32)), ("X", c))
    ratio = np.abs(f16vals(So[G + o[o >= 0]]) - ref[o >= 0]) / bound[o >= 0]
    assert ratio.max() <= 1.0, ("S_out", c, float(ratio.max()))
    return float(ratio.max())


# ---------------------------------------------------------------------------------------------- the sine term itself
def check_sin_term(run, impl):
    """The error of the Snake term s = sin^2(ea v) / eb at f32 resolution, through cancellation: S = 0, no bias, so
    v = the old X, any f32; eb (per channel, f32, of either sign: the arithmetic does not care) is chosen so that
    v + s lands at about +-1.5 * 2^-12, where v + s is exact in f32 (Sterbenz) and fp16 resolves 2^-22.  Then
    S_out - (v + s_ref) = s_got - s_ref up to half that spacing.  Each of the 128 channels has its own (ea, v) with
    ea in [0.5, 4], |v| in [1/16, 8] (|x| = |ea v| up to 32), each of the 128 rows moves v by a few f32 steps.
    Returns max over all elements of (|S_out - ref| - 2^-23) |eb| = the measured e_sin, which must not exceed
    impl.e_sin."""
    c = conv_shape(1, 1, 0, 64, 128, 128, 1)
    S = np.zeros((1, 128, 64), np.uint16)
    W = np.zeros((128, 64), np.uint16)
    o, _ = out_index(c)
    worst, worst_at, total = 0.0, None, 0
    for rep in range(24):
        rng = np.random.default_rng(7000 + rep)
        ea = np.exp(rng.uniform(math.log(0.5), math.log(4.0), 128)).astype(np.float32)
        v0 = np.exp(rng.uniform(math.log(1.0 / 16), math.log(8.0), 128)) * rng.choice([-1.0, 1.0], 128)
        if rep % 4 == 0:                                        # the far end of the argument range
            ea[:64], v0[:64] = np.float32(4.0), np.sign(v0[:64]) * rng.uniform(6.0, 8.0, 64)
        v0 = v0.astype(np.float32)
        s2 = np.sin(ea.astype(np.float64) * v0.astype(np.float64)) ** 2
        target = 1.5 * 2.0 ** -12 * rng.choice([-1.0, 1.0], 128)
        with np.errstate(divide="ignore"):
            eb = (s2 / (target - v0.astype(np.float64))).astype(np.float32)
        usable = np.isfinite(eb) & (np.abs(eb) >= 2.0 ** -6) & (np.abs(eb) <= 16.0)
        eb = np.where(usable, eb, np.float32(1.0)).astype(np.float32)
        v = np.broadcast_to(v0, (128, 128)).copy()
        v = (v.view(np.int32) - np.arange(128, dtype=np.int32)[:, None]).view(np.float32)   # row r: r f32 steps towards zero
        ref = snake64(v.astype(np.float64), ea.astype(np.float64)[None, :], eb.astype(np.float64)[None, :])
        fine = usable[None, :] & (np.abs(ref) >= 2.0 ** -13) & (np.abs(ref) < 2.0 ** -11)
        X0, S0 = buffers(c, o, v)
        _, So = run_conv(run, c, S, W, snake=(ea, eb), X0=X0, S_out0=S0, resid=True)
        got = f16vals(So[G + o.reshape(-1)]).reshape(128, 128)
        err = np.maximum(np.abs(got - ref) - 2.0 ** -23, 0.0) * np.abs(eb.astype(np.float64))[None, :]
        allowed = impl["e_sin"](np.abs(ea.astype(np.float64)[None, :] * v.astype(np.float64)))
        bad = fine & (err > allowed)
        assert not bad.any(), ("sine term", rep, float((err / allowed)[fine].max()), np.argwhere(bad)[:4].tolist())
        total += int(fine.sum())
        if fine.any() and err[fine].max() > worst:
            i = np.argwhere(fine & (err == err[fine].max()))[0]
            worst = float(err[fine].max())
            worst_at = dict(rep=rep, ea=float(ea[i[1]]), v=float(v[i[0], i[1]]), eb=float(eb[i[1]]))
    assert total > 100000, total
    return worst, worst_at, total


# ---------------------------------------------------------------------------------------------- (e) fused k1 conv
FRAGILE_CAP = 0.10


def fused_seed(c):
    return 4000 + 7 * c["M"] + c["taps"] + c["dil"]


def fused_case(c, seed):
    """Inputs and the float64 reference of a fused launch.  First conv: 16 non-zeros ~ N(0, 0.5) per row (sparse_rows), so
    that sum |s||w| stays within a few times |v| and c = 16 + 3 (chain_c); bias ~ N(0, 1); Snake2 with ea in [0.5, 2], eb in
    [2, 4] (inputs chosen so that the fragile share stays under the cap with either implementation's e_sin);
    W2 ~ N(0, 0.05) dense.  Returns everything check_fused needs, with the fragile mask and its share."""
    rng = np.random.default_rng(seed)
    S = f16bits(rng.standard_normal((c["items"], c["T_in"], c["Cin"])))
    W = f16bits(sparse_rows(rng, 128, c["taps"], c["Cin"], 16, lambda: rng.standard_normal() * 0.5))
    bias = rng.standard_normal(128).astype(np.float32)
    ea2, eb2 = snake_params(rng, 128, (0.5, 2.0), (2.0, 4.0))
    W2 = f16bits(rng.standard_normal((128, 128)) * 0.05)
    bias2 = (rng.standard_normal(128) * 0.5).astype(np.float32)
    x_old = rng.standard_normal((c["M"], 128)).astype(np.float32)
    return dict(S=S, W=W, bias=bias, ea2=ea2, eb2=eb2, W2=W2, bias2=bias2, x_old=x_old)


def fused_reference(c, d, impl):
    A, Wv = a_rows(c, f16vals(d["S"])), f16vals(d["W"])
    b1 = d["bias"].astype(np.float64)[None, :]
    v1 = A @ Wv.T + b1
    e_v1 = chain_c(Wv)[None, :] * U * (np.abs(A) @ np.abs(Wv).T + np.abs(b1))
    ea, eb = d["ea2"].astype(np.float64)[None, :], d["eb2"].astype(np.float64)[None, :]
    y = snake64(v1, ea, eb)
    delta = e_v1 * (1 + ea / eb) + impl["e_sin"](np.abs(ea * v1)) / eb
    y16 = f16round(y)
    h = y16.astype(np.float16)
    with np.errstate(over="ignore"):
        up = np.nextafter(h, np.float16(np.inf)).astype(np.float64)
        dn = np.nextafter(h, np.float16(-np.inf)).astype(np.float64)
    dist = np.minimum(0.5 * (y16 + up) - y, y - 0.5 * (y16 + dn))            # to the nearest rounding boundary
    fragile = dist <= delta
    W2v = f16vals(d["W2"])
    b2, x64 = d["bias2"].astype(np.float64)[None, :], d["x_old"].astype(np.float64)
    z = x64 + (y16 @ W2v.T + b2)
    ulp = np.maximum(up - y16, y16 - dn)
    bound = (128 + 3) * U * (np.abs(y16) @ np.abs(W2v).T + np.abs(b2) + np.abs(x64)) + (fragile * ulp) @ np.abs(W2v).T
    return z, bound, float(fragile.mean())


def check_fused(run, c, impl):
    """y16 = f16(Snake2(conv1 + bias)) in float64, z = y16 . W2^T + bias2, then residual and store.  The implementation's
    y16[k] may differ by one fp16 spacing only where the reference's unrounded y lies within delta_k = e_v (1 + ea / eb)
    + e_sin / eb of a rounding boundary (fragile k):
    |X - z_ref| <= (128 + 3) u (sum |y||w2| + |bias2| + |x_old|) + sum_{k fragile} |w2[n][k]| ulp16(y_k).
    At most FRAGILE_CAP of the (row, k) pairs may be fragile (asserted).  S_out (no Snake) is the fp16 word of the X that
    was stored.  A halo shape also runs with the generic staging: same bits.  Returns (worst err / bound, fragile share)."""
    d = fused_case(c, fused_seed(c))
    z, bound, share = fused_reference(c, d, impl)
    assert share <= FRAGILE_CAP, ("fragile share", c, share)
    o, _ = out_index(c)
    X0, S0 = buffers(c, o, d["x_old"])
    outs, worst = [], 0.0
    for halo in ((True, False) if is_halo(c) else (True,)):
        X, So = run_conv(run, c, d["S"], d["W"], halo=halo, bias=d["bias"], W2_bits=d["W2"], bias2=d["bias2"],
                         snake2=(d["ea2"], d["eb2"]), X0=X0, S_out0=S0, resid=True, store_x=True)
        keep = np.ones(X.size, bool)
        keep[G + o.reshape(-1)] = False
        assert same_bits(X[keep], X0[keep]).all() and (So[keep] == S0[keep]).all(), ("sentinels", c, halo)
        got = X[G + o.reshape(-1)].reshape(z.shape)
        ratio = np.abs(got.astype(np.float64) - z) / bound
        worst = max(worst, float(ratio.max()))
        assert ratio.max() <= 1.0, ("X", c, halo, float(ratio.max()))
        assert (So[G + o.reshape(-1)] == f16bits(got).reshape(-1)).all(), ("S_out is not f16(X)", c, halo)
        outs.append((X, So))
    if len(outs) == 2:
        np.testing.assert_array_equal(outs[0][0].view(np.uint32), outs[1][0].view(np.uint32))
        np.testing.assert_array_equal(outs[0][1], outs[1][1])
    return worst, share


# ---------------------------------------------------------------------------------------------- (g) conv_out
CONV_OUT_T = (1, 3, 7, 8, 9, 130)         # 130: 17 strips, the 16-strip workgroup boundary inside a sequence


def conv_out_ref(Sv, Wv):
    """out[i][t][o] = sum_k sum_c W[o][k][c] S[i][t + k - 3][c] in float64, and the same on magnitudes"""
    items, T, _ = Sv.shape
    out, mag = np.zeros((items, T, Wv.shape[0])), np.zeros((items, T, Wv.shape[0]))
    for i in range(items):
        for t in range(T):
            for k in range(7):
                ti = t + k - 3
                if 0 <= ti < T:
                    out[i, t] += Wv[:, k, :] @ Sv[i, ti]
                    mag[i, t] += np.abs(Wv[:, k, :]) @ np.abs(Sv[i, ti])
    return out, mag


def check_conv_out(run, T, items, out_ch):
    """Exact integers (|S|, |W| <= 4) bit for bit; S ~ N(0, 1), W ~ N(0, 0.05) with |got - ref| <= (7 * 128 + 1) u
    sum |s||w|; the guards keep their sentinel in both."""
    rng = np.random.default_rng(5000 + 10 * T + 3 * items + out_ch)
    n = items * T * out_ch
    out0 = x_sentinel(2 * G + n)
    Si, Wi = rng.integers(-4, 5, (items, T, 128)), rng.integers(-4, 5, (out_ch, 7, 128))
    ref, _ = conv_out_ref(Si.astype(np.float64), Wi.astype(np.float64))
    want = out0.copy()
    want[G:G + n] = ref.reshape(-1).astype(np.float32)
    assert_same_bits(run(f16bits(Si), f16bits(Wi), out0, guard=G), want, ("conv_out exact", T, items, out_ch))
    S, W = f16bits(rng.standard_normal((items, T, 128))), f16bits(rng.standard_normal((out_ch, 7, 128)) * 0.05)
    ref, mag = conv_out_ref(f16vals(S), f16vals(W))
    got = run(S, W, out0, guard=G)
    assert same_bits(got[:G], out0[:G]).all() and same_bits(got[G + n:], out0[G + n:]).all(), ("guards", T, items, out_ch)
    ratio = np.abs(got[G:G + n].astype(np.float64) - ref.reshape(-1)) / ((7 * 128 + 1) * U * mag.reshape(-1))
    assert ratio.max() <= 1.0, ("conv_out random", T, items, out_ch, float(ratio.max()))
    return float(ratio.max())


# ---------------------------------------------------------------------------------------------- (h) pack_f16 / to_f16
F16_SPECIALS = np.array([0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -20), -2.0 ** -25, 3e-6,
                         -2.5 * 2.0 ** -24, 1.5 * 2.0 ** -24, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, -(2.0 ** -14 - 2.0 ** -24),
                         1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 1 + 2.0 ** -11 + 2.0 ** -20, 2049.0, 2051.0,
                         65504.0, 65519.996, 65520.0, -65520.0, 1e6, -1e6, np.inf, -np.inf, np.nan, 6.0e-8, 1e-10],
                        np.float32)
PACK_N = 4096 * 256 + 257                 # the grid-stride loop of 4096 x 256 threads makes a second trip


def check_pack(run, rows, C, Cpad):
    """Bit-equal to numpy's astype(float16) (round to nearest even, subnormals kept, overflow to +-inf), NaN stays NaN;
    pad columns are +0.  C == Cpad is to_f16_kernel."""
    rng = np.random.default_rng(6000 + C + Cpad)
    x = rng.standard_normal(rows * C).astype(np.float32) * np.exp(rng.uniform(-20, 12, rows * C)).astype(np.float32)
    at = rng.permutation(rows * C)[:min(rows * C, 40 * len(F16_SPECIALS))]
    x[at] = np.resize(F16_SPECIALS, at.size)
    x[-min(len(F16_SPECIALS), x.size):] = F16_SPECIALS[:min(len(F16_SPECIALS), x.size)]       # the loop's second trip
    x = x.reshape(rows, C)
    got = run(x, Cpad)
    with np.errstate(over="ignore"):
        want = np.zeros((rows, Cpad), np.uint16)
        want[:, :C] = x.astype(np.float16).view(np.uint16)
    nan = np.isnan(x)
    gv = got[:, :C].view(np.float16)
    assert np.isnan(gv[nan]).all(), "a NaN did not stay NaN"
    ok = (got == want)
    ok[:, :C] |= nan
    assert ok.all(), (rows, C, Cpad, np.argwhere(~ok)[:4].tolist())


# ---------------------------------------------------------------------------------------------- the tests themselves
def runners(lib=None):
    """The capi.kernel_* wrappers of the VAE kernels bound to `lib` (None: the GPU self-test library)."""
    import functools
    import types
    from acestep_mi355x import capi
    return types.SimpleNamespace(conv_gemm=functools.partial(capi.kernel_conv_gemm, lib=lib),
                                 conv_out=functools.partial(capi.kernel_conv_out, lib=lib),
                                 pack_f16=functools.partial(capi.kernel_pack_f16, lib=lib))


def _report(name, impl, what, worst):
    print(f"{name} {impl['name']} {what}: worst err/bound {worst:.3f}")


class VaeKernelChecks:
    """The test functions; a test file subclasses this as Test..., sets IMPL and provides the module fixture `k`
    (runners(lib))."""
    IMPL = None

    # -- (a)
    @pytest.mark.parametrize("p", PLAIN)
    def test_exact_plain(self, k, p):
        for i, c in enumerate(plain_shapes(p)):
            check_exact(k.conv_gemm, c, i % 3)

    def test_exact_many_m_tiles(self, k):
        check_exact(k.conv_gemm, big_shape(), 0)

    def test_exact_undefined_rows_keep_sentinel(self, k):
        """T_out two rows longer than the rows of a sequence: payload rows the launch does not define"""
        for hd in (0, 3):
            c = conv_shape(7, 3, 9, 128 if hd else 64, 128, 130, 3)
            c["T_out"] += 2
            for variant in range(3):
                check_exact(k.conv_gemm, c, variant)

    @pytest.mark.parametrize("fused", [False, True])
    @pytest.mark.parametrize("hd", [1, 3, 9])
    def test_exact_halo(self, k, hd, fused):
        for i, c in enumerate(halo_shapes(hd)):
            got = check_exact(k.conv_gemm, c, i % 3, fused=fused)
            ref = check_exact(k.conv_gemm, c, i % 3, fused=fused, halo=False)
            for a, b in zip(got, ref):
                assert (a is None and b is None) or same_bits(a, b).all(), (c, "halo != generic")

    @pytest.mark.parametrize("p", FUSE2_GENERIC)
    def test_exact_fused_generic(self, k, p):
        for i, c in enumerate(fuse2_generic_shapes(p)):
            check_exact(k.conv_gemm, c, i % 3, fused=True)

    @pytest.mark.parametrize("p", CONVT)
    def test_exact_transposed(self, k, p):
        for i, c in enumerate(convt_shapes(p)):
            check_exact(k.conv_gemm, c, i % 3)

    @pytest.mark.parametrize("p", STRIDED)
    def test_exact_strided(self, k, p):
        for i, c in enumerate(strided_shapes(p)):
            check_exact(k.conv_gemm, c, i % 3)

    # -- (b)
    @pytest.mark.parametrize("hd", [1, 3, 9])
    def test_onehot_halo(self, k, hd):
        for c in halo_shapes(hd):
            check_onehot(k.conv_gemm, c)

    @pytest.mark.parametrize("p", PLAIN)
    def test_onehot_plain(self, k, p):
        for c in plain_shapes(p):
            check_onehot(k.conv_gemm, c)

    def test_onehot_many_m_tiles(self, k):
        check_onehot(k.conv_gemm, big_shape())

    @pytest.mark.parametrize("p", STRIDED)
    def test_onehot_strided(self, k, p):
        for c in strided_shapes(p):
            check_onehot(k.conv_gemm, c)

    # -- (c), (f)
    @pytest.mark.parametrize("p", PLAIN)
    def test_random_plain(self, k, p):
        _report("conv_gemm random", self.IMPL, f"plain {p}", max(check_random(k.conv_gemm, c, self.IMPL) for c in plain_shapes(p)))

    def test_random_many_m_tiles(self, k):
        _report("conv_gemm random", self.IMPL, "11 M-tiles + 7", check_random(k.conv_gemm, big_shape(), self.IMPL))

    @pytest.mark.parametrize("hd", [1, 3, 9])
    def test_random_halo_equals_generic(self, k, hd):
        _report("conv_gemm random", self.IMPL, f"halo {hd}", max(check_random(k.conv_gemm, c, self.IMPL) for c in halo_shapes(hd)))

    @pytest.mark.parametrize("p", CONVT)
    def test_random_transposed(self, k, p):
        _report("conv_gemm random", self.IMPL, f"transposed {p}", max(check_random(k.conv_gemm, c, self.IMPL) for c in convt_shapes(p)))

    @pytest.mark.parametrize("p", STRIDED)
    def test_random_strided(self, k, p):
        _report("conv_gemm random", self.IMPL, f"strided {p}", max(check_random(k.conv_gemm, c, self.IMPL) for c in strided_shapes(p)))

    # -- (d)
    def test_snake_epilogue(self, k):
        shapes = ([conv_shape(7, 1, 3, 64, 128, 150, 3), conv_shape(7, 3, 9, 256, 256, 129, 1), convt_shape(2, 192, 1, 37, 3, 128),
                   convt_shape(10, 64, 5, 37, 1), strided_shape(4, 64, 256, 81, 3)] +
                  [conv_shape(7, hd, 3 * hd, 128, 128, Mi, it) for hd in (1, 3, 9) for Mi, it in ((55, 3), (300, 1))])
        _report("conv_gemm snake", self.IMPL, "S_out", max(check_snake(k.conv_gemm, c, self.IMPL) for c in shapes))

    def test_snake_epilogue_exact_v(self, k):
        shapes = [conv_shape(7, 1, 3, 64, 128, 150, 3), conv_shape(7, 9, 27, 128, 128, 129, 3), convt_shape(6, 64, 3, 37, 3)]
        _report("conv_gemm snake", self.IMPL, "exact v", max(check_snake_exact_v(k.conv_gemm, c, self.IMPL) for c in shapes))

    def test_sine_term(self, k):
        worst, at, total = check_sin_term(k.conv_gemm, self.IMPL)
        print(f"conv_gemm sine term {self.IMPL['name']}: max |s_got - s_ref| |eb| = {worst:.3e} = {worst / U:.1f} u over "
              f"{total} elements, at {at}")
        if self.IMPL is KERNEL:
            assert E_SIN_KERNEL < 2.0 ** -14, "the Snake's sine error is no longer far below the fp16 rounding"

    # -- (e), (f)
    @pytest.mark.parametrize("hd", [1, 3, 9])
    def test_fused_halo_equals_generic(self, k, hd):
        r = [check_fused(k.conv_gemm, c, self.IMPL) for c in halo_shapes(hd)]
        _report("conv_gemm fused", self.IMPL, f"halo {hd}, largest fragile share {max(s for _, s in r):.4f}", max(w for w, _ in r))

    @pytest.mark.parametrize("p", FUSE2_GENERIC)
    def test_fused_generic(self, k, p):
        r = [check_fused(k.conv_gemm, c, self.IMPL) for c in fuse2_generic_shapes(p)]
        _report("conv_gemm fused", self.IMPL, f"generic {p}, largest fragile share {max(s for _, s in r):.4f}", max(w for w, _ in r))

    def test_fused_fragile_share_under_cap_for_both_implementations(self, k):
        """the reference alone, no launch: the cap holds with the kernel's e_sin and with the emulation's"""
        shapes = [c for hd in (1, 3, 9) for c in halo_shapes(hd)] + [c for p in FUSE2_GENERIC for c in fuse2_generic_shapes(p)]
        for impl in (KERNEL, EMULATION):
            shares = [fused_reference(c, fused_case(c, fused_seed(c)), impl)[2] for c in shapes]
            print(f"conv_gemm fused, e_sin of the {impl['name']}: largest fragile share {max(shares):.4f}")
            assert max(shares) <= FRAGILE_CAP

    # -- (g)
    @pytest.mark.parametrize("out_ch", [1, 2])
    def test_conv_out(self, k, out_ch):
        _report("conv_out", self.IMPL, f"out_ch {out_ch}",
                max(check_conv_out(k.conv_out, T, it, out_ch) for T in CONV_OUT_T for it in ITEMS))

    # -- (h)
    @pytest.mark.parametrize("rows,C,Cpad", [(1, PACK_N, PACK_N), (7, 5, 5), (16389, 2, 64), (7, 5, 8), (3, 64, 64)])
    def test_pack_f16(self, k, rows, C, Cpad):
        check_pack(k.pack_f16, rows, C, Cpad)

    # -- refused arguments
    def test_entries_refuse_bad_arguments(self, k):
        """What launch_conv_gemm refuses comes back as the error status (1), what the entry cannot size a buffer from as
        INVALID_ARG (2); X and S_out are untouched."""
        def call(status, c, fused=False, guard=G, **over):
            c = dict(c, **over)
            S = np.ones((c["items"], c["T_in"], c["Cin"]), np.uint16)
            W = np.ones((c["N"], c["taps"] * c["Cin"]), np.uint16)
            X0, S0 = x_sentinel(2 * guard + payload(c)), s_sentinel(2 * guard + payload(c))
            kw = dict(W2_bits=np.zeros((c["Cout"], c["Cout"]), np.uint16), snake2=(np.ones(c["N"]), np.ones(c["N"]))) if fused else {}
            with pytest.raises(RuntimeError, match=f"status={status}") as e:
                k.conv_gemm(S, W, M=c["M"], Cout=c["Cout"], T_out=c["T_out"], taps=c["taps"], dil=c["dil"], pad=c["pad"],
                            in_stride=c["in_stride"], up=c["up"], crop=c["crop"], guard=guard, X0=X0, S_out0=S0,
                            store_x=True, **kw)
            assert same_bits(e.value.X, X0).all() and (e.value.S_out == S0).all(), ("a refused call wrote", c)
        base = conv_shape(7, 1, 3, 64, 128, 20, 2)
        call(1, conv_shape(7, 1, 3, 96, 128, 20, 2))                        # Cin = 96
        call(1, conv_shape(7, 1, 3, 64, 192, 20, 2))                        # N = 192
        call(1, convt_shape(64, 6, 0, 5, 1))                                # Cout = 6 (N = 384)
        call(1, base, M=41)                                                 # M not divisible by items
        call(1, conv_shape(7, 1, 3, 128, 256, 20, 2), fused=True)           # W2 with N = 256
        call(1, base, Cout=64)                                              # N != Cout
        call(2, base, guard=2)                                              # a guard that breaks the 16-byte accesses
        call(2, base, taps=0)
        with pytest.raises(RuntimeError, match="status=2"):
            k.conv_out(np.zeros((1, 4, 128), np.uint16), np.zeros((3, 7, 128), np.uint16), np.zeros(12, np.float32))
        with pytest.raises(RuntimeError, match="status=2"):
            k.pack_f16(np.zeros((2, 8), np.float32), 4)
