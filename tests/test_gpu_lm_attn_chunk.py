"""GPU test of the LM chunk attention (kernels/lm_attn_chunk.hip) through ace_mi_kernel_lm_attention_chunk: float64 NumPy
on the same fp16 cache bytes and f32 Q.  The bound is the decode attention's (tests/lm_kernel_cases.py check_attention,
KERNEL's chain constant at the row's own key count): the operand precision is the same, the fp16 hi + lo splits of Q and
P add about 2^-22.  Masked slots and every slot >= past + n hold fp16 NaN in K and V."""
import numpy as np
import pytest

import lm_kernel_cases as kc

pytestmark = pytest.mark.gpu
D, F16_NAN = 128, 0x7E00
SCALE = np.float32(1.0 / np.sqrt(D))

# (hq, hkv, n, past, B, out_type, mask): rep 1 / 2 / 4; n across the 8-, 16- and 32-token row tiles; past across a wave's
# 64 keys, the 256-key range and a two-range merge; 'pad260' masks the whole first range, 'all' every key of sequence 0
CASES = [(1, 1, 1, 1, 1, 0, "none"), (4, 2, 2, 63, 2, 1, "pad3"), (8, 2, 17, 64, 1, 0, "none"),
         (4, 2, 33, 255, 2, 0, "pad3"), (2, 2, 33, 256, 1, 1, "none"), (8, 2, 33, 300, 2, 0, "all"),
         (4, 2, 17, 300, 2, 1, "pad260"), (4, 1, 2, 255, 1, 0, "none"), (4, 2, 1, 256, 2, 0, "pad3"),
         (2, 2, 17, 1, 1, 0, "none"), (8, 2, 1, 300, 1, 1, "none"), (4, 2, 33, 63, 1, 0, "all")]


def inputs(hq, hkv, n, past, B, mask):
    rng = np.random.default_rng(7000 + 97 * past + 13 * n + hq + B)
    cap = past + n + 3
    q = (rng.standard_normal((B, n, hq, D)) * 4.0).astype(np.float32)
    k = rng.standard_normal((B, hkv, cap, D)).astype(np.float16).view(np.uint16)
    v = rng.standard_normal((B, hkv, cap, D)).astype(np.float16).view(np.uint16)
    km = np.ones((B, cap), np.int32)
    if mask.startswith("pad"):
        km[B - 1, :min(int(mask[3:]), past)] = 0
    elif mask == "all":
        km[0] = 0
    off = np.broadcast_to((km == 0)[:, None, :, None], k.shape).copy()
    off[:, :, past + n:] = True
    return q, np.where(off, F16_NAN, k).astype(np.uint16), np.where(off, F16_NAN, v).astype(np.uint16), km


def reference(q, k, v, km, past):
    """(ref, sum_j p_j |v_jd|, delta_s, chain constant) per row [B][n][hq]; a row without a visible key gives 0"""
    B, n, hq, _ = q.shape
    rep = hq // k.shape[1]
    kf, vf = kc.vals(k, 1), kc.vals(v, 1)
    ref, pv = np.zeros(q.shape), np.zeros(q.shape)
    delta, c = np.zeros(q.shape[:3] + (1,)), np.zeros(q.shape[:3] + (1,))
    for b in range(B):
        for t in range(n):
            on = np.flatnonzero(km[b, :past + t + 1])
            c[b, t] = kc.KERNEL["attn_c"](past + t + 1)
            for h in range(hq if on.size else 0):
                qv = q[b, t, h].astype(np.float64)
                s = float(SCALE) * (kf[b, h // rep, on] @ qv)
                p = np.exp(s - s.max())
                p /= p.sum()
                ref[b, t, h], pv[b, t, h] = p @ vf[b, h // rep, on], p @ np.abs(vf[b, h // rep, on])
                delta[b, t, h] = 16 * kc.U * float(SCALE) * np.max(np.abs(kf[b, h // rep, on]) @ np.abs(qv))
    return ref, pv, delta, c


@pytest.mark.parametrize("hq,hkv,n,past,B,out_type,mask", CASES)
def test_chunk_attention_against_float64(hq, hkv, n, past, B, out_type, mask):
    from acestep_mi355x import capi
    q, k, v, km = inputs(hq, hkv, n, past, B, mask)
    got = capi.kernel_lm_attention_chunk(q, k, v, km, past, float(SCALE), out_type=out_type)
    again = capi.kernel_lm_attention_chunk(q, k, v, km, past, float(SCALE), out_type=out_type)
    assert got.tobytes() == again.tobytes()
    ref, pv, delta, c = reference(q, k, v, km, past)
    gv = kc.vals(got, out_type)
    assert np.isfinite(gv).all()
    dead = ~np.array([[km[b, :past + t + 1].any() for t in range(n)] for b in range(B)])
    assert (got[dead] == 0).all(), "a row without a visible key is not +0"
    e = (c * kc.U + 2 * delta) * pv
    bound = e + kc.half_ulp(np.abs(ref) + e, out_type)
    err = np.abs(gv - ref)
    print(f"chunk attention hq {hq} hkv {hkv} n {n} past {past} B {B} {mask}: worst err/bound {np.max(err / bound):.3f}")
    assert (err <= bound).all()
    if n == 1 and mask == "none":   # the decode kernel on the same arrays: each within `bound` of the same reference
        dec = capi.kernel_lm_attention(q[:, 0], k, v, km, past + 1, float(SCALE), out_type=out_type)
        assert (np.abs(kc.vals(dec, out_type) - gv[:, 0]) <= 2 * bound[:, 0]).all()
