"""Shared by tests/test_gpu_attn_probs.py (kernels/attn_probs.hip through the self-test library) and
tests/test_attn_probs_cpu.py (its host restatement kernels/attn_probs_host.h through the host library): shapes, input
builders, the float64 reference written from the definition in csrc/kernels.h (launch_attn_probs) on the fp16-rounded
operands, the bound, and one check_* function per property.  Every check takes the callable that runs the kernel
(capi.kernel_attn_probs bound to a library).

The operation: for every listed head h, with KV head h // (Hq // Hkv),
    P[q][k] = exp(s - max_k s) / sum_k exp(s - max_k s),  s = scale * (q . k) + (0 | -inf by the key mask),
q and k rounded to fp16 (the hi planes), f32 accumulate; a masked key is exactly 0, a row without a key all zeros.

The bound (u = 2^-24, the unit roundoff of f32; T = ceil(nk / 64) key tiles).  The operands are fp16 values, so every
product is exact in f32 and the reference and the kernel multiply the same numbers.
  score:  128 additions (the MFMA chain, or the host's index-order chain) and the scale multiply move s_k by at most
          e_k = 129 u A_k, A_k = scale sum_d |q_d| |k_d|.
  exponent: s_k - max is rounded once more: u D, D = (max - min of the row's unmasked scores) + 2 max_k e_k.
  numerator: exp(.) carries the exponent's error e_k + u D and the device exponential's own relative error E_EXP.
  denominator: the same per term (at most max_k e_k + u D + E_EXP, a weighted mean of the terms' errors), and the sum:
          the kernel's lanes keep a running sum that is rescaled by exp(old max - new max) once per further tile and
          once more when the 16 lanes of a row merge -- T more factors, each E_EXP + u (its multiply) + u D (its
          argument) -- and the additions: 4 T in a lane's chain + 4 in the merge, nk - 1 in the host's, so max(nk, 4 T + 4) u.
  division: u.
  rho_k = (e_k + u D + E_EXP) + (max e + u D + E_EXP) + T (E_EXP + u + u D) + max(nk, 4 T + 4) u + u, and
  |P_got - P_ref| <= P_ref expm1(rho_k (1 + 2^-10)) + 2^-149  (the factor covers the second-order terms of the
  quotient, the constant a subnormal result).  A row's sum is within sum_k of that of 1.

E_EXP is measured, not derived (check_exp_term): the largest relative error of exp as the kernel's outputs show it,
E_EXP = 4 x that maximum (the margin the Snake epilogue's sine term got, tests/vae_kernel_cases.py)."""
import math

import numpy as np
import pytest

U = 2.0 ** -24
HQ, HKV, D = 4, 2, 128
NQ = (1, 17, 128, 130)            # one row; a ragged 16-row block; exactly one workgroup; a second workgroup of 2 rows
NK = (1, 63, 64, 65, 130)         # either side of the 64-key tile; three tiles with a ragged last one
BATCH = (1, 2)
HEAD_LISTS = ([0], [1, 0, 3], [3, 3])   # out of order with two heads of one KV head; a duplicate
SHAPES = [(nq, nk, B) for nq in NQ for nk in NK for B in BATCH]
SENT = 0x7FC5A5A5                 # NaN sentinel word the output holds before the launch

# check_exp_term's maximum on the MI355X (gfx950), 2026-10-20: 1.4415e-07 = 2.42 u at a = 1.0625, over 1024 arguments
# in (-16, 0] (the two output roundings of the quotient it is read from included); the host restatement's libm expf
# shows 1.3049e-07 = 2.19 u the same way
E_EXP_MEASURED = 1.4415e-7
E_EXP = 4 * E_EXP_MEASURED


def f16(x):
    """float -> the nearest fp16 value, as float32 (what the prep kernel's hi plane holds)"""
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def sentinel(shape):
    return np.full(shape, SENT, np.uint32).view(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def masks(nk, B):
    """[B][nk] int32: one key masked mid-tile and a masked tail, different per item; None at B = 1 with nk < 3"""
    m = np.ones((B, nk), np.int32)
    for b in range(B):
        if nk > 2:
            m[b, nk // 2 - b] = 0
        if nk > 4:
            m[b, nk - 1 - b:] = 0
    return m


def reference(q, k, heads, mask, scale):
    """float64 P [n_heads][B][nq][nk] of fp16-exact q [B][nq][HQ*D], k [B][nk][HKV*D], and its bound (module docstring)"""
    q = np.asarray(q, np.float64).reshape(q.shape[0], q.shape[1], HQ, D)
    k = np.asarray(k, np.float64).reshape(k.shape[0], k.shape[1], HKV, D)
    B, nq, nk = q.shape[0], q.shape[1], k.shape[1]
    sc = float(np.float32(scale))
    T = -(-nk // 64)
    P = np.zeros((len(heads), B, nq, nk))
    bound = np.zeros_like(P)
    for i, h in enumerate(heads):
        for b in range(B):
            qh, kh = q[b, :, h], k[b, :, h // (HQ // HKV)]
            s = sc * (qh @ kh.T)
            e = 129 * U * sc * (np.abs(qh) @ np.abs(kh).T)
            ok = np.ones(nk, bool) if mask is None else np.asarray(mask)[b] != 0
            if not ok.any():
                continue
            s, e = s[:, ok], e[:, ok]
            mx = s.max(axis=1, keepdims=True)
            ex = np.exp(s - mx)
            p = ex / ex.sum(axis=1, keepdims=True)
            emax = e.max(axis=1, keepdims=True)
            Dr = (mx - s.min(axis=1, keepdims=True)) + 2 * emax
            rho = (e + U * Dr + E_EXP) + (emax + U * Dr + E_EXP) + T * (E_EXP + U + U * Dr) + max(nk, 4 * T + 4) * U + U
            P[i, b][:, ok] = p
            bound[i, b][:, ok] = p * np.expm1(rho * (1 + 2.0 ** -10)) + 2.0 ** -149
    return P, bound


def random_inputs(nq, nk, B, seed):
    rng = np.random.default_rng(seed)
    return f16(1.5 * rng.standard_normal((B, nq, HQ * D))), f16(rng.standard_normal((B, nk, HKV * D)))


def _report(what, worst):
    print(f"attn_probs {what}: worst err / bound = {worst:.3f}")


# ---------------------------------------------------------------------------------------------- checks
def check_zero_q(run, nq, nk, B, heads):
    """all-zero Q: every score is 0, exp(0) = 1, the sum is the integer count: P = f32(1 / n_unmasked) bit for bit,
    masked keys exactly +0; the sentinel-filled output is written everywhere (and nowhere else: the entry fails then)"""
    rng = np.random.default_rng(nq * 1000 + nk)
    q = np.zeros((B, nq, HQ * D), np.float32)
    k = f16(rng.standard_normal((B, nk, HKV * D)))
    for mask in ([None] if nk < 3 else [None, masks(nk, B)]):
        got = run(q, k, HQ, HKV, heads, kmask=mask, out0=sentinel((len(heads), B, nq, nk)))
        want = np.zeros_like(got)
        for b in range(B):
            ok = np.ones(nk, bool) if mask is None else mask[b] != 0
            want[:, b][:, :, ok] = np.float32(1.0) / np.float32(ok.sum())
        assert (bits(got) == bits(want)).all(), (nq, nk, B, heads, np.argwhere(bits(got) != bits(want))[:4].tolist())


def check_fully_masked(run, nq, nk, B, heads):
    """an item whose keys are all masked is all zeros (not NaN); the other item is unaffected"""
    q, k = random_inputs(nq, nk, B, 7)
    mask = np.ones((B, nk), np.int32)
    mask[B - 1] = 0
    got = run(q, k, HQ, HKV, heads, kmask=mask, out0=sentinel((len(heads), B, nq, nk)))
    assert (bits(got[:, B - 1]) == 0).all()
    if B > 1:
        ref, bound = reference(q, k, heads, mask, 1 / math.sqrt(D))
        assert (np.abs(got[:, 0] - ref[:, 0]) <= bound[:, 0]).all()


def onehot_inputs(nq, nk, B):
    """key k of KV head g, item b: 4 at dim (k + 11 g + 17 b) % 128 (2 for keys >= 128, which share a dim with key
    k - 128); query q of head h, item b: 4 at the dim of its target key t = (7 q + 3 h + 5 b) % min(nk, 128) in ITS KV
    head and item -- another KV head, another item or a transposed write moves the maximum"""
    q = np.zeros((B, nq, HQ, D), np.float32)
    k = np.zeros((B, nk, HKV, D), np.float32)
    t = np.zeros((B, nq, HQ), np.int64)
    for b in range(B):
        for g in range(HKV):
            for key in range(nk):
                k[b, key, g, (key + 11 * g + 17 * b) % D] = 4.0 if key < D else 2.0
        for h in range(HQ):
            for r in range(nq):
                t[b, r, h] = (7 * r + 3 * h + 5 * b) % min(nk, D)
                q[b, r, h, (t[b, r, h] + 11 * (h // (HQ // HKV)) + 17 * b) % D] = 4.0
    return q.reshape(B, nq, HQ * D), k.reshape(B, nk, HKV * D), t


def check_onehot(run, nq, nk, B, heads):
    q, k, t = onehot_inputs(nq, nk, B)
    got = run(q, k, HQ, HKV, heads, scale=1.0, out0=sentinel((len(heads), B, nq, nk)))
    for i, h in enumerate(heads):
        assert (got[i].argmax(axis=-1) == t[:, :, h]).all(), (nq, nk, B, h)
    ref, bound = reference(q, k, heads, None, 1.0)
    assert (np.abs(got - ref) <= bound).all()


def check_random(run, nq, nk, B, heads):
    """random fp16-representable operands against the float64 softmax under the derived bound; row sums; two runs"""
    q, k = random_inputs(nq, nk, B, nq * 131 + nk * 7 + B)
    mask = masks(nk, B) if (B == 2 and nk > 2) else None
    got = run(q, k, HQ, HKV, heads, kmask=mask, out0=sentinel((len(heads), B, nq, nk)))
    again = run(q, k, HQ, HKV, heads, kmask=mask)
    assert (bits(got) == bits(again)).all(), "two runs differ"
    ref, bound = reference(q, k, heads, mask, 1 / math.sqrt(D))
    assert np.isfinite(got).all()
    assert (bits(got[ref == 0]) == 0).all(), "a masked key is not exactly +0"
    ratio = np.abs(got.astype(np.float64) - ref) / np.where(ref > 0, bound, 1.0)
    rows = np.abs(got.astype(np.float64).sum(axis=-1) - 1.0) / bound.sum(axis=-1)
    worst = float(max(ratio[ref > 0].max(), rows.max()))
    assert worst <= 1.0, (nq, nk, B, heads, worst)
    return worst


def check_exp_term(run):
    """E_EXP by a quotient: two keys with the exact scores 0 and -a (one-hot operands, scale 1): P1 / P0 = exp(-a) as
    the kernel computed it, times the two roundings of the outputs.  a = j / 64, j < 1024: arguments in (-16, 0]."""
    a = np.arange(1024, dtype=np.float32) / 64
    q = np.zeros((1, 1024, HQ * D), np.float32)
    q[0, :, 0] = a
    k = np.zeros((1, 2, HKV * D), np.float32)
    k[0, 1, 0] = -1.0
    got = run(q, k, HQ, HKV, [0], scale=1.0).astype(np.float64)[0, 0]
    rel = np.abs(got[:, 1] / got[:, 0] / np.exp(-a.astype(np.float64)) - 1.0)
    j = int(rel.argmax())
    print(f"attn_probs exp term: max rel error {rel.max():.4e} = {rel.max() / U:.2f} u at a = {a[j]}; "
          f"E_EXP_MEASURED = {E_EXP_MEASURED:.4e}, E_EXP = {E_EXP:.4e}")
    assert rel.max() <= E_EXP, (rel.max(), E_EXP)
    return float(rel.max())


def runner(lib=None):
    from acestep_mi355x import capi
    return lambda *a, **kw: capi.kernel_attn_probs(*a, lib=lib, **kw)


class AttnProbsChecks:
    """the test classes of both files: `run` is a module fixture returning the kernel's runner"""

    @pytest.mark.parametrize("nq,nk,B", SHAPES)
    def test_zero_q_is_uniform_bit_exact(self, run, nq, nk, B):
        for heads in HEAD_LISTS:
            check_zero_q(run, nq, nk, B, heads)

    @pytest.mark.parametrize("nq,nk,B", [(17, 65, 1), (130, 130, 2), (1, 1, 2)])
    def test_fully_masked_item_is_zero(self, run, nq, nk, B):
        for heads in HEAD_LISTS:
            check_fully_masked(run, nq, nk, B, heads)

    @pytest.mark.parametrize("nq,nk,B", SHAPES)
    def test_onehot_maximum_lands_on_its_key(self, run, nq, nk, B):
        for heads in HEAD_LISTS:
            check_onehot(run, nq, nk, B, heads)

    @pytest.mark.parametrize("nq,nk,B", SHAPES)
    def test_random_within_derived_bound(self, run, nq, nk, B):
        worst = max(check_random(run, nq, nk, B, heads) for heads in HEAD_LISTS)
        _report(f"random nq={nq} nk={nk} B={B}", worst)

    def test_exp_term(self, run):
        check_exp_term(run)

    def test_longer_head_list_than_one_launch(self, run):
        """more listed heads than one launch carries by value (ATTN_PROBS_MAX_HEADS = 32): the second launch's maps"""
        heads = [(3 * i) % HQ for i in range(35)]
        q, k = random_inputs(17, 65, 1, 3)
        got = run(q, k, HQ, HKV, heads, out0=sentinel((35, 1, 17, 65)))
        one = {h: run(q, k, HQ, HKV, [h])[0] for h in set(heads)}
        for i, h in enumerate(heads):
            assert (bits(got[i]) == bits(one[h])).all(), i

    def test_bad_head_is_refused(self, run):
        q, k = random_inputs(1, 1, 1, 0)
        with pytest.raises(RuntimeError):
            run(q, k, HQ, HKV, [HQ])
