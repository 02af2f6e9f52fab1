"""Shared by tests/test_gpu_lm_attn_shared.py (lm_attn_shared_kernel of kernels/lm_decode.hip through the self-test
library) and tests/test_lm_attn_shared_cpu.py (kernels/lm_attn_shared_host.h through the LM host library): decode
attention over a cache whose sequences come in G groups of S that share positions [0, n_shared).

Each case is checked twice: the output words equal kernel_lm_attention's on the same arrays bit for bit, and they pass
lm_kernel_cases.check_attention against the float64 reference with that helper's bound."""
import numpy as np
import pytest

import lm_kernel_cases as lk

# (G, S, hq, hkv, n_shared, nk, mask, out_type).  n_shared / 256 ranges are shared: one (256..511) or two (512); nk puts
# a one-key range (257, 513, 769), a straddling range (300, 511) or a longer tail (700) behind them.  REP = hq / hkv =
# 4 serves 4 items per workgroup, so S = 6 and 8 run two chunks (6: a ragged one), S = 3, 5, 7 a ragged single chunk.
# Masks: 'pad3' / 'pad256' left padding of the last group (256: a wholly masked shared range, m = -inf into the
# merge), 'tail': zeros behind n_shared in one sequence only.  The last two rows have no shared range (n_shared < 256)
# or a single range (nk <= 256): launch_lm_attention itself.
CASES = (
    (1, 2, 2, 2, 256, 257, "none", 0),
    (2, 3, 4, 2, 300, 301, "pad3", 1),
    (2, 4, 4, 1, 511, 700, "tail", 0),
    (1, 8, 4, 1, 512, 513, "none", 1),
    (1, 8, 2, 2, 512, 769, "pad256", 0),
    (2, 4, 4, 2, 512, 769, "pad256", 1),
    (1, 5, 4, 2, 256, 300, "tail", 1),
    (1, 6, 4, 1, 300, 301, "pad3", 0),
    (1, 7, 2, 2, 512, 513, "none", 0),
    (2, 4, 4, 2, 255, 400, "pad3", 0),
    (2, 2, 4, 1, 199, 200, "none", 1),
)


def case_id(c):
    return "G%dS%d-hq%dkv%d-sh%d-nk%d-%s-out%d" % c


def inputs(case):
    """attn_inputs for G sequences, each repeated S times; then positions >= n_shared and every q drawn per sequence"""
    G, S, hq, hkv, n_shared, nk, mask, _ = case
    rng = np.random.default_rng(list(case[:6]))
    _, kc, vc, km = lk.attn_inputs(rng, G, hq, hkv, nk, "none" if mask == "tail" else mask)
    kc, vc, km = (np.repeat(a, S, axis=0) for a in (kc, vc, km))
    B = G * S
    fresh = (B, hkv, nk - n_shared, lk.D)
    kc[:, :, n_shared:nk] = rng.standard_normal(fresh).astype(np.float16).view(np.uint16)
    vc[:, :, n_shared:nk] = rng.standard_normal(fresh).astype(np.float16).view(np.uint16)
    if mask == "tail":
        off = n_shared + np.arange(0, nk - n_shared - 1, 3)
        km[B - 1, off] = 0
        kc[B - 1, :, off] = vc[B - 1, :, off] = np.float16(lk.BIG).view(np.uint16)
    q = (rng.standard_normal((B, hq, lk.D)) * 4.0).astype(np.float32)
    return q, kc, vc, km


def run_case(k, impl, case):
    S, n_shared, nk, out_type = case[1], case[4], case[5], case[7]
    q, kc, vc, km = inputs(case)
    got = []

    def shared(*a, out_type):
        got.append(k.attention_shared(*a, n_shared, S, out_type=out_type))
        return got[0]
    r = lk.check_attention(shared, out_type, q, kc, vc, km, nk, impl, case)
    print(f"lm_attention_shared {impl['name']} {case_id(case)}: worst err/bound {r:.3f}")
    want = k.attention(q, kc, vc, km, nk, float(lk.ATTN_SCALE), out_type=out_type)
    same = got[0] == want
    assert same.all(), (case, np.argwhere(~same)[:4].tolist())


def run_refusals(k):
    """INVALID_ARG (status 2): more than 8 sequences, S < 1, the newest key shared (n_shared >= nk), a GQA ratio that
    no items x REP <= 16 tile covers.  A batch that is not G * S cannot be expressed in the entry's arguments: the
    wrapper refuses it."""
    G, S, hq, hkv, n_shared, nk = 2, 4, 4, 2, 256, 300
    q, kc, vc, km = inputs((G, S, hq, hkv, n_shared, nk, "none", 0))
    sc = float(lk.ATTN_SCALE)
    q8 = np.zeros((8, 8, lk.D), np.float32)
    bad = [
        lambda: k.attention_shared(q, kc, vc, km, nk, sc, nk, S),
        lambda: k.attention_shared(q, kc, vc, km, 200, sc, 512, S),
        lambda: k.attention_shared(q, kc, vc, km, nk, sc, -1, S),
        lambda: k.attention_shared(q, kc, vc, km, nk, sc, n_shared, 0),
        lambda: k.attention_shared(np.repeat(q, 2, 0), np.repeat(kc, 2, 0), np.repeat(vc, 2, 0), np.repeat(km, 2, 0), nk, sc,
                                   n_shared, S),
        lambda: k.attention_shared(q8, kc[:, :1], vc[:, :1], km, nk, sc, n_shared, S),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(RuntimeError, match="status=2"):
            f()
            pytest.fail(f"bad call {i} was accepted")
    with pytest.raises(ValueError, match="whole number of groups"):
        k.attention_shared(q, kc, vc, km, nk, sc, n_shared, 3)


def runners(lib=None):
    """capi.kernel_lm_attention and kernel_lm_attention_shared bound to `lib` (None: the GPU self-test library)"""
    import functools
    import types
    from acestep_mi355x import capi
    return types.SimpleNamespace(attention=functools.partial(capi.kernel_lm_attention, lib=lib),
                                 attention_shared=functools.partial(capi.kernel_lm_attention_shared, lib=lib))
