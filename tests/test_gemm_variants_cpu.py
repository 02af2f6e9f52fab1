"""The GEMM variant table and tile picker (csrc/gemm_variants.h) on the CPU, through the host-emulation library's
ace_mi_gemm_resolve / ace_mi_gemm_variant_row / ace_mi_gemm_variant_arg_ok (pure functions, no device).

tests/golden/gemm_picks.json was written by the picker as it stood before the table existed (pick_variant, its
`supports` lambda, pick_variant_q and launch_gemm's prep remap, copied into a stand-alone program): "auto" is the
automatic pick over a grid of shapes on both sides of every threshold in the rules, "rows" are forced / overriding
variants with what was launched in the end (the id itself, or the automatic pick where the id does not handle the
shape).  The 240 s picks and the table copy below are written by hand, so that a change to a rule or a row has to be
made twice, on purpose."""
import ctypes
import itertools
import json
import os

import pytest

from hostlib import CLANG, build_host_lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_picks.json")
WFMT_NAME = {0: "bf16", 2: "q8_0"}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(CLANG):
        pytest.skip("host clang++ not available")
    return ctypes.CDLL(build_host_lib())


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def capi():
    from acestep_mi355x import capi
    return capi


def test_auto_picks_match_golden(lib, golden):
    a = golden["auto"]
    grid = list(itertools.product(a["wfmt"], a["prep"], a["M"], a["N"], a["K"]))
    assert len(grid) == len(a["variant"]) == 2 * 2 * 30 * 8 * 6
    bad = []
    for (wfmt, prep, M, N, K), want in zip(grid, a["variant"]):
        got = capi().gemm_resolve(M, N, K, WFMT_NAME[wfmt], prep=bool(prep), lib=lib)
        if got != want:
            bad.append((wfmt, prep, M, N, K, want, got))
    assert not bad, bad[:20]


def test_forced_and_override_match_golden(lib, golden):
    assert golden["columns"] == ["forced", "override", "M", "N", "K", "wfmt", "prep", "variant"]
    assert len(golden["rows"]) > 2000
    bad = []
    for forced, ov, M, N, K, wfmt, prep, want in golden["rows"]:
        got = capi().gemm_resolve(M, N, K, WFMT_NAME[wfmt], prep=bool(prep), forced=forced, override=ov, lib=lib)
        if got != want:
            bad.append((forced, ov, M, N, K, wfmt, prep, want, got))
    assert not bad, bad[:20]


def test_unsupported_forced_variant_falls_back(lib):
    """What test_gemm_all_variants' docstring relies on: a forced variant that does not handle the shape is ignored."""
    r = lambda **kw: capi().gemm_resolve(300, 512, 128, lib=lib, **kw)
    auto = r()
    assert r(forced=7) == 7
    assert r(forced=207) == auto          # K = 128: one K-tile per part
    assert r(forced=20) == auto           # a quantized-only tile on dense weights
    assert r(forced=216) == auto and r(forced=218) == auto  # tiles without split-K
    assert r(forced=0x10000 + 216) == 216  # diagnostics: no support check
    assert capi().gemm_resolve(300, 384, 128, forced=10, lib=lib) == capi().gemm_resolve(300, 384, 128, lib=lib)
    q = lambda **kw: capi().gemm_resolve(300, 512, 512, "q8_0", lib=lib, **kw)
    assert q(forced=4) == 4 and q(forced=204) == q() and q(forced=8) == q() and q(forced=223) == 223
    assert q(override=4) == q()           # overrides are for dense weights


# 240 s (M = 3000): from the rules' comments and DESIGN.md section 4, not from the golden
PICKS_240S = [
    ("bf16", "qkv", 4096, 2048, 4),
    ("bf16", "gate|up", 12288, 2048, 4),
    ("bf16", "o / cross", 2048, 2048, 7),
    ("bf16", "down", 2048, 6144, 7),
    ("bf16", "proj_out", 128, 2048, 9),
    ("q8_0", "gate|up", 12288, 2048, 21),
    ("q8_0", "qkv", 4096, 2048, 21),
    ("q8_0", "o / cross", 2048, 2048, 25),
    ("q8_0", "down", 2048, 6144, 25),
]


@pytest.mark.parametrize("wfmt,layer,N,K,want", PICKS_240S)
def test_picks_at_240s(lib, wfmt, layer, N, K, want):
    assert capi().gemm_resolve(3000, N, K, wfmt, lib=lib) == want, layer


def test_q8_0_short_sequences_pick_7(lib):
    for M in (1, 125, 750, 1024):
        for N, K in ((4096, 2048), (12288, 2048), (2048, 2048), (2048, 6144), (128, 2048)):
            assert capi().gemm_resolve(M, N, K, "q8_0", lib=lib) == 7, (M, N, K)


# id -> (dense kernel, quantized kernel, largest dense split-K, largest quantized split-K, prep sibling); kernels as
# (family, BM, BN, WM, WN, depth), fields a family does not have 0 (gemm_qr_kernel: WN = its waves)
NONE = ("none", 0, 0, 0, 0, 0)
TABLE = {
    0: (("gemm_kernel", 128, 128, 2, 2, 0), ("gemm_q_kernel", 128, 128, 2, 2, 0), 1, 1, 0),
    1: (("gemm_kernel", 128, 128, 2, 2, 1), ("gemm_q_kernel", 128, 128, 2, 2, 0), 2, 1, 1),
    2: (("gemm_kernel", 256, 256, 2, 4, 1), ("gemm_q_kernel", 256, 256, 2, 4, 0), 1, 1, 3),
    3: (("gemm_kernel", 256, 128, 2, 2, 1), ("gemm_q_kernel", 256, 128, 2, 2, 0), 2, 1, 3),
    4: (("gemm_kernel", 192, 128, 2, 2, 1), ("gemm_q_kernel", 192, 128, 2, 2, 0), 2, 1, 4),
    5: (("gemm_kernel", 192, 256, 2, 4, 1), ("gemm_q_kernel", 192, 256, 2, 4, 0), 1, 1, 4),
    6: (("gemm_kernel", 192, 64, 2, 2, 1), NONE, 4, 1, 1),
    7: (("gemm_kernel", 96, 128, 2, 2, 1), ("gemm_q_kernel", 96, 128, 2, 2, 0), 4, 1, 7),
    8: (("gemm_kernel", 64, 128, 2, 2, 1), NONE, 4, 1, 8),
    9: (("gemm_kernel", 64, 64, 2, 2, 1), NONE, 4, 1, 8),
    10: (("gemm8_kernel", 256, 256, 0, 0, 0), NONE, 2, 1, 10),
    11: (("gemm8_kernel", 192, 256, 0, 0, 0), NONE, 2, 1, 11),
    12: (("gemm_kernel", 64, 64, 2, 2, 4), NONE, 4, 1, 13),
    13: (("gemm_kernel", 64, 128, 2, 2, 3), NONE, 4, 1, 13),
    14: (("gemm_kernel", 96, 128, 2, 2, 3), NONE, 4, 1, 14),
    15: (("gemm_kernel", 128, 128, 2, 2, 3), NONE, 4, 1, 15),
    16: (("gemm_kernel", 192, 128, 4, 2, 1), NONE, 1, 1, 16),
    18: (("gemm_ws_kernel", 192, 128, 0, 0, 3), NONE, 1, 1, 18),
    20: (NONE, ("gemm_qr_kernel", 192, 128, 0, 4, 0), 1, 1, 20),
    21: (NONE, ("gemm_qr_kernel", 192, 256, 0, 8, 0), 1, 1, 21),
    22: (NONE, ("gemm_qr_kernel", 128, 128, 0, 4, 0), 1, 4, 22),
    23: (NONE, ("gemm_qr_kernel", 64, 128, 0, 4, 0), 1, 4, 23),
    24: (NONE, ("gemm_qr_kernel", 256, 128, 0, 4, 0), 1, 1, 24),
    25: (NONE, ("gemm_wsq_kernel", 192, 128, 0, 0, 3), 1, 1, 25),
}


def test_table_rows(lib):
    for vid in range(-1, 130):
        row = capi().gemm_variant_row(vid, lib=lib)
        if vid not in TABLE:
            assert row is None, vid
            continue
        dense, quant, ds, qs, sib = TABLE[vid]
        assert (row["dense"], row["quant"], row["dense_split"], row["quant_split"], row["prep_sibling"]) == \
            (dense, quant, ds, qs, sib), (vid, row)
        assert row["needs_n256"] == (256 in (dense[2], quant[2])), vid
        assert row["name"].startswith(f"{(dense if dense != NONE else quant)[1]}x{(dense if dense != NONE else quant)[2]},"), row


def test_arg_check_is_the_old_expression(lib):
    def old_abi(v):          # runtime/util_abi.cpp before the table (C's % truncates toward zero)
        m = v % 100 if v >= 0 else -(-v % 100)
        return not (v < -1 or m > 25 or v > 424)

    def old_selftest(v):     # ace_mi_kernel_gemm_q before the table
        vb = (v & 0xffff) if v >= 0 else v
        m = vb % 100 if vb >= 0 else -(-vb % 100)
        return not (v < -1 or v > 0x1ffff or m > 25 or vb > 424)

    for base in range(-2, 501):
        for v in (base, base + 0x10000 if base >= 0 else base, base + 0x20000 if base >= 0 else base):
            assert capi().gemm_variant_arg_ok(v, lib=lib) == old_abi(v), v
            assert capi().gemm_variant_arg_ok(v, allow_unchecked=True, lib=lib) == old_selftest(v), v
    # the holes pass the range check (and fail at launch: "gemm: bad variant")
    assert capi().gemm_variant_arg_ok(17, lib=lib) and capi().gemm_variant_arg_ok(19, lib=lib)
    assert not capi().gemm_variant_arg_ok(425, lib=lib) and capi().gemm_variant_arg_ok(424, lib=lib)


# the parametrize lists of the GPU tests (tests/test_gpu_kernels.py, test_gpu_quant.py, test_gpu_forward.py), as literals
GPU_TEST_VARIANTS = {
    "test_gemm_all_variants": [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 204, 207, 208, 210, 211, 212,
                               307, 409, 413, 414],
    "test_gemm_residual_epilogues": [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 204, 207, 210, 211, 213,
                                     215, 408],
    "test_gemm_tiles_bit_identical": [18, 4],
    "test_gemm_splitk_deterministic": [204, 207, 211, 212, 307, 408],
    "test_gemm_q_matches_dequantized_product": [-1, 1, 2, 3, 4, 5, 7, 20, 21, 22, 23, 24, 25, 222, 223, 423],
    "test_gemm_q_short_k_q8_0": [-1, 1, 3, 4, 20, 22, 23, 24, 25],
    "test_gemm_q_residual_epilogues": [-1, 20, 21, 22, 23, 24, 25, 222, 423],
    "test_fused_qkv_prep_is_bit_exact": [-1, 10, 11, 16, 18, 7],
}


def test_gpu_test_variants_have_rows(lib):
    for name, ids in GPU_TEST_VARIANTS.items():
        quant = "gemm_q" in name
        for v in ids:
            if v < 0:
                continue
            assert capi().gemm_variant_arg_ok(v, lib=lib), (name, v)
            row = capi().gemm_variant_row(v % 100, lib=lib)
            assert row is not None, (name, v)
            assert row["quant" if quant else "dense"][0] != "none", (name, v)
            if v >= 200:
                assert v // 100 <= row["quant_split" if quant else "dense_split"], (name, v)
