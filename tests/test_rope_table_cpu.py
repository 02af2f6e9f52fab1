"""The one RoPE table of the runtime (csrc/runtime/devmem.h, RopeTable) through the host-emulation library's
ace_mi_rope_table / ace_mi_rope_table_steps, byte for byte.

tests/golden/rope_table_*.bin were written by a stand-alone program that held the three loops the engines had before
the table existed (DitEngine::rope_table, the block in BlockRunner::run, the block in LmEngine::begin), copied verbatim
and built with the host library's flags; it asserted that the three agree byte for byte.  Each file is cos [40][D/2]
followed by sin [40][D/2], float32.  No tolerance: ggml's float recurrence with cos / sin taken in double and rounded
once is an identity on one toolchain's libm."""
import ctypes
import os

import numpy as np
import pytest

from hostlib import CLANG, build_host_lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = {"d128": (40, 128, 1e6, "rope_table_n40_d128_theta1e6.bin"), "d64": (40, 64, 1e4, "rope_table_n40_d64_theta1e4.bin")}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(CLANG):
        pytest.skip("host clang++ not available")
    return ctypes.CDLL(build_host_lib())


def capi():
    from acestep_mi355x import capi
    return capi


def golden(case):
    n, hd, theta, name = CASES[case]
    raw = np.fromfile(os.path.join(GOLDEN, name), np.float32)
    assert raw.size == 2 * n * (hd // 2)
    return raw[:raw.size // 2].reshape(n, hd // 2), raw[raw.size // 2:].reshape(n, hd // 2)


def same_bytes(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("case", list(CASES))
def test_table_equals_the_former_loops(lib, case):
    n, hd, theta, _ = CASES[case]
    cs, sn = capi().rope_table(n, hd, theta, lib=lib)
    gc, gs = golden(case)
    assert same_bytes(cs, gc) and same_bytes(sn, gs)


def test_shorter_request_keeps_the_longer_table(lib):
    """ensure(40) then ensure(17): row p does not depend on n, so the 40 rows stay where they are."""
    rows, cs, sn = capi().rope_table_steps([(40, 128, 1e6), (17, 128, 1e6)], lib=lib)
    gc, gs = golden("d128")
    assert rows == [40, 40]
    assert same_bytes(cs, gc) and same_bytes(sn, gs)
    # and a longer one rebuilds: the first 40 rows are the same values again
    rows, cs, sn = capi().rope_table_steps([(17, 128, 1e6), (40, 128, 1e6), (41, 128, 1e6)], lib=lib)
    assert rows == [17, 40, 41]
    assert same_bytes(cs[:40], gc) and same_bytes(sn[:40], gs)


def test_theta_or_head_dim_change_rebuilds(lib):
    gc, gs = golden("d128")
    # theta alone, at fewer rows than held: the table is the new theta's, 17 rows of it
    rows, cs, sn = capi().rope_table_steps([(40, 128, 1e6), (17, 128, 1e4)], lib=lib)
    fresh = capi().rope_table(17, 128, 1e4, lib=lib)
    assert rows == [40, 17]
    assert same_bytes(cs, fresh[0]) and same_bytes(sn, fresh[1])
    assert not same_bytes(cs, gc[:17])
    # head_dim and theta: the other fixture
    rows, cs, sn = capi().rope_table_steps([(40, 128, 1e6), (40, 64, 1e4)], lib=lib)
    hc, hs = golden("d64")
    assert rows == [40, 40]
    assert same_bytes(cs, hc) and same_bytes(sn, hs)
    # and back
    rows, cs, sn = capi().rope_table_steps([(40, 64, 1e4), (40, 128, 1e6)], lib=lib)
    assert same_bytes(cs, gc) and same_bytes(sn, gs)


def test_bad_arguments_are_refused(lib):
    for bad in ((0, 128, 1e6), (4, 127, 1e6), (4, 0, 1e6), (4, 128, 0.0)):
        with pytest.raises(ValueError):
            capi().rope_table(*bad, lib=lib)
