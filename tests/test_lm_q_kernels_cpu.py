"""The checks of tests/lm_q_kernel_cases.py against the plain C++ restatement of the block-plane decode kernels
(csrc/kernels/lm_decode_q_host.h through the LM host library): proves the block packers, the references, the bounds and
the entries' buffer handling without a GPU.  tests/test_gpu_lm_q_kernels.py runs the same checks on the gfx950 kernels."""
import ctypes

import numpy as np
import pytest

import ggml_blocks_np as gb
import lm_q_kernel_cases as lq


@pytest.fixture(scope="module")
def k():
    from lmhostlib import build_lm_host_lib
    return lq.runners(ctypes.CDLL(build_lm_host_lib()))


class TestLmQKernelsOnHostRestatement(lq.LmQKernelChecks):
    IMPL = lq.EMULATION


def test_packers_round_trip_through_the_numpy_dequant():
    """pack_* with arbitrary fields against ggml_blocks_np.dequant's reading of the block structs."""
    rng = np.random.default_rng(3)
    rows, nb = 3, 2
    d = rng.integers(1, 9, (rows, nb)).astype(np.float32) / 8
    q = rng.integers(-128, 128, (rows, nb, 32))
    assert np.array_equal(gb.dequant(lq.pack_q8_0(d, q), "q8_0"), (d[..., None] * q).reshape(rows, -1).astype(np.float32))
    sc, mn = rng.integers(0, 64, (rows, nb, 8)), rng.integers(0, 64, (rows, nb, 8))
    q = rng.integers(0, 16, (rows, nb, 256))
    want = (d[..., None, None] * sc[..., None] * q.reshape(rows, nb, 8, 32) - 2 * d[..., None, None] * mn[..., None])
    assert np.array_equal(gb.dequant(lq.pack_q4_k(d, 2 * d, sc, mn, q), "q4_k"), want.reshape(rows, -1).astype(np.float32))
    sc = rng.integers(-128, 128, (rows, nb, 16))
    q = rng.integers(-32, 32, (rows, nb, 256))
    want = d[..., None, None] * sc[..., None] * q.reshape(rows, nb, 16, 16)
    assert np.array_equal(gb.dequant(lq.pack_q6_k(d, sc, q), "q6_k"), want.reshape(rows, -1).astype(np.float32))


def test_kernel_chain_formula():
    """the kernel's documented chains at the shapes the engine runs (0.6B: K 1024 / 2048 / 3072; 1.7B: 2048 / 6144)"""
    assert [lq.kernel_chain("q4_k", K) for K in (256, 1024, 2048, 3072, 6144)] == [37, 37, 38, 70, 102]
    assert [lq.kernel_chain("q8_0", K) for K in (32, 512, 1024, 2048, 3072)] == [21, 21, 22, 38, 54]
    assert lq.kernel_chain("q6_k", 1280) == 38
