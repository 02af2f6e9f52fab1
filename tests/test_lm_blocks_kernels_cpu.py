"""The checks of tests/lm_blocks_kernel_cases.py against the plain C++ restatement of the raw-block decode kernels
(csrc/kernels/lm_decode_blocks_host.h through the LM host library): proves the references, the bounds and the entries'
buffer handling without a GPU.  tests/test_gpu_lm_blocks_kernels.py runs the same checks on the gfx950 kernels."""
import ctypes

import pytest

import lm_blocks_kernel_cases as lb


@pytest.fixture(scope="module")
def k():
    from lmhostlib import build_lm_host_lib
    return lb.runners(ctypes.CDLL(build_lm_host_lib()))


class TestLmBlocksKernelsOnHostRestatement(lb.LmBlocksKernelChecks):
    IMPL = lb.EMULATION
