"""The checks of tests/lm_kernel_cases.py against the host emulation of the LM decode kernels (tests/host/lm_emul.cpp
through the ace_mi_kernel_lm_* entries of the LM host library): proves the float64 references, the bounds and the
entries' buffer handling on a machine without a GPU.  tests/test_gpu_lm_kernels.py runs the same checks on the gfx950
kernels."""
import ctypes

import pytest

import lm_kernel_cases as lk


@pytest.fixture(scope="module")
def k():
    from lmhostlib import build_lm_host_lib
    return lk.runners(ctypes.CDLL(build_lm_host_lib()))


class TestLmKernelsOnHostEmulation(lk.LmKernelChecks):
    IMPL = lk.EMULATION
