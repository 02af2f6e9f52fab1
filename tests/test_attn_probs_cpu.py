"""The checks of tests/attn_probs_cases.py against the host restatement of the attention-probability kernel
(kernels/attn_probs_host.h through the ace_mi_kernel_attn_probs entry of the host library): proves the float64
reference, the bound and the entry's buffer handling on a machine without a GPU.  tests/test_gpu_attn_probs.py runs the
same checks on the gfx950 kernel."""
import ctypes

import pytest

import attn_probs_cases as ac


@pytest.fixture(scope="module")
def run():
    from hostlib import build_host_lib
    return ac.runner(ctypes.CDLL(build_host_lib()))


class TestAttnProbsOnHostRestatement(ac.AttnProbsChecks):
    pass
