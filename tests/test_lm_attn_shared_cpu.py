"""The cases of tests/lm_attn_shared_cases.py against the host twin of the shared-prefix decode attention
(kernels/lm_attn_shared_host.h through ace_mi_kernel_lm_attention_shared of the LM host library), beside the host
emulation's launch_lm_attention.  tests/test_gpu_lm_attn_shared.py runs the same cases on the gfx950 kernel."""
import ctypes

import pytest

import lm_attn_shared_cases as sc
import lm_kernel_cases as lk


@pytest.fixture(scope="module")
def k():
    from lmhostlib import build_lm_host_lib
    return sc.runners(ctypes.CDLL(build_lm_host_lib()))


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_shared_attention_equals_plain_attention(k, case):
    sc.run_case(k, lk.EMULATION, case)


def test_shared_attention_refusals(k):
    sc.run_refusals(k)
