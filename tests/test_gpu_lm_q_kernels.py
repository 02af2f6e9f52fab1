"""GPU parity of the decode step's block-plane kernels (kernels/lm_decode_q.hip) through the ace_mi_kernel_lm_skinny_q /
ace_mi_kernel_lm_embed_q self-test entries, against the references of tests/lm_q_kernel_cases.py: every format, both
lane mappings, every trip boundary up to K = 2560, all three epilogues, B = 1..8.  tests/test_lm_q_kernels_cpu.py runs
the same checks on the plain C++ restatement."""
import pytest

import lm_q_kernel_cases as lq

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def k():
    return lq.runners()


class TestLmQKernelsOnGpu(lq.LmQKernelChecks):
    IMPL = lq.KERNEL
