"""GPU parity of the LM decode kernels (kernels/lm_decode.hip), one by one through the ace_mi_kernel_lm_* self-test
entries, against the float64 references of tests/lm_kernel_cases.py: every template instance (type x batch x epilogue
of the skinny product, GQA ratio x output type of the attention, the merge, both embedding formats), K loops of several
trips, split attention over three ranges, masked ranges, saturating and subnormal cache values.
tests/test_lm_kernels_cpu.py runs the same checks on the host emulation."""
import pytest

import lm_kernel_cases as lk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def k():
    return lk.runners()


class TestLmKernelsOnGpu(lk.LmKernelChecks):
    IMPL = lk.KERNEL
