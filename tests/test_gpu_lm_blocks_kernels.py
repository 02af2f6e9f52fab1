"""GPU parity of the decode step's raw-block kernels (kernels/lm_decode_blocks.hip) through the
ace_mi_kernel_lm_skinny_blocks / ace_mi_kernel_lm_embed_blocks self-test entries, against the float64 references of
tests/lm_blocks_kernel_cases.py.  tests/test_lm_blocks_kernels_cpu.py runs the same checks on the C++ restatement."""
import pytest

import lm_blocks_kernel_cases as lb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def k():
    return lb.runners()


class TestLmBlocksKernelsOnGpu(lb.LmBlocksKernelChecks):
    IMPL = lb.KERNEL
