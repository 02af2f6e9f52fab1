"""GPU checks of the attention-probability kernel (kernels/attn_probs.hip) through the ace_mi_kernel_attn_probs
self-test entry, against the float64 reference and the derived bound of tests/attn_probs_cases.py: every edge of the
128-query / 64-key tiling, out-of-order and duplicate head lists, masks, bit-exact uniform rows, sentinels.
tests/test_attn_probs_cpu.py runs the same checks on the host restatement."""
import pytest

import attn_probs_cases as ac

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run():
    return ac.runner()


class TestAttnProbsOnGpu(ac.AttnProbsChecks):
    pass
