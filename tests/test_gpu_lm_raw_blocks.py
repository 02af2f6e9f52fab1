"""GPU tests of the causal LM's raw-block mode (ACE_MI_LM_RAW_BLOCKS=1: kernels/lm_decode_blocks.hip in the decode step,
the expansion scratch in the prefill) against the default mode on the same files.  Checks: tests/lm_raw_blocks_cases.py."""
import pytest

import lm_raw_blocks_cases as lr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pairs():
    from acestep_mi355x.capi import GGMLCAPIBridge
    made = {}

    def get(variant):
        if variant not in made:
            made[variant] = lr.load_pair(GGMLCAPIBridge, variant)
        return made[variant]
    yield get
    for pair in made.values():
        for br in pair:
            br.close()


class TestLmRawBlocksOnGpu(lr.LmRawBlocksChecks):
    DEVICE = "cuda"
    LABEL = "gpu"
