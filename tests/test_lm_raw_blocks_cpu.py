"""The causal LM's raw-block mode on the CPU: the LM engine and the loader over the host library (tests/lmhostlib.py:
csrc/kernels/lm_decode_blocks_host.h for the step on raw blocks) through the checks of tests/lm_raw_blocks_cases.py.
tests/test_gpu_lm_raw_blocks.py runs them on the GPU."""
import pytest

import lm_raw_blocks_cases as lr


@pytest.fixture(scope="module")
def pairs():
    from acestep_mi355x.capi import GGMLCAPIBridge
    from lmhostlib import build_lm_host_lib
    lib = build_lm_host_lib()
    made = {}

    def get(variant):
        if variant not in made:
            made[variant] = lr.load_pair(lambda: GGMLCAPIBridge(lib_path=lib), variant)
        return made[variant]
    yield get
    for pair in made.values():
        for br in pair:
            br.close()


class TestLmRawBlocksOnHostEmulation(lr.LmRawBlocksChecks):
    DEVICE = "cpu"
    LABEL = "host"
