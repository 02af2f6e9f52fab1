"""The causal LM on GGUF checkpoints, on the CPU: the LM engine (runtime/lm.cpp) and the loader over the host library
(tests/lmhostlib.py: host GEMMs for the prefill, csrc/kernels/lm_decode_q_host.h for the step on block planes) through
the checks of tests/lm_gguf_cases.py.  Case a on the tied Q4_K model and on `mixed` (planes beside bf16 images); the
GPU suite (tests/test_gpu_lm_gguf.py) runs every variant and case."""
import pytest

import lm_gguf_cases as lg


@pytest.fixture(scope="module")
def host_lib():
    from lmhostlib import build_lm_host_lib
    return build_lm_host_lib()


@pytest.fixture(scope="module")
def new_bridge(host_lib):
    from acestep_mi355x.capi import GGMLCAPIBridge
    return lambda: GGMLCAPIBridge(lib_path=host_lib)


@pytest.fixture(scope="module")
def loaded(new_bridge):
    made = {}

    def get(variant):
        if variant not in made:
            made[variant] = new_bridge()
            made[variant].load_lm(lg.checkpoint(variant))
        return made[variant]
    yield get
    for br in made.values():
        br.close()


class TestLmGgufOnHostEmulation(lg.LmGgufChecks):
    DEVICE = "cpu"
    LABEL = "host"
    CASES = (("q4_k", "a"), ("mixed", "a"))
