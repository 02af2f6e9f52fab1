"""GPU tests of the LM cache fan-out: kernels/lm_fanout.hip through ace_mi_kernel_lm_cache_fanout, the runtime entries
ace_mi_lm_fanout / ace_mi_lm_uniforms on the tiny synthetic checkpoint, and hook.install_lm_backend's batch_codes
switch.  The cases are those of tests/lm_fanout_cases.py; every comparison is of bits or of tokens."""
import pytest

import lm_cases as lc
import lm_fanout_cases as fc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def bridge():
    from acestep_mi355x.capi import GGMLCAPIBridge
    br = GGMLCAPIBridge()
    br.load_lm(lc.checkpoint("tied"))
    yield br
    br.close()


@pytest.mark.parametrize("case", fc.kernel_cases(), ids=fc.case_id)
def test_fanout_kernel_copies_bits(case):
    fc.run_kernel_case(case, None)


def test_fanout_kernel_refusals():
    fc.run_kernel_refusals(None)


@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("params", [fc.SAMPLED, fc.ARGMAX], ids=["sampled", "argmax"])
def test_fanout_equals_sequential_runs(bridge, S, params):
    fc.run_equality(bridge, DEV, S, params)


def test_fanout_equals_sequential_runs_across_the_attention_split(bridge):
    """a 250-token prompt: the 24 steps cross LM_SPLIT_KEYS (256 keys), where decode attention splits and merges"""
    fc.run_equality(bridge, DEV, 4, fc.SAMPLED, n_prompt=250)


def test_fanout_equals_sequential_runs_on_block_planes():
    """a Q8_0 GGUF checkpoint: the step's products run kernels/lm_decode_q.hip, 8 rows in its widest row tile"""
    import lm_gguf_cases as gc
    from acestep_mi355x.capi import GGMLCAPIBridge
    br = GGMLCAPIBridge()
    try:
        br.load_lm(gc.checkpoint("q8_0"))
        fc.run_equality(br, DEV, 4, fc.SAMPLED)
    finally:
        br.close()


def test_uniforms(bridge):
    fc.run_uniforms(bridge, DEV)


def test_fanout_refusals(bridge):
    fc.run_refusals(bridge, DEV)


def test_fanout_before_load():
    fc.run_not_loaded(None, DEV)


def test_hook_batch_codes_equals_sequential(bridge):
    fc.run_hook_equal(bridge, DEV, 4, 2.0, [11, 12, 13, 14])
