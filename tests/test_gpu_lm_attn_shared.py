"""GPU tests of the shared-prefix decode attention: lm_attn_shared_kernel (kernels/lm_decode.hip) through
ace_mi_kernel_lm_attention_shared, and the engine's batched loop with ACE_MI_LM_SHARED_PREFIX on and off.  The kernel
cases are those of tests/lm_attn_shared_cases.py; the engine case is lm_fanout_cases.run_equality's recipe."""
import pytest

import lm_attn_shared_cases as sc
import lm_cases as lc
import lm_fanout_cases as fc
import lm_kernel_cases as lk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def k():
    return sc.runners(None)


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_shared_attention_equals_plain_attention(k, case):
    sc.run_case(k, lk.KERNEL, case)


def test_shared_attention_refusals(k):
    sc.run_refusals(k)


@pytest.mark.parametrize("switch", ["1", "0"])
def test_batched_loop_equals_sequential_runs_over_a_shared_range(monkeypatch, switch):
    """A 265-token prompt (one whole range of 256 keys inside the shared prefix), G = 2, S = 4: with the switch on and
    off the loop's tokens and the logits of a decode step equal those of the one-item runs bit for bit, hence each
    other's."""
    from acestep_mi355x.capi import GGMLCAPIBridge
    monkeypatch.setenv("ACE_MI_LM_SHARED_PREFIX", switch)
    br = GGMLCAPIBridge()
    try:
        br.load_lm(lc.checkpoint("tied"))
        fc.run_equality(br, "cuda", 4, fc.SAMPLED, n_prompt=265)
    finally:
        br.close()
