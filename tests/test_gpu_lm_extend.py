"""GPU tests of ace_mi_lm_extend / ace_mi_lm_truncate on the tiny synthetic checkpoints (dense, GGUF block planes, raw
blocks) and of hook.install_lm_backend's reuse_score_prompt keyword.  Cases and tolerances: tests/lm_extend_cases.py."""
import pytest

import lm_cases as lc
import lm_extend_cases as ec
import lm_score_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def bridge():
    yield from sc.open_bridge(None, lc.checkpoint("tied"))


@pytest.fixture(scope="module")
def delta(bridge):
    return sc.route_delta(bridge, lc.fixture()["tied/a/logits"], DEV)


@pytest.mark.parametrize("B,P,n", [(1, 5, 1), (2, 7, 9), (2, 250, 17), (1, 300, 40)])
def test_extend_equals_single_steps(bridge, delta, B, P, n):
    ec.run_extend_vs_steps(bridge, DEV, delta, B, P, n)


@pytest.mark.parametrize("B,P,T", [(1, 9, 6), (2, 270, 10)])
def test_extend_scores_like_a_full_prefill(bridge, delta, B, P, T):
    ec.run_scoring(bridge, DEV, delta, B, P, T)


@pytest.mark.parametrize("variant", ["q8_0", "mixed_raw"])
def test_extend_on_block_weights(variant, monkeypatch):
    """a GGUF checkpoint in block planes; the mixed-type one with its Q5_K matrices kept as raw blocks"""
    import lm_gguf_cases as gc
    if variant == "mixed_raw":
        monkeypatch.setenv("ACE_MI_LM_RAW_BLOCKS", "1")
    name = variant.split("_raw")[0]
    for br in sc.open_bridge(None, gc.checkpoint(name)):
        d = sc.route_delta(br, gc.fixture()[name + "/a/logits"], DEV)
        ec.run_extend_vs_steps(br, DEV, d, 2, 7, 9)
        ec.run_scoring(br, DEV, d, 2, 9, 6)


def test_extend_refusals(bridge):
    ec.run_refusals(bridge, None, DEV)


def test_hook_reuses_the_score_prompt(bridge, delta):
    ec.run_hook(bridge, DEV, delta)
