"""GPU tests of teacher-forced scoring: kernels/lm_score.hip through ace_mi_kernel_lm_score against float64, the runtime
entry ace_mi_lm_score on the tiny synthetic checkpoints against the engine's own per-prefix forwards, and
hook.install_lm_backend's scoring_module keyword.  Cases and the derivation of every bound: tests/lm_score_cases.py."""
import pytest

import lm_cases as lc
import lm_score_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def bridge():
    yield from sc.open_bridge(None, lc.checkpoint("tied"))


@pytest.fixture(scope="module")
def delta(bridge):
    return sc.route_delta(bridge, lc.fixture()["tied/a/logits"], DEV)


@pytest.mark.parametrize("param", sc.kernel_params(), ids=sc.param_id)
def test_score_kernel_against_float64(param):
    sc.run_kernel_case(param, None)


def test_score_kernel_refusals():
    sc.run_kernel_refusals(None)


@pytest.mark.parametrize("score_from", [1, 5, 11])
@pytest.mark.parametrize("B", [1, 2])
def test_score_equals_prefix_forwards(bridge, delta, B, score_from):
    sc.run_engine(bridge, DEV, delta, B, score_from)


@pytest.mark.parametrize("variant", ["untied", "q8_0", "mixed_raw"])
def test_score_on_other_heads(variant, monkeypatch):
    """an untied dense head read in place; a Q8_0 head in block planes, expanded for the call; the mixed-type GGUF with
    its Q5_K matrices kept as raw blocks (the prefill expands them) and a Q6_K head"""
    import lm_gguf_cases as gc
    if variant == "mixed_raw":
        monkeypatch.setenv("ACE_MI_LM_RAW_BLOCKS", "1")
    name = variant.split("_raw")[0]
    model, fixture = ((lc.checkpoint(name), lc.fixture()) if name == "untied" else (gc.checkpoint(name), gc.fixture()))
    for br in sc.open_bridge(None, model):
        sc.run_engine(br, DEV, sc.route_delta(br, fixture[name + "/a/logits"], DEV), 2, 5)


def test_score_refusals(bridge):
    sc.run_refusals(bridge, None, DEV)


def test_hook_scoring_module(bridge, delta):
    sc.run_hook(bridge, DEV, delta)
