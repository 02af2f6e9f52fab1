"""CPU checks of ace_mi_lm_extend / ace_mi_lm_truncate on the LM host library (tests/lmhostlib.py, the chunk path
through kernels/lm_attn_chunk_host.h): the engine-level refusals and the extend-against-single-steps equivalence of
tests/lm_extend_cases.py, which tests/test_gpu_lm_extend.py runs on the GPU."""
import pytest

import lm_cases as lc
import lm_extend_cases as ec
import lm_score_cases as sc
from lmhostlib import build_lm_host_lib


@pytest.fixture(scope="module")
def bridge():
    yield from sc.open_bridge(build_lm_host_lib(), lc.checkpoint("tied"))


@pytest.mark.parametrize("B,P,n", [(1, 5, 1), (2, 7, 9)])
def test_extend_equals_single_steps(bridge, B, P, n):
    ec.run_extend_vs_steps(bridge, "cpu", sc.route_delta(bridge, lc.fixture()["tied/a/logits"], "cpu"), B, P, n)


def test_extend_scores_like_a_full_prefill(bridge):
    ec.run_scoring(bridge, "cpu", sc.route_delta(bridge, lc.fixture()["tied/a/logits"], "cpu"), 2, 9, 6)


def test_extend_refusals(bridge):
    ec.run_refusals(bridge, build_lm_host_lib(), "cpu")
