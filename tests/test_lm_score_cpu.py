"""CPU checks of teacher-forced scoring on the LM host library (tests/lmhostlib.py): kernels/lm_score_host.h through
ace_mi_kernel_lm_score, the runtime entry ace_mi_lm_score and hook.install_lm_backend's scoring_module keyword.  The
cases are those of tests/lm_score_cases.py, which test_gpu_lm_score.py runs on the GPU."""
import ctypes

import pytest

import lm_cases as lc
import lm_score_cases as sc
from lmhostlib import build_lm_host_lib


@pytest.fixture(scope="module")
def bridge():
    yield from sc.open_bridge(build_lm_host_lib(), lc.checkpoint("tied"))


@pytest.fixture(scope="module")
def delta(bridge):
    return sc.route_delta(bridge, lc.fixture()["tied/a/logits"], "cpu")


@pytest.mark.parametrize("param", sc.kernel_params(4), ids=sc.param_id)
def test_score_kernel_against_float64(param):
    sc.run_kernel_case(param, ctypes.CDLL(build_lm_host_lib()))


def test_score_kernel_refusals():
    sc.run_kernel_refusals(ctypes.CDLL(build_lm_host_lib()))


@pytest.mark.parametrize("score_from", [1, 5, 11])
@pytest.mark.parametrize("B", [1, 2])
def test_score_equals_prefix_forwards(bridge, delta, B, score_from):
    sc.run_engine(bridge, "cpu", delta, B, score_from)


def test_score_refusals(bridge):
    sc.run_refusals(bridge, build_lm_host_lib(), "cpu")


def test_hook_scoring_module(bridge, delta):
    sc.run_hook(bridge, "cpu", delta)
