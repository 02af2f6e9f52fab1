"""The token-selection kernel's host restatement (kernels/lm_sample_host.h) and the engine loop (runtime/lm.cpp
ace_mi_lm_select / ace_mi_lm_generate, hook.install_lm_backend device_codes) on the LM host library: the cases of
tests/lm_sample_cases.py that test_gpu_lm_sample.py runs on the GPU."""
import numpy as np
import pytest

import lm_cases as lc
import lm_sample_cases as sc


@pytest.fixture(scope="module")
def lib():
    import ctypes
    from lmhostlib import build_lm_host_lib
    return ctypes.CDLL(build_lm_host_lib())


@pytest.fixture(scope="module")
def bridge():
    from acestep_mi355x.capi import GGMLCAPIBridge
    from lmhostlib import build_lm_host_lib
    br = GGMLCAPIBridge(lib_path=build_lm_host_lib())
    br.load_lm(lc.checkpoint("tied"))
    yield br
    br.close()


@pytest.mark.parametrize("name,case", sc.toleranced_cases(), ids=[n for n, _ in sc.toleranced_cases()])
def test_select_cases(lib, name, case):
    worst = sc.run_toleranced(case, lib)
    print(f"host {name}: worst distance / eps = {worst:.3f}")


def test_select_exact_properties(lib):
    sc.run_exact_properties(lib)


@pytest.mark.parametrize("B,cfg", [(2, 2.0), (1, 1.0)])
def test_generate_is_forward_plus_select(bridge, lib, B, cfg):
    sc.run_composition(bridge, "cpu", sc.chain_source(lib), B, cfg, n_prompt=5, capacity=32, n=6)


def test_generate_stop(bridge):
    sc.run_stop(bridge, "cpu")


def test_generate_seeded(bridge):
    sc.run_seeded(bridge, "cpu")


def test_generate_errors(bridge):
    sc.run_errors(bridge, "cpu")


def test_hook_device_codes(bridge):
    sc.run_hook(bridge, "cpu")


def test_entries_before_load():
    from lmhostlib import build_lm_host_lib
    sc.run_not_loaded(build_lm_host_lib(), "cpu")
