"""GPU tests of token selection (kernels/lm_sample.hip through ace_mi_kernel_lm_select) and of the engine loop
(ace_mi_lm_select / ace_mi_lm_generate, hook.install_lm_backend device_codes): the cases and numpy references of
tests/lm_sample_cases.py, whose docstring derives the tolerance."""
import numpy as np
import pytest

import lm_cases as lc
import lm_gguf_cases as gc
import lm_sample_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def bridges():
    from acestep_mi355x.capi import GGMLCAPIBridge
    made = {}

    def get(variant):
        if variant not in made:
            br = GGMLCAPIBridge()
            br.load_lm(gc.checkpoint("q8_0") if variant == "q8_0" else lc.checkpoint(variant))
            made[variant] = br
        return made[variant]
    yield get
    for br in made.values():
        br.close()


@pytest.mark.parametrize("name,case", sc.toleranced_cases(), ids=[n for n, _ in sc.toleranced_cases()])
def test_select_cases(name, case):
    worst = sc.run_toleranced(case, None)
    print(f"gpu {name}: worst distance / eps = {worst:.3f}")


def test_select_exact_properties():
    sc.run_exact_properties(None)


@pytest.mark.parametrize("variant,B,cfg,n_prompt", [("tied", 2, 2.0, 9), ("untied", 1, 1.0, 9), ("q8_0", 2, 2.0, 9),
                                                    ("tied", 2, 2.0, 250)])
def test_generate_is_forward_plus_select(bridges, variant, B, cfg, n_prompt):
    """n_prompt 250: the loop's steps cross LM_SPLIT_KEYS (256 keys), where decode attention starts to split"""
    sc.run_composition(bridges(variant), DEV, sc.chain_source(None), B, cfg, n_prompt=n_prompt, capacity=n_prompt + 16)


@pytest.mark.parametrize("variant", ["tied", "untied"])
def test_generate_stop(bridges, variant):
    sc.run_stop(bridges(variant), DEV)


def test_generate_seeded(bridges):
    sc.run_seeded(bridges("tied"), DEV)


def test_generate_errors(bridges):
    sc.run_errors(bridges("untied"), DEV)


def test_hook_device_codes(bridges):
    sc.run_hook(bridges("tied"), DEV)


def test_entries_before_load():
    sc.run_not_loaded(None, DEV)
