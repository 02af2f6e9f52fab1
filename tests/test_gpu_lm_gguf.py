"""GPU tests of the causal LM on GGUF checkpoints (ace_mi_load_lm on a .gguf, kernels/lm_decode_q.hip) against
tests/golden/lm_qwen3_gguf.npz: every variant of acestep_mi355x.synthetic.LM_GGUF_VARIANTS through cases a and b, `mixed`
also through e (the split attention).  Checks and bound: tests/lm_gguf_cases.py.  Measured rel-L2: DESIGN.md §5."""
import pytest

import lm_gguf_cases as lg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def new_bridge():
    from acestep_mi355x.capi import GGMLCAPIBridge
    return lambda: GGMLCAPIBridge()


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


class TestLmGgufOnGpu(lg.LmGgufChecks):
    DEVICE = "cuda"
    LABEL = "gpu"
    CASES = tuple((v, c) for v in lg.VARIANTS for c in ("a", "b")) + (("mixed", "e"),)
