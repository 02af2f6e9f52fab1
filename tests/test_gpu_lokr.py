"""LyCORIS LoKr adapters on the MI355X: the merge kernels (kernels/lokr.hip) through ace_mi_kernel_lokr_merge against
numpy bit for bit and against float64 np.kron within the derived bound (cases, reference and bound are those of
tests/test_lokr_cpu.py), and the engine's HIP path against a numpy-merged checkpoint."""
import numpy as np
import pytest

from test_lokr_cpu import KERNEL_CASES, check_kernel_case, forward_triple, lokr_adapter
from test_lora_cpu import inputs, rel

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_merge_kernel_matches_numpy(name):
    check_kernel_case(name)


@pytest.mark.parametrize("kw,scale,dtype", [
    (dict(form="w2_lowrank", r=4, targets=("q_proj", "v_proj", "o_proj", "gate_proj")), 0.37, "BF16"),
    (dict(form="both_lowrank", r=3, scalar=0.5), 1.0, "F16"),
])
def test_lokr_equals_merged_checkpoint_and_unload_restores(kw, scale, dtype):
    plain, got, after, ref, _ = forward_triple(None, lokr_adapter(seed=5, **kw), scale, inputs(T=40, L=7), dtype)
    np.testing.assert_array_equal(got, ref)
    assert rel(got, plain) > 1e-4
    np.testing.assert_array_equal(after, plain)
