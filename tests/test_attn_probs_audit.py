"""CPU: the MFMA operand write-after-read audit of tests/test_mfma_war_audit.py (tools/audit_mfma_war.py) over the
attention-probability kernel's built code: attn_probs_kernel runs two waves per SIMD, so no VALU and no load may write an
A / B register within 8 issue slots of the MFMA that reads it."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import audit_mfma_war as aw  # noqa: E402

S = os.path.join(ROOT, "ace-step-1.5-ggml_amd", "build", "attn_probs-hip-amdgcn-amd-amdhsa-gfx950.s")


def test_attn_probs_kernel_is_clean_of_operand_overwrites():
    if not os.path.exists(S):
        pytest.fail(f"{S} missing: build the library first (make -C ace-step-1.5-ggml_amd/csrc, or __graft_entry__.build())")
    funcs = {k: f for k, f in aw.parse(S).items() if "attn_probs_kernel" in k}
    assert len(funcs) == 1, sorted(funcs)
    assert aw.audit(S, window=8, valu_only=False) == {}
