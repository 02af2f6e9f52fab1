"""GPU: ace_mi_dit_forward_capture and the decoder.forward hook's output_attentions path on the MI355X with cuda
tensors (the checks of tests/dit_capture_cases.py; tests/test_dit_capture_cpu.py runs them on the host library)."""
import tempfile

import pytest

import dit_capture_cases as dc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiny_ckpt():
    from acestep_mi355x.synthetic import TINY_CONFIG, write_checkpoint
    d = tempfile.mkdtemp(prefix="acemi_cap_")
    write_checkpoint(d, TINY_CONFIG, seed=0, dtype="BF16")
    return d


@pytest.fixture(scope="module")
def env(tiny_ckpt):
    br = TestDitCaptureOnGpu.bridge()
    br.load_dit(tiny_ckpt)
    yield br, dc.CudaMem(), "cuda"
    br.close()


class TestDitCaptureOnGpu(dc.DitCaptureChecks):
    @staticmethod
    def bridge():
        from acestep_mi355x.capi import GGMLCAPIBridge
        return GGMLCAPIBridge(device=0)
