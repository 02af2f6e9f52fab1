"""The checks of tests/dit_capture_cases.py on the host library (the product's runtime with the host restatements of the
kernels, "device" pointers = host pointers): the capture entry's validation, the walk's launch point, pair order, early
exit, the q8 parity walk and the hook's tuple, on a machine without a GPU.  tests/test_gpu_dit_capture.py runs them on
the MI355X."""
import os
import tempfile

import pytest

import dit_capture_cases as dc
from hostlib import CLANG, build_host_lib


@pytest.fixture(scope="module")
def tiny_ckpt():
    from acestep_mi355x.synthetic import TINY_CONFIG, write_checkpoint
    d = tempfile.mkdtemp(prefix="acemi_capc_")
    write_checkpoint(d, TINY_CONFIG, seed=0, dtype="BF16")
    return d


@pytest.fixture(scope="module")
def env(tiny_ckpt):
    if not os.path.exists(CLANG):
        pytest.skip("host clang++ not available")
    br = TestDitCaptureOnHostLibrary.bridge()
    br.load_dit(tiny_ckpt)
    yield br, dc.HostMem(), "cpu"
    br.close()


class TestDitCaptureOnHostLibrary(dc.DitCaptureChecks):
    @staticmethod
    def bridge():
        from acestep_mi355x.capi import GGMLCAPIBridge
        br = GGMLCAPIBridge(lib_path=build_host_lib())
        br.host_memory = True
        return br
