"""The checks of tests/vae_kernel_cases.py against the host emulation of the VAE conv kernels (tests/host/kernel_emul.cpp
through the ace_mi_kernel_conv_gemm / conv_out / pack_f16 entries of the host library): proves the float64 references,
the bounds, the fragile-share cap and the entries' buffer handling on a machine without a GPU.
tests/test_gpu_vae_kernels.py runs the same checks on the gfx950 kernels."""
import ctypes

import pytest

import vae_kernel_cases as vk


@pytest.fixture(scope="module")
def k():
    from hostlib import build_host_lib
    return vk.runners(ctypes.CDLL(build_host_lib()))


class TestVaeKernelsOnHostEmulation(vk.VaeKernelChecks):
    IMPL = vk.EMULATION
