"""GPU parity of the VAE conv kernels (kernels/vae.hip), one by one through the ace_mi_kernel_conv_gemm /
ace_mi_kernel_conv_out / ace_mi_kernel_pack_f16 self-test entries, against the float64 references of
tests/vae_kernel_cases.py: every instance of conv_gemm_kernel (fused or not x halo dilation 0, 1, 3, 9), the three index
maps (conv, strided conv, transposed conv with centre crop), several sequences per launch, tiles that straddle
sequences, the ragged last M-group, sequences shorter than their halo, conv_out's strips and the fp16 packers.
tests/test_vae_kernels_cpu.py runs the same checks on the host emulation."""
import pytest

import vae_kernel_cases as vk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def k():
    return vk.runners()


class TestVaeKernelsOnGpu(vk.VaeKernelChecks):
    IMPL = vk.KERNEL
