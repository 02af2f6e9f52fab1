"""CPU checks of the LM cache fan-out on the LM host library (tests/lmhostlib.py): the host restatement of the kernel
(kernels/lm_fanout_host.h) through ace_mi_kernel_lm_cache_fanout, the runtime entries ace_mi_lm_fanout /
ace_mi_lm_uniforms, a stand-alone driver of them under ASan + UBSan, and hook.install_lm_backend's batch_codes switch.
The cases are those of tests/lm_fanout_cases.py, which test_gpu_lm_fanout.py runs on the GPU."""
import pytest

import lm_cases as lc
import lm_fanout_cases as fc


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


@pytest.mark.parametrize("case", fc.kernel_cases(), ids=fc.case_id)
def test_fanout_kernel_copies_bits(lib, case):
    fc.run_kernel_case(case, lib)


def test_fanout_kernel_refusals(lib):
    fc.run_kernel_refusals(lib)


@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("params", [fc.SAMPLED, fc.ARGMAX], ids=["sampled", "argmax"])
def test_fanout_equals_sequential_runs(bridge, S, params):
    fc.run_equality(bridge, "cpu", S, params)


def test_uniforms(bridge):
    fc.run_uniforms(bridge, "cpu")


def test_fanout_refusals(bridge):
    fc.run_refusals(bridge, "cpu")


def test_fanout_before_load():
    from lmhostlib import build_lm_host_lib
    fc.run_not_loaded(build_lm_host_lib(), "cpu")


def test_fanout_under_asan_ubsan():
    """tests/host/lm_fanout_asan_driver.cpp, a stand-alone program, over the host-emulated kernels with ASan + UBSan."""
    import os
    import subprocess
    import tempfile
    from lmhostlib import CLANG, host_flags, lm_host_sources, ROOT
    if not os.path.exists(CLANG):
        pytest.skip("host clang++ not available")
    exe = os.path.join(tempfile.mkdtemp(prefix="acemi_lm_fanout_asan_"), "lm_fanout_asan_driver")
    subprocess.run([CLANG, "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-fno-sanitize-recover=undefined", *host_flags(), *lm_host_sources(),
                    os.path.join(ROOT, "tests", "host", "lm_fanout_asan_driver.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, lc.checkpoint("tied")], capture_output=True, text=True, timeout=600, env=env)
    print(r.stdout[-2000:], r.stderr[-6000:])
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stderr[-6000:]


@pytest.mark.parametrize("n_items", [3, 5])
@pytest.mark.parametrize("seeds", [[11, 12, 13, 14, 15], None], ids=["seeds", "torch_seed"])
def test_hook_batch_codes_equals_sequential(bridge, n_items, seeds):
    """5 items under CFG: groups of 4 + 1"""
    fc.run_hook_equal(bridge, "cpu", n_items, 2.0, seeds)


def test_hook_batch_codes_without_cfg(bridge):
    """one row per item: 3 items in one group of up to 8"""
    fc.run_hook_equal(bridge, "cpu", 3, 1.0, [21, 22, 23])


def test_hook_batch_codes_fallbacks(bridge):
    fc.run_hook_fallbacks(bridge, "cpu")
