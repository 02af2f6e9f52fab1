"""Build (once per source content) the LM host-emulation library: tests/hostlib.py's sources plus the LM engine
(runtime/lm.cpp) and tests/host/lm_emul.cpp, the host restatement of kernels/lm_decode.hip."""
import hashlib
import os
import subprocess
import tempfile

from hostlib import CLANG, CSRC, ROOT, RUNTIME

LM_RUNTIME = RUNTIME + ("lm.cpp", "selftest_lm.cpp")   # selftest_lm.cpp: the ace_mi_kernel_lm_* entries over lm_emul.cpp
EMUL = ("kernel_emul.cpp", "lm_emul.cpp")


def lm_host_sources():
    return [os.path.join(CSRC, "runtime", f) for f in LM_RUNTIME] + [os.path.join(ROOT, "tests", "host", f) for f in EMUL]


def host_flags():
    return ["-std=c++17", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC, "-ffp-contract=off",
            "-pthread", "-Wno-unused-result"]


def build_lm_host_lib() -> str:
    h = hashlib.sha1(" ".join(LM_RUNTIME + EMUL).encode())
    for d in (os.path.join(CSRC, "runtime"), CSRC, os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host")):
        for f in sorted(os.listdir(d)):
            if f.endswith((".cpp", ".h")):
                with open(os.path.join(d, f), "rb") as fh:
                    h.update(f.encode() + fh.read())
    out_dir = os.path.join(tempfile.gettempdir(), "acemi_lmhostlib_" + h.hexdigest()[:16])
    out = os.path.join(out_dir, "libacestep_mi355x_lmhost.so")
    if not os.path.exists(out):
        os.makedirs(out_dir, exist_ok=True)
        tmp = out + f".{os.getpid()}.tmp"
        subprocess.run([CLANG, "-O2", "-shared", "-Wl,-Bsymbolic", *host_flags(), *lm_host_sources(), "-o", tmp], check=True)
        os.replace(tmp, out)
    return out
