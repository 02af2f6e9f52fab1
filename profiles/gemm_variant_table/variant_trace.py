"""Launches of every forced GEMM variant (dense bf16: four each; Q8_0: one each), then a tiny DiT forward (the fused-prep GEMM); run under a
kernel trace from the root of a built tree."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.getcwd()
sys.path.insert(0, os.path.join(ROOT, "ace-step-1.5-ggml_amd"))
sys.path.insert(0, ROOT)
from acestep_mi355x import capi  # noqa: E402
from acestep_mi355x.capi import GGMLCAPIBridge  # noqa: E402
from acestep_mi355x.synthetic import TINY_CONFIG, write_checkpoint  # noqa: E402
from oracle.ggml_numerics import f32_to_bf16_bits  # noqa: E402

M, N, K = 300, 512, 256
DENSE = list(range(0, 17)) + [18]
DENSE += [200 + v for v in (1, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)]
QUANT = [0, 1, 2, 3, 4, 5, 7, 20, 21, 22, 23, 24, 25, 222, 223]

rng = np.random.default_rng(0)
a = f32_to_bf16_bits(rng.standard_normal((M, K)).astype(np.float32))
w = (rng.standard_normal((N, K)) * 0.05).astype(np.float32)
wb = f32_to_bf16_bits(w)
blocks = capi.quantize(w, "q8_0")
sums = []
# (capi.gemm_variant forces the product library's picker; the dense self-test GEMMs run in the self-test library, which
#  has a picker state of its own -- ace_mi_bench_gemm forces that one: 3 warm-up launches + 1 timed per id)
for v in DENSE:
    capi.bench_gemm(M, N, K, variant=v, epi=0, act_type=0, iters=1)
    sums.append(("dense", v, 0.0))
for v in QUANT:
    out = capi.kernel_gemm_q(a, blocks, "q8_0", epi=0, variant=v)
    sums.append(("q8_0", v, float(np.abs(out).sum())))
with tempfile.TemporaryDirectory() as d:
    write_checkpoint(d, TINY_CONFIG, seed=0, dtype="BF16")
    br = GGMLCAPIBridge(device=0)
    br.load_dit(d)
    T, L = 96, 16
    h = rng.standard_normal((T, 64)).astype(np.float32)
    c = rng.standard_normal((T, 128)).astype(np.float32)
    e = rng.standard_normal((L, TINY_CONFIG["hidden_size"])).astype(np.float32)
    got = br.dit_forward_tfirst(h, c, e, None, None, 0.75, 0.75)
    br.close()
sums.append(("forward", -1, float(np.abs(got).sum())))
for s in sums:
    print(*s)
print("launches:", len(DENSE) + len(QUANT), "+ one forward")
