"""Time of the raw-block expansion (kernels/dequant_blocks.hip) per ggml type at the gate|up shape (12288 x 2048) and at
an N = 2048 projection (2048 x 2048), with the plane kernel (launch_dequant_bf16, unchanged) on the same Q8_0 / Q4_K /
Q6_K blocks in the same run as the baseline.  Each figure is the average of `iters` launches that rotate through enough
buffer copies to exceed the memory-side cache, after 3 warm-up launches; `repeats` such runs give the median and the
spread.  Prints one JSON line per (type, shape): ms (median, min, max), bytes per weight (read + 2 written), GB/s, and
for the three shared types the raw / planes ratio.
Usage: python tools/dequant_blocks_time.py [iters=20] [repeats=5]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ace-step-1.5-ggml_amd"))
from acestep_mi355x import capi  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
PLANE_READ = {"q8_0": 1.0 + 4 / 32, "q4_k": 0.5 + 8 / 32, "q6_k": 1.0 + 4 / 16}  # q plane + f32 scales, per weight
for N, K in ((12288, 2048), (2048, 2048)):
    for qtype in ("q4_0", "q4_1", "q5_0", "q5_1", "iq4_nl", "q2_k", "q3_k", "q5_k", "q8_0", "q4_k", "q6_k"):
        bv, bb = capi._BLOCK[qtype]
        row = {"type": qtype, "N": N, "K": K}
        for planes in ((False, True) if qtype in PLANE_READ else (False,)):
            ms = [capi.bench_dequant_blocks(qtype, N, K, iters, planes=planes) for _ in range(repeats)]
            med = statistics.median(ms)
            bpw = (PLANE_READ[qtype] if planes else bb / bv) + 2.0
            row["planes" if planes else "raw"] = {"ms": round(med, 4), "min": round(min(ms), 4), "max": round(max(ms), 4),
                                                  "bytes_per_weight": round(bpw, 4),
                                                  "GBps": round(N * K * bpw / med / 1e6, 1)}
        if "planes" in row:
            row["raw_over_planes"] = round(row["raw"]["ms"] / row["planes"]["ms"], 3)
        print(json.dumps(row), flush=True)
