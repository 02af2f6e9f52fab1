"""Time of the LoRA image build on the headline DiT (24 layers, bf16): an adapter on all seven projections of self
attention, cross attention and the MLP of every layer is loaded and its images rebuilt a few times
(ace_mi_dit_set_lora_scale; lora_info()["merge_ms"] = launch to completion of the merge launches).  Prints one JSON
line: ms per build, bytes moved (2 B read + 2 B written per adapted weight, plus A and B once) and GB/s.
Usage: python tools/lora_merge_time.py [rank=64] [builds=5]"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ace-step-1.5-ggml_amd"))
import bench  # noqa: E402
from acestep_mi355x.capi import GGMLCAPIBridge  # noqa: E402
from acestep_mi355x.synthetic import LORA_ALL_TARGETS, lora_module_dims, make_config, write_lora_adapter  # noqa: E402

r = int(sys.argv[1]) if len(sys.argv) > 1 else 64
builds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
cfg = make_config()
ckpt = bench.workload_checkpoint()
with tempfile.TemporaryDirectory() as d:
    write_lora_adapter(d, cfg, r=r, alpha=2.0 * r, targets=LORA_ALL_TARGETS, seed=0, dtype="BF16")
    br = GGMLCAPIBridge(device=0)
    br.load_dit(ckpt)
    br.load_lora(d, 1.0)
    ms = [br.lora_info()["merge_ms"]]
    for i in range(builds):
        br.set_lora_scale(0.5 + 0.1 * i)
        ms.append(br.lora_info()["merge_ms"])
    info = br.lora_info()
    br.close()
weights = ab = 0
for m in LORA_ALL_TARGETS:
    fin, fout = lora_module_dims(cfg, m)
    weights += fin * fout * cfg["num_hidden_layers"]
    ab += r * (fin + fout) * 4 * cfg["num_hidden_layers"]
best = min(ms[1:])
moved = 4 * weights + ab
print(json.dumps(dict(rank=r, modules=info["num_modules"], images=info["num_images"], image_bytes=info["image_bytes"],
                      first_ms=round(ms[0], 3), rebuild_ms=[round(x, 3) for x in ms[1:]], best_ms=round(best, 3),
                      adapted_weights=weights, bytes_moved=moved, gb_per_s=round(moved / best / 1e6, 1),
                      valu_ops_per_weight=2 * r)))
