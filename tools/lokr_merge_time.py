"""Time of the LoKr image build on the headline DiT (24 layers, bf16): a LyCORIS LoKr adapter on q/k/v/o of self and
cross attention of every layer is loaded and its images rebuilt a few times (ace_mi_dit_set_lora_scale;
lora_info()["merge_ms"] = first launch to completion of the factor and merge launches, host clock around a stream
synchronise).  Prints one JSON line: ms per build, bytes moved (2 B read + 2 B written per adapted weight, plus the
factors once) and GB/s.
Usage: python tools/lokr_merge_time.py [form=full] [rank=16] [builds=5]   (form: full | w2_lowrank | both_lowrank)"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ace-step-1.5-ggml_amd"))
import bench  # noqa: E402
from acestep_mi355x.capi import GGMLCAPIBridge  # noqa: E402
from acestep_mi355x.synthetic import (LORA_ATTN_TARGETS, _expand_targets, lokr_factorization, lora_module_dims,  # noqa: E402
                                      make_config, write_lokr_adapter)

form = sys.argv[1] if len(sys.argv) > 1 else "full"
r = int(sys.argv[2]) if len(sys.argv) > 2 else 16
builds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
cfg = make_config()
ckpt = bench.workload_checkpoint()
with tempfile.TemporaryDirectory() as d:
    write_lokr_adapter(d, cfg, r=r, alpha=2.0 * r, form=form, targets=LORA_ATTN_TARGETS, seed=0, dtype="BF16")
    br = GGMLCAPIBridge(device=0)
    br.load_dit(ckpt)
    br.load_lora(d, 1.0)
    ms = [br.lora_info()["merge_ms"]]
    for i in range(builds):
        br.set_lora_scale(0.5 + 0.1 * i)
        ms.append(br.lora_info()["merge_ms"])
    info = br.lora_info()
    br.close()
weights = factors = 0
shapes = {}
for m in _expand_targets(LORA_ATTN_TARGETS):
    fin, fout = lora_module_dims(cfg, m)
    (a, c), (b, dd) = lokr_factorization(fout), lokr_factorization(fin)
    shapes[m] = [a, b, c, dd]
    weights += fin * fout * cfg["num_hidden_layers"]
    factors += 4 * cfg["num_hidden_layers"] * ((r * (a + b) if form == "both_lowrank" else a * b) +
                                               (c * dd if form == "full" else r * (c + dd)))
best = min(ms[1:])
moved = 4 * weights + factors
print(json.dumps(dict(form=form, rank=r, modules=info["num_modules"], images=info["num_images"],
                      image_bytes=info["image_bytes"], kron_shapes=shapes, first_ms=round(ms[0], 3),
                      rebuild_ms=[round(x, 3) for x in ms[1:]], best_ms=round(best, 3), adapted_weights=weights,
                      bytes_moved=moved, gb_per_s=round(moved / best / 1e6, 1))))
