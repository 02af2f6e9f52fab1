#!/usr/bin/env python
"""Wall time of one auto score (the reference's calculate_pmi_score_per_condition: eight targets against one prompt,
seven of about 10 tokens and one of about 500) on the engine, synthetic BF16 weights at the Qwen3-0.6B shape, two ways:

  full    eight ace_mi_lm_score calls on prompt + target (what hook.install_lm_backend does by default);
  reuse   one prefill of the prompt, then per target ace_mi_lm_truncate(P - 1) + ace_mi_lm_extend([last prompt token] +
          target, score_from = 1) (reuse_score_prompt=True).

Each way runs --reps times after one warm run; the table gives the median per prompt length.  Run it under
`rocprofv3 --kernel-trace --stats` for the chunk attention kernel's own time per launch (= per layer).

  python tools/lm_score_reuse_time.py [--prompts 1200,3000] [--reps 5] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ace-step-1.5-ggml_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

TARGETS = (10,) * 7 + (500,)


def main():
    import torch
    from acestep_mi355x.capi import GGMLCAPIBridge
    from lm_decode_time import SHAPES, _write
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompts", default="1200,3000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--vocab", type=int, default=151936)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    cfg = dict(SHAPES["0.6b"], vocab_size=a.vocab)
    rows = []
    with tempfile.TemporaryDirectory() as d:
        br = GGMLCAPIBridge(device=0)
        br.load_lm(_write(d, cfg))
        g = torch.Generator().manual_seed(3)
        for P in (int(p) for p in a.prompts.split(",")):
            ids = torch.randint(0, a.vocab, (1, P + max(TARGETS)), generator=g, dtype=torch.int32).cuda()

            def full():
                for T in TARGETS:
                    br.lm_begin(1, P + T)
                    br.lm_score(ids[:, :P + T], None, P)

            def reuse():
                br.lm_begin(1, P + max(TARGETS))
                br.lm_forward(ids[:, :P], None)
                for T in TARGETS:
                    br.lm_truncate(P - 1)
                    br.lm_extend(ids[:, P - 1:P + T], None, score_from=1)

            ms = {}
            for name, fn in (("full", full), ("reuse", reuse)):
                fn()
                torch.cuda.synchronize()
                t = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    t.append((time.perf_counter() - t0) * 1e3)
                ms[name] = statistics.median(t)
            rows.append(dict(prompt=P, full_ms=ms["full"], reuse_ms=ms["reuse"], ratio=ms["full"] / ms["reuse"]))
            print(f"P {P}: full {ms['full']:.2f} ms, reuse {ms['reuse']:.2f} ms, ratio {ms['full'] / ms['reuse']:.2f}x", flush=True)
        br.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f)


if __name__ == "__main__":
    main()
