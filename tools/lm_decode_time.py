#!/usr/bin/env python
"""ms per decode step of the engine's causal LM (ace_mi_lm_forward, n = 1) with synthetic weights at the Qwen3-0.6B and
Qwen3-1.7B shapes (the models' public config.json), beside two numbers from the same run:

  * the bytes a step must read (every layer's matrices and the head once, plus the KV cache of B sequences) divided by
    the HBM bandwidth (8.0 TB/s peak, 6.3 TB/s measured achievable);
  * the per-token time of transformers' Qwen3ForCausalLM in torch eager (bf16) on the same GPU with the same weights,
    called as the reference's _forward_pass calls it: model(input_ids=[B, 1], attention_mask, past_key_values,
    use_cache=True).

The 5 Hz LM extends the stock vocabulary with audio-code tokens: --vocab sets the size (default: stock Qwen3, 151936).
Each step is timed on its own with a pair of events after warm-up steps; the table gives median, min and max.

--gguf Q8_0,Q4_K,Q6_K adds, per type, the same engine measurement on a GGUF checkpoint of that type at the same shape
(every 2-D tensor in random valid blocks of the type, norms F32, tied head: the step then runs kernels/lm_decode_q.hip
on the block planes, 1.125 / 0.75 / 1.25 bytes per weight); torch eager is measured for the dense checkpoint only.

--generate measures the audio-code phase instead (B = 2 as one CFG pair, cache 1024, candidates = 64 000 contiguous ids
+ EOS, top-k off / 50 x top-p off / 0.9), ms per token of
  (a) the engine step alone (ace_mi_lm_forward, n = 1);
  (b) the path without the engine loop: the step plus the per-token torch work of the reference's loops restated here
      (CFG mix, mask add, temperature, topk, the full sort / softmax / cumsum / scatter of top-p, softmax, multinomial,
      .item(), the EOS test and the two torch.cat that grow the ids and the mask);
  (c) ace_mi_lm_generate: --calls calls of --steps tokens each, the call's wall time / tokens (the prefill is outside);
  and the selection kernel alone (ace_mi_lm_select).  (a), (b) and the kernel are timed per token with event pairs.

  python tools/lm_decode_time.py --models 0.6b,1.7b --steps 30 --warmup 5 [--gguf Q8_0,Q4_K,Q6_K] [--no-torch]
                                 [--json out.json]
  python tools/lm_decode_time.py --generate --models 0.6b,1.7b --steps 30 --warmup 5 [--calls 5] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ace-step-1.5-ggml_amd"))
sys.path.insert(0, ROOT)

SHAPES = {  # Qwen/Qwen3-0.6B and Qwen/Qwen3-1.7B config.json
    "0.6b": dict(hidden_size=1024, num_hidden_layers=28, num_attention_heads=16, num_key_value_heads=8,
                 intermediate_size=3072, head_dim=128, max_position_embeddings=40960, rms_norm_eps=1e-6,
                 rope_theta=1000000.0),
    "1.7b": dict(hidden_size=2048, num_hidden_layers=28, num_attention_heads=16, num_key_value_heads=8,
                 intermediate_size=6144, head_dim=128, max_position_embeddings=40960, rms_norm_eps=1e-6,
                 rope_theta=1000000.0),
}
HBM_PEAK, HBM_MEASURED = 8.0e12, 6.3e12


PLANE_BYTES = {"Q8_0": 1.125, "Q4_K": 0.75, "Q6_K": 1.25}   # resident (and read) bytes per weight of the block planes


def step_bytes(cfg, B, cache_len, bytes_per_weight=2.0):
    H, I, D = cfg["hidden_size"], cfg["intermediate_size"], cfg["head_dim"]
    qd, kd = cfg["num_attention_heads"] * D, cfg["num_key_value_heads"] * D
    layer = (qd + 2 * kd) * H + H * qd + 2 * I * H + H * I
    weights = int((cfg["num_hidden_layers"] * layer + cfg["vocab_size"] * H) * bytes_per_weight)
    cache = B * cache_len * cfg["num_hidden_layers"] * 2 * kd * 2          # K and V, fp16
    return weights, cache


def time_steps(step, n_warm, n_steps):
    import torch
    for _ in range(n_warm):
        step()
    ms = []
    for _ in range(n_steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms))


def engine_times(ckpt, cfg, Bs, lens, warm, steps):
    import torch
    from acestep_mi355x.capi import GGMLCAPIBridge
    br = GGMLCAPIBridge()
    br.load_lm(ckpt)
    out = {}
    g = torch.Generator().manual_seed(0)
    for B in Bs:
        for L in lens:
            br.lm_begin(B, L + warm + steps)
            ids = torch.randint(0, cfg["vocab_size"], (B, L), generator=g, dtype=torch.int32).cuda()
            br.lm_forward(ids)
            tok = ids[:, :1].contiguous()
            out[(B, L)] = time_steps(lambda: br.lm_forward(tok), warm, steps)
    br.close()
    return out


def generate_times(ckpt, cfg, warm, steps, calls, cache=1024, n_codes=64000):
    """rows of the --generate table for one checkpoint"""
    import time
    import torch
    from acestep_mi355x.capi import GGMLCAPIBridge
    br = GGMLCAPIBridge()
    br.load_lm(ckpt)
    V, B, S, cfg_scale, temp = cfg["vocab_size"], 2, 1, 2.0, 0.85
    eos = V - n_codes - 10
    allowed = torch.cat([torch.tensor([eos]), torch.arange(V - n_codes, V)]).to(torch.int32).cuda()
    mask = torch.full((1, V), float("-inf"), device="cuda")
    mask[0, allowed.long()] = 0
    g = torch.Generator().manual_seed(0)
    prompt = torch.randint(0, V, (B, cache), generator=g, dtype=torch.int32).cuda()
    rows = []

    def fresh():
        br.lm_begin(B, cache + (warm + steps) * (calls + 2))
        return br.lm_forward(prompt)

    for top_k in (0, 50):
        for top_p in (1.0, 0.9):
            kw = dict(allowed_ids=allowed, stop_id=eos, cfg_scale=cfg_scale, pre_temperature=temp, temperature=temp,
                      top_k=top_k, top_p=top_p)
            logits = fresh()
            tok = prompt[:, :1].contiguous()
            a_ms = time_steps(lambda: br.lm_forward(tok), warm, steps)
            u = torch.full((S,), 0.5, device="cuda")
            k_ms = time_steps(lambda: br.lm_select(logits, uniforms=u, min_tokens=10 ** 6, **kw), warm, steps)
            state = dict(ids=prompt.long(), am=torch.ones((B, cache), dtype=torch.long, device="cuda"), logits=fresh())

            def parent():
                x = state["logits"]
                z = x[S:].float() + cfg_scale * (x[:S].float() - x[S:].float())
                z = z + mask
                z[:, eos] = float("-inf")
                z = z / temp
                gone = torch.full_like(z, float("-inf"))
                if top_k:       # one topk launch, then the mask
                    floor = torch.topk(z, top_k, dim=-1).values.amin(dim=-1, keepdim=True)
                    z = torch.where(z >= floor, z, gone)
                if top_p < 1.0:  # the full descending sort, softmax and running sum, and the scatter back to id order
                    order = torch.argsort(z, dim=-1, descending=True)
                    mass = torch.cumsum(torch.softmax(torch.gather(z, 1, order).float(), dim=-1), dim=-1)
                    before = torch.roll(mass, 1, dims=-1)       # mass strictly ahead of each rank
                    before[:, 0] = 0.0
                    drop = torch.zeros_like(z, dtype=torch.bool).scatter(1, order, before > top_p)
                    z = torch.where(drop, gone, z)
                nxt = torch.multinomial(torch.softmax(z.float() / temp, dim=-1), num_samples=1).squeeze(1)
                for b in range(S):
                    nxt[b].item()
                bool(torch.any(nxt == eos))
                col = nxt.unsqueeze(1).repeat(2, 1)
                state["ids"] = torch.cat([state["ids"], col], dim=1)
                state["am"] = torch.cat([state["am"], torch.ones((B, 1), device="cuda", dtype=torch.long)], dim=1)
                state["logits"] = br.lm_forward(col)
            b_ms = time_steps(parent, warm, steps)
            logits = fresh()
            br.lm_generate(logits, warm, seed=1, min_tokens=warm, **kw)
            per = []
            for i in range(calls):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                br.lm_generate(logits, steps, seed=2 + i, min_tokens=steps, **kw)
                torch.cuda.synchronize()
                per.append((time.perf_counter() - t0) * 1e3 / steps)
                br.lm_forward(tok)      # the last token of a call is not fed back: the next call needs fresh logits
            c_ms = dict(median=statistics.median(per), min=min(per), max=max(per))
            rows.append(dict(top_k=top_k, top_p=top_p, step=a_ms, parent=b_ms, generate=c_ms, select=k_ms))
    br.close()
    return rows


def torch_times(ckpt, cfg, Bs, lens, warm, steps):
    import torch
    from safetensors.torch import load_file
    from transformers import Qwen3Config, Qwen3ForCausalLM
    hf = Qwen3Config(**{k: v for k, v in cfg.items() if k not in ("architectures",)}, attention_bias=False)
    with torch.device("cuda"):
        model = Qwen3ForCausalLM(hf).to(torch.bfloat16).eval()
    missing, unexpected = model.load_state_dict(load_file(os.path.join(ckpt, "model.safetensors"), device="cuda"),
                                                strict=False)
    assert not unexpected, unexpected
    model.tie_weights()
    out = {}
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for B in Bs:
            for L in lens:
                ids = torch.randint(0, cfg["vocab_size"], (B, L), generator=g).cuda()
                state = {"mask": torch.ones((B, L), dtype=torch.long, device="cuda")}
                state["past"] = model(input_ids=ids, attention_mask=state["mask"], use_cache=True).past_key_values
                tok = ids[:, :1].contiguous()

                def step():
                    state["mask"] = torch.cat([state["mask"], state["mask"][:, :1]], dim=1)
                    o = model(input_ids=tok, attention_mask=state["mask"], past_key_values=state["past"], use_cache=True)
                    state["past"] = o.past_key_values
                    return o.logits[:, -1, :]
                out[(B, L)] = time_steps(step, warm, steps)
                del state
    del model
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="0.6b,1.7b")
    ap.add_argument("--vocab", type=int, default=151936)
    ap.add_argument("--batch", default="1,2")
    ap.add_argument("--cache", default="256,1024,4096")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--gguf", default="", help="comma-separated block types (Q8_0, Q4_K, Q6_K) to time as GGUF files")
    ap.add_argument("--json", default=None)
    ap.add_argument("--generate", action="store_true", help="time the audio-code phase: step, per-token torch path, engine loop")
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    if a.generate:
        return main_generate(a)
    Bs, lens = [int(x) for x in a.batch.split(",")], [int(x) for x in a.cache.split(",")]
    rows = []
    print("| model | B | cache | engine ms/step median (min-max) | bytes/step MB (weights + cache) | bytes / 8.0 TB/s ms "
          "| bytes / 6.3 TB/s ms | torch eager ms/token median (min-max) | torch / engine |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name in a.models.split(","):
        cfg = dict(SHAPES[name], vocab_size=a.vocab)
        with tempfile.TemporaryDirectory(prefix="acemi_lmtime_") as d:
            _write(d, cfg)
            eng = engine_times(d, cfg, Bs, lens, a.warmup, a.steps)
            ref = {} if a.no_torch else torch_times(d, dict(cfg, tie_word_embeddings=True), Bs, lens, a.warmup, a.steps)
        runs = [(name, 2.0, eng, ref)]
        for qt in [q for q in a.gguf.split(",") if q]:
            with tempfile.TemporaryDirectory(prefix="acemi_lmtime_gguf_") as d:
                _write_gguf(d, cfg, qt)
                runs.append((f"{name} {qt}", PLANE_BYTES[qt], engine_times(d, cfg, Bs, lens, a.warmup, a.steps), {}))
        for label, bpw, eng, ref in runs:
            for B in Bs:
                for L in lens:
                    w, c = step_bytes(cfg, B, L, bpw)
                    e, t = eng[(B, L)], ref.get((B, L))
                    name = label
                    row = dict(model=name, B=B, cache=L, engine_ms=e, weight_bytes=w, cache_bytes=c,
                               roofline_peak_ms=(w + c) / HBM_PEAK * 1e3, roofline_measured_ms=(w + c) / HBM_MEASURED * 1e3,
                               torch_ms=t)
                    rows.append(row)
                    ts = f"{t['median']:.3f} ({t['min']:.3f}-{t['max']:.3f})" if t else "-"
                    ratio = f"{t['median'] / e['median']:.2f}x" if t else "-"
                    print(f"| {name} | {B} | {L} | {e['median']:.3f} ({e['min']:.3f}-{e['max']:.3f}) | "
                          f"{(w + c) / 1e6:.0f} ({w / 1e6:.0f} + {c / 1e6:.0f}) | {row['roofline_peak_ms']:.3f} | "
                          f"{row['roofline_measured_ms']:.3f} | {ts} | {ratio} |", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


def main_generate(a):
    fmt = lambda t: f"{t['median']:.3f} ({t['min']:.3f}-{t['max']:.3f})"
    print("| model | top-k | top-p | (a) step ms | (b) step + torch per-token ms | (c) lm_generate ms/token | select alone ms "
          "| (c) - (a) | (c) <= (b) |")
    print("|---|---|---|---|---|---|---|---|---|")
    out = []
    for name in a.models.split(","):
        cfg = dict(SHAPES[name], vocab_size=a.vocab)
        with tempfile.TemporaryDirectory(prefix="acemi_lmtime_") as d:
            _write(d, cfg)
            for r in generate_times(d, cfg, a.warmup, a.steps, a.calls):
                out.append(dict(r, model=name))
                print(f"| {name} | {r['top_k'] or 'off'} | {r['top_p'] if r['top_p'] < 1 else 'off'} | {fmt(r['step'])} | "
                      f"{fmt(r['parent'])} | {fmt(r['generate'])} | {fmt(r['select'])} | "
                      f"{r['generate']['median'] - r['step']['median']:.3f} | "
                      f"{'yes' if r['generate']['median'] <= r['parent']['median'] else 'NO'} |", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


def _write(d, cfg):
    """write_lm_checkpoint with the multi-threaded torch generator (hundreds of millions of values)."""
    from acestep_mi355x.synthetic import lm_tensor_specs, write_checkpoint
    cfg = dict(cfg, architectures=["Qwen3ForCausalLM"], tie_word_embeddings=True)
    return write_checkpoint(d, cfg, seed=1, dtype="BF16", backend="torch", specs=lm_tensor_specs(cfg, tied=True))


def _write_gguf(d, cfg, qtype):
    """config.json + model.gguf: every 2-D tensor in random valid blocks of qtype (synthetic.random_blocks: timing needs
    bytes, not values), norms F32 ones, no lm_head.weight (tied)."""
    import numpy as np
    from acestep_mi355x.synthetic import lm_tensor_specs, random_blocks, write_gguf_tensors
    cfg = dict(cfg, architectures=["Qwen3ForCausalLM"], tie_word_embeddings=True)
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(cfg, f)
    rng = np.random.default_rng(1)
    tensors = {}
    for name, shape, kind in lm_tensor_specs(cfg, tied=True):
        if kind == "norm":
            tensors[name] = (shape, "F32", np.ones(shape, "<f4").tobytes())
        else:
            tensors[name] = (shape, qtype, random_blocks(qtype, shape[0], shape[1], rng).tobytes())
    return write_gguf_tensors(os.path.join(d, "model.gguf"), tensors)


if __name__ == "__main__":
    main()
