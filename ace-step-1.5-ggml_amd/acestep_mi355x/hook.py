"""`decoder.forward` drop-in for the ACE-Step Python pipeline.

Mirrors `_install_ggml_dit_backend` (scripts/run_non_ggml_real_case.py:445-538): it
replaces `dit_handler.model.decoder.forward` with a function of the same keyword
signature (hidden_states, timestep, timestep_r, attention_mask,
encoder_hidden_states, encoder_attention_mask, context_latents, use_cache,
past_key_values, ..., output_attentions) returning `(pred, past_key_values[, None])`
(or the cross-attention maps in place of `None` when a `custom_layers_config` selects heads),
and marks the handler with `_ggml_dit_backend` / `_ggml_dit_decoder_forward_hooked`
(read by acestep/handler.py:2740-2746).

Unlike the reference hook (device->host copy, serial per-item ctypes calls, host->device
copy every step, :502-529), tensors already on the GPU are handed over as device
pointers on torch's current stream and the whole batch runs in one call
(`ace_mi_dit_forward_batched`, <= 8 items per launch).  CPU tensors go through the
reference host-pointer entry `ace_ggml_dit_forward`, one item at a time; both paths
compute on the MI355X.
"""
from __future__ import annotations

import types
from typing import Any

import numpy as np

MAX_BATCH_PER_CALL = 8


def _timesteps(ts, bsz: int, device, torch):
    """timestep(_r) as a float32 [bsz] tensor on `device` (tensor scalar/[B], list or float)."""
    if isinstance(ts, torch.Tensor):
        t = ts.detach().to(device=device, dtype=torch.float32).reshape(-1)
        if t.numel() == 1:
            t = t.expand(bsz)
        return t.contiguous()
    if isinstance(ts, (list, tuple)):
        return torch.tensor([float(x) for x in ts], dtype=torch.float32, device=device)
    return torch.full((bsz,), float(ts), dtype=torch.float32, device=device)


def _mask(m, shape, device, torch):
    if m is None:
        return None
    return (m.detach().to(device) > 0).to(torch.int32).reshape(shape).contiguous()


def dit_forward_torch(bridge, hidden_states, timestep, timestep_r, attention_mask, encoder_hidden_states,
                      encoder_attention_mask, context_latents):
    """One batched DiT step on torch tensors; returns pred with hidden_states' dtype/device."""
    import torch

    hs = hidden_states.detach()
    bsz, seq_len, audio = hs.shape
    dev = hs.device
    ctx = context_latents.detach().to(device=dev, dtype=torch.float32).contiguous()
    enc = encoder_hidden_states.detach().to(device=dev, dtype=torch.float32).contiguous()
    x = hs.to(dtype=torch.float32).contiguous()
    am = _mask(attention_mask, (bsz, seq_len), dev, torch)
    eam = _mask(encoder_attention_mask, (bsz, enc.shape[1]), dev, torch)
    t = _timesteps(timestep, bsz, dev, torch)
    r = _timesteps(timestep_r, bsz, dev, torch)
    enc_len = int(enc.shape[1])
    if dev.type == "cuda":
        out = torch.empty((bsz, seq_len, audio), dtype=torch.float32, device=dev)
        with _OrderedCall(bridge, dev) as stream:
            for b0 in range(0, bsz, MAX_BATCH_PER_CALL):
                b1 = min(bsz, b0 + MAX_BATCH_PER_CALL)
                n = b1 - b0
                bridge.dit_forward_batched_device(
                    n, seq_len, enc_len, x[b0:b1].data_ptr(), ctx[b0:b1].data_ptr(),
                    enc[b0:b1].data_ptr() if enc_len > 0 else 0,
                    am[b0:b1].data_ptr() if am is not None else 0,
                    eam[b0:b1].data_ptr() if eam is not None else 0,
                    t[b0:b1].data_ptr(), r[b0:b1].data_ptr(), out[b0:b1].data_ptr(), stream)
        return out.to(hidden_states.dtype)
    # host tensors: reference host-pointer ABI, one item per call (compute still on the GPU)
    out_np = np.empty((bsz, seq_len, audio), dtype=np.float32)
    am_np = am.numpy() if am is not None else np.ones((bsz, seq_len), np.int32)
    eam_np = eam.numpy() if eam is not None else np.ones((bsz, enc_len), np.int32)
    for b in range(bsz):
        out_np[b] = bridge.dit_forward_tfirst(x[b].numpy(), ctx[b].numpy(), enc[b].numpy(), am_np[b], eam_np[b],
                                              float(t[b]), float(r[b]))
    return torch.from_numpy(out_np).to(dev).to(hidden_states.dtype)


def dit_capture_torch(bridge, hidden_states, timestep, timestep_r, attention_mask, encoder_hidden_states,
                      encoder_attention_mask, context_latents, layers_config, early_exit: bool):
    """One DiT step that also returns the cross-attention maps of `layers_config` = {layer: [heads]} (what the reference
    decoder returns under output_attentions=True with a custom_layers_config; acestep/handler.py get_lyric_timestamp /
    get_lyric_score read it).  Returns (pred, attentions): attentions is a tuple of max(layer) + 1 tensors
    [B, Hq, Np, L] in hidden_states' dtype on its device -- a selected layer holds the captured heads (every other
    head zero), an unselected layer is a stride-0 view of one zero.  With early_exit the walk stops at the last
    selected layer and pred is zeros.  The tensors are handed over as pointers on torch's current stream
    (ace_mi_dit_forward_capture, <= 8 items per call); host tensors are moved to the bridge's GPU and the results back
    (a bridge whose library computes in host memory says so with `host_memory = True`)."""
    import torch

    pairs = [(int(layer), int(h)) for layer in sorted(layers_config) for h in layers_config[layer]]
    if not pairs:
        raise ValueError("custom_layers_config selects no head")
    hs = hidden_states.detach()
    bsz, seq_len, audio = hs.shape
    home = hs.device
    info = bridge.info
    dev = home
    if home.type != "cuda" and not getattr(bridge, "host_memory", False):  # host tensors: computed on the GPU
        dev = torch.device("cuda", max(0, int(info.device)))
    ctx = context_latents.detach().to(device=dev, dtype=torch.float32).contiguous()
    enc = encoder_hidden_states.detach().to(device=dev, dtype=torch.float32).contiguous()
    x = hs.to(device=dev, dtype=torch.float32).contiguous()
    enc_len = int(enc.shape[1])
    am = _mask(attention_mask, (bsz, seq_len), dev, torch)
    eam = _mask(encoder_attention_mask, (bsz, enc_len), dev, torch)
    t = _timesteps(timestep, bsz, dev, torch)
    r = _timesteps(timestep_r, bsz, dev, torch)
    n_heads, patch = int(info.num_heads), int(info.patch_size)
    n_patch = (seq_len + patch - 1) // patch
    out = torch.zeros((bsz, seq_len, audio), dtype=torch.float32, device=dev)
    probs = torch.empty((bsz, len(pairs), n_patch, enc_len), dtype=torch.float32, device=dev)
    with _OrderedCall(bridge, dev) as stream:
        for b0 in range(0, bsz, MAX_BATCH_PER_CALL):
            b1 = min(bsz, b0 + MAX_BATCH_PER_CALL)
            n = b1 - b0
            chunk = torch.empty((len(pairs), n, n_patch, enc_len), dtype=torch.float32, device=dev)
            bridge.dit_forward_capture_device(
                n, seq_len, enc_len, x[b0:b1].data_ptr(), ctx[b0:b1].data_ptr(), enc[b0:b1].data_ptr(),
                am[b0:b1].data_ptr() if am is not None else 0, eam[b0:b1].data_ptr() if eam is not None else 0,
                t[b0:b1].data_ptr(), r[b0:b1].data_ptr(), pairs, bool(early_exit),
                0 if early_exit else out[b0:b1].data_ptr(), chunk.data_ptr(), stream)
            probs[b0:b1] = chunk.transpose(0, 1)
    dtype = hidden_states.dtype
    out, probs = out.to(home), probs.to(home)
    dev = home
    zero = torch.zeros((), dtype=dtype, device=dev)
    attentions = []
    for layer in range(max(layers_config) + 1):
        idx = [j for j, p in enumerate(pairs) if p[0] == layer]
        if not idx:
            attentions.append(zero.expand(bsz, n_heads, n_patch, enc_len))  # stride 0: no memory
            continue
        full = torch.zeros((bsz, n_heads, n_patch, enc_len), dtype=dtype, device=dev)
        full[:, [pairs[j][1] for j in idx]] = probs[:, idx].to(dtype)
        attentions.append(full)
    return out.to(dtype), tuple(attentions)


def install_dit_backend(dit_handler: Any, bridge) -> None:
    """Replace dit_handler.model.decoder.forward with the MI355X engine.

    output_attentions=True with a non-empty custom_layers_config dict (and a bridge that has
    dit_forward_capture_device) returns the cross-attention maps as outputs[2] (dit_capture_torch), so the handler's
    get_lyric_timestamp / get_lyric_score work unmodified; in every other case outputs[2] is None."""
    decoder = dit_handler.model.decoder
    original_forward = decoder.forward

    def decoder_forward_mi355x(self, hidden_states, timestep, timestep_r, attention_mask, encoder_hidden_states,
                               encoder_attention_mask, context_latents, use_cache=None, past_key_values=None,
                               cache_position=None, position_ids=None, output_attentions=False,
                               return_hidden_states=None, custom_layers_config=None, enable_early_exit=False,
                               **flash_attn_kwargs):
        if hidden_states is None or hidden_states.dim() != 3:
            return original_forward(hidden_states=hidden_states, timestep=timestep, timestep_r=timestep_r,
                                    attention_mask=attention_mask, encoder_hidden_states=encoder_hidden_states,
                                    encoder_attention_mask=encoder_attention_mask, context_latents=context_latents,
                                    use_cache=use_cache, past_key_values=past_key_values,
                                    cache_position=cache_position, position_ids=position_ids,
                                    output_attentions=output_attentions, return_hidden_states=return_hidden_states,
                                    custom_layers_config=custom_layers_config,
                                    enable_early_exit=enable_early_exit, **flash_attn_kwargs)
        if (output_attentions and isinstance(custom_layers_config, dict) and custom_layers_config
                and hasattr(bridge, "dit_forward_capture_device")):
            pred, attentions = dit_capture_torch(bridge, hidden_states, timestep, timestep_r, attention_mask,
                                                 encoder_hidden_states, encoder_attention_mask, context_latents,
                                                 custom_layers_config, bool(enable_early_exit))
            return (pred, past_key_values, attentions)
        pred = dit_forward_torch(bridge, hidden_states, timestep, timestep_r, attention_mask, encoder_hidden_states,
                                 encoder_attention_mask, context_latents)
        outputs = (pred, past_key_values)
        if output_attentions:
            outputs += (None,)
        return outputs

    decoder.forward = types.MethodType(decoder_forward_mi355x, decoder)
    setattr(dit_handler, "_ggml_dit_backend", "mi355x-capi")
    setattr(dit_handler, "_ggml_dit_decoder_forward_hooked", True)
    install_lora_backend(dit_handler, bridge)


def install_lora_backend(dit_handler: Any, bridge) -> None:
    """Route the handler's LoRA controls (acestep/core/generation/handler/lora/lifecycle.py:11-106,
    controls.py:12-115) to the engine.  The reference versions wrap `model.decoder` in a PeftModel, which the hooked
    decoder.forward never runs, so an adapter loaded through them would be ignored; these drive
    `bridge.load_lora / set_lora_scale / unload_lora` instead, keep `lora_loaded`, `use_lora` and `lora_scale` as the
    reference methods do, return status strings in their style, need no `peft` and leave `model.decoder` alone."""
    import math
    import os

    for name, default in (("lora_loaded", False), ("use_lora", False), ("lora_scale", 1.0)):
        if not hasattr(dit_handler, name):
            setattr(dit_handler, name, default)

    def load_lora_mi355x(self, lora_path: str) -> str:
        if getattr(self, "model", None) is None:
            return "❌ Model not initialized. Please initialize service first."
        if not lora_path or not str(lora_path).strip():
            return "❌ Please provide a LoRA path."
        lora_path = str(lora_path).strip()
        if not os.path.exists(lora_path):
            return f"❌ LoRA path not found: {lora_path}"
        if not os.path.exists(os.path.join(lora_path, "adapter_config.json")):
            return f"❌ Invalid LoRA adapter: adapter_config.json not found in {lora_path}"
        try:
            bridge.load_lora(lora_path, float(self.lora_scale))
        except Exception as e:  # the previous adapter (if any) stays loaded in the engine
            return f"❌ Failed to load LoRA: {str(e)}"
        self.lora_loaded = True
        self.use_lora = True
        return f"✅ LoRA loaded from {lora_path}"

    def unload_lora_mi355x(self) -> str:
        if not self.lora_loaded:
            return "⚠️ No LoRA adapter loaded."
        try:
            bridge.unload_lora()
        except Exception as e:
            return f"❌ Failed to unload LoRA: {str(e)}"
        self.lora_loaded = False
        self.use_lora = False
        self.lora_scale = 1.0
        return "✅ LoRA unloaded, using base model"

    def set_use_lora_mi355x(self, use_lora: bool) -> str:
        if use_lora and not self.lora_loaded:
            return "❌ No LoRA adapter loaded. Please load a LoRA first."
        self.use_lora = bool(use_lora)
        if self.lora_loaded:
            try:  # off = engine scale 0 (base weights, adapter resident); on = back to the remembered lora_scale
                bridge.set_lora_scale(float(self.lora_scale) if use_lora else 0.0)
            except Exception as e:
                return f"❌ Failed to toggle LoRA: {str(e)}"
        return f"✅ LoRA {'enabled' if use_lora else 'disabled'}"

    def set_lora_scale_mi355x(self, scale: float) -> str:
        if not self.lora_loaded:
            return "⚠️ No LoRA loaded"
        try:
            scale_value = float(scale)
        except (TypeError, ValueError):
            return "❌ Invalid LoRA scale: please provide a numeric value between 0 and 1."
        if not math.isfinite(scale_value):
            return "❌ Invalid LoRA scale: please provide a finite numeric value between 0 and 1."
        self.lora_scale = max(0.0, min(1.0, scale_value))
        if not self.use_lora:
            return f"✅ LoRA scale: {self.lora_scale:.2f} (LoRA disabled)"
        try:
            bridge.set_lora_scale(self.lora_scale)
        except Exception as e:
            return f"❌ Failed to set LoRA scale: {str(e)}"
        return f"✅ LoRA scale: {self.lora_scale:.2f}"

    dit_handler.load_lora = types.MethodType(load_lora_mi355x, dit_handler)
    dit_handler.unload_lora = types.MethodType(unload_lora_mi355x, dit_handler)
    dit_handler.set_use_lora = types.MethodType(set_use_lora_mi355x, dit_handler)
    dit_handler.set_lora_scale = types.MethodType(set_lora_scale_mi355x, dit_handler)
    setattr(dit_handler, "_ggml_lora_backend", "mi355x-capi")


def _tile_plan(T: int, chunk_size: int, overlap: int):
    """Windows of the reference tiled decode (run_non_ggml_real_case.py:597-611): returns
    (stride, [(core_start, core_end, win_start, win_end)])."""
    max_overlap = max(0, (chunk_size // 2) - 1)
    if overlap > max_overlap:
        overlap = max_overlap
    stride = chunk_size - 2 * overlap
    if stride <= 0:
        overlap = max(0, chunk_size // 4)
        stride = chunk_size - 2 * overlap
        if stride <= 0:
            stride, overlap = max(1, chunk_size), 0
    steps = -(-T // stride)
    plan = []
    for i in range(steps):
        cs = i * stride
        ce = min(cs + stride, T)
        plan.append((cs, ce, max(0, cs - overlap), min(T, ce + overlap)))
    return plan


HIP_STREAM_LEGACY = 1  # hipStreamLegacy: the legacy default stream, which torch's default stream is


class _OrderedCall:
    """Order one library call on device tensors against torch's current stream: the library runs on that
    stream, so both sides are in stream order with no host synchronisation.  torch's default stream has
    handle 0, which the C-ABI reads as "the context's own stream" (include/acestep_mi355x.h), so it is handed
    over as hipStreamLegacy, the same legacy default stream under its explicit handle."""

    def __init__(self, bridge, dev):
        import torch
        self.bridge = bridge
        # host tensors (the host-emulated library of the CPU tests) are ordered by program order
        ts = torch.cuda.current_stream(dev) if torch.device(dev).type == "cuda" else None
        self.stream = (ts.cuda_stream or HIP_STREAM_LEGACY) if ts is not None else 0

    def __enter__(self):
        return self.stream

    def __exit__(self, *exc):
        return False


def _trim(bridge, n: int, cs: int, ce: int, ws: int, we: int):
    """(samples of a window of n frames, leading trim, trailing trim) of the reference tiled decode."""
    total = bridge.vae_out_len(n)
    up = float(total) / float(max(1, n))
    return total, int(round((cs - ws) * up)), int(round((we - ce) * up))


def tiled_out_len(bridge, T: int, chunk_size: int, overlap: int) -> int:
    """Samples per item that vae_decode_torch returns for T latent frames (no decode)."""
    plan = [(0, T, 0, T)] if T <= chunk_size else _tile_plan(T, chunk_size, overlap)
    n = 0
    for cs, ce, ws, we in plan:
        total, ts, te = _trim(bridge, we - ws, cs, ce, ws, we)
        n += (total - te if te > 0 else total) - ts
    return n


def vae_decode_torch(bridge, latents_bct, chunk_size: int, overlap: int):
    """latents [B, C, T] (ROCm tensor) -> audio [B, channels, samples] on the same device, decoding
    each window with ace_mi_vae_decode_device on torch's current stream (no host round trip).
    Windowing and trimming are those of the reference tiled decode, so outputs match it."""
    import torch
    B, C, T = latents_bct.shape
    dev = latents_bct.device
    lat = latents_bct.detach().to(torch.float32)
    outs = []
    plan = [(0, T, 0, T)] if T <= chunk_size else _tile_plan(T, chunk_size, overlap)
    for b in range(B):
        parts = []
        for cs, ce, ws, we in plan:
            win = lat[b, :, ws:we].transpose(0, 1).contiguous()        # [frames, C]
            n = we - ws
            total, ts, te = _trim(bridge, n, cs, ce, ws, we)
            wav = torch.empty((total, bridge.audio_channels), dtype=torch.float32, device=dev)
            with _OrderedCall(bridge, dev) as stream:
                bridge.vae_decode_device(win.data_ptr(), n, wav.data_ptr(), stream)
            parts.append(wav[ts:wav.shape[0] - te if te > 0 else wav.shape[0]])
        outs.append(torch.cat(parts, dim=0).transpose(0, 1))            # [channels, samples]
    return torch.stack(outs, dim=0)


def install_vae_backend(dit_handler: Any, bridge, chunk_size_default: int = 32, overlap_default: int = 8) -> None:
    """Replace dit_handler.tiled_decode (the `_install_ggml_vae_backend` seam,
    scripts/run_non_ggml_real_case.py:541-659) with the MI355X VAE decoder."""

    def tiled_decode_mi355x(self, latents, chunk_size=None, overlap=None, offload_wav_to_cpu=None):
        import torch
        if not isinstance(latents, torch.Tensor):
            raise TypeError(f"latents must be torch.Tensor, got {type(latents)!r}")
        if latents.dim() != 3:
            raise ValueError(f"latents must have shape [B,C,T], got {tuple(latents.shape)}")
        cs = int(chunk_size) if chunk_size is not None and int(chunk_size) > 0 else int(chunk_size_default)
        ov = int(overlap) if overlap is not None else int(overlap_default)
        x = latents if latents.is_cuda else latents.to("cuda")
        out = vae_decode_torch(bridge, x, cs, max(0, ov))
        if offload_wav_to_cpu is None and hasattr(self, "_should_offload_wav_to_cpu"):
            offload_wav_to_cpu = self._should_offload_wav_to_cpu()
        return out.cpu() if offload_wav_to_cpu else out

    dit_handler.tiled_decode = types.MethodType(tiled_decode_mi355x, dit_handler)
    setattr(dit_handler, "_ggml_vae_backend", "mi355x-capi")


class _LmOutput:
    """What the reference loops read of a CausalLMOutputWithPast: .logits and .past_key_values."""

    def __init__(self, logits, past_key_values):
        self.logits = logits
        self.past_key_values = past_key_values


class _LmCacheHandle:
    """Opaque past_key_values: the cache itself lives in the engine; only the newest handle is live."""

    def __init__(self, serial: int):
        self.serial = serial
        self.length = 0

    def get_seq_length(self, *a, **kw) -> int:
        return self.length


class _GenerationConfig:
    use_cache = True


class EngineCausalLM:
    """`llm_handler.llm` drop-in for the reference's `pt` backend (acestep/llm_inference.py:345-367, :2259-2471): the
    two custom loops only ever call `model(input_ids=..., attention_mask=..., past_key_values=..., use_cache=...)` and
    read `.logits[:, -1, :]` and `.past_key_values`.  The engine supplies the logits (ace_mi_lm_forward); the
    constrained-decoding FSM, CFG mixing and sampling stay in the reference's Python, unless install_lm_backend was
    given device_codes=True: then the audio-code phase runs in the engine (generate_codes, ace_mi_lm_generate)."""

    def __init__(self, bridge, device=None, max_new_tokens: int = 4096):
        import torch
        self.bridge = bridge
        self.info = bridge.lm_info()
        self.device = torch.device(device if device is not None else "cuda")
        self.generation_config = _GenerationConfig()
        self.max_new_tokens = int(max_new_tokens)
        self._live = None
        self._serial = 0

    def eval(self):
        return self

    def to(self, *a, **kw):
        return self

    def generate(self, *a, **kw):
        raise NotImplementedError("the engine-backed LM serves the reference's custom loops "
                                  "_generate_with_constrained_decoding and _generate_with_cfg_custom; "
                                  "transformers' generate() is not supported")

    def __call__(self, input_ids=None, attention_mask=None, past_key_values=None, use_cache=True, capacity=None, **kw):
        """capacity: positions to reserve for a new prefill (default: the prompt plus max_new_tokens); a caller that
        fans the cache out afterwards (generate_codes_fanout) reserves the prompt alone."""
        if input_ids is None or input_ids.dim() != 2:
            raise ValueError("input_ids must be a [B, n] tensor")
        B, n = int(input_ids.shape[0]), int(input_ids.shape[1])
        if past_key_values is None:
            cap = min(self.info["max_positions"], n + self.max_new_tokens if capacity is None else max(int(capacity), n))
            self.bridge.lm_begin(B, cap)
            self._serial += 1
            self._live = _LmCacheHandle(self._serial)
        else:
            if past_key_values is not self._live:
                raise ValueError("stale past_key_values: the engine holds one KV cache, that of the newest prefill")
            if n != 1:
                raise ValueError("with past_key_values the engine decodes one token per call: input_ids must be [B, 1]")
        mask = None
        if attention_mask is not None:  # the loops pass the whole grown mask; the engine wants the appended columns
            if attention_mask.shape[-1] < n:
                raise ValueError("attention_mask is shorter than input_ids")
            mask = attention_mask[:, attention_mask.shape[-1] - n:]
        logits = self.bridge.lm_forward(input_ids, mask)
        self._live.length += n
        self._last_logits = logits
        return _LmOutput(logits[:, None, :], self._live)

    forward = __call__

    def generate_codes(self, n_codes: int, allowed_ids, eos_id: int, cfg_scale: float = 1.0, codes_temperature=None,
                       temperature: float = 1.0, top_k=None, top_p=None, repetition_penalty: float = 1.0,
                       prompt_ids=None, seed: int = 0, uniforms=None):
        """n_codes tokens of the audio-code phase in one engine call (bridge.lm_generate) on the live cache, starting
        from the logits of the newest forward: candidates = allowed_ids (ascending) without eos_id, which the duration
        constraint blocks for all n_codes tokens; the caller appends EOS.  cfg_scale > 1 mixes the two halves of the
        batch.  A repetition penalty needs prompt_ids [S, n]: every id the sampled sequences hold so far.  uniforms
        [n_codes, S] replace the engine's own draws from `seed`.  Returns int32 [S, n_codes]; the cache then holds
        n_codes - 1 more tokens, the last one is not fed back."""
        import torch
        if self._live is None or getattr(self, "_last_logits", None) is None:
            raise ValueError("generate_codes: no live cache; run the prompt through the model first")
        logits = self._last_logits
        S = logits.shape[0] // 2 if cfg_scale > 1.0 else logits.shape[0]
        seen = None
        if repetition_penalty != 1.0:
            if prompt_ids is None:
                raise ValueError("generate_codes: a repetition penalty needs prompt_ids")
            seen = torch.zeros((S, logits.shape[1]), dtype=torch.uint8, device=logits.device)
            seen.scatter_(1, prompt_ids[:S].to(device=logits.device, dtype=torch.long), 1)
        pre = 0.0
        if codes_temperature is not None:
            pre = float(codes_temperature) if codes_temperature > 0 else 1e-6
        tokens, n = self.bridge.lm_generate(
            logits, int(n_codes), uniforms=uniforms, seen=seen, allowed_ids=allowed_ids, stop_id=eos_id,
            min_tokens=int(n_codes), cfg_scale=cfg_scale, pre_temperature=pre, temperature=temperature, top_k=top_k,
            top_p=top_p, repetition_penalty=repetition_penalty, seed=seed)
        self._live.length += int(n_codes) - 1
        self._last_logits = None  # scratch of the loop now
        return tokens[:, :n]

    def generate_codes_fanout(self, seeds, n_codes: int, allowed_ids, eos_id: int, prompt_ids=None, **kw):
        """The audio-code phase of len(seeds) items that share the prompt in the live cache, in one engine loop: the
        cache of the prefill (one row, or the conditional / unconditional pair) is fanned out bit for bit to one
        sequence (pair) per item (bridge.lm_fanout), then generate_codes runs once with uniforms [n_codes, S] whose
        column s is the engine's stream of seeds[s] (bridge.lm_uniforms), so item s gets the tokens a one-item
        generate_codes(seed=seeds[s]) on the same prefill gets.  prompt_ids [1, n] (a repetition penalty): the ids every
        item holds so far.  kw: generate_codes' cfg_scale, temperatures, top_k, top_p, repetition_penalty.  Handles
        from before the call are stale.  Returns int32 [S, n_codes]."""
        import torch
        if self._live is None or getattr(self, "_last_logits", None) is None:
            raise ValueError("generate_codes_fanout: no live cache; run the prompt through the model first")
        S, n_codes = len(seeds), int(n_codes)
        length = self._live.length
        cap = min(self.info["max_positions"], length + n_codes)
        logits = self.bridge.lm_fanout(S, cap, self._last_logits)
        self._serial += 1
        self._live = _LmCacheHandle(self._serial)
        self._live.length = length
        self._last_logits = logits
        u = np.stack([np.asarray(self.bridge.lm_uniforms(seed, n_codes), np.float32) for seed in seeds], axis=1)
        if prompt_ids is not None:
            prompt_ids = prompt_ids[:1].repeat(S, 1)
        return self.generate_codes(n_codes, allowed_ids, eos_id, prompt_ids=prompt_ids,
                                   uniforms=torch.from_numpy(np.ascontiguousarray(u)), **kw)


def _state_name(proc) -> str:
    st = getattr(proc, "state", None)
    return getattr(st, "name", str(st))


def _codes_handoff(proc):
    """(allowed ids, eos id, codes left) when the constrained processor is in its audio-code phase with everything the
    engine loop needs, else None."""
    import torch
    if proc is None or not getattr(proc, "enabled", True) or _state_name(proc) != "CODES_GENERATION":
        return None  # a disabled processor applies no mask and counts nothing: nothing to hand over
    target, eos = getattr(proc, "target_codes", None), getattr(proc, "eos_token_id", None)
    mask = getattr(proc, "non_audio_code_mask", None)
    if target is None or eos is None or mask is None:
        return None
    left = int(target) - int(getattr(proc, "codes_count", 0))
    if left < 1:
        return None
    allowed = torch.nonzero(torch.isfinite(mask.reshape(-1).float())).reshape(-1)
    allowed = allowed[allowed != int(eos)]
    if allowed.numel() < 1:
        return None
    return allowed, int(eos), left


def _penalise(logits, ids, penalty: float):
    """HF RepetitionPenaltyLogitsProcessor on [S, vocab] logits for the ids [S, n] seen so far."""
    import torch
    score = torch.gather(logits, 1, ids)
    score = torch.where(score < 0, score * penalty, score / penalty)
    return logits.scatter(1, ids, score)


def _engine_loop(handler, ids, mask, max_new_tokens, temperature, cfg_scale, top_k, top_p, repetition_penalty,
                 pad_token_id, streamer, proc):
    """The handler's token loop with the audio-code phase handed to the engine.  cfg_scale None: every row is sampled;
    otherwise the first half of the batch is conditional, the second unconditional, and both get the sampled token."""
    import torch
    model, device = handler.llm, handler.device
    S = ids.shape[0] // 2 if cfg_scale is not None else ids.shape[0]
    rep = 2 if cfg_scale is not None else 1
    out = ids.clone()
    am = mask.clone() if mask is not None else torch.ones_like(ids)
    eos = getattr(getattr(handler, "llm_tokenizer", None), "eos_token_id", None)
    if eos is None:
        eos = pad_token_id
    extra = handler._build_logits_processor(repetition_penalty) if hasattr(handler, "_build_logits_processor") else None
    past = None
    step = 0
    with torch.inference_mode():
        while step < max_new_tokens:
            res = model(input_ids=out if past is None else out[:, -1:], attention_mask=am, past_key_values=past,
                        use_cache=True)
            past = res.past_key_values
            hand = None
            if streamer is None and isinstance(model, EngineCausalLM) and (cfg_scale is None or cfg_scale > 1.0):
                hand = _codes_handoff(proc)
            if hand is not None:
                allowed, eos_id, left = hand
                n = min(left, max_new_tokens - step)
                seed = int(torch.randint(0, 2 ** 62, (1,)).item())  # torch's seeded CPU generator picks the stream
                toks = model.generate_codes(
                    n, allowed, eos_id, cfg_scale=cfg_scale if cfg_scale is not None else 1.0,
                    codes_temperature=getattr(proc, "codes_temperature", None), temperature=temperature, top_k=top_k,
                    top_p=top_p, repetition_penalty=repetition_penalty, prompt_ids=out[:S], seed=seed)
                toks = toks.to(device=out.device, dtype=out.dtype)
                out = torch.cat([out, toks.repeat(rep, 1)], dim=1)
                proc.codes_count = int(getattr(proc, "codes_count", 0)) + n
                step += n
                if n == left and step < max_new_tokens:  # the forced EOS of the duration constraint
                    out = torch.cat([out, torch.full((out.shape[0], 1), eos_id, dtype=out.dtype, device=out.device)], dim=1)
                    st = getattr(proc, "state", None)
                    proc.state = type(st)["COMPLETED"] if hasattr(type(st), "__members__") else "COMPLETED"
                break
            logits = res.logits[:, -1, :]
            if cfg_scale is not None:
                logits = logits[S:].float() + cfg_scale * (logits[:S].float() - logits[S:].float())
            cur = out[:S]
            if proc is not None:
                logits = proc(cur, logits)
            if extra is not None:
                for f in extra:
                    logits = f(cur, logits)
            elif repetition_penalty != 1.0:
                logits = _penalise(logits, cur, repetition_penalty)
            logits = handler._apply_top_k_filter(logits, top_k)
            logits = handler._apply_top_p_filter(logits, top_p)
            nxt = handler._sample_tokens(logits, temperature)
            if proc is not None:
                for b in range(nxt.shape[0]):
                    proc.update_state(nxt[b].item())
            stop = bool(torch.any(nxt == eos))
            if pad_token_id is not None and pad_token_id != eos:
                stop = stop or bool(torch.any(nxt == pad_token_id))
            col = nxt.unsqueeze(1)
            out = torch.cat([out, col.repeat(rep, 1)], dim=1)
            am = torch.cat([am, torch.ones((am.shape[0], 1), device=am.device, dtype=am.dtype)], dim=1)
            if streamer is not None:
                streamer.put(col)
            step += 1
            if stop:
                break
    if streamer is not None:
        streamer.end()
    return out


LM_FANOUT_ROWS = 8  # the engine's rows per decode step (LM_MAX_BATCH): 4 items under CFG, otherwise 8


def _run_pt_fanout(handler, prompts, temperature, cfg_scale, negative_prompt, top_k, top_p, repetition_penalty,
                   use_constrained_decoding, constrained_decoding_debug, target_duration, generation_phase, caption,
                   lyrics, cot_text, seeds):
    """The handler's batch mode of `_run_pt` (acestep/llm_inference.py) for items that share one prompt: per group of
    4 (CFG) or 8 items one prefill, one cache fan-out and one engine loop, then per item what `_run_pt_single` does
    with its loop's output.  Item i gets the text the sequential path gives it: the same prefill, the engine stream of
    the seed that path would draw (torch.manual_seed(seeds[i]) where given, then the torch.randint of _engine_loop),
    and a decode step whose rows do not depend on the batch.  Returns None, before anything ran on the engine, when the
    call is not one this path serves."""
    import torch
    model = handler.llm
    if not isinstance(prompts, (list, tuple)) or len(prompts) < 2 or any(p != prompts[0] for p in prompts[1:]):
        return None
    if not isinstance(model, EngineCausalLM):
        return None
    cfg = float(cfg_scale) > 1.0
    if not cfg and not use_constrained_decoding:
        return None  # the reference calls transformers' generate() here

    def processor():  # the settings _run_pt hands _run_pt_single for a batch item
        return handler._setup_constrained_processor(
            use_constrained_decoding=use_constrained_decoding, constrained_decoding_debug=constrained_decoding_debug,
            target_duration=target_duration, user_metadata=None, stop_at_reasoning=False, skip_genres=True,
            skip_caption=True, skip_language=True, generation_phase=generation_phase, is_batch=False)

    if _codes_handoff(processor()) is None:
        return None  # tokens come before the code phase (or there is none): the per-token path
    tok = handler.llm_tokenizer
    if target_duration is not None and target_duration > 0:
        max_new_tokens = int(max(10, min(600, target_duration)) * 5) + 500
    else:
        max_new_tokens = getattr(getattr(model, "config", None), "max_new_tokens", 4096)
    if hasattr(handler, "max_model_len"):
        max_new_tokens = min(max_new_tokens, handler.max_model_len - 64)
    texts = []
    per_group = LM_FANOUT_ROWS // (2 if cfg else 1)
    with handler._load_model_context():
        if cfg:
            uncond = handler._build_unconditional_prompt(caption=caption, lyrics=lyrics, cot_text=cot_text,
                                                         negative_prompt=negative_prompt,
                                                         generation_phase=generation_phase, is_batch=False)
            side = tok.padding_side
            tok.padding_side = "left"
            enc = tok([prompts[0], uncond], return_tensors="pt", padding=True, truncation=True)
            tok.padding_side = side
        else:
            enc = tok(prompts[0], return_tensors="pt", padding=False, truncation=True)
        ids = enc["input_ids"].to(handler.device)
        am = enc.get("attention_mask", None)
        am = am.to(handler.device) if am is not None else torch.ones_like(ids)
        for g0 in range(0, len(prompts), per_group):
            items = range(g0, min(g0 + per_group, len(prompts)))
            proc = processor()
            allowed, eos_id, left = _codes_handoff(proc)
            n = min(left, max_new_tokens)
            item_seeds = []
            for i in items:
                if seeds and i < len(seeds):
                    torch.manual_seed(seeds[i])
                    if torch.cuda.is_available():
                        torch.cuda.manual_seed_all(seeds[i])
                item_seeds.append(int(torch.randint(0, 2 ** 62, (1,)).item()))
            with torch.inference_mode():
                model(input_ids=ids, attention_mask=am, past_key_values=None, use_cache=True, capacity=ids.shape[1])
                toks = model.generate_codes_fanout(
                    item_seeds, n, allowed, eos_id, prompt_ids=ids[:1], cfg_scale=float(cfg_scale) if cfg else 1.0,
                    codes_temperature=getattr(proc, "codes_temperature", None), temperature=temperature, top_k=top_k,
                    top_p=top_p, repetition_penalty=repetition_penalty)
            toks = toks.to(device="cpu", dtype=ids.dtype)
            proc.codes_count = int(getattr(proc, "codes_count", 0)) + n
            if n == left and n < max_new_tokens:  # the forced EOS of the duration constraint
                toks = torch.cat([toks, torch.full((toks.shape[0], 1), eos_id, dtype=toks.dtype)], dim=1)
                st = getattr(proc, "state", None)
                proc.state = type(st)["COMPLETED"] if hasattr(type(st), "__members__") else "COMPLETED"
            for s in range(len(items)):
                texts.append(tok.decode(toks[s], skip_special_tokens=False))
    return texts


def install_lm_backend(llm_handler: Any, bridge, max_new_tokens: int = 4096, device_codes: bool = False,
                       batch_codes: bool = False) -> None:
    """Point the reference LLM handler's `pt` backend at the engine: `llm_handler.llm` becomes an EngineCausalLM over
    the LM that `bridge.load_lm` loaded (needs no `transformers`).

    device_codes=True also replaces the handler's two loops (_generate_with_constrained_decoding,
    _generate_with_cfg_custom; same signatures and return values) with engine-aware ones: token by token they do what
    the reference loops do (engine logits, the handler's own filters and sampler, the processor's __call__ and
    update_state) until the constrained processor is in CODES_GENERATION with target_codes, eos_token_id and a
    non_audio_code_mask; everything left then runs in one generate_codes call, codes_count and the COMPLETED state are
    written back and EOS is appended.  A streamer, a processor that is disabled or has no target or mask, no
    processor, or a cfg_scale <= 1 in the CFG loop keep the per-token path.  Off by default: the engine draws from its own seeded uniforms, not torch.multinomial, so the same
    torch seed gives other (equally distributed) codes.

    batch_codes=True (only together with device_codes=True, else ValueError) also replaces the handler's `_run_pt`
    (same signature and return value): a list of at least 2 equal prompts, whose constrained processor is in
    CODES_GENERATION with target_codes, eos_token_id and a mask right after its set-up (so no token is sampled before the
    code phase), runs in groups of 4 items under CFG (cfg_scale > 1), otherwise 8: one prefill, one cache fan-out and one
    generate_codes call per group (_run_pt_fanout), each item with the engine stream the sequential path would give
    it, so the returned texts are the sequential path's.  Anything else runs the handler's own sequential `_run_pt`."""
    if batch_codes and not device_codes:
        raise ValueError("install_lm_backend: batch_codes=True needs device_codes=True")
    device = getattr(llm_handler, "device", None)
    if device is None or str(device) in ("auto", "cpu"):
        device = "cuda"
    llm_handler.llm = EngineCausalLM(bridge, device=device, max_new_tokens=max_new_tokens)
    llm_handler.llm_backend = "pt"
    setattr(llm_handler, "_ggml_lm_backend", "mi355x-capi")
    if device_codes:
        def constrained_mi355x(self, input_ids, attention_mask, max_new_tokens, temperature, top_k, top_p,
                               repetition_penalty, pad_token_id, streamer, constrained_processor=None):
            return _engine_loop(self, input_ids, attention_mask, max_new_tokens, temperature, None, top_k, top_p,
                                repetition_penalty, pad_token_id, streamer, constrained_processor)

        def cfg_mi355x(self, batch_input_ids, batch_attention_mask, max_new_tokens, temperature, cfg_scale, top_k, top_p,
                       repetition_penalty, pad_token_id, streamer, constrained_processor=None):
            return _engine_loop(self, batch_input_ids, batch_attention_mask, max_new_tokens, temperature, float(cfg_scale),
                                top_k, top_p, repetition_penalty, pad_token_id, streamer, constrained_processor)

        llm_handler._generate_with_constrained_decoding = types.MethodType(constrained_mi355x, llm_handler)
        llm_handler._generate_with_cfg_custom = types.MethodType(cfg_mi355x, llm_handler)
        setattr(llm_handler, "_ggml_lm_device_codes", True)
    if batch_codes:
        sequential = llm_handler._run_pt

        def run_pt_mi355x(self, formatted_prompts, temperature, cfg_scale, negative_prompt, top_k, top_p,
                          repetition_penalty, use_constrained_decoding=True, constrained_decoding_debug=False,
                          target_duration=None, user_metadata=None, stop_at_reasoning=False, skip_genres=True,
                          skip_caption=False, skip_language=False, generation_phase="cot", caption="", lyrics="",
                          cot_text="", seeds=None):
            out = _run_pt_fanout(self, formatted_prompts, temperature, cfg_scale, negative_prompt, top_k, top_p,
                                 repetition_penalty, use_constrained_decoding, constrained_decoding_debug,
                                 target_duration, generation_phase, caption, lyrics, cot_text, seeds)
            if out is not None:
                return out
            return sequential(formatted_prompts, temperature, cfg_scale, negative_prompt, top_k, top_p,
                              repetition_penalty, use_constrained_decoding, constrained_decoding_debug, target_duration,
                              user_metadata, stop_at_reasoning, skip_genres, skip_caption, skip_language,
                              generation_phase, caption, lyrics, cot_text, seeds)

        llm_handler._run_pt = types.MethodType(run_pt_mi355x, llm_handler)
        setattr(llm_handler, "_ggml_lm_batch_codes", True)


def install_text_encoder_backend(dit_handler: Any, bridge) -> None:
    """`_install_ggml_text_encoder_backend` (scripts/run_non_ggml_real_case.py:406-428): route
    `dit_handler.infer_text_embeddings` / `infer_lyric_embeddings` through the GPU text encoder
    (ace_ggml_text_encoder_forward / _embeddings), one call per row as the reference does."""
    import torch

    hidden_dim = int(dit_handler.text_encoder.config.hidden_size)

    def _rows(ids):
        if not isinstance(ids, torch.Tensor):
            ids = torch.tensor(ids, dtype=torch.long)
        return ids.detach().cpu().numpy().astype(np.int32, copy=False)

    def infer_text_embeddings_mi355x(self, text_token_idss):
        out = np.stack([bridge.text_forward_full(r, hidden_dim) for r in _rows(text_token_idss)], axis=0)
        return torch.from_numpy(out).to(self.device).to(self.dtype)

    def infer_lyric_embeddings_mi355x(self, lyric_token_ids):
        out = np.stack([bridge.text_forward_embeddings(r, hidden_dim) for r in _rows(lyric_token_ids)], axis=0)
        return torch.from_numpy(out).to(self.device).to(self.dtype)

    dit_handler.infer_text_embeddings = types.MethodType(infer_text_embeddings_mi355x, dit_handler)
    dit_handler.infer_lyric_embeddings = types.MethodType(infer_lyric_embeddings_mi355x, dit_handler)
