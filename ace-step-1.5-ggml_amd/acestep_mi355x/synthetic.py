"""Synthetic DiT checkpoints with the real ACE-Step 1.5 tensor names and shapes.

No checkpoints are available offline, so tests and benchmarks use random
weights written in the reference's on-disk format: `config.json` with the keys
read by acestep_dit_config.cpp:58-87 and `model.safetensors` with the
`decoder.*` names loaded by acestep_dit_model.cpp:870-1082.  2-D weights and
biases ~ N(0, 0.02); norm weights ~ 1 + N(0, 0.02); AdaLN tables ~ N(0, 0.02).
"""
from __future__ import annotations

import hashlib
import json
import os
import struct
import tempfile
from typing import Dict, Iterator, Tuple

import numpy as np

FULL_CONFIG = dict(
    hidden_size=2048, intermediate_size=6144, num_hidden_layers=24, num_attention_heads=16,
    num_key_value_heads=8, head_dim=128, max_position_embeddings=32768, rms_norm_eps=1e-6,
    rope_theta=1000000.0, patch_size=2, in_channels=192, audio_acoustic_hidden_dim=64,
    use_sliding_window=True, sliding_window=128, attention_bias=False,
)


def make_config(**overrides) -> dict:
    cfg = dict(FULL_CONFIG)
    cfg.update(overrides)
    n = cfg["num_hidden_layers"]
    # acestep/mlx_dit/model.py:447-451 default: even layers sliding, odd layers full
    cfg.setdefault("layer_types", ["sliding_attention" if (i + 1) % 2 else "full_attention" for i in range(n)])
    if len(cfg["layer_types"]) != n:
        cfg["layer_types"] = ["sliding_attention" if (i + 1) % 2 else "full_attention" for i in range(n)]
    return cfg


TINY_CONFIG = make_config(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                          num_key_value_heads=2, head_dim=128, sliding_window=16)

# Condition-encoder keys (acestep_dit_config.cpp:69-73).  The released config values are not in the
# reference tree; these are the Qwen3-Embedding-0.6B text width and a guess at the layer counts, used
# only to size synthetic checkpoints.
COND_KEYS = dict(text_hidden_dim=1024, num_lyric_encoder_hidden_layers=8, timbre_hidden_dim=64,
                 num_timbre_encoder_hidden_layers=4, timbre_fix_frame=750)
TINY_COND_CONFIG = make_config(**{k: v for k, v in TINY_CONFIG.items() if k != "layer_types"},
                               text_hidden_dim=256, num_lyric_encoder_hidden_layers=2, timbre_hidden_dim=64,
                               num_timbre_encoder_hidden_layers=2, timbre_fix_frame=8)


def tensor_specs(cfg: dict) -> Iterator[Tuple[str, Tuple[int, ...], str]]:
    """(name, shape, kind) for every DiT decoder tensor; kind in {w, b, norm, table}."""
    H, I, D = cfg["hidden_size"], cfg["intermediate_size"], cfg["head_dim"]
    hq, hkv = cfg["num_attention_heads"], cfg["num_key_value_heads"]
    cin, audio, P = cfg["in_channels"], cfg["audio_acoustic_hidden_dim"], cfg["patch_size"]
    yield "decoder.proj_in.1.weight", (H, cin, P), "w"
    yield "decoder.proj_in.1.bias", (H,), "b"
    yield "decoder.proj_out.1.weight", (H, audio, P), "w"
    yield "decoder.proj_out.1.bias", (audio,), "b"
    yield "decoder.condition_embedder.weight", (H, H), "w"
    yield "decoder.condition_embedder.bias", (H,), "b"
    yield "decoder.norm_out.weight", (H,), "norm"
    yield "decoder.scale_shift_table", (1, 2, H), "table"
    for tag in ("time_embed", "time_embed_r"):
        p = f"decoder.{tag}."
        yield p + "linear_1.weight", (H, 256), "w"
        yield p + "linear_1.bias", (H,), "b"
        yield p + "linear_2.weight", (H, H), "w"
        yield p + "linear_2.bias", (H,), "b"
        yield p + "time_proj.weight", (6 * H, H), "w"
        yield p + "time_proj.bias", (6 * H,), "b"
    for i in range(cfg["num_hidden_layers"]):
        p = f"decoder.layers.{i}."
        yield p + "self_attn_norm.weight", (H,), "norm"
        for a in ("self_attn", "cross_attn"):
            yield p + f"{a}.q_proj.weight", (hq * D, H), "w"
            yield p + f"{a}.k_proj.weight", (hkv * D, H), "w"
            yield p + f"{a}.v_proj.weight", (hkv * D, H), "w"
            yield p + f"{a}.o_proj.weight", (H, hq * D), "w"
            yield p + f"{a}.q_norm.weight", (D,), "norm"
            yield p + f"{a}.k_norm.weight", (D,), "norm"
        yield p + "cross_attn_norm.weight", (H,), "norm"
        yield p + "mlp_norm.weight", (H,), "norm"
        yield p + "mlp.gate_proj.weight", (I, H), "w"
        yield p + "mlp.up_proj.weight", (I, H), "w"
        yield p + "mlp.down_proj.weight", (H, I), "w"
        yield p + "scale_shift_table", (1, 6, H), "table"
    # condition encoders (acestep_dit_model.cpp:885-996), after the decoder so that adding them leaves
    # the decoder's random draws unchanged
    th = cfg.get("text_hidden_dim", 0)
    if th:
        yield "encoder.text_projector.weight", (H, th), "w"
    for tag, n_key, in_dim in (("lyric", "num_lyric_encoder_hidden_layers", th or 1024),
                               ("timbre", "num_timbre_encoder_hidden_layers",
                                cfg.get("timbre_hidden_dim", 0) or cfg["audio_acoustic_hidden_dim"])):
        n = cfg.get(n_key, 0)
        if not n:
            continue
        p = f"encoder.{tag}_encoder."
        yield p + "embed_tokens.weight", (H, in_dim), "w"
        yield p + "embed_tokens.bias", (H,), "b"
        yield p + "norm.weight", (H,), "norm"
        if tag == "timbre":
            yield p + "special_token", (1, 1, H), "table"
        for i in range(n):
            q = f"{p}layers.{i}."
            yield q + "input_layernorm.weight", (H,), "norm"
            yield q + "self_attn.q_proj.weight", (hq * D, H), "w"
            yield q + "self_attn.k_proj.weight", (hkv * D, H), "w"
            yield q + "self_attn.v_proj.weight", (hkv * D, H), "w"
            yield q + "self_attn.o_proj.weight", (H, hq * D), "w"
            yield q + "self_attn.q_norm.weight", (D,), "norm"
            yield q + "self_attn.k_norm.weight", (D,), "norm"
            yield q + "post_attention_layernorm.weight", (H,), "norm"
            yield q + "mlp.gate_proj.weight", (I, H), "w"
            yield q + "mlp.up_proj.weight", (I, H), "w"
            yield q + "mlp.down_proj.weight", (H, I), "w"


def _bf16_bits(x: np.ndarray) -> np.ndarray:
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) >> np.uint32(16)).astype("<u2")


def _encode(values: np.ndarray, dtype: str) -> bytes:
    if dtype == "BF16":
        return _bf16_bits(values).tobytes()
    if dtype == "F16":
        return values.astype("<f2").tobytes()
    if dtype == "F32":
        return values.astype("<f4").tobytes()
    raise ValueError(dtype)


# Qwen3-Embedding-0.6B, the ACE-Step text encoder (config keys of qwen_config.cpp:52-61; tensor names of
# qwen_model.cpp:425-467, no "model." prefix)
TEXT_FULL_CONFIG = dict(vocab_size=151669, hidden_size=1024, num_hidden_layers=28, num_attention_heads=16,
                        num_key_value_heads=8, intermediate_size=3072, head_dim=128, max_position_embeddings=32768,
                        rms_norm_eps=1e-6, rope_theta=1000000.0)
TEXT_TINY_CONFIG = dict(TEXT_FULL_CONFIG, vocab_size=1000, hidden_size=256, num_hidden_layers=2,
                        num_attention_heads=4, num_key_value_heads=2, intermediate_size=512)


def text_tensor_specs(cfg: dict) -> Iterator[Tuple[str, Tuple[int, ...], str]]:
    H, I, D = cfg["hidden_size"], cfg["intermediate_size"], cfg["head_dim"]
    hq, hkv = cfg["num_attention_heads"], cfg["num_key_value_heads"]
    yield "embed_tokens.weight", (cfg["vocab_size"], H), "w"
    yield "norm.weight", (H,), "norm"
    for i in range(cfg["num_hidden_layers"]):
        p = f"layers.{i}."
        yield p + "input_layernorm.weight", (H,), "norm"
        yield p + "post_attention_layernorm.weight", (H,), "norm"
        yield p + "self_attn.q_proj.weight", (hq * D, H), "w"
        yield p + "self_attn.k_proj.weight", (hkv * D, H), "w"
        yield p + "self_attn.v_proj.weight", (hkv * D, H), "w"
        yield p + "self_attn.o_proj.weight", (H, hq * D), "w"
        yield p + "self_attn.q_norm.weight", (D,), "norm"
        yield p + "self_attn.k_norm.weight", (D,), "norm"
        yield p + "mlp.gate_proj.weight", (I, H), "w"
        yield p + "mlp.up_proj.weight", (I, H), "w"
        yield p + "mlp.down_proj.weight", (H, I), "w"


def lm_tensor_specs(cfg: dict, tied: bool = True, model_prefix: bool = True):
    """A HF Qwen3ForCausalLM state dict: the text model's tensors under "model." and, untied, lm_head.weight."""
    for name, shape, kind in text_tensor_specs(cfg):
        yield ("model." if model_prefix else "") + name, shape, kind
    if not tied:
        yield "lm_head.weight", (cfg["vocab_size"], cfg["hidden_size"]), "w"


def write_lm_checkpoint(out_dir: str, cfg: Optional[dict] = None, seed: int = 7, tied: bool = True, dtype: str = "BF16",
                        model_prefix: bool = True, std: float = 0.02) -> str:
    """config.json + model.safetensors of a tiny causal LM (the 5 Hz LM's format: Qwen3ForCausalLM) built on
    TEXT_TINY_CONFIG / text_tensor_specs; `tied` leaves lm_head.weight out and sets tie_word_embeddings."""
    cfg = dict(TEXT_TINY_CONFIG if cfg is None else cfg, architectures=["Qwen3ForCausalLM"],
               tie_word_embeddings=bool(tied))
    return write_checkpoint(out_dir, cfg, seed=seed, dtype=dtype, std=std,
                            specs=lm_tensor_specs(cfg, tied=tied, model_prefix=model_prefix))


def write_checkpoint(out_dir: str, cfg: dict, seed: int = 0, dtype: str = "BF16", std: float = 0.02,
                     backend: str = "numpy", specs=None, qk_norm_scale: float = 1.0,
                     qk_norm_tags=("self_attn", "cross_attn")) -> str:
    """Write config.json + model.safetensors into out_dir; returns out_dir.
    backend "numpy" (default, used by the golden fixtures) or "torch" (multi-threaded, ~10x
    faster for the 1.5 B-parameter benchmark checkpoint; different random values).
    specs: tensor list (default: the DiT's, tensor_specs(cfg); text_tensor_specs for Qwen3).
    qk_norm_scale: multiplies the DiT's q_norm / k_norm weights (self and cross attention), so the
    post-norm logits q.k/sqrt(D) have a standard deviation of ~scale^2 instead of ~1: the peaked-softmax
    regime of trained checkpoints (|logit| of tens) for the attention-precision tests; qk_norm_tags picks the
    attention blocks it applies to."""
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "config.json"), "w", encoding="utf-8") as f:
        json.dump(cfg, f, indent=1)
    specs = list(tensor_specs(cfg) if specs is None else specs)
    esz = {"BF16": 2, "F16": 2, "F32": 4}[dtype]
    header: Dict[str, dict] = {}
    off = 0
    for name, shape, _ in specs:
        n = int(np.prod(shape)) * esz
        header[name] = {"dtype": dtype, "shape": list(shape), "data_offsets": [off, off + n]}
        off += n
    hjson = json.dumps(header, separators=(",", ":")).encode("utf-8")
    hjson += b" " * ((8 - len(hjson) % 8) % 8)
    rng = np.random.default_rng(seed)
    gen = None
    if backend == "torch":
        import torch
        gen = torch.Generator().manual_seed(seed)
    tmp = os.path.join(out_dir, "model.safetensors.tmp")
    with open(tmp, "wb") as f:
        f.write(struct.pack("<Q", len(hjson)))
        f.write(hjson)
        for name, shape, kind in specs:
            if gen is not None:
                import torch
                t = torch.randn(shape, generator=gen, dtype=torch.float32) * std
                if kind == "norm":
                    t = t + 1.0
                    if _is_qk_norm(name, qk_norm_tags):
                        t = t * qk_norm_scale
                tt = {"BF16": torch.bfloat16, "F16": torch.float16, "F32": torch.float32}[dtype]
                f.write(t.to(tt).view(torch.int16 if dtype != "F32" else torch.int32).numpy().tobytes())
                continue
            v = rng.standard_normal(size=shape, dtype=np.float32) * np.float32(std)
            if kind == "norm":
                v = v + np.float32(1.0)
                if _is_qk_norm(name, qk_norm_tags):
                    v = v * np.float32(qk_norm_scale)
            f.write(_encode(v, dtype))
    os.replace(tmp, os.path.join(out_dir, "model.safetensors"))
    return out_dir


def _is_qk_norm(name: str, tags=("self_attn", "cross_attn")) -> bool:
    return (name.startswith("decoder.layers.") and name.endswith(("q_norm.weight", "k_norm.weight")) and
            any(f".{t}." in name for t in tags))


def cached_checkpoint(cfg: dict, seed: int = 0, dtype: str = "BF16", root: str | None = None,
                      backend: str = "numpy", kind: str = "dit", qk_norm_scale: float = 1.0,
                      qk_norm_tags=("self_attn", "cross_attn")) -> str:
    """Write the checkpoint once per (cfg, seed, dtype, backend, kind, qk_norm_scale) under a cache dir and
    reuse it.  kind "dit" (tensor_specs) or "text" (the Qwen3 text encoder, text_tensor_specs)."""
    key_parts = [cfg, seed, dtype, backend] + ([kind] if kind != "dit" else []) + \
        ([float(qk_norm_scale)] if qk_norm_scale != 1.0 else []) + \
        ([list(qk_norm_tags)] if tuple(qk_norm_tags) != ("self_attn", "cross_attn") else [])
    key = hashlib.sha1(json.dumps(key_parts, sort_keys=True).encode()).hexdigest()[:16]
    root = root or os.environ.get("ACE_MI_SYNTH_DIR") or os.path.join(tempfile.gettempdir(), "acestep_mi355x_synth")
    d = os.path.join(root, key)
    if not os.path.exists(os.path.join(d, "model.safetensors")):
        specs = text_tensor_specs(cfg) if kind == "text" else None
        write_checkpoint(d, cfg, seed=seed, dtype=dtype, backend=backend, specs=specs, qk_norm_scale=qk_norm_scale,
                         qk_norm_tags=qk_norm_tags)
    return d


# ----------------------------------------------------------------------------- VAE (Oobleck)
# diffusers AutoencoderOobleck layout read by acestep_vae_model.cpp:760-955 (decoder.* only: the
# MI355X engine implements decode; encode is out of scope this round).
VAE_FULL_CONFIG = dict(audio_channels=2, encoder_hidden_size=128, decoder_channels=128, decoder_input_channels=64,
                       sampling_rate=48000, downsampling_ratios=[2, 4, 4, 6, 10], channel_multiples=[1, 2, 4, 8, 16])
VAE_TINY_CONFIG = dict(VAE_FULL_CONFIG, downsampling_ratios=[2, 3], channel_multiples=[1, 2])


def vae_tensor_specs(cfg: dict) -> Iterator[Tuple[str, Tuple[int, ...], str]]:
    """(name, shape, kind) of every decoder tensor; kind in {g, v, b, snake}."""
    ch, lat, aud = cfg["decoder_channels"], cfg["decoder_input_channels"], cfg["audio_channels"]
    strides = list(reversed(cfg["downsampling_ratios"]))
    cm = [1] + list(cfg["channel_multiples"])
    n = len(strides)

    def conv(prefix, cout, cin, k, bias=True, transposed=False):
        d0 = cin if transposed else cout
        yield prefix + ".weight_g", (d0, 1, 1), "g"
        yield prefix + ".weight_v", ((cin, cout, k) if transposed else (cout, cin, k)), "v"
        if bias:
            yield prefix + ".bias", (cout,), "b"

    def snk(prefix, c):
        yield prefix + ".alpha", (1, c, 1), "snake"
        yield prefix + ".beta", (1, c, 1), "snake"

    yield from conv("decoder.conv1", ch * cm[-1], lat, 7)
    for i, s in enumerate(strides):
        cin, cout = ch * cm[n - i], ch * cm[n - i - 1]
        p = f"decoder.block.{i}"
        yield from snk(p + ".snake1", cin)
        yield from conv(p + ".conv_t1", cout, cin, 2 * s, transposed=True)
        for j in range(3):
            q = f"{p}.res_unit{j + 1}"
            yield from snk(q + ".snake1", cout)
            yield from conv(q + ".conv1", cout, cout, 7)
            yield from snk(q + ".snake2", cout)
            yield from conv(q + ".conv2", cout, cout, 1)
    yield from snk("decoder.snake1", ch)
    yield from conv("decoder.conv2", aud, ch, 7, bias=False)
    # encoder (diffusers OobleckEncoder; acestep_vae_model.cpp:925-937)
    eh = cfg["encoder_hidden_size"]
    dn = list(cfg["downsampling_ratios"])
    yield from conv("encoder.conv1", eh, aud, 7)
    for i, s in enumerate(dn):
        cin, cout = eh * cm[i], eh * cm[i + 1]
        p = f"encoder.block.{i}"
        for j in range(3):
            q = f"{p}.res_unit{j + 1}"
            yield from snk(q + ".snake1", cin)
            yield from conv(q + ".conv1", cin, cin, 7)
            yield from snk(q + ".snake2", cin)
            yield from conv(q + ".conv2", cin, cin, 1)
        yield from snk(p + ".snake1", cin)
        yield from conv(p + ".conv1", cout, cin, 2 * s)
    yield from snk("encoder.snake1", eh * cm[-1])
    yield from conv("encoder.conv2", eh, eh * cm[-1], 3)


def write_vae_checkpoint(out_dir: str, cfg: dict, seed: int = 0, dtype: str = "F32") -> str:
    """config.json + diffusion_pytorch_model.safetensors with weight-normed convs: weight_v ~ N(0,1),
    weight_g ~ 0.6 + U(0, 0.4) (keeps activations O(1) through the residual stack), biases ~ N(0, 0.02),
    snake alpha/beta ~ N(0, 0.1)."""
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "config.json"), "w", encoding="utf-8") as f:
        json.dump(cfg, f, indent=1)
    specs = list(vae_tensor_specs(cfg))
    esz = {"BF16": 2, "F16": 2, "F32": 4}[dtype]
    header: Dict[str, dict] = {}
    off = 0
    for name, shape, _ in specs:
        nb = int(np.prod(shape)) * esz
        header[name] = {"dtype": dtype, "shape": list(shape), "data_offsets": [off, off + nb]}
        off += nb
    hjson = json.dumps(header, separators=(",", ":")).encode("utf-8")
    hjson += b" " * ((8 - len(hjson) % 8) % 8)
    rng = np.random.default_rng(seed)
    tmp = os.path.join(out_dir, "diffusion_pytorch_model.safetensors.tmp")
    with open(tmp, "wb") as f:
        f.write(struct.pack("<Q", len(hjson)))
        f.write(hjson)
        for name, shape, kind in specs:
            if kind == "v":
                v = rng.standard_normal(size=shape, dtype=np.float32)
            elif kind == "g":
                v = (np.float32(0.6) + np.float32(0.4) * rng.random(size=shape, dtype=np.float32))
            elif kind == "b":
                v = rng.standard_normal(size=shape, dtype=np.float32) * np.float32(0.02)
            else:
                v = rng.standard_normal(size=shape, dtype=np.float32) * np.float32(0.1)
            f.write(_encode(v, dtype))
    os.replace(tmp, os.path.join(out_dir, "diffusion_pytorch_model.safetensors"))
    return out_dir


# ----------------------------------------------------------------------------- GGUF export
GGML_TYPES = {"F32": 0, "F16": 1, "Q4_0": 2, "Q4_1": 3, "Q5_0": 6, "Q5_1": 7, "Q8_0": 8, "Q2_K": 10, "Q3_K": 11,
              "Q4_K": 12, "Q5_K": 13, "Q6_K": 14, "IQ4_NL": 20, "BF16": 30}
_QUANT_ARG = {"F16": None, "Q8": "Q8_0", "Q8_0": "Q8_0", "Q6": "Q6_K", "Q6_K": "Q6_K", "Q4": "Q4_K", "Q4_K": "Q4_K"}
_QBLOCK = {"Q8_0": 32, "Q4_K": 256, "Q6_K": 256}


def _read_safetensors_f32(path: str) -> Dict[str, np.ndarray]:
    with open(path, "rb") as f:
        n = struct.unpack("<Q", f.read(8))[0]
        header = json.loads(f.read(n))
        base = 8 + n
        out = {}
        for name, info in header.items():
            if name == "__metadata__":
                continue
            b0, b1 = info["data_offsets"]
            f.seek(base + b0)
            raw = f.read(b1 - b0)
            dt = info["dtype"]
            if dt == "F32":
                v = np.frombuffer(raw, "<f4").astype(np.float32)
            elif dt == "F16":
                v = np.frombuffer(raw, "<f2").astype(np.float32)
            elif dt == "BF16":
                v = (np.frombuffer(raw, "<u2").astype(np.uint32) << 16).view(np.float32)
            else:
                raise ValueError(dt)
            out[name] = v.reshape(info["shape"])
    return out


def write_gguf(safetensors_path: str, out_path: str, quant: str = "Q8", arch: str = "acestep") -> str:
    """GGUF export with the rules of acestep_ggml/tools/export_safetensors_to_gguf.py:192-281: every
    float tensor with >= 2 dims whose last dim is a multiple of the block size is quantized (Q8/Q6/Q4),
    everything else is stored F16.  Block bytes come from this library's ggml encoders
    (ace_mi_quantize; the reference script uses gguf-py / ggml's C quantizer).  GGUF v3, alignment 32,
    numpy shape reversed into ggml ne order."""
    from . import capi
    qname = _QUANT_ARG[quant.upper()]
    tensors = _read_safetensors_f32(safetensors_path)
    entries = []
    for name, v in tensors.items():
        if qname and v.ndim >= 2 and v.shape[-1] % _QBLOCK[qname] == 0:
            rows = int(np.prod(v.shape[:-1]))
            data = capi.quantize(v.reshape(rows, v.shape[-1]), qname.lower()).tobytes()
            entries.append((name, v.shape, GGML_TYPES[qname], data))
        else:
            entries.append((name, v.shape, GGML_TYPES["F16"], v.astype("<f2").tobytes()))

    return _write_gguf_entries(entries, out_path, arch)


def _write_gguf_entries(entries, out_path: str, arch: str = "acestep") -> str:
    """GGUF v3, alignment 32: entries (name, numpy shape, ggml type id, data bytes); the shape is reversed into ggml
    ne order."""
    def s(x: str) -> bytes:
        b = x.encode("utf-8")
        return struct.pack("<Q", len(b)) + b

    kv = [("general.architecture", 8, s(arch)), ("general.type", 8, s("model")),
          ("general.quantization_version", 4, struct.pack("<I", 2))]
    head = b"GGUF" + struct.pack("<IQQ", 3, len(entries), len(kv))
    for k, t, val in kv:
        head += s(k) + struct.pack("<I", t) + val
    off = 0
    infos = b""
    for name, shape, gt, data in entries:
        ne = list(reversed(shape))
        infos += s(name) + struct.pack("<I", len(ne)) + b"".join(struct.pack("<Q", d) for d in ne)
        infos += struct.pack("<IQ", gt, off)
        off += (len(data) + 31) // 32 * 32
    blob = head + infos
    blob += b"\0" * ((32 - len(blob) % 32) % 32)
    tmp = out_path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(blob)
        for _, _, _, data in entries:
            f.write(data)
            f.write(b"\0" * ((32 - len(data) % 32) % 32))
    os.replace(tmp, out_path)
    return out_path


# ggml block types: values per block, bytes per block, byte offsets of the fp16 fields (ggml-common.h block_* structs)
GGML_BLOCKS = {
    "Q4_0": (32, 18, (0,)), "Q4_1": (32, 20, (0, 2)), "Q5_0": (32, 22, (0,)), "Q5_1": (32, 24, (0, 2)),
    "Q8_0": (32, 34, (0,)), "Q2_K": (256, 84, (80, 82)), "Q3_K": (256, 110, (108,)), "Q4_K": (256, 144, (0, 2)),
    "Q5_K": (256, 176, (0, 2)), "Q6_K": (256, 210, (208,)), "IQ4_NL": (32, 18, (0,)),
}
# (scale, min as a multiple of the scale) that give dequantized values of std ~ 0.02, roughly centred, for uniformly
# random code bytes; the second is 0 for types without a min field
_RANDOM_BLOCK_SCALES = {
    "Q4_0": (0.0043, 0.0), "Q4_1": (0.0043, -7.5), "Q5_0": (0.0022, 0.0), "Q5_1": (0.0022, -15.5),
    "Q8_0": (0.00027, 0.0), "IQ4_NL": (0.00029, 0.0), "Q2_K": (0.0024, 1.5), "Q3_K": (0.0005, 0.0),
    "Q4_K": (0.00012, 7.5), "Q5_K": (0.00006, 15.5), "Q6_K": (0.000015, 0.0),
}


def random_blocks(gtype: str, rows: int, cols: int, rng: np.random.Generator) -> np.ndarray:
    """Valid random ggml blocks uint8 [rows][cols / block][block bytes]: uniformly random code bytes, every fp16 field
    overwritten by a finite value sized so that the dequantized weights have std ~ 0.02.  Not an encoder: nothing
    is fitted to any values."""
    bv, bb, fields = GGML_BLOCKS[gtype]
    assert cols % bv == 0, (gtype, cols)
    nb = cols // bv
    blk = rng.integers(0, 256, size=(rows, nb, bb), dtype=np.uint8)
    scale, min_mult = _RANDOM_BLOCK_SCALES[gtype]
    d = (scale * (0.5 + rng.random(size=(rows, nb)))).astype(np.float32)
    if min_mult == 0.0:  # symmetric types: either sign
        d = d * np.where(rng.random(size=(rows, nb)) < 0.5, -1.0, 1.0).astype(np.float32)
    vals = [d] + ([d * np.float32(min_mult) * (0.9 + 0.2 * rng.random(size=(rows, nb))).astype(np.float32)]
                  if len(fields) > 1 else [])
    for off, v in zip(fields, vals):
        h = v.astype("<f2")
        assert np.all(np.isfinite(h.astype(np.float32)))
        blk[:, :, off:off + 2] = h.view(np.uint8).reshape(rows, nb, 2)
    return blk


def q5_k_m_types(name: str, shape) -> Optional[str]:
    """The type layout of a llama.cpp-style Q5_K_M file: Q5_K, with v_proj and down_proj in Q6_K."""
    return "Q6_K" if ("v_proj" in name or "down_proj" in name) else "Q5_K"


def write_gguf_typed(safetensors_path: str, out_path: str, types, seed: int = 0, arch: str = "acestep"):
    """GGUF export with a type per tensor: `types` is a dict name -> type name or a callable (name, shape) -> type
    name (None / a missing name: the tensor is stored F16), consulted for float tensors with >= 2 dims whose last
    dim is a multiple of the type's block.  Q8_0 / Q4_K / Q6_K blocks come from this library's encoders like
    write_gguf's; the decode-only types (Q4_0, Q4_1, Q5_0, Q5_1, Q2_K, Q3_K, Q5_K, IQ4_NL) get random_blocks -- valid
    blocks that do not approximate the checkpoint's values; BF16 / F16 / F32 store the values.  Returns the entries
    {name: (numpy shape, type name, data bytes)}."""
    from . import capi
    tensors = _read_safetensors_f32(safetensors_path)
    rng = np.random.default_rng(seed)
    entries, out = [], {}
    for name, v in tensors.items():
        t = types(name, v.shape) if callable(types) else types.get(name)
        if t is not None and v.ndim >= 2 and t in GGML_BLOCKS and v.shape[-1] % GGML_BLOCKS[t][0] == 0:
            rows = int(np.prod(v.shape[:-1]))
            if t in _QBLOCK:
                data = capi.quantize(v.reshape(rows, v.shape[-1]), t.lower()).tobytes()
            else:
                data = random_blocks(t, rows, v.shape[-1], rng).tobytes()
        elif t == "BF16":
            u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
            data = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype("<u2").tobytes()
        elif t == "F32":
            data = v.astype("<f4").tobytes()
        else:
            t, data = "F16", v.astype("<f2").tobytes()
        entries.append((name, v.shape, GGML_TYPES[t], data))
        out[name] = (tuple(v.shape), t, data)
    _write_gguf_entries(entries, out_path, arch)
    return out


def write_gguf_tensors(out_path: str, tensors, arch: str = "acestep") -> str:
    """A GGUF file of ready-made tensors {name: (numpy shape, type name, data bytes)}."""
    return _write_gguf_entries([(n, sh, GGML_TYPES[t], data) for n, (sh, t, data) in tensors.items()], out_path, arch)


# Tiny causal-LM GGUFs (ace_mi_load_lm): a type per projection, HF tensor names, norms in F32.
LM_GGUF_VARIANTS = {
    "q8_0": dict(tied=False, types="Q8_0"),
    "q4_k": dict(tied=True, types="Q4_K"),
    "q6_k": dict(tied=True, types="Q6_K"),
    # a fused QKV of differing types and a type without planes (o_proj): both become bf16 images
    "mixed": dict(tied=True, types=dict(q_proj="Q4_K", k_proj="Q4_K", gate_proj="Q4_K", up_proj="Q4_K", v_proj="Q6_K",
                                        down_proj="Q6_K", o_proj="Q5_K", embed_tokens="Q6_K")),
}


def write_lm_gguf(out_dir: str, types, tied: bool = True, seed: int = 7, cfg: Optional[dict] = None,
                  model_prefix: bool = True, file_name: str = "model.gguf") -> str:
    """config.json + a GGUF of the tiny causal LM of write_lm_checkpoint(seed, tied): `types` is one type name for every
    2-D tensor, or a dict keyed by the tensor's module (q_proj, ..., embed_tokens, lm_head; a missing key: F16) -- the
    per-tensor map handed to write_gguf_typed, whose encoders / random blocks make the bytes; 1-D tensors (norms) are
    F32.  Deterministic in (types, tied, seed).  Returns the GGUF's path."""
    import tempfile
    src = tempfile.mkdtemp(prefix="acemi_lm_gguf_src_")
    write_lm_checkpoint(src, cfg=cfg, seed=seed, tied=tied, model_prefix=model_prefix)

    def pick(name, shape):
        if len(shape) < 2:
            return "F32"
        if isinstance(types, str):
            return types
        return types.get(name.split(".")[-2])

    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(src, "config.json"), "rb") as f, open(os.path.join(out_dir, "config.json"), "wb") as g:
        g.write(f.read())
    out = os.path.join(out_dir, file_name)
    write_gguf_typed(os.path.join(src, "model.safetensors"), out, pick, seed=seed)
    return out


# ----------------------------------------------------------------------------- PEFT LoRA adapters
# What peft's save_pretrained writes for the reference trainer (acestep/training/lora_utils.py, configs.py:12-38:
# r = 8, alpha = 16, targets q_proj,k_proj,v_proj,o_proj): adapter_config.json + adapter_model.safetensors with
# base_model.model.layers.{i}.{self_attn|cross_attn|mlp}.{x}_proj.lora_{A,B}.weight, A [r][in], B [out][r].
LORA_ATTN_TARGETS = ("q_proj", "k_proj", "v_proj", "o_proj")
LORA_MLP_TARGETS = ("gate_proj", "up_proj", "down_proj")
LORA_ALL_TARGETS = tuple(f"{a}.{p}" for a in ("self_attn", "cross_attn") for p in LORA_ATTN_TARGETS) + \
    tuple(f"mlp.{p}" for p in LORA_MLP_TARGETS)


def lora_module_dims(cfg: dict, module: str) -> Tuple[int, int]:
    """(in, out) of decoder module "self_attn.q_proj" / "mlp.down_proj" / ..."""
    H, I, D = cfg["hidden_size"], cfg["intermediate_size"], cfg["head_dim"]
    qd, kd = cfg["num_attention_heads"] * D, cfg["num_key_value_heads"] * D
    proj = module.split(".")[-1]
    return {"q_proj": (H, qd), "k_proj": (H, kd), "v_proj": (H, kd), "o_proj": (qd, H), "gate_proj": (H, I),
            "up_proj": (H, I), "down_proj": (I, H)}[proj]


def _expand_targets(targets) -> Tuple[str, ...]:
    """Target names as peft takes them: a bare projection ("q_proj") means every block that has one."""
    out = []
    for t in targets:
        if "." in t:
            out.append(t)
        elif t in LORA_ATTN_TARGETS:
            out += [f"self_attn.{t}", f"cross_attn.{t}"]
        else:
            out.append(f"mlp.{t}")
    return tuple(dict.fromkeys(out))


def write_lora_adapter(out_dir: str, cfg: dict, r=8, alpha: float = 16.0, targets=LORA_ATTN_TARGETS, seed: int = 0,
                       dtype: str = "F32", rslora: bool = False, std: float = 0.02, alpha_pattern=None,
                       key_prefix: str = "base_model.model.", adapter_name: str | None = None,
                       extra_config=None) -> str:
    """Write adapter_config.json + adapter_model.safetensors by hand.  A and B ~ N(0, std) (peft initialises B to
    zero; a non-zero B makes the delta visible).  r: one rank, or a dict module-suffix -> rank (rank_pattern).
    targets: "q_proj" (self and cross) or "self_attn.q_proj" / "mlp.up_proj".  adapter_name: written as the
    lora_A.<name>.weight key form."""
    os.makedirs(out_dir, exist_ok=True)
    mods = _expand_targets(targets)
    r_default = r if isinstance(r, int) else 8
    rank_pattern = {} if isinstance(r, int) else dict(r)
    conf = dict(peft_type="LORA", task_type=None, base_model_name_or_path=None, r=r_default, lora_alpha=alpha,
                lora_dropout=0.0, bias="none", target_modules=sorted({m.split(".")[-1] for m in mods}),
                modules_to_save=None, use_rslora=bool(rslora), use_dora=False, rank_pattern=rank_pattern,
                alpha_pattern=dict(alpha_pattern or {}), fan_in_fan_out=False, inference_mode=True)
    conf.update(extra_config or {})
    with open(os.path.join(out_dir, "adapter_config.json"), "w", encoding="utf-8") as f:
        json.dump(conf, f, indent=1)
    rng = np.random.default_rng(seed)
    tensors = []
    seg = "" if adapter_name is None else f".{adapter_name}"
    for i in range(cfg["num_hidden_layers"]):
        for m in mods:
            fin, fout = lora_module_dims(cfg, m)
            name = f"layers.{i}.{m}"
            rk = r_default
            for pat, v in rank_pattern.items():
                if name == pat or name.endswith("." + pat):
                    rk = int(v)
            tensors.append((f"{key_prefix}{name}.lora_A{seg}.weight",
                            rng.standard_normal((rk, fin), dtype=np.float32) * np.float32(std)))
            tensors.append((f"{key_prefix}{name}.lora_B{seg}.weight",
                            rng.standard_normal((fout, rk), dtype=np.float32) * np.float32(std)))
    write_safetensors(os.path.join(out_dir, "adapter_model.safetensors"), tensors, dtype)
    return out_dir


def write_safetensors(path: str, tensors, dtype: str) -> None:
    """tensors: [(name, f32 array)] written as `dtype` (BF16 / F16 / F32)."""
    esz = {"BF16": 2, "F16": 2, "F32": 4}[dtype]
    header: Dict[str, dict] = {}
    off = 0
    for name, v in tensors:
        n = int(v.size) * esz
        header[name] = {"dtype": dtype, "shape": list(v.shape), "data_offsets": [off, off + n]}
        off += n
    hjson = json.dumps(header, separators=(",", ":")).encode("utf-8")
    hjson += b" " * ((8 - len(hjson) % 8) % 8)
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(struct.pack("<Q", len(hjson)))
        f.write(hjson)
        for _, v in tensors:
            f.write(_encode(np.asarray(v, np.float32), dtype))
    os.replace(tmp, path)


def _read_safetensors_raw(path: str):
    """{name: (dtype, shape, raw words / f32 array)} without widening the 16-bit tensors."""
    with open(path, "rb") as f:
        n = struct.unpack("<Q", f.read(8))[0]
        header = json.loads(f.read(n))
        base = 8 + n
        out = {}
        for name, info in header.items():
            if name == "__metadata__":
                continue
            b0, b1 = info["data_offsets"]
            f.seek(base + b0)
            raw = f.read(b1 - b0)
            dt = info["dtype"]
            out[name] = (dt, tuple(info["shape"]), np.frombuffer(raw, "<f4" if dt == "F32" else "<u2").copy())
    return out


def lora_acc(A: np.ndarray, B: np.ndarray) -> np.ndarray:
    """The merge kernel's accumulator [out][in]: acc = 0; for j ascending: acc = acc + B[:, j] * A[j, :], the
    multiply and the add each rounded to float32 (an explicit loop; `@` would accumulate otherwise)."""
    A = np.ascontiguousarray(A, np.float32)
    B = np.ascontiguousarray(B, np.float32)
    acc = np.zeros((B.shape[0], A.shape[1]), np.float32)
    for j in range(A.shape[0]):
        acc = acc + B[:, j:j + 1] * A[j:j + 1, :]
    return acc


def lora_merge_bits(base_bits: np.ndarray, acc: np.ndarray, eff, fmt: str) -> np.ndarray:
    """rne16(f32(base) + eff * acc) on raw 16-bit words (fmt "BF16" / "F16")."""
    t = np.float32(eff) * acc.astype(np.float32)
    if fmt == "F16":
        w = np.ascontiguousarray(base_bits, "<u2").view("<f2").astype(np.float32)
        return (w + t).astype("<f2").view("<u2")
    w = (np.ascontiguousarray(base_bits, "<u2").astype(np.uint32) << 16).view(np.float32)
    return _bf16_bits(w + t)


def lora_eff(scale: float, alpha: float, r: int, rslora: bool = False) -> np.float32:
    """f32(scale) * f32(alpha / r) (alpha / sqrt(r) with use_rslora), the engine's per-module scale."""
    unit = np.float32(alpha / np.sqrt(float(r))) if rslora else np.float32(alpha / float(r))
    return np.float32(scale) * unit


def read_lora_adapter(adapter_dir: str) -> Tuple[dict, Dict[str, Tuple[np.ndarray, np.ndarray]]]:
    """(adapter config, {"layers.0.self_attn.q_proj": (A f32 [r][in], B f32 [out][r])})."""
    with open(os.path.join(adapter_dir, "adapter_config.json"), "r", encoding="utf-8") as f:
        conf = json.load(f)
    raw = _read_safetensors_f32(os.path.join(adapter_dir, "adapter_model.safetensors"))
    mods: Dict[str, list] = {}
    for key, v in raw.items():
        k = key[len("base_model.model."):] if key.startswith("base_model.model.") else key
        k = k[len("decoder."):] if k.startswith("decoder.") else k
        parts = k.split(".")
        which = parts.index("lora_A") if "lora_A" in parts else parts.index("lora_B")
        name = ".".join(parts[:which])
        mods.setdefault(name, [None, None])[0 if parts[which] == "lora_A" else 1] = v.astype(np.float32)
    return conf, {k: (a, b) for k, (a, b) in mods.items()}


def merged_checkpoint(base_dir: str, adapter_dir: str, scale: float, out_dir: str) -> str:
    """A checkpoint whose targeted decoder weights are rne16(f32(W) + eff * acc) in the base's own 16-bit dtype,
    with the merge kernel's arithmetic restated in numpy (lora_acc / lora_merge_bits); every other tensor is
    copied bit for bit.  An engine that loads it runs the same kernels on the same weight bits as the engine
    that loaded base_dir + the adapter at `scale`."""
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(base_dir, "config.json"), "r", encoding="utf-8") as f:
        cfg_text = f.read()
    with open(os.path.join(out_dir, "config.json"), "w", encoding="utf-8") as f:
        f.write(cfg_text)
    conf, mods = read_lora_adapter(adapter_dir)
    tensors = _read_safetensors_raw(os.path.join(base_dir, "model.safetensors"))
    pats = conf.get("alpha_pattern") or {}
    for name, (A, B) in mods.items():
        key = f"decoder.{name}.weight"
        dt, shape, words = tensors[key]
        if dt not in ("BF16", "F16"):
            raise ValueError(f"{key}: merged_checkpoint needs a 16-bit base ({dt})")
        alpha = conf["lora_alpha"]
        for pat, v in pats.items():
            if name == pat or name.endswith("." + pat):
                alpha = v
        eff = lora_eff(scale, alpha, A.shape[0], bool(conf.get("use_rslora")))
        merged = lora_merge_bits(words.reshape(shape), lora_acc(A, B), eff, dt)
        tensors[key] = (dt, shape, merged.reshape(-1))
    header: Dict[str, dict] = {}
    off = 0
    for name, (dt, shape, words) in tensors.items():
        header[name] = {"dtype": dt, "shape": list(shape), "data_offsets": [off, off + words.nbytes]}
        off += words.nbytes
    hjson = json.dumps(header, separators=(",", ":")).encode("utf-8")
    hjson += b" " * ((8 - len(hjson) % 8) % 8)
    tmp = os.path.join(out_dir, "model.safetensors.tmp")
    with open(tmp, "wb") as f:
        f.write(struct.pack("<Q", len(hjson)))
        f.write(hjson)
        for _, (_, _, words) in tensors.items():
            f.write(words.tobytes())
    os.replace(tmp, os.path.join(out_dir, "model.safetensors"))
    return out_dir
