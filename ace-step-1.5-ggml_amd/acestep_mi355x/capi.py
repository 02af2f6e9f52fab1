"""ctypes bindings of libacestep_mi355x.so.

`GGMLCAPIBridge` keeps the reference bridge's surface
(scripts/run_non_ggml_real_case.py:135-354: constructor args, `load_dit`,
`dit_forward_tfirst`, `close`, RuntimeError "<where> failed: <last_error>
(status=N)") so reference callers switch by pointing `lib_path` at this
library.  The MI355X extensions (`dit_forward_batched_device`,
`dit_sample_device`) take raw device pointers (e.g. torch ROCm
`tensor.data_ptr()`) and keep everything on the GPU.
"""
from __future__ import annotations

import atexit
import ctypes
import os
from pathlib import Path
from typing import List, Optional, Tuple

import numpy as np

from . import LIB_PATH

ACE_GGML_OK = 0
ACE_GGML_ERR = 1
ACE_GGML_ERR_INVALID_ARG = 2
ACE_GGML_ERR_IO = 3
ACE_GGML_ERR_UNSUPPORTED = 4

# Every symbol declared in include/acestep_ggml.h and include/acestep_mi355x.h.
EXPORTED_SYMBOLS = (
    "ace_ggml_create", "ace_ggml_destroy", "ace_ggml_last_error", "ace_ggml_load_dit", "ace_ggml_dit_forward",
    "ace_mi_create_on_device", "ace_mi_dit_get_info", "ace_mi_dit_weight_desc", "ace_mi_dit_forward_batched", "ace_mi_dit_sample",
    "ace_mi_dit_sample_ex", "ace_mi_dit_forward_capture",
    "ace_mi_profile_enable", "ace_mi_dit_set_attn_precision", "ace_mi_profile_reset", "ace_mi_profile_get", "ace_mi_probe_gemm",
    "ace_mi_synchronize", "ace_mi_dit_load_lora", "ace_mi_dit_set_lora_scale", "ace_mi_dit_unload_lora",
    "ace_mi_dit_lora_info",
    "ace_mi_gemm_variant", "ace_ggml_load_vae", "ace_ggml_vae_get_info", "ace_ggml_vae_decode",
    "ace_mi_vae_out_len", "ace_mi_vae_decode_device", "ace_ggml_vae_encode", "ace_mi_vae_enc_out_len",
    "ace_mi_vae_encode_device", "ace_mi_quantize", "ace_mi_dequantize",
    "ace_mi_cond_get_info", "ace_mi_text_project", "ace_mi_lyric_encode", "ace_mi_timbre_encode",
    "ace_mi_build_condition", "ace_ggml_load_lm", "ace_ggml_load_text_encoder", "ace_ggml_text_encoder_forward",
    "ace_ggml_text_encoder_forward_masked", "ace_ggml_text_encoder_forward_embeddings",
    "ace_ggml_text_encoder_forward_layers", "ace_ggml_generate_audio_simple", "ace_ggml_generate_audio_style_lyric_simple",
    "ace_ggml_generate_audio_style_lyric_timbre_simple", "ace_mi_reference_noise",
    "ace_mi_load_lm", "ace_mi_lm_get_info", "ace_mi_lm_begin", "ace_mi_lm_forward", "ace_mi_lm_reset",
    "ace_mi_lm_select", "ace_mi_lm_generate", "ace_mi_lm_fanout", "ace_mi_lm_uniforms",
)

# Every symbol declared in include/acestep_mi355x_selftest.h: the TEST library (libacestep_mi355x_selftest.so = the
# product objects + the kernel self-test / micro-benchmark entries); the product library does not export them.
SELFTEST_SYMBOLS = ("ace_mi_kernel_gemm", "ace_mi_kernel_attention", "ace_mi_kernel_attn_probs", "ace_mi_bench_attention", "ace_mi_bench_gemm",
                    "ace_mi_kernel_gemm_q", "ace_mi_kernel_dequant", "ace_mi_bench_gemm_q", "ace_mi_kernel_gemm_a8",
                    "ace_mi_kernel_gemm_a8_mode", "ace_mi_kernel_attn_kh", "ace_mi_kernel_lora_merge",
                    "ace_mi_kernel_dequant_blocks", "ace_mi_kernel_dequant_segments", "ace_mi_bench_dequant_blocks",
                    "ace_mi_gemm_resolve", "ace_mi_gemm_variant_row", "ace_mi_gemm_variant_arg_ok",
                    "ace_mi_kernel_attn_policy", "ace_mi_attn_plan", "ace_mi_attn_plan_block", "ace_mi_attn_plan_tiles",
                    "ace_mi_kernel_lm_skinny", "ace_mi_kernel_lm_embed", "ace_mi_kernel_lm_qkv_post",
                    "ace_mi_kernel_lm_prefill_kv", "ace_mi_kernel_lm_attention", "ace_mi_kernel_lm_skinny_q",
                    "ace_mi_kernel_lm_embed_q", "ace_mi_kernel_lm_select", "ace_mi_kernel_lm_cache_fanout",
                    "ace_mi_kernel_conv_gemm", "ace_mi_kernel_conv_out", "ace_mi_kernel_pack_f16",
                    "ace_mi_rope_table", "ace_mi_rope_table_steps")

# qtype codes of ace_mi_quantize & co. (names as parse_quant_type, acestep_dit_model.cpp:27-37)
QTYPES = {"q8_0": 1, "q4_k": 2, "q6_k": 3,
          # decode-only (GGUF files carry them; dequantize and the raw-block kernels read them)
          "q4_0": 4, "q4_1": 5, "q5_0": 6, "q5_1": 7, "q2_k": 8, "q3_k": 9, "q5_k": 10, "iq4_nl": 11}
# ggml type ids of the block types (GGUF tensor type field; the raw-block kernels take these)
GGML_BLOCK_TYPES = {"q4_0": 2, "q4_1": 3, "q5_0": 6, "q5_1": 7, "q8_0": 8, "q2_k": 10, "q3_k": 11, "q4_k": 12,
                    "q5_k": 13, "q6_k": 14, "iq4_nl": 20}


class AceInitParams(ctypes.Structure):
    _fields_ = [
        ("n_threads", ctypes.c_int32),
        ("use_metal", ctypes.c_int32),
        ("compute_buffer_bytes", ctypes.c_size_t),
    ]


class AceMiDitInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "hidden_size", "intermediate_size", "num_layers", "num_heads", "num_kv_heads", "head_dim",
        "patch_size", "in_channels", "audio_dim", "sliding_window", "act_type", "device")] + [
        ("weight_bytes", ctypes.c_int64)]


class AceMiCondInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "hidden_size", "lyric_in_dim", "timbre_in_dim", "text_projector_in", "has_lyric_encoder", "lyric_layers",
        "has_timbre_encoder", "timbre_layers")]


class AceMiLoraInfo(ctypes.Structure):
    _fields_ = [("loaded", ctypes.c_int32), ("scale", ctypes.c_float), ("lora_alpha", ctypes.c_float),
                ("min_rank", ctypes.c_int32), ("max_rank", ctypes.c_int32), ("num_modules", ctypes.c_int32),
                ("num_images", ctypes.c_int32), ("image_bytes", ctypes.c_int64), ("merge_ms", ctypes.c_double)]


class AceMiLmInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "vocab_size", "hidden_size", "num_layers", "num_heads", "num_kv_heads", "head_dim", "max_positions", "tied",
        "act_type", "batch", "capacity", "cache_len")] + [("weight_bytes", ctypes.c_int64),
                                                          ("cache_bytes", ctypes.c_int64)]


class AceMiLmSampleParams(ctypes.Structure):
    """ace_mi_lm_sample_params (include/acestep_mi355x.h)."""
    _fields_ = [("cfg_scale", ctypes.c_float), ("pre_temperature", ctypes.c_float), ("repetition_penalty", ctypes.c_float),
                ("top_k", ctypes.c_int32), ("top_p", ctypes.c_float), ("temperature", ctypes.c_float),
                ("d_allowed", ctypes.c_void_p), ("n_allowed", ctypes.c_int32), ("stop_id", ctypes.c_int32),
                ("min_tokens", ctypes.c_int32), ("seed", ctypes.c_uint64)]


class AceMiKernelLmSelectArgs(ctypes.Structure):
    """ace_mi_kernel_lm_select_args (include/acestep_mi355x_selftest.h)."""
    _fields_ = [("B", ctypes.c_int32), ("vocab", ctypes.c_int32), ("ld_logits", ctypes.c_int32),
                ("cfg_scale", ctypes.c_float), ("pre_temperature", ctypes.c_float), ("repetition_penalty", ctypes.c_float),
                ("top_k", ctypes.c_int32), ("top_p", ctypes.c_float), ("temperature", ctypes.c_float),
                ("n_allowed", ctypes.c_int32), ("stop_id", ctypes.c_int32), ("block_stop", ctypes.c_int32),
                ("force_stop", ctypes.c_int32), ("n_emitted", ctypes.c_int32), ("ld_seen", ctypes.c_int32),
                ("token_stride", ctypes.c_int32), ("ld_processed", ctypes.c_int32),
                ("logits", ctypes.c_void_p), ("allowed", ctypes.c_void_p), ("uniform", ctypes.c_void_p),
                ("seen", ctypes.c_void_p), ("tokens", ctypes.c_void_p), ("next_ids", ctypes.c_void_p),
                ("done", ctypes.c_void_p), ("processed", ctypes.c_void_p), ("chains", ctypes.c_void_p)]


class AceMiConvGemmArgs(ctypes.Structure):
    """ace_mi_conv_gemm_args (include/acestep_mi355x_selftest.h)."""
    _fields_ = [(n, ctypes.c_int32) for n in (
        "T_in", "Cin", "taps", "dil", "pad", "in_stride", "M", "N", "Cout", "up", "crop", "T_out", "resid", "store_x",
        "items", "guard")] + [(n, ctypes.c_void_p) for n in (
            "S", "W", "bias", "snake_ea", "snake_eb", "W2", "bias2", "snake2_ea", "snake2_eb", "X", "S_out")]


class AceMiBlockSeg(ctypes.Structure):
    _fields_ = [("type", ctypes.c_int32), ("rows", ctypes.c_int32), ("row0", ctypes.c_int32), ("step", ctypes.c_int32),
                ("group", ctypes.c_int32), ("blocks", ctypes.POINTER(ctypes.c_uint8))]


class AceMiLoraJob(ctypes.Structure):
    _fields_ = [("row0", ctypes.c_int32), ("rows", ctypes.c_int32), ("r", ctypes.c_int32), ("rows_mod", ctypes.c_int32),
                ("A", ctypes.POINTER(ctypes.c_float)), ("B", ctypes.POINTER(ctypes.c_float)), ("eff", ctypes.c_float),
                ("map", ctypes.c_int32), ("row_off", ctypes.c_int32), ("half", ctypes.c_int32),
                ("copy_rest", ctypes.c_int32)]


_LIB = None


def load_library(path: Optional[str] = None) -> ctypes.CDLL:
    """Load and bind the shared library (raises if it was not built: there is no fallback)."""
    global _LIB
    p = path or os.environ.get("ACE_MI_LIB") or LIB_PATH
    if _LIB is not None and path is None:
        return _LIB
    if not os.path.exists(p):
        raise RuntimeError(f"libacestep_mi355x.so not found at {p}: run __graft_entry__.build() / make -C "
                           "ace-step-1.5-ggml_amd/csrc")
    # One HIP runtime per process: torch ships its own libamdhip64 (same SONAME
    # libamdhip64.so.7).  Loading torch first makes this library bind to that
    # already-loaded runtime, so torch device pointers and our kernels share it.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(p)
    vp, i32, f32, sz = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float, ctypes.c_size_t
    fp = ctypes.POINTER(ctypes.c_float)
    ip = ctypes.POINTER(ctypes.c_int32)
    lib.ace_ggml_create.argtypes = [ctypes.POINTER(AceInitParams), ctypes.POINTER(vp)]
    lib.ace_ggml_create.restype = ctypes.c_int
    lib.ace_mi_create_on_device.argtypes = [ctypes.POINTER(AceInitParams), i32, ctypes.POINTER(vp)]
    lib.ace_mi_create_on_device.restype = ctypes.c_int
    lib.ace_ggml_destroy.argtypes = [vp]
    lib.ace_ggml_destroy.restype = None
    lib.ace_ggml_last_error.argtypes = [vp]
    lib.ace_ggml_last_error.restype = ctypes.c_char_p
    lib.ace_ggml_load_dit.argtypes = [vp, ctypes.c_char_p]
    lib.ace_ggml_load_dit.restype = ctypes.c_int
    lib.ace_ggml_dit_forward.argtypes = [vp, fp, fp, fp, ip, ip, i32, i32, f32, f32, fp, sz]
    lib.ace_ggml_dit_forward.restype = ctypes.c_int
    lib.ace_mi_dit_get_info.argtypes = [vp, ctypes.POINTER(AceMiDitInfo)]
    lib.ace_mi_dit_get_info.restype = ctypes.c_int
    lib.ace_mi_dit_weight_desc.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t]
    lib.ace_mi_dit_weight_desc.restype = ctypes.c_int
    lib.ace_mi_dit_forward_batched.argtypes = [vp, i32, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp]
    lib.ace_mi_dit_forward_batched.restype = ctypes.c_int
    lib.ace_mi_dit_forward_capture.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, ip, ip, i32, vp, vp, vp]
    lib.ace_mi_dit_forward_capture.restype = ctypes.c_int
    lib.ace_mi_dit_sample.argtypes = [vp, i32, vp, vp, vp, vp, vp, i32, i32, fp, i32, vp]
    lib.ace_mi_dit_sample.restype = ctypes.c_int
    lib.ace_mi_dit_sample_ex.argtypes = [vp, i32, vp, vp, vp, vp, vp, i32, i32, fp, i32, i32, vp, i32, vp, vp, i32, vp]
    lib.ace_mi_dit_sample_ex.restype = ctypes.c_int
    lib.ace_mi_profile_enable.argtypes = [vp, i32]
    lib.ace_mi_dit_set_attn_precision.argtypes = [vp, i32]
    lib.ace_mi_dit_set_attn_precision.restype = ctypes.c_int
    lib.ace_mi_profile_enable.restype = ctypes.c_int
    lib.ace_mi_profile_reset.argtypes = [vp]
    lib.ace_mi_profile_reset.restype = ctypes.c_int
    lib.ace_mi_profile_get.argtypes = [vp, ctypes.c_char_p, sz, ctypes.POINTER(ctypes.c_double), ip, i32, ip]
    lib.ace_mi_profile_get.restype = ctypes.c_int
    lib.ace_mi_probe_gemm.argtypes = [vp, i32, i32, i32]
    lib.ace_mi_probe_gemm.restype = ctypes.c_int
    lib.ace_mi_synchronize.argtypes = [vp]
    lib.ace_mi_synchronize.restype = ctypes.c_int
    lib.ace_mi_dit_load_lora.argtypes = [vp, ctypes.c_char_p, f32]
    lib.ace_mi_dit_load_lora.restype = ctypes.c_int
    lib.ace_mi_dit_set_lora_scale.argtypes = [vp, f32]
    lib.ace_mi_dit_set_lora_scale.restype = ctypes.c_int
    lib.ace_mi_dit_unload_lora.argtypes = [vp]
    lib.ace_mi_dit_unload_lora.restype = ctypes.c_int
    lib.ace_mi_dit_lora_info.argtypes = [vp, ctypes.POINTER(AceMiLoraInfo)]
    lib.ace_mi_dit_lora_info.restype = ctypes.c_int
    lib.ace_mi_gemm_variant.argtypes = [i32]
    lib.ace_mi_gemm_variant.restype = ctypes.c_int
    i64, u8p = ctypes.c_int64, ctypes.POINTER(ctypes.c_uint8)
    lib.ace_ggml_load_vae.argtypes = [vp, ctypes.c_char_p]
    lib.ace_ggml_load_vae.restype = ctypes.c_int
    lib.ace_ggml_vae_get_info.argtypes = [vp, ip, ip, ip]
    lib.ace_ggml_vae_get_info.restype = ctypes.c_int
    lib.ace_ggml_vae_decode.argtypes = [vp, fp, i32, fp, sz]
    lib.ace_ggml_vae_decode.restype = ctypes.c_int
    lib.ace_mi_vae_out_len.argtypes = [vp, i32, ctypes.POINTER(i64)]
    lib.ace_mi_vae_out_len.restype = ctypes.c_int
    lib.ace_mi_vae_decode_device.argtypes = [vp, vp, i32, vp, vp]
    lib.ace_mi_vae_decode_device.restype = ctypes.c_int
    lib.ace_ggml_vae_encode.argtypes = [vp, fp, i32, fp, sz]
    lib.ace_ggml_vae_encode.restype = ctypes.c_int
    lib.ace_mi_vae_enc_out_len.argtypes = [vp, i32, ctypes.POINTER(i64)]
    lib.ace_mi_vae_enc_out_len.restype = ctypes.c_int
    lib.ace_mi_vae_encode_device.argtypes = [vp, vp, i32, vp, vp]
    lib.ace_mi_vae_encode_device.restype = ctypes.c_int
    lib.ace_mi_quantize.argtypes = [i32, fp, i64, i64, u8p, sz]
    lib.ace_mi_quantize.restype = ctypes.c_int64
    lib.ace_mi_dequantize.argtypes = [i32, u8p, i64, i64, fp]
    lib.ace_mi_dequantize.restype = ctypes.c_int
    for name in ("ace_ggml_load_lm", "ace_ggml_load_text_encoder"):
        getattr(lib, name).argtypes = [vp, ctypes.c_char_p]
        getattr(lib, name).restype = ctypes.c_int
    lib.ace_ggml_text_encoder_forward.argtypes = [vp, ip, i32, fp, sz]
    lib.ace_ggml_text_encoder_forward.restype = ctypes.c_int
    lib.ace_ggml_text_encoder_forward_masked.argtypes = [vp, ip, ip, i32, fp, sz]
    lib.ace_ggml_text_encoder_forward_masked.restype = ctypes.c_int
    lib.ace_ggml_text_encoder_forward_embeddings.argtypes = [vp, ip, i32, fp, sz]
    lib.ace_ggml_text_encoder_forward_embeddings.restype = ctypes.c_int
    lib.ace_ggml_text_encoder_forward_layers.argtypes = [vp, ip, ip, i32, i32, i32, fp, sz]
    lib.ace_ggml_text_encoder_forward_layers.restype = ctypes.c_int
    lib.ace_ggml_generate_audio_simple.argtypes = [vp, ip, i32, i32, f32, i32, fp, sz, ip, ip]
    lib.ace_ggml_generate_audio_simple.restype = ctypes.c_int
    lib.ace_ggml_generate_audio_style_lyric_simple.argtypes = [vp, ip, i32, ip, i32, i32, f32, i32, fp, sz, ip, ip]
    lib.ace_ggml_generate_audio_style_lyric_simple.restype = ctypes.c_int
    lib.ace_ggml_generate_audio_style_lyric_timbre_simple.argtypes = [vp, ip, i32, ip, i32, fp, ip, i32, i32, i32, f32,
                                                                      i32, fp, sz, ip, ip]
    lib.ace_ggml_generate_audio_style_lyric_timbre_simple.restype = ctypes.c_int
    lib.ace_mi_reference_noise.argtypes = [i32, i64, fp]
    lib.ace_mi_reference_noise.restype = ctypes.c_int
    lib.ace_mi_cond_get_info.argtypes = [vp, ctypes.POINTER(AceMiCondInfo)]
    lib.ace_mi_cond_get_info.restype = ctypes.c_int
    lib.ace_mi_text_project.argtypes = [vp, fp, i32, i32, fp, sz]
    lib.ace_mi_text_project.restype = ctypes.c_int
    lib.ace_mi_lyric_encode.argtypes = [vp, fp, i32, fp, sz]
    lib.ace_mi_lyric_encode.restype = ctypes.c_int
    lib.ace_mi_timbre_encode.argtypes = [vp, fp, ip, i32, i32, fp, sz]
    lib.ace_mi_timbre_encode.restype = ctypes.c_int
    lib.ace_mi_build_condition.argtypes = [vp, fp, i32, fp, i32, i32, fp, ip, i32, i32, fp, sz, ip, sz, ip]
    lib.ace_mi_build_condition.restype = ctypes.c_int
    # the LM entries live in their own translation unit (runtime/lm.cpp); a host-emulation library built without it
    # (tests/hostlib.py) has none of them, and the bridge's lm_* methods then fail on the missing symbol
    if hasattr(lib, "ace_mi_load_lm"):
        lib.ace_mi_load_lm.argtypes = [vp, ctypes.c_char_p]
        lib.ace_mi_load_lm.restype = ctypes.c_int
        lib.ace_mi_lm_get_info.argtypes = [vp, ctypes.POINTER(AceMiLmInfo)]
        lib.ace_mi_lm_get_info.restype = ctypes.c_int
        lib.ace_mi_lm_begin.argtypes = [vp, i32, i32]
        lib.ace_mi_lm_begin.restype = ctypes.c_int
        lib.ace_mi_lm_forward.argtypes = [vp, vp, vp, i32, vp, vp]
        lib.ace_mi_lm_forward.restype = ctypes.c_int
        lib.ace_mi_lm_reset.argtypes = [vp]
        lib.ace_mi_lm_reset.restype = ctypes.c_int
        pp = ctypes.POINTER(AceMiLmSampleParams)
        lib.ace_mi_lm_select.argtypes = [vp, pp, vp, vp, vp, i32, i32, vp, vp]
        lib.ace_mi_lm_select.restype = ctypes.c_int
        lib.ace_mi_lm_generate.argtypes = [vp, pp, vp, i32, vp, vp, vp, ip, vp]
        lib.ace_mi_lm_generate.restype = ctypes.c_int
        lib.ace_mi_lm_fanout.argtypes = [vp, i32, i32, vp, vp]
        lib.ace_mi_lm_fanout.restype = ctypes.c_int
        lib.ace_mi_lm_uniforms.argtypes = [ctypes.c_uint64, i64, fp]
        lib.ace_mi_lm_uniforms.restype = ctypes.c_int
    if path is None:
        _LIB = lib
    return lib


_SELFTEST = None


def _bind_gemm_variants(lib: ctypes.CDLL) -> ctypes.CDLL:
    i32, ip = ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)
    lib.ace_mi_gemm_resolve.argtypes = [i32, i32, i32, i32, i32, i32, i32, ip]
    lib.ace_mi_gemm_resolve.restype = ctypes.c_int
    lib.ace_mi_gemm_variant_row.argtypes = [i32, ip, ctypes.c_char_p, ctypes.c_size_t]
    lib.ace_mi_gemm_variant_row.restype = ctypes.c_int
    lib.ace_mi_gemm_variant_arg_ok.argtypes = [i32, i32]
    lib.ace_mi_gemm_variant_arg_ok.restype = ctypes.c_int
    return lib


def _bind_rope_table(lib: ctypes.CDLL) -> ctypes.CDLL:
    i32, ip, fp = ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
    lib.ace_mi_rope_table.argtypes = [i32, i32, ctypes.c_float, fp, fp]
    lib.ace_mi_rope_table.restype = ctypes.c_int
    lib.ace_mi_rope_table_steps.argtypes = [i32, ip, ip, fp, ip, fp, fp]
    lib.ace_mi_rope_table_steps.restype = ctypes.c_int
    return lib


def _bind_attn_plan(lib: ctypes.CDLL) -> ctypes.CDLL:
    i32, ip = ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)
    lib.ace_mi_kernel_attn_policy.argtypes = [ip]
    lib.ace_mi_kernel_attn_policy.restype = ctypes.c_int
    lib.ace_mi_attn_plan.argtypes = [ip, ip, ip]
    lib.ace_mi_attn_plan.restype = ctypes.c_int
    lib.ace_mi_attn_plan_block.argtypes = [i32, i32, i32, i32, i32, ip]
    lib.ace_mi_attn_plan_block.restype = ctypes.c_int
    lib.ace_mi_attn_plan_tiles.argtypes = [i32, i32, i32, i32, i32, i32, i32, ip]
    lib.ace_mi_attn_plan_tiles.restype = ctypes.c_int
    return lib


def selftest_library_path() -> str:
    """Path of the TEST library (a superset of the product ABI that also reads the test-only environment hooks,
    runtime/test_hooks.cpp)."""
    return os.environ.get("ACE_MI_SELFTEST_LIB") or os.path.join(os.path.dirname(LIB_PATH), "libacestep_mi355x_selftest.so")


def load_selftest_library() -> ctypes.CDLL:
    """The TEST library (kernel self-tests / micro-benchmarks, include/acestep_mi355x_selftest.h), built beside the
    product library by the same make; the product library is loaded first (one HIP runtime per process)."""
    global _SELFTEST
    if _SELFTEST is not None:
        return _SELFTEST
    load_library()
    p = selftest_library_path()
    if not os.path.exists(p):
        raise RuntimeError(f"libacestep_mi355x_selftest.so not found at {p}: make -C ace-step-1.5-ggml_amd/csrc")
    lib = ctypes.CDLL(p)
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    fp = ctypes.POINTER(ctypes.c_float)
    ip = ctypes.POINTER(ctypes.c_int32)
    u16p, u8p = ctypes.POINTER(ctypes.c_uint16), ctypes.POINTER(ctypes.c_uint8)
    u16p = ctypes.POINTER(ctypes.c_uint16)
    lib.ace_mi_kernel_gemm.argtypes = [i32, i32, i32, i32, i32, u16p, u16p, fp, fp, u16p]
    lib.ace_mi_kernel_gemm.restype = ctypes.c_int
    lib.ace_mi_kernel_attention.argtypes = [i32, i32, i32, i32, i32, i32, f32, i32, fp, fp, ip, fp]
    lib.ace_mi_kernel_attention.restype = ctypes.c_int
    _bind_attn_probs(lib)
    lib.ace_mi_bench_gemm.argtypes = [i32, i32, i32, i32, i32, i32, i32, fp]
    lib.ace_mi_bench_attention.argtypes = [i32, i32, i32, i32, i32, i32, i32, i32, fp]
    lib.ace_mi_bench_attention.restype = ctypes.c_int
    lib.ace_mi_bench_gemm.restype = ctypes.c_int
    lib.ace_mi_kernel_gemm_q.argtypes = [i32, i32, i32, i32, i32, i32, u16p, u8p, fp, fp, u16p]
    lib.ace_mi_kernel_gemm_q.restype = ctypes.c_int
    lib.ace_mi_kernel_dequant.argtypes = [i32, i32, i32, u8p, u16p]
    lib.ace_mi_kernel_dequant.restype = ctypes.c_int
    lib.ace_mi_bench_gemm_q.argtypes = [i32, i32, i32, i32, i32, i32, i32, fp]
    lib.ace_mi_bench_gemm_q.restype = ctypes.c_int
    i8p = ctypes.POINTER(ctypes.c_int8)
    lib.ace_mi_kernel_gemm_a8.argtypes = [i32, i32, i32, i32, i32, fp, u8p, fp, fp, i8p, fp, fp]
    lib.ace_mi_kernel_gemm_a8.restype = ctypes.c_int
    lib.ace_mi_kernel_gemm_a8_mode.argtypes = [i32]
    lib.ace_mi_kernel_gemm_a8_mode.restype = ctypes.c_int
    lib.ace_mi_kernel_attn_kh.argtypes = [i32]
    lib.ace_mi_kernel_attn_kh.restype = ctypes.c_int
    lib.ace_mi_kernel_lora_merge.argtypes = [i32, i32, i32, i32, i32, u16p, u16p, ctypes.POINTER(AceMiLoraJob), i32]
    lib.ace_mi_kernel_lora_merge.restype = ctypes.c_int
    _bind_dequant_blocks(lib)
    lib.ace_mi_bench_dequant_blocks.argtypes = [i32, i32, i32, i32, i32, fp]
    lib.ace_mi_bench_dequant_blocks.restype = ctypes.c_int
    _bind_gemm_variants(lib)
    _bind_attn_plan(lib)
    _bind_lm_kernels(lib)
    _bind_vae_kernels(lib)
    _bind_rope_table(lib)
    _SELFTEST = lib
    return lib


def _fptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _iptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


class GGMLCAPIBridge:
    """Drop-in for the reference GGMLCAPIBridge (DiT part) backed by the MI355X library."""

    ACE_GGML_OK = ACE_GGML_OK

    def __init__(self, lib_path: Optional[Path] = None, n_threads: int = 0, compute_buffer_mb: int = 0,
                 use_metal: bool = False, device: Optional[int] = None):
        self.lib_path = str(lib_path) if lib_path else LIB_PATH
        self.lib = load_library(None if lib_path is None else str(lib_path))
        self.ctx = ctypes.c_void_p()
        self.closed = False
        self.use_metal = bool(use_metal)
        params = AceInitParams(n_threads=int(n_threads), use_metal=1 if use_metal else 0,
                               compute_buffer_bytes=int(compute_buffer_mb) * 1024 * 1024)
        if device is None:
            st = self.lib.ace_ggml_create(ctypes.byref(params), ctypes.byref(self.ctx))
        else:
            st = self.lib.ace_mi_create_on_device(ctypes.byref(params), int(device), ctypes.byref(self.ctx))
        self._ensure_ok(st, "ace_ggml_create")
        atexit.register(self.close)
        self.info: Optional[AceMiDitInfo] = None
        self.host_memory = False  # True: the library's "device" pointers are host pointers (a host build of the runtime)
        self.audio_channels = 0
        self.hop_length = 0
        self.latent_channels = 0

    # -- reference surface -------------------------------------------------
    def _last_error(self) -> str:
        msg = self.lib.ace_ggml_last_error(self.ctx)
        return msg.decode("utf-8", errors="replace") if msg else "unknown error"

    def _ensure_ok(self, status: int, where: str) -> None:
        if status != self.ACE_GGML_OK:
            raise RuntimeError(f"{where} failed: {self._last_error()} (status={status})")

    def close(self) -> None:
        if not self.closed and self.ctx:
            self.lib.ace_ggml_destroy(self.ctx)
            self.closed = True

    def load_dit(self, model_dir) -> None:
        st = self.lib.ace_ggml_load_dit(self.ctx, str(model_dir).encode("utf-8"))
        self._ensure_ok(st, "ace_ggml_load_dit")
        info = AceMiDitInfo()
        self._ensure_ok(self.lib.ace_mi_dit_get_info(self.ctx, ctypes.byref(info)), "ace_mi_dit_get_info")
        self.info = info

    def dit_weight_desc(self) -> str:
        """The device formats of the loaded 2-D weights ("bf16", "q4_K planes", "ggml raw blocks (q5_K, q6_K)", ...)."""
        buf = ctypes.create_string_buffer(256)
        self._ensure_ok(self.lib.ace_mi_dit_weight_desc(self.ctx, buf, len(buf)), "ace_mi_dit_weight_desc")
        return buf.value.decode("utf-8")

    def dit_forward_tfirst(self, hidden_states_tfirst, context_latents_tfirst, encoder_hidden_states_tfirst,
                           attention_mask, encoder_attention_mask, timestep: float, timestep_r: float) -> np.ndarray:
        """[T, D], [T, Ctx], [L, H], [T] int32, [L] int32 -> vt [T, D] float32 (host buffers)."""
        hs = np.ascontiguousarray(hidden_states_tfirst, dtype=np.float32)
        ctx = np.ascontiguousarray(context_latents_tfirst, dtype=np.float32)
        enc = np.ascontiguousarray(encoder_hidden_states_tfirst, dtype=np.float32)
        am = None if attention_mask is None else np.ascontiguousarray(attention_mask, dtype=np.int32)
        eam = None if encoder_attention_mask is None else np.ascontiguousarray(encoder_attention_mask, dtype=np.int32)
        if hs.ndim != 2 or ctx.ndim != 2 or enc.ndim != 2:
            raise ValueError("dit inputs must be 2D arrays [T,D]/[T,Ctx]/[L,H]")
        seq_len = int(hs.shape[0])
        enc_len = int(enc.shape[0])
        out = np.empty_like(hs, dtype=np.float32)
        st = self.lib.ace_ggml_dit_forward(self.ctx, _fptr(hs), _fptr(ctx), _fptr(enc), _iptr(am), _iptr(eam),
                                           seq_len, enc_len, float(timestep), float(timestep_r), _fptr(out),
                                           out.nbytes)
        self._ensure_ok(st, "ace_ggml_dit_forward")
        return out

    def load_vae(self, model_dir) -> None:
        """ace_ggml_load_vae + ace_ggml_vae_get_info (run_non_ggml_real_case.py:243-253)."""
        self._ensure_ok(self.lib.ace_ggml_load_vae(self.ctx, str(model_dir).encode("utf-8")), "ace_ggml_load_vae")
        lat, aud, hop = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        st = self.lib.ace_ggml_vae_get_info(self.ctx, ctypes.byref(lat), ctypes.byref(aud), ctypes.byref(hop))
        self._ensure_ok(st, "ace_ggml_vae_get_info")
        self.latent_channels, self.audio_channels, self.hop_length = int(lat.value), int(aud.value), int(hop.value)

    def vae_decode_tfirst(self, latents_tfirst) -> np.ndarray:
        """latents [T, C] f32 -> audio [T*hop, channels] f32 (host buffers; :283-305)."""
        if self.audio_channels <= 0 or self.hop_length <= 0:
            raise RuntimeError("VAE not initialized in ggml bridge")
        lat = np.ascontiguousarray(latents_tfirst, dtype=np.float32)
        n_frames = int(lat.shape[0])
        out_samples = n_frames * self.hop_length
        out = np.empty((out_samples * self.audio_channels,), dtype=np.float32)
        st = self.lib.ace_ggml_vae_decode(self.ctx, _fptr(lat), n_frames, _fptr(out), out.nbytes)
        self._ensure_ok(st, "ace_ggml_vae_decode")
        return out.reshape(out_samples, self.audio_channels)

    def vae_encode_tfirst(self, audio_tfirst) -> np.ndarray:
        """audio [samples, channels] f32 -> latent mean [samples // hop, latent_channels] (host buffers)."""
        if self.latent_channels <= 0 or self.hop_length <= 0:
            raise RuntimeError("VAE not initialized in ggml bridge")
        a = np.ascontiguousarray(audio_tfirst, dtype=np.float32)
        n = int(a.shape[0])
        out = np.empty((n // self.hop_length, self.latent_channels), dtype=np.float32)
        st = self.lib.ace_ggml_vae_encode(self.ctx, _fptr(a), n, _fptr(out), out.nbytes)
        self._ensure_ok(st, "ace_ggml_vae_encode")
        return out

    # -- Qwen3 text encoder (acestep_ggml.h:41-94; the reference's ctypes callers are
    #    acestep_ggml/tools/compare_text_encoder.py and run_style_lyric_pipeline.py) ----------------
    def load_text_encoder(self, model_dir) -> None:
        st = self.lib.ace_ggml_load_text_encoder(self.ctx, str(model_dir).encode("utf-8"))
        self._ensure_ok(st, "ace_ggml_load_text_encoder")
        with open(os.path.join(str(model_dir) if not str(model_dir).endswith(".gguf")
                               else os.path.dirname(str(model_dir)), "config.json"), "r", encoding="utf-8") as f:
            import json
            self.text_hidden = int(json.load(f)["hidden_size"])

    def text_encoder_forward(self, token_ids, attention_mask=None, n_layers: Optional[int] = None,
                             apply_final_norm: bool = True) -> np.ndarray:
        """Causal Qwen3 forward: ids [n] -> hidden states [n, hidden] (the _layers entry when n_layers is
        given, _masked with a mask, the plain entry otherwise)."""
        ids = np.ascontiguousarray(token_ids, dtype=np.int32)
        am = None if attention_mask is None else np.ascontiguousarray(attention_mask, dtype=np.int32)
        out = np.empty((ids.shape[0], self.text_hidden), np.float32)
        if n_layers is not None:
            st = self.lib.ace_ggml_text_encoder_forward_layers(self.ctx, _iptr(ids), _iptr(am), ids.shape[0],
                                                               int(n_layers), 1 if apply_final_norm else 0,
                                                               _fptr(out), out.nbytes)
        elif am is not None:
            st = self.lib.ace_ggml_text_encoder_forward_masked(self.ctx, _iptr(ids), _iptr(am), ids.shape[0],
                                                               _fptr(out), out.nbytes)
        else:
            st = self.lib.ace_ggml_text_encoder_forward(self.ctx, _iptr(ids), ids.shape[0], _fptr(out), out.nbytes)
        self._ensure_ok(st, "ace_ggml_text_encoder_forward")
        return out

    # -- the 5 Hz causal LM with its KV cache (include/acestep_mi355x.h ace_mi_load_lm / ace_mi_lm_*) -----------
    def load_lm(self, model_dir) -> None:
        """A HF Qwen3ForCausalLM directory into the LM slot (the text encoder stays resident beside it)."""
        self._ensure_ok(self.lib.ace_mi_load_lm(self.ctx, str(model_dir).encode("utf-8")), "ace_mi_load_lm")

    def lm_info(self) -> dict:
        info = AceMiLmInfo()
        self._ensure_ok(self.lib.ace_mi_lm_get_info(self.ctx, ctypes.byref(info)), "ace_mi_lm_get_info")
        return {n: int(getattr(info, n)) for n, _ in AceMiLmInfo._fields_}

    def lm_begin(self, batch: int, capacity: int) -> None:
        self._ensure_ok(self.lib.ace_mi_lm_begin(self.ctx, int(batch), int(capacity)), "ace_mi_lm_begin")

    def lm_reset(self) -> None:
        self._ensure_ok(self.lib.ace_mi_lm_reset(self.ctx), "ace_mi_lm_reset")

    def lm_forward_device(self, d_ids: int, d_mask: int, n: int, d_logits: int, stream: int = 0) -> None:
        st = self.lib.ace_mi_lm_forward(self.ctx, d_ids, d_mask or None, int(n), d_logits, stream or None)
        self._ensure_ok(st, "ace_mi_lm_forward")

    def lm_forward(self, input_ids, attention_mask=None):
        """Append input_ids [B, n] (torch tensor on the engine's device; attention_mask [B, n] for the same columns,
        or None) and return the last position's logits as an f32 [B, vocab] tensor on that device, in stream
        order on torch's current stream (the stream rules of hook.dit_forward_torch)."""
        import torch
        from .hook import _OrderedCall
        ids = input_ids.detach().to(torch.int32).contiguous()
        if ids.dim() != 2:
            raise ValueError("lm_forward: input_ids must be [B, n]")
        dev = ids.device
        am = None
        if attention_mask is not None:
            am = (attention_mask.detach().to(dev) != 0).to(torch.int32).contiguous()
            if am.shape != ids.shape:
                raise ValueError("lm_forward: attention_mask must cover exactly the appended columns")
        if getattr(self, "_lm_vocab", None) is None:
            self._lm_vocab = self.lm_info()["vocab_size"]
        out = torch.empty((ids.shape[0], self._lm_vocab), dtype=torch.float32, device=dev)
        with _OrderedCall(self, dev) as stream:
            self.lm_forward_device(ids.data_ptr(), am.data_ptr() if am is not None else 0, ids.shape[1],
                                   out.data_ptr(), stream)
        return out

    def _lm_sample_params(self, dev, allowed_ids=None, stop_id=-1, min_tokens=0, cfg_scale=1.0, pre_temperature=0.0,
                          temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0, seed=0):
        """(ace_mi_lm_sample_params, the device tensor it points into): allowed_ids = ascending ids or None."""
        import torch
        allowed = None
        if allowed_ids is not None:
            allowed = torch.as_tensor(allowed_ids).detach().to(device=dev, dtype=torch.int32).contiguous().reshape(-1)
        p = AceMiLmSampleParams(
            cfg_scale=float(cfg_scale), pre_temperature=float(pre_temperature or 0.0),
            repetition_penalty=float(repetition_penalty), top_k=int(top_k or 0),
            top_p=float(top_p if top_p is not None else 1.0), temperature=float(temperature),
            d_allowed=allowed.data_ptr() if allowed is not None and allowed.numel() else None,
            n_allowed=int(allowed.numel()) if allowed is not None else 0,
            stop_id=-1 if stop_id is None else int(stop_id), min_tokens=int(min_tokens), seed=int(seed) & (2 ** 64 - 1))
        if allowed is not None and allowed.numel() == 0:
            p.d_allowed = ctypes.c_void_p(1).value  # an empty list stays a list: the entry refuses n_allowed < 1
        return p, allowed

    def lm_select(self, logits, uniforms=None, seen=None, n_emitted: int = 0, force_stop: bool = False, **params):
        """One token per sampled sequence from `logits` [B, vocab] (f32 tensor on the engine's device, as lm_forward
        returns them): ace_mi_lm_select with the keyword parameters of _lm_sample_params.  uniforms: f32 [S] (needed
        when temperature > 0); seen: uint8 [S, vocab] map, updated in place.  Returns int32 [S], in stream order on
        torch's current stream (the stream rules of lm_forward)."""
        import torch
        from .hook import _OrderedCall
        if logits.dtype != torch.float32 or not logits.is_contiguous() or logits.dim() != 2:
            raise ValueError("lm_select: logits must be a contiguous f32 [B, vocab] tensor")
        dev = logits.device
        p, keep = self._lm_sample_params(dev, **params)
        S = logits.shape[0] // 2 if p.cfg_scale > 1.0 else logits.shape[0]
        u = None
        if uniforms is not None:
            u = uniforms.detach().to(device=dev, dtype=torch.float32).contiguous()
            if u.numel() != S and not (p.cfg_scale > 1.0 and logits.shape[0] % 2):  # an odd pair batch: the entry refuses
                raise ValueError("lm_select: uniforms must hold one value per sampled sequence")
        if seen is not None and (seen.dtype != torch.uint8 or not seen.is_contiguous() or seen.device != dev
                                 or tuple(seen.shape) != (S, logits.shape[1])):
            raise ValueError("lm_select: seen must be a contiguous uint8 [S, vocab] tensor on the logits' device")
        out = torch.empty((max(S, 1),), dtype=torch.int32, device=dev)
        with _OrderedCall(self, dev) as stream:
            st = self.lib.ace_mi_lm_select(self.ctx, ctypes.byref(p), logits.data_ptr(),
                                           u.data_ptr() if u is not None else None,
                                           seen.data_ptr() if seen is not None else None, int(n_emitted),
                                           1 if force_stop else 0, out.data_ptr(), stream or None)
        self._ensure_ok(st, "ace_mi_lm_select")
        del keep
        return out[:S]

    def lm_generate(self, logits, n_max: int, uniforms=None, seen=None, **params):
        """The engine-side decode loop (ace_mi_lm_generate) on the live cache: `logits` [B, vocab] f32 are those of the
        last lm_forward and are overwritten.  uniforms: f32 [n_max, S] or None (the engine then draws them from
        params' seed).  Returns (tokens int32 [S, n_max], n_out); the call returns once the loop has run."""
        import torch
        from .hook import _OrderedCall
        if logits.dtype != torch.float32 or not logits.is_contiguous() or logits.dim() != 2:
            raise ValueError("lm_generate: logits must be a contiguous f32 [B, vocab] tensor")
        dev = logits.device
        p, keep = self._lm_sample_params(dev, **params)
        S = logits.shape[0] // 2 if p.cfg_scale > 1.0 else logits.shape[0]
        n_max = int(n_max)
        u = None
        if uniforms is not None:
            u = uniforms.detach().to(device=dev, dtype=torch.float32).contiguous()
            if u.numel() != max(n_max, 0) * S:
                raise ValueError("lm_generate: uniforms must be [n_max, S]")
        if seen is not None and (seen.dtype != torch.uint8 or not seen.is_contiguous() or seen.device != dev
                                 or tuple(seen.shape) != (S, logits.shape[1])):
            raise ValueError("lm_generate: seen must be a contiguous uint8 [S, vocab] tensor on the logits' device")
        out = torch.zeros((max(S, 1), max(n_max, 1)), dtype=torch.int32, device=dev)
        n_out = ctypes.c_int32(0)
        with _OrderedCall(self, dev) as stream:
            st = self.lib.ace_mi_lm_generate(self.ctx, ctypes.byref(p), logits.data_ptr(), n_max,
                                             u.data_ptr() if u is not None else None,
                                             seen.data_ptr() if seen is not None else None, out.data_ptr(),
                                             ctypes.byref(n_out), stream or None)
        self._ensure_ok(st, "ace_mi_lm_generate")
        del keep
        return out[:S], int(n_out.value)

    def lm_fanout(self, copies: int, capacity: int, logits=None):
        """Re-lay the live cache of G = 1 or 2 sequences for G * copies sequences of up to `capacity` positions
        (ace_mi_lm_fanout): sequence g * copies + s is a bit copy of sequence g.  logits: the f32 [G, vocab] tensor of
        the prefill, or None; returns the [G * copies, vocab] tensor whose row g * copies + s is row g (None without
        logits).  Synchronous."""
        import torch
        from .hook import _OrderedCall
        copies = int(copies)
        if logits is None:
            self._ensure_ok(self.lib.ace_mi_lm_fanout(self.ctx, copies, int(capacity), None, None), "ace_mi_lm_fanout")
            return None
        if logits.dtype != torch.float32 or not logits.is_contiguous() or logits.dim() != 2:
            raise ValueError("lm_fanout: logits must be a contiguous f32 [G, vocab] tensor")
        G = logits.shape[0]
        out = torch.empty((G * max(copies, 1), logits.shape[1]), dtype=torch.float32, device=logits.device)
        out[:G].copy_(logits)
        with _OrderedCall(self, logits.device) as stream:
            st = self.lib.ace_mi_lm_fanout(self.ctx, copies, int(capacity), out.data_ptr(), stream or None)
        self._ensure_ok(st, "ace_mi_lm_fanout")
        return out

    def lm_uniforms(self, seed: int, n: int) -> np.ndarray:
        """The engine's uniform stream for one sequence (ace_mi_lm_uniforms): n f32 values of `seed`, what lm_generate
        draws with uniforms=None and S == 1."""
        out = np.empty((int(n),), np.float32)
        st = self.lib.ace_mi_lm_uniforms(int(seed) & (2 ** 64 - 1), int(n), _fptr(out))
        self._ensure_ok(st, "ace_mi_lm_uniforms")
        return out

    # reference GGMLCAPIBridge names (scripts/run_non_ggml_real_case.py:255-281)
    def text_forward_full(self, token_ids, hidden_dim: int) -> np.ndarray:
        ids = np.ascontiguousarray(token_ids, dtype=np.int32)
        out = np.empty((ids.shape[0] * int(hidden_dim),), np.float32)
        st = self.lib.ace_ggml_text_encoder_forward(self.ctx, _iptr(ids), ids.shape[0], _fptr(out), out.nbytes)
        self._ensure_ok(st, "ace_ggml_text_encoder_forward")
        return out.reshape(ids.shape[0], int(hidden_dim))

    def text_forward_embeddings(self, token_ids, hidden_dim: int) -> np.ndarray:
        ids = np.ascontiguousarray(token_ids, dtype=np.int32)
        out = np.empty((ids.shape[0] * int(hidden_dim),), np.float32)
        st = self.lib.ace_ggml_text_encoder_forward_embeddings(self.ctx, _iptr(ids), ids.shape[0], _fptr(out),
                                                               out.nbytes)
        self._ensure_ok(st, "ace_ggml_text_encoder_forward_embeddings")
        return out.reshape(ids.shape[0], int(hidden_dim))

    def text_encoder_embeddings(self, token_ids) -> np.ndarray:
        ids = np.ascontiguousarray(token_ids, dtype=np.int32)
        out = np.empty((ids.shape[0], self.text_hidden), np.float32)
        st = self.lib.ace_ggml_text_encoder_forward_embeddings(self.ctx, _iptr(ids), ids.shape[0], _fptr(out),
                                                               out.nbytes)
        self._ensure_ok(st, "ace_ggml_text_encoder_forward_embeddings")
        return out

    # -- end-to-end generation (acestep_ggml.h:110-152; reference caller:
    #    acestep_ggml/tools/run_unified_prompt_style_lyric_timbre.py) ------------------------------------
    def generate_audio(self, seq_len: int, shift: float = 3.0, seed: int = 0, token_ids=None, style_ids=None,
                       lyric_ids=None, refer=None, refer_order_mask=None) -> np.ndarray:
        """audio [samples, channels]: ace_ggml_generate_audio_simple when token_ids is given, else the
        style/lyric(/timbre) entry."""
        if self.audio_channels <= 0 or self.hop_length <= 0:
            raise RuntimeError("VAE not initialized in ggml bridge")
        out = np.empty((int(seq_len) * self.hop_length * self.audio_channels,), np.float32)
        ns, nc = ctypes.c_int32(0), ctypes.c_int32(0)
        arr = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)
        if token_ids is not None:
            ids = arr(token_ids)
            st = self.lib.ace_ggml_generate_audio_simple(self.ctx, _iptr(ids), len(ids), int(seq_len), float(shift),
                                                         int(seed), _fptr(out), out.nbytes, ctypes.byref(ns),
                                                         ctypes.byref(nc))
        else:
            si, li = arr(style_ids), arr(lyric_ids)
            n_s = 0 if si is None else len(si)
            n_l = 0 if li is None else len(li)
            if refer is None:
                st = self.lib.ace_ggml_generate_audio_style_lyric_simple(
                    self.ctx, _iptr(si), n_s, _iptr(li), n_l, int(seq_len), float(shift), int(seed), _fptr(out),
                    out.nbytes, ctypes.byref(ns), ctypes.byref(nc))
            else:
                rf = np.ascontiguousarray(refer, dtype=np.float32)
                om = arr(refer_order_mask)
                st = self.lib.ace_ggml_generate_audio_style_lyric_timbre_simple(
                    self.ctx, _iptr(si), n_s, _iptr(li), n_l, _fptr(rf), _iptr(om), int(rf.shape[0]),
                    int(rf.shape[1]), int(seq_len), float(shift), int(seed), _fptr(out), out.nbytes,
                    ctypes.byref(ns), ctypes.byref(nc))
        self._ensure_ok(st, "ace_ggml_generate_audio")
        return out[: ns.value * nc.value].reshape(ns.value, nc.value)

    # -- condition encoders (include/acestep_mi355x.h; acestep_ggml.cpp:1624-1899, :2414-2556) -------
    def cond_info(self) -> AceMiCondInfo:
        info = AceMiCondInfo()
        self._ensure_ok(self.lib.ace_mi_cond_get_info(self.ctx, ctypes.byref(info)), "ace_mi_cond_get_info")
        return info

    def text_project(self, states) -> np.ndarray:
        """encoder.text_projector: [n, in] -> [n, H]."""
        x = np.ascontiguousarray(states, dtype=np.float32)
        out = np.empty((x.shape[0], self.cond_info().hidden_size), np.float32)
        st = self.lib.ace_mi_text_project(self.ctx, _fptr(x), int(x.shape[0]), int(x.shape[1]), _fptr(out), out.nbytes)
        self._ensure_ok(st, "ace_mi_text_project")
        return out

    def lyric_encode(self, lyric_embeds) -> np.ndarray:
        """Lyric encoder: token embeddings [n, text_hidden] -> [n, H]."""
        x = np.ascontiguousarray(lyric_embeds, dtype=np.float32)
        out = np.empty((x.shape[0], self.cond_info().hidden_size), np.float32)
        st = self.lib.ace_mi_lyric_encode(self.ctx, _fptr(x), int(x.shape[0]), _fptr(out), out.nbytes)
        self._ensure_ok(st, "ace_mi_lyric_encode")
        return out

    def timbre_encode(self, refer, order_mask=None) -> np.ndarray:
        """Timbre encoder: references [n_refer, refer_len, timbre_in] -> [n_refer, H]."""
        x = np.ascontiguousarray(refer, dtype=np.float32)
        om = None if order_mask is None else np.ascontiguousarray(order_mask, dtype=np.int32)
        out = np.empty((x.shape[0], self.cond_info().hidden_size), np.float32)
        st = self.lib.ace_mi_timbre_encode(self.ctx, _fptr(x), _iptr(om), int(x.shape[0]), int(x.shape[1]),
                                           _fptr(out), out.nbytes)
        self._ensure_ok(st, "ace_mi_timbre_encode")
        return out

    def build_condition(self, style_states=None, lyric_embeds=None, refer=None, refer_order_mask=None,
                        text_hidden: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """(encoder_hidden_states [len, H], encoder_attention_mask [len]) from text-encoder style states,
        lyric token embeddings and timbre references."""
        ss = None if style_states is None else np.ascontiguousarray(style_states, dtype=np.float32)
        le = None if lyric_embeds is None else np.ascontiguousarray(lyric_embeds, dtype=np.float32)
        rf = None if refer is None else np.ascontiguousarray(refer, dtype=np.float32)
        om = None if refer_order_mask is None else np.ascontiguousarray(refer_order_mask, dtype=np.int32)
        ns = 0 if ss is None else int(ss.shape[0])
        nl = 0 if le is None else int(le.shape[0])
        nr, rl = (0, 0) if rf is None else (int(rf.shape[0]), int(rf.shape[1]))
        if text_hidden is None:
            text_hidden = int(ss.shape[1]) if ss is not None else (int(le.shape[1]) if le is not None else 0)
        H = self.cond_info().hidden_size
        cap = max(ns + nl + nr, 1)
        enc = np.empty((cap, H), np.float32)
        mask = np.empty(cap, np.int32)
        n = ctypes.c_int32(0)
        st = self.lib.ace_mi_build_condition(self.ctx, _fptr(ss), ns, _fptr(le), nl, int(text_hidden), _fptr(rf),
                                             _iptr(om), nr, rl, _fptr(enc), enc.nbytes, _iptr(mask), mask.nbytes,
                                             ctypes.byref(n))
        self._ensure_ok(st, "ace_mi_build_condition")
        return enc[: n.value].copy(), mask[: n.value].copy()

    # -- MI355X extensions ---------------------------------------------------
    def vae_enc_out_len(self, n_samples: int) -> int:
        n = ctypes.c_int64(0)
        st = self.lib.ace_mi_vae_enc_out_len(self.ctx, int(n_samples), ctypes.byref(n))
        self._ensure_ok(st, "ace_mi_vae_enc_out_len")
        return int(n.value)

    def vae_encode_device(self, d_audio: int, n_samples: int, d_out: int, stream: int = 0) -> None:
        st = self.lib.ace_mi_vae_encode_device(self.ctx, d_audio, int(n_samples), d_out, stream or None)
        self._ensure_ok(st, "ace_mi_vae_encode_device")

    def vae_out_len(self, n_frames: int) -> int:
        n = ctypes.c_int64(0)
        self._ensure_ok(self.lib.ace_mi_vae_out_len(self.ctx, int(n_frames), ctypes.byref(n)), "ace_mi_vae_out_len")
        return int(n.value)

    def vae_decode_device(self, d_latents: int, n_frames: int, d_out: int, stream: int = 0) -> None:
        st = self.lib.ace_mi_vae_decode_device(self.ctx, d_latents, int(n_frames), d_out, stream or None)
        self._ensure_ok(st, "ace_mi_vae_decode_device")

    def dit_forward_batched_device(self, batch: int, seq_len: int, enc_len: int, d_hidden: int, d_context: int,
                                   d_enc: int, d_mask: int, d_enc_mask: int, d_t: int, d_r: int, d_out: int,
                                   stream: int = 0) -> None:
        st = self.lib.ace_mi_dit_forward_batched(self.ctx, int(batch), d_hidden or None, d_context or None,
                                                 d_enc or None, d_mask or None, d_enc_mask or None, int(seq_len),
                                                 int(enc_len), d_t, d_r, d_out, stream or None)
        self._ensure_ok(st, "ace_mi_dit_forward_batched")

    def dit_forward_capture_device(self, batch: int, seq_len: int, enc_len: int, d_hidden: int, d_context: int,
                                   d_enc: int, d_mask: int, d_enc_mask: int, d_t: int, d_r: int, pairs, early_exit: bool,
                                   d_out: int, d_probs: int, stream: int = 0) -> None:
        """ace_mi_dit_forward_capture: pairs = [(layer, head), ...]; d_probs device f32 [len(pairs)][batch][Np][enc_len]
        in that order; d_out may be 0 with early_exit."""
        layers = np.ascontiguousarray([int(p[0]) for p in pairs], dtype=np.int32)
        heads = np.ascontiguousarray([int(p[1]) for p in pairs], dtype=np.int32)
        st = self.lib.ace_mi_dit_forward_capture(self.ctx, int(batch), int(seq_len), int(enc_len), d_hidden or None,
                                                 d_context or None, d_enc or None, d_mask or None, d_enc_mask or None,
                                                 d_t, d_r, len(layers), _iptr(layers), _iptr(heads),
                                                 1 if early_exit else 0, d_out or None, d_probs or None, stream or None)
        self._ensure_ok(st, "ace_mi_dit_forward_capture")

    def dit_sample_device(self, batch: int, seq_len: int, enc_len: int, d_xt: int, d_context: int, d_enc: int,
                          d_mask: int, d_enc_mask: int, schedule: List[float], stream: int = 0) -> None:
        sched = np.ascontiguousarray(schedule, dtype=np.float32)
        st = self.lib.ace_mi_dit_sample(self.ctx, int(batch), d_xt, d_context or None, d_enc or None,
                                        d_mask or None, d_enc_mask or None, int(seq_len), int(enc_len),
                                        _fptr(sched), int(sched.shape[0]), stream or None)
        self._ensure_ok(st, "ace_mi_dit_sample")

    def dit_sample_ex_device(self, batch: int, seq_len: int, enc_len: int, d_xt: int, d_context: int, d_enc: int,
                             d_mask: int, d_enc_mask: int, schedule: List[float], sde: bool = False, d_noise: int = 0,
                             cover_steps: int = -1, d_context_nc: int = 0, d_enc_nc: int = 0,
                             cache_cross: bool = True, stream: int = 0) -> None:
        """The MLX/PyTorch generation loop on the device (ace_mi_dit_sample_ex)."""
        sched = np.ascontiguousarray(schedule, dtype=np.float32)
        st = self.lib.ace_mi_dit_sample_ex(self.ctx, int(batch), d_xt, d_context or None, d_enc or None,
                                           d_mask or None, d_enc_mask or None, int(seq_len), int(enc_len),
                                           _fptr(sched), int(sched.shape[0]), 1 if sde else 0, d_noise or None,
                                           int(cover_steps), d_context_nc or None, d_enc_nc or None,
                                           1 if cache_cross else 0, stream or None)
        self._ensure_ok(st, "ace_mi_dit_sample_ex")

    # -- PEFT LoRA adapters (include/acestep_mi355x.h) -----------------------------------------------
    def load_lora(self, path, scale: float = 1.0) -> None:
        """Load adapter_config.json + adapter_model.safetensors of `path` at strength `scale` (replaces any
        previous adapter; synchronous)."""
        st = self.lib.ace_mi_dit_load_lora(self.ctx, str(path).encode("utf-8"), float(scale))
        self._ensure_ok(st, "ace_mi_dit_load_lora")

    def set_lora_scale(self, scale: float) -> None:
        """Rebuild the adapted weights from the base at a new strength (0 = base weights, adapter kept)."""
        self._ensure_ok(self.lib.ace_mi_dit_set_lora_scale(self.ctx, float(scale)), "ace_mi_dit_set_lora_scale")

    def unload_lora(self) -> None:
        self._ensure_ok(self.lib.ace_mi_dit_unload_lora(self.ctx), "ace_mi_dit_unload_lora")

    def lora_info(self) -> dict:
        info = AceMiLoraInfo()
        self._ensure_ok(self.lib.ace_mi_dit_lora_info(self.ctx, ctypes.byref(info)), "ace_mi_dit_lora_info")
        return dict(loaded=bool(info.loaded), scale=float(info.scale), lora_alpha=float(info.lora_alpha),
                    min_rank=int(info.min_rank), max_rank=int(info.max_rank), num_modules=int(info.num_modules),
                    num_images=int(info.num_images), image_bytes=int(info.image_bytes), merge_ms=float(info.merge_ms))

    def synchronize(self) -> None:
        self._ensure_ok(self.lib.ace_mi_synchronize(self.ctx), "ace_mi_synchronize")

    def set_attn_precision(self, mode: str) -> None:
        """DiT attention operand precision for subsequent forwards: "fp16", "split", "f32", "f8c" or "pv8"
        (include/acestep_mi355x.h, ace_mi_dit_set_attn_precision)."""
        code = {"fp16": 0, "split": 1, "f32": 2, "f8c": 3, "pv8": 4}[mode]
        self._ensure_ok(self.lib.ace_mi_dit_set_attn_precision(self.ctx, code), "ace_mi_dit_set_attn_precision")

    def profile_enable(self, on: bool) -> None:
        self._ensure_ok(self.lib.ace_mi_profile_enable(self.ctx, 1 if on else 0), "ace_mi_profile_enable")

    def profile_reset(self) -> None:
        self._ensure_ok(self.lib.ace_mi_profile_reset(self.ctx), "ace_mi_profile_reset")

    def profile_get(self) -> List[Tuple[str, float, int]]:
        cap = 64
        names = ctypes.create_string_buffer(8192)
        ms = (ctypes.c_double * cap)()
        counts = (ctypes.c_int32 * cap)()
        n = ctypes.c_int32(0)
        self._ensure_ok(self.lib.ace_mi_profile_get(self.ctx, names, 8192, ms, counts, cap, ctypes.byref(n)),
                        "ace_mi_profile_get")
        raw = names.raw.split(b"\0")
        return [(raw[i].decode(), float(ms[i]), int(counts[i])) for i in range(min(n.value, cap))]

    def probe_gemm(self, which: int, m_rows: int, iters: int) -> None:
        self._ensure_ok(self.lib.ace_mi_probe_gemm(self.ctx, int(which), int(m_rows), int(iters)),
                        "ace_mi_probe_gemm")


# ---- kernel self-test wrappers (GPU parity tests) ----------------------------
def kernel_gemm(a_bits: np.ndarray, w_bits: np.ndarray, act_type: int = 0, epi: int = 0,
                bias: Optional[np.ndarray] = None, x: Optional[np.ndarray] = None) -> np.ndarray:
    """a_bits [M][K], w_bits [N][K] uint16 words; epi 0 -> f32 [M][N], epi 4 -> uint16 [M][N/2];
    epi 3 / 2 -> f32 x + C (* gate) with x [M][N] f32 and, for epi 2, the gate [N] passed as `bias`."""
    lib = load_selftest_library()
    a = np.ascontiguousarray(a_bits, dtype=np.uint16)
    w = np.ascontiguousarray(w_bits, dtype=np.uint16)
    M, K = a.shape
    N = w.shape[0]
    u16p = ctypes.POINTER(ctypes.c_uint16)
    b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
    if epi in (2, 3):
        out = np.array(x, dtype=np.float32, order="C", copy=True)
        st = lib.ace_mi_kernel_gemm(act_type, epi, M, N, K, a.ctypes.data_as(u16p), w.ctypes.data_as(u16p),
                                    _fptr(b), _fptr(out), None)
    elif epi == 0:
        out = np.empty((M, N), dtype=np.float32)
        st = lib.ace_mi_kernel_gemm(act_type, epi, M, N, K, a.ctypes.data_as(u16p), w.ctypes.data_as(u16p),
                                    _fptr(b), _fptr(out), None)
    else:
        out = np.empty((M, N // 2), dtype=np.uint16)
        st = lib.ace_mi_kernel_gemm(act_type, epi, M, N, K, a.ctypes.data_as(u16p), w.ctypes.data_as(u16p),
                                    _fptr(b), None, out.ctypes.data_as(u16p))
    if st != ACE_GGML_OK:
        raise RuntimeError(f"ace_mi_kernel_gemm failed (status={st})")
    return out


def kernel_attention(q: np.ndarray, kv: np.ndarray, hq: int, hkv: int, window: int = 0,
                     kmask: Optional[np.ndarray] = None, scale: Optional[float] = None,
                     split: bool = True, causal: bool = False, pv_split: bool = False, f8: bool = False) -> np.ndarray:
    """q [B][nq][hq*128] f32, kv [B][nk][2*hkv*128] f32 -> out [B][nq][hq*128] f32 (bf16-rounded).
    split: hi/lo fp16 Q.K; pv_split: hi/lo fp16 P.V too (both = the fully f32-faithful mode); f8 (with both):
    the f8c mode (fp8 correction products); f8 with pv_split and not split: the pv8 mode (fp16 Q.K, f8c P.V)."""
    lib = load_selftest_library()
    q = np.ascontiguousarray(q, dtype=np.float32)
    kv = np.ascontiguousarray(kv, dtype=np.float32)
    B, nq, _ = q.shape
    nk = kv.shape[1]
    km = None if kmask is None else np.ascontiguousarray(kmask, dtype=np.int32)
    out = np.empty_like(q)
    sc = float(scale) if scale is not None else 1.0 / np.sqrt(128.0)
    st = lib.ace_mi_kernel_attention(B, hq, hkv, nq, nk, int(window), sc, (1 if split else 0) | (2 if causal else 0)
                                     | (8 if pv_split else 0) | (16 if f8 else 0), _fptr(q), _fptr(kv),
                                     _iptr(km), _fptr(out))
    if st != ACE_GGML_OK:
        raise RuntimeError(f"ace_mi_kernel_attention failed (status={st})")
    return out


def _bind_attn_probs(lib):
    i32, fp, ip = ctypes.c_int32, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    lib.ace_mi_kernel_attn_probs.argtypes = [i32, i32, i32, i32, i32, ctypes.c_float, fp, fp, ip, i32, ip, fp]
    lib.ace_mi_kernel_attn_probs.restype = ctypes.c_int
    return lib


def kernel_attn_probs(q: np.ndarray, k: np.ndarray, hq: int, hkv: int, heads, kmask: Optional[np.ndarray] = None,
                      scale: Optional[float] = None, out0: Optional[np.ndarray] = None, lib=None) -> np.ndarray:
    """One launch_attn_probs: q [B][nq][hq*128] f32, k [B][nk][hkv*128] f32 (the kernel reads their fp16 roundings),
    kmask [B][nk] int32 or None, heads = the listed query heads -> f32 [len(heads)][B][nq][nk].  out0: the output
    array's contents before the launch (sentinels; default NaN).  The entry fails when the launch wrote outside the
    output.  `lib`: a loaded library that exports the entry (default: the GPU self-test library)."""
    lib = _bind_attn_probs(lib) if lib is not None else load_selftest_library()
    q = np.ascontiguousarray(q, dtype=np.float32)
    k = np.ascontiguousarray(k, dtype=np.float32)
    B, nq, _ = q.shape
    nk = k.shape[1]
    hd = np.ascontiguousarray(heads, dtype=np.int32)
    km = None if kmask is None else np.ascontiguousarray(kmask, dtype=np.int32)
    shape = (len(hd), B, nq, nk)
    out = np.full(shape, np.nan, np.float32) if out0 is None else np.ascontiguousarray(out0, dtype=np.float32).copy()
    assert out.shape == shape, (out.shape, shape)
    sc = float(scale) if scale is not None else 1.0 / np.sqrt(128.0)
    st = lib.ace_mi_kernel_attn_probs(B, hq, hkv, nq, nk, sc, _fptr(q), _fptr(k), _iptr(km), len(hd), _iptr(hd), _fptr(out))
    if st != ACE_GGML_OK:
        raise RuntimeError(f"ace_mi_kernel_attn_probs failed (status={st})")
    return out


def bench_attention(B: int, hq: int, hkv: int, nq: int, nk: int, window: int = 0, split: bool = True,
                    causal: bool = False, masked: bool = False, iters: int = 20, pv_split: bool = False,
                    f8: bool = False) -> float:
    """Average ms per launch of the engine's attention kernel on pseudo-random operands (GPU)."""
    lib = load_selftest_library()
    ms = ctypes.c_float(0.0)
    flags = (1 if split else 0) | (2 if causal else 0) | (4 if masked else 0) | (8 if pv_split else 0) | \
        (16 if f8 else 0)
    st = lib.ace_mi_bench_attention(B, hq, hkv, nq, nk, int(window), flags, iters, ctypes.byref(ms))
    if st != ACE_GGML_OK:
        raise RuntimeError(f"ace_mi_bench_attention failed (status={st})")
    return float(ms.value)


def bench_gemm(M: int, N: int, K: int, variant: int = -1, epi: int = 0, act_type: int = 0, iters: int = 20) -> float:
    """Average ms per launch of the engine GEMM on random operands (GPU)."""
    lib = load_selftest_library()
    ms = ctypes.c_float(0.0)
    st = lib.ace_mi_bench_gemm(act_type, epi, variant, M, N, K, iters, ctypes.byref(ms))
    if st != ACE_GGML_OK:
        raise RuntimeError(f"ace_mi_bench_gemm failed (status={st})")
    return float(ms.value)


_BLOCK = {"q8_0": (32, 34), "q4_k": (256, 144), "q6_k": (256, 210), "q4_0": (32, 18), "q4_1": (32, 20),
          "q5_0": (32, 22), "q5_1": (32, 24), "q2_k": (256, 84), "q3_k": (256, 110), "q5_k": (256, 176),
          "iq4_nl": (32, 18)}


def quantize(x: np.ndarray, qtype: str) -> np.ndarray:
    """The loader's ggml block encoder on host rows: f32 [rows][cols] -> uint8 [rows][nb][block bytes]."""
    lib = load_library()
    x = np.ascontiguousarray(x, dtype=np.float32)
    rows, cols = x.shape
    qk, bb = _BLOCK[qtype]
    out = np.empty((rows, cols // qk, bb), dtype=np.uint8)
    n = lib.ace_mi_quantize(QTYPES[qtype], _fptr(x), rows, cols, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                            out.nbytes)
    if n != out.nbytes:
        raise ValueError(f"ace_mi_quantize failed ({qtype}, cols={cols})")
    return out


def dequantize(raw: np.ndarray, qtype: str) -> np.ndarray:
    lib = load_library()
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    rows, nb, _ = raw.shape
    cols = nb * _BLOCK[qtype][0]
    out = np.empty((rows, cols), dtype=np.float32)
    st = lib.ace_mi_dequantize(QTYPES[qtype], raw.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), rows, cols,
                               _fptr(out))
    if st != ACE_GGML_OK:
        raise ValueError(f"ace_mi_dequantize failed (status={st})")
    return out


def kernel_dequant(w_blocks: np.ndarray, qtype: str) -> np.ndarray:
    """Staged dequant kernel: ggml block bytes [N][nb][bb] -> bf16 words [N][K] of bf16(dequant(W))."""
    lib = load_selftest_library()
    w = np.ascontiguousarray(w_blocks, dtype=np.uint8)
    N, nb = w.shape[0], w.shape[1]
    K = nb * _BLOCK[qtype][0]
    out = np.empty((N, K), dtype=np.uint16)
    st = lib.ace_mi_kernel_dequant(QTYPES[qtype], N, K, w.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                   out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)))
    if st != ACE_GGML_OK:
        raise RuntimeError(f"ace_mi_kernel_dequant failed (status={st})")
    return out


def _bind_dequant_blocks(lib):
    i32 = ctypes.c_int32
    u16p, u8p = ctypes.POINTER(ctypes.c_uint16), ctypes.POINTER(ctypes.c_uint8)
    lib.ace_mi_kernel_dequant_blocks.argtypes = [i32, i32, i32, u8p, u16p]
    lib.ace_mi_kernel_dequant_blocks.restype = ctypes.c_int
    lib.ace_mi_kernel_dequant_segments.argtypes = [i32, ctypes.POINTER(AceMiBlockSeg), i32, i32, u16p]
    lib.ace_mi_kernel_dequant_segments.restype = ctypes.c_int
    return lib


def kernel_dequant_blocks(blocks: np.ndarray, qtype: str, lib=None) -> np.ndarray:
    """The raw-block expansion (launch_dequant_blocks) of one matrix: ggml block bytes [N][nb][bb] of any block type
    -> bf16 words [N][K] of rne_bf16(ggml dequant).  `lib`: a loaded library that exports the entry (default: the GPU
    self-test library)."""
    lib = _bind_dequant_blocks(lib) if lib is not None else load_selftest_library()
    w = np.ascontiguousarray(blocks, dtype=np.uint8)
    N, nb = w.shape[0], w.shape[1]
    K = nb * _BLOCK[qtype][0]
    out = np.empty((N, K), dtype=np.uint16)
    st = lib.ace_mi_kernel_dequant_blocks(GGML_BLOCK_TYPES[qtype], N, K, w.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                          out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)))
    if st != ACE_GGML_OK:
        raise RuntimeError(f"ace_mi_kernel_dequant_blocks failed (status={st})")
    return out


def kernel_dequant_segments(out_bits: np.ndarray, segs, lib=None) -> np.ndarray:
    """launch_dequant_blocks on row segments, one call: out_bits uint16 [rows][K] = the initial content of the
    destination; each segment a dict (qtype, blocks [n][nb][bb], row0, step = 1, group = 1): source row r lands at row
    row0 + (r // group) * group * step + r % group.  Returns the destination after the launches."""
    lib = _bind_dequant_blocks(lib) if lib is not None else load_selftest_library()
    out = np.array(out_bits, dtype=np.uint16, order="C", copy=True)
    keep = []
    arr = (AceMiBlockSeg * len(segs))()
    for i, g in enumerate(segs):
        b = np.ascontiguousarray(g["blocks"], dtype=np.uint8)
        keep.append(b)
        arr[i] = AceMiBlockSeg(type=GGML_BLOCK_TYPES[g["qtype"]], rows=int(b.shape[0]), row0=int(g["row0"]),
                               step=int(g.get("step", 1)), group=int(g.get("group", 1)),
                               blocks=b.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    st = lib.ace_mi_kernel_dequant_segments(len(segs), arr, out.shape[0], out.shape[1],
                                            out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)))
    if st != ACE_GGML_OK:
        raise RuntimeError(f"ace_mi_kernel_dequant_segments failed (status={st})")
    return out


def bench_dequant_blocks(qtype: str, N: int, K: int, iters: int = 20, planes: bool = False) -> float:
    """Average ms of one [N][K] expansion: the raw-block kernel, or (planes) the plane kernel on the same blocks."""
    lib = load_selftest_library()
    ms = ctypes.c_float(0.0)
    st = lib.ace_mi_bench_dequant_blocks(GGML_BLOCK_TYPES[qtype], 1 if planes else 0, N, K, iters, ctypes.byref(ms))
    if st != ACE_GGML_OK:
        raise RuntimeError(f"ace_mi_bench_dequant_blocks failed (status={st})")
    return float(ms.value)


LORA_ROWS_PLAIN, LORA_ROWS_INTERLEAVE = 0, 1


def kernel_lora_merge(base_bits: Optional[np.ndarray], out_bits: np.ndarray, cols: int, jobs, fmt: str = "bf16",
                      lib=None) -> np.ndarray:
    """launch_lora_merge on host arrays, all `jobs` in one launch: base_bits [rows][ld_base] (None = in place) and
    out_bits [rows][ld_out] uint16 words (out_bits = the initial content of the destination); each job a dict
    (row0, rows, A [r][cols] f32 or None, B [rows_mod][r] f32 or None, eff, map, row_off, half, copy_rest).
    Returns the destination after the launch.  `lib`: a loaded library that exports the entry (default: the GPU
    self-test library)."""
    lib = lib or load_selftest_library()
    out = np.array(out_bits, dtype=np.uint16, order="C", copy=True)
    base = None if base_bits is None else np.ascontiguousarray(base_bits, dtype=np.uint16)
    keep = []
    arr = (AceMiLoraJob * len(jobs))()
    for i, j in enumerate(jobs):
        A = None if j.get("A") is None else np.ascontiguousarray(j["A"], dtype=np.float32)
        B = None if j.get("B") is None else np.ascontiguousarray(j["B"], dtype=np.float32)
        keep += [A, B]
        arr[i] = AceMiLoraJob(row0=int(j["row0"]), rows=int(j["rows"]), r=0 if A is None else int(A.shape[0]),
                              rows_mod=0 if B is None else int(B.shape[0]), A=_fptr(A), B=_fptr(B),
                              eff=float(j.get("eff", 0.0)), map=int(j.get("map", 0)), row_off=int(j.get("row_off", 0)),
                              half=int(j.get("half", 0)), copy_rest=1 if j.get("copy_rest") else 0)
    u16p = ctypes.POINTER(ctypes.c_uint16)
    st = lib.ace_mi_kernel_lora_merge({"bf16": 0, "fp16": 1}[fmt], out.shape[0], int(cols),
                                      0 if base is None else base.shape[1], out.shape[1],
                                      None if base is None else base.ctypes.data_as(u16p), out.ctypes.data_as(u16p),
                                      arr, len(jobs))
    if st != ACE_GGML_OK:
        raise RuntimeError(f"ace_mi_kernel_lora_merge failed (status={st})")
    return out


LM_EPI_STORE, LM_EPI_RESID, LM_EPI_SWIGLU = 0, 1, 2


def _bind_lm_kernels(lib):
    i32, f32 = ctypes.c_int32, ctypes.c_float
    fp, ip, u16p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint16)
    lib.ace_mi_kernel_lm_skinny.argtypes = [i32] * 7 + [u16p, u16p, fp, u16p]
    lib.ace_mi_kernel_lm_embed.argtypes = [i32] * 4 + [u16p, ip, fp]
    lib.ace_mi_kernel_lm_qkv_post.argtypes = [i32] * 6 + [f32, fp, fp, fp, fp, fp, ip, fp, u16p, u16p, ip]
    lib.ace_mi_kernel_lm_prefill_kv.argtypes = [i32] * 6 + [f32, fp, fp, fp, fp, ip, u16p, u16p, ip]
    lib.ace_mi_kernel_lm_attention.argtypes = [i32] * 6 + [f32, fp, u16p, u16p, ip, u16p]
    u8p = ctypes.POINTER(ctypes.c_uint8)
    lib.ace_mi_kernel_lm_skinny_q.argtypes = [i32] * 8 + [u16p, u8p, fp, u16p, ip]
    lib.ace_mi_kernel_lm_embed_q.argtypes = [i32] * 4 + [u8p, ip, fp]
    lib.ace_mi_kernel_lm_select.argtypes = [ctypes.POINTER(AceMiKernelLmSelectArgs)]
    lib.ace_mi_kernel_lm_cache_fanout.argtypes = [i32] * 7 + [u16p, u16p, ip, u16p, u16p, ip]
    for name in ("skinny", "embed", "qkv_post", "prefill_kv", "attention", "skinny_q", "embed_q", "select",
                 "cache_fanout"):
        getattr(lib, "ace_mi_kernel_lm_" + name).restype = ctypes.c_int
    return lib


def _u16ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16))


def _lm_lib(lib):
    """`lib`: a loaded library that exports the ace_mi_kernel_lm_* entries (default: the GPU self-test library)."""
    return _bind_lm_kernels(lib) if lib is not None else load_selftest_library()


def _lm_status(name: str, st: int):
    if st != ACE_GGML_OK:
        raise RuntimeError(f"ace_mi_kernel_lm_{name} failed (status={st})")


def kernel_lm_skinny(x_bits: np.ndarray, w_bits: np.ndarray, y0: np.ndarray, epi: int = 0, act_type: int = 0,
                     lib=None) -> np.ndarray:
    """launch_lm_skinny on host arrays: x_bits [B][ldx] and w_bits [N][K] 16-bit words of act_type (0 bf16, 1 fp16);
    y0 [B][ldy] = the initial content of the destination, float32 for epi 0 (store) / 1 (add), uint16 for epi 2
    (SwiGLU on gate|up interleaved rows, N / 2 columns).  Returns the destination after the launch, padding included."""
    lib = _lm_lib(lib)
    x = np.ascontiguousarray(x_bits, dtype=np.uint16)
    w = np.ascontiguousarray(w_bits, dtype=np.uint16)
    y = np.array(y0, dtype=np.uint16 if epi == LM_EPI_SWIGLU else np.float32, order="C", copy=True)
    st = lib.ace_mi_kernel_lm_skinny(act_type, epi, x.shape[0], w.shape[0], w.shape[1], x.shape[1], y.shape[1],
                                     _u16ptr(x), _u16ptr(w), None if epi == LM_EPI_SWIGLU else _fptr(y),
                                     _u16ptr(y) if epi == LM_EPI_SWIGLU else None)
    _lm_status("skinny", st)
    return y


def kernel_lm_embed(table_bits: np.ndarray, ids: np.ndarray, fmt: int = 0, lib=None) -> np.ndarray:
    """launch_lm_embed: table_bits [vocab][H] 16-bit words of fmt (0 bf16, 1 fp16), ids [n] int32 -> f32 [n][H]."""
    lib = _lm_lib(lib)
    t = np.ascontiguousarray(table_bits, dtype=np.uint16)
    i = np.ascontiguousarray(ids, dtype=np.int32)
    out = np.full((i.shape[0], t.shape[1]), np.nan, dtype=np.float32)
    _lm_status("embed", lib.ace_mi_kernel_lm_embed(fmt, i.shape[0], t.shape[0], t.shape[1], _u16ptr(t), _iptr(i),
                                                   _fptr(out)))
    return out


def _block_rows(blocks: np.ndarray, qtype: str):
    """uint8 [rows][nb][block bytes] -> (contiguous array, rows, K)"""
    b = np.ascontiguousarray(blocks, dtype=np.uint8)
    qk, bb = _BLOCK[qtype]
    if b.ndim != 3 or b.shape[2] != bb:
        raise ValueError(f"{qtype} blocks must be [rows][nb][{bb}]")
    return b, b.shape[0], b.shape[1] * qk


def kernel_lm_skinny_q(x_bits: np.ndarray, blocks: np.ndarray, qtype: str, y0: np.ndarray, epi: int = 0, n_rows=None,
                       lib=None, with_chain: bool = False):
    """launch_lm_skinny_q on host arrays: x_bits [B][ldx] bf16 words, blocks uint8 [rows][K / block][block bytes] ggml
    blocks of qtype ("q8_0", "q4_k", "q6_k"), re-laid out into the loader's planes by the entry; n_rows (default: all)
    is the N of the product, rows past it are uploaded but must not be read.  y0 as kernel_lm_skinny.  Returns the
    destination after the launch, padding included (with_chain: and the kernel's longest f32 addition chain)."""
    lib = _lm_lib(lib)
    x = np.ascontiguousarray(x_bits, dtype=np.uint16)
    b, rows, K = _block_rows(blocks, qtype)
    N = rows if n_rows is None else int(n_rows)
    y = np.array(y0, dtype=np.uint16 if epi == LM_EPI_SWIGLU else np.float32, order="C", copy=True)
    chain = ctypes.c_int32(0)
    st = lib.ace_mi_kernel_lm_skinny_q(QTYPES[qtype], epi, x.shape[0], N, rows, K, x.shape[1], y.shape[1], _u16ptr(x),
                                       b.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                       None if epi == LM_EPI_SWIGLU else _fptr(y),
                                       _u16ptr(y) if epi == LM_EPI_SWIGLU else None, ctypes.byref(chain))
    _lm_status("skinny_q", st)
    return (y, int(chain.value)) if with_chain else y


def kernel_lm_embed_q(blocks: np.ndarray, qtype: str, ids: np.ndarray, lib=None) -> np.ndarray:
    """launch_lm_embed_q: blocks uint8 [vocab][H / block][block bytes] of qtype, ids [n] int32 -> f32 [n][H]."""
    lib = _lm_lib(lib)
    b, vocab, H = _block_rows(blocks, qtype)
    i = np.ascontiguousarray(ids, dtype=np.int32)
    out = np.full((i.shape[0], H), np.nan, dtype=np.float32)
    _lm_status("embed_q", lib.ace_mi_kernel_lm_embed_q(QTYPES[qtype], i.shape[0], vocab, H,
                                                       b.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), _iptr(i),
                                                       _fptr(out)))
    return out


def kernel_lm_cache_fanout(k_src: np.ndarray, v_src: np.ndarray, mask_src: np.ndarray, k_dst: np.ndarray,
                           v_dst: np.ndarray, mask_dst: np.ndarray, n: int, lib=None):
    """launch_lm_cache_fanout on host arrays: sources [layers][G][hkv][cap_src][128] uint16 with mask [G][cap_src] int32,
    destinations [layers][G * S][hkv][cap_dst][128] with mask [G * S][cap_dst] (their contents before the launch are
    uploaded).  Returns copies of all six arrays after the launch, in the order given."""
    lib = _lm_lib(lib)
    ks, vs, kd, vd = (np.array(a, dtype=np.uint16, order="C") for a in (k_src, v_src, k_dst, v_dst))
    ms, md = (np.array(a, dtype=np.int32, order="C") for a in (mask_src, mask_dst))
    layers, G, hkv, cap_src = ks.shape[:4]
    GS, cap_dst = kd.shape[1], kd.shape[3]
    if (vs.shape != ks.shape or vd.shape != kd.shape or ks.shape[4] != 128 or kd.shape[4] != 128 or GS % G or
            kd.shape[0] != layers or kd.shape[2] != hkv or ms.shape != (G, cap_src) or md.shape != (GS, cap_dst)):
        raise ValueError("kernel_lm_cache_fanout: inconsistent shapes")
    st = lib.ace_mi_kernel_lm_cache_fanout(layers, G, GS // G, hkv, cap_src, cap_dst, int(n), _u16ptr(ks), _u16ptr(vs),
                                           _iptr(ms), _u16ptr(kd), _u16ptr(vd), _iptr(md))
    _lm_status("cache_fanout", st)
    return ks, vs, ms, kd, vd, md


def kernel_lm_qkv_post(qkv: np.ndarray, hq: int, hkv: int, pos: int, eps: float, q_norm, k_norm, rope_cos, rope_sin,
                       mask_new, k_cache: np.ndarray, v_cache: np.ndarray, key_mask: np.ndarray, lib=None):
    """launch_lm_qkv_post: qkv [B][ld] f32, norms [128], rope tables [capacity][64], mask_new [B] int32 or None; the
    caches [B][hkv][capacity][128] uint16 and key_mask [B][capacity] int32 hold the initial content.  Returns
    (q_out [B][hq][128] f32, k_cache, v_cache, key_mask) after the launch."""
    lib = _lm_lib(lib)
    x = np.ascontiguousarray(qkv, dtype=np.float32)
    qn, kn = (np.ascontiguousarray(a, dtype=np.float32) for a in (q_norm, k_norm))
    cs, sn = (np.ascontiguousarray(a, dtype=np.float32) for a in (rope_cos, rope_sin))
    mn = None if mask_new is None else np.ascontiguousarray(mask_new, dtype=np.int32)
    kc, vc = (np.array(a, dtype=np.uint16, order="C", copy=True) for a in (k_cache, v_cache))
    km = np.array(key_mask, dtype=np.int32, order="C", copy=True)
    B, cap = km.shape
    q = np.full((B, hq, 128), np.nan, dtype=np.float32)
    st = lib.ace_mi_kernel_lm_qkv_post(B, hq, hkv, cap, pos, x.shape[1], eps, _fptr(x), _fptr(qn), _fptr(kn), _fptr(cs),
                                       _fptr(sn), _iptr(mn), _fptr(q), _u16ptr(kc), _u16ptr(vc), _iptr(km))
    _lm_status("qkv_post", st)
    return q, kc, vc, km


def kernel_lm_prefill_kv(qkv: np.ndarray, n: int, hq: int, hkv: int, eps: float, k_norm, rope_cos, rope_sin, mask,
                         k_cache: np.ndarray, v_cache: np.ndarray, key_mask: np.ndarray, lib=None):
    """launch_lm_prefill_kv: qkv [B * n][ld] f32 (rows b * n + t), mask [B][n] int32 or None; caches and key_mask as
    kernel_lm_qkv_post.  Returns (qkv, k_cache, v_cache, key_mask) after the launch."""
    lib = _lm_lib(lib)
    x = np.array(qkv, dtype=np.float32, order="C", copy=True)
    kn = np.ascontiguousarray(k_norm, dtype=np.float32)
    cs, sn = (np.ascontiguousarray(a, dtype=np.float32) for a in (rope_cos, rope_sin))
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.int32)
    kc, vc = (np.array(a, dtype=np.uint16, order="C", copy=True) for a in (k_cache, v_cache))
    km = np.array(key_mask, dtype=np.int32, order="C", copy=True)
    B, cap = km.shape
    st = lib.ace_mi_kernel_lm_prefill_kv(B, hq, hkv, cap, n, x.shape[1], eps, _fptr(x), _fptr(kn), _fptr(cs), _fptr(sn),
                                         _iptr(m), _u16ptr(kc), _u16ptr(vc), _iptr(km))
    _lm_status("prefill_kv", st)
    return x, kc, vc, km


def kernel_lm_attention(q: np.ndarray, k_cache: np.ndarray, v_cache: np.ndarray, key_mask: np.ndarray, nk: int,
                        scale: float, out_type: int = 0, lib=None) -> np.ndarray:
    """launch_lm_attention over keys 0 .. nk-1: q [B][hq][128] f32, caches [B][hkv][capacity][128] uint16 (fp16 words),
    key_mask [B][capacity] int32 -> uint16 [B][hq][128] words of out_type (0 bf16, 1 fp16)."""
    lib = _lm_lib(lib)
    qq = np.ascontiguousarray(q, dtype=np.float32)
    kc, vc = (np.ascontiguousarray(a, dtype=np.uint16) for a in (k_cache, v_cache))
    km = np.ascontiguousarray(key_mask, dtype=np.int32)
    B, hq = qq.shape[0], qq.shape[1]
    out = np.full((B, hq, 128), 0x7fff, dtype=np.uint16)
    st = lib.ace_mi_kernel_lm_attention(out_type, B, hq, kc.shape[1], kc.shape[2], nk, scale, _fptr(qq), _u16ptr(kc),
                                        _u16ptr(vc), _iptr(km), _u16ptr(out))
    _lm_status("attention", st)
    return out


def kernel_lm_select(logits: np.ndarray, cfg_scale=1.0, pre_temperature=0.0, repetition_penalty=1.0, top_k=0, top_p=1.0,
                     temperature=1.0, allowed=None, stop_id=-1, block_stop=False, force_stop=False, n_emitted=0,
                     uniform=None, seen=None, tokens0=None, token_stride=1, next_ids0=None, done0=None, processed0=None,
                     vocab=None, lib=None) -> dict:
    """launch_lm_select on host arrays: logits [B][ld] f32 whose first `vocab` columns count (default: all).  seen
    [S][ld_seen] uint8, tokens0 [S * token_stride] int32, next_ids0 [B], done0 [1 + S] and processed0 [S][ld_processed]
    give the initial content of the in-out buffers (None = not passed, but for tokens0).  Returns a dict of the buffers
    after the launch: tokens, seen, next_ids, done, processed, chains."""
    lib = _lm_lib(lib)
    x = np.ascontiguousarray(logits, dtype=np.float32)
    B, ld = x.shape
    vocab = ld if vocab is None else int(vocab)
    S = B // 2 if cfg_scale > 1.0 else B
    al = None if allowed is None else np.ascontiguousarray(allowed, dtype=np.int32)
    u = None if uniform is None else np.ascontiguousarray(uniform, dtype=np.float32)
    tok = (np.full((max(S, 1) * token_stride,), -7, np.int32) if tokens0 is None
           else np.array(tokens0, dtype=np.int32, order="C", copy=True))
    sn = None if seen is None else np.array(seen, dtype=np.uint8, order="C", copy=True)
    nx = None if next_ids0 is None else np.array(next_ids0, dtype=np.int32, order="C", copy=True)
    dn = None if done0 is None else np.array(done0, dtype=np.int32, order="C", copy=True)
    pr = None if processed0 is None else np.array(processed0, dtype=np.float32, order="C", copy=True)
    chains = np.zeros(3, np.int32)

    def ptr(a):
        return None if a is None else a.ctypes.data

    g = AceMiKernelLmSelectArgs(
        B=B, vocab=vocab, ld_logits=ld, cfg_scale=cfg_scale, pre_temperature=pre_temperature,
        repetition_penalty=repetition_penalty, top_k=int(top_k), top_p=top_p, temperature=temperature,
        n_allowed=0 if al is None else int(al.shape[0]), stop_id=int(stop_id), block_stop=int(bool(block_stop)),
        force_stop=int(bool(force_stop)), n_emitted=int(n_emitted), ld_seen=0 if sn is None else sn.shape[1],
        token_stride=int(token_stride), ld_processed=0 if pr is None else pr.shape[1], logits=ptr(x), allowed=ptr(al),
        uniform=ptr(u), seen=ptr(sn), tokens=ptr(tok), next_ids=ptr(nx), done=ptr(dn), processed=ptr(pr),
        chains=ptr(chains))
    _lm_status("select", lib.ace_mi_kernel_lm_select(ctypes.byref(g)))
    return {"tokens": tok, "seen": sn, "next_ids": nx, "done": dn, "processed": pr, "chains": chains}


def _bind_vae_kernels(lib):
    i32, fp, u16p = ctypes.c_int32, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint16)
    lib.ace_mi_kernel_conv_gemm.argtypes = [ctypes.POINTER(AceMiConvGemmArgs)]
    lib.ace_mi_kernel_conv_out.argtypes = [u16p, i32, i32, u16p, i32, fp, i32]
    lib.ace_mi_kernel_pack_f16.argtypes = [fp, ctypes.c_int64, i32, i32, u16p]
    for name in ("conv_gemm", "conv_out", "pack_f16"):
        getattr(lib, "ace_mi_kernel_" + name).restype = ctypes.c_int
    return lib


def _vae_lib(lib):
    """`lib`: a loaded library that exports the VAE kernel entries (default: the GPU self-test library)."""
    return _bind_vae_kernels(lib) if lib is not None else load_selftest_library()


def kernel_conv_gemm(S_bits: np.ndarray, W_bits: np.ndarray, *, M: int, Cout: int, T_out: int, taps: int = 1, dil: int = 1,
                     pad: int = 0, in_stride: int = 1, up: int = 1, crop: int = 0, bias=None, snake=None, W2_bits=None,
                     bias2=None, snake2=None, X0=None, S_out0=None, resid: bool = False, store_x: bool = False,
                     guard: int = 0, halo: bool = True, lib=None):
    """One launch_conv_gemm (ConvGemmArgs of csrc/kernels.h) on host arrays: S_bits [items][T_in][Cin] and W_bits
    [N][taps * Cin] fp16 words; bias [N] ([Cout] for up > 1), snake / snake2 = (ea, eb) f32 pairs, W2_bits [Cout][Cout],
    bias2 [Cout]; X0 (float32) and S_out0 (uint16), either may be None, are flat arrays of guard + items * T_out * Cout +
    guard elements holding the initial content.  halo=False runs with ACE_MI_VAE_HALO=0 (the generic staging for the
    residual units' k7 convs); the variable is restored afterwards.  Returns (X, S_out) after the launch, guards
    included (None where none was given).  Raises RuntimeError with the status on a refused call; the exception carries
    the two arrays as the entry left them (.X, .S_out)."""
    lib = _vae_lib(lib)
    S = np.ascontiguousarray(S_bits, dtype=np.uint16)
    W = np.ascontiguousarray(W_bits, dtype=np.uint16)
    if S.ndim != 3 or W.ndim != 2:
        raise ValueError("S_bits must be [items][T_in][Cin], W_bits [N][taps * Cin]")
    items, T_in, Cin = S.shape
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
    b, b2 = f32(bias), f32(bias2)
    ea, eb = (None, None) if snake is None else (f32(snake[0]), f32(snake[1]))
    ea2, eb2 = (None, None) if snake2 is None else (f32(snake2[0]), f32(snake2[1]))
    W2 = None if W2_bits is None else np.ascontiguousarray(W2_bits, dtype=np.uint16)
    X = None if X0 is None else np.array(X0, dtype=np.float32, order="C", copy=True)
    So = None if S_out0 is None else np.array(S_out0, dtype=np.uint16, order="C", copy=True)
    n = 2 * guard + items * T_out * Cout
    for a in (X, So):
        if a is not None and a.size != n:
            raise ValueError(f"X0 / S_out0 must hold guard + items * T_out * Cout + guard = {n} elements")
    ptr = lambda a: None if a is None else a.ctypes.data
    g = AceMiConvGemmArgs(T_in=T_in, Cin=Cin, taps=taps, dil=dil, pad=pad, in_stride=in_stride, M=M, N=W.shape[0],
                          Cout=Cout, up=up, crop=crop, T_out=T_out, resid=int(bool(resid)), store_x=int(bool(store_x)),
                          items=items, guard=guard, S=ptr(S), W=ptr(W), bias=ptr(b), snake_ea=ptr(ea), snake_eb=ptr(eb),
                          W2=ptr(W2), bias2=ptr(b2), snake2_ea=ptr(ea2), snake2_eb=ptr(eb2), X=ptr(X), S_out=ptr(So))
    old = os.environ.get("ACE_MI_VAE_HALO")
    if halo:
        os.environ.pop("ACE_MI_VAE_HALO", None)
    else:
        os.environ["ACE_MI_VAE_HALO"] = "0"
    try:
        st = lib.ace_mi_kernel_conv_gemm(ctypes.byref(g))
    finally:
        if old is None:
            os.environ.pop("ACE_MI_VAE_HALO", None)
        else:
            os.environ["ACE_MI_VAE_HALO"] = old
    if st != ACE_GGML_OK:
        err = RuntimeError(f"ace_mi_kernel_conv_gemm failed (status={st})")
        err.X, err.S_out = X, So          # the arrays the entry was given, for a caller that checks they are untouched
        raise err
    return X, So


def kernel_conv_out(S_bits: np.ndarray, W_bits: np.ndarray, out0: np.ndarray, guard: int = 0, lib=None) -> np.ndarray:
    """launch_conv_out (decoder.conv2) on host arrays: S_bits [items][T][128] and W_bits [out_ch][7][128] fp16 words, out0
    a flat float32 array of guard + items * T * out_ch + guard elements (the initial content).  Returns it after the launch."""
    lib = _vae_lib(lib)
    S = np.ascontiguousarray(S_bits, dtype=np.uint16)
    W = np.ascontiguousarray(W_bits, dtype=np.uint16)
    if S.ndim != 3 or S.shape[2] != 128 or W.ndim != 3 or W.shape[1:] != (7, 128):
        raise ValueError("S_bits must be [items][T][128], W_bits [out_ch][7][128]")
    out = np.array(out0, dtype=np.float32, order="C", copy=True)
    if out.size != 2 * guard + S.shape[0] * S.shape[1] * W.shape[0]:
        raise ValueError("out0 must hold guard + items * T * out_ch + guard elements")
    st = lib.ace_mi_kernel_conv_out(_u16ptr(S), S.shape[1], S.shape[0], _u16ptr(W), W.shape[0], _fptr(out), guard)
    if st != ACE_GGML_OK:
        raise RuntimeError(f"ace_mi_kernel_conv_out failed (status={st})")
    return out


def kernel_pack_f16(x: np.ndarray, Cpad: int, lib=None) -> np.ndarray:
    """x [rows][C] f32 -> fp16 words [rows][Cpad], columns >= C zero: pack_f16_kernel, or to_f16_kernel when Cpad == C.
    The destination starts as 0x7FFF words."""
    lib = _vae_lib(lib)
    xx = np.ascontiguousarray(x, dtype=np.float32)
    y = np.full((xx.shape[0], Cpad), 0x7FFF, np.uint16)
    st = lib.ace_mi_kernel_pack_f16(_fptr(xx), xx.shape[0], xx.shape[1], Cpad, _u16ptr(y))
    if st != ACE_GGML_OK:
        raise RuntimeError(f"ace_mi_kernel_pack_f16 failed (status={st})")
    return y


def kernel_gemm_q(a_bits: np.ndarray, w_blocks: np.ndarray, qtype: str, epi: int = 0, variant: int = -1,
                  bias: Optional[np.ndarray] = None, x: Optional[np.ndarray] = None) -> np.ndarray:
    """Dequant-fused GEMM: a_bits bf16 words [M][K], w_blocks ggml block bytes [N][nb][bb].  epi 2 / 3: returns
    x + acc (* bias as the per-column gate for 2)."""
    lib = load_selftest_library()
    a = np.ascontiguousarray(a_bits, dtype=np.uint16)
    w = np.ascontiguousarray(w_blocks, dtype=np.uint8)
    M, K = a.shape
    N = w.shape[0]
    u16p = ctypes.POINTER(ctypes.c_uint16)
    u8p = ctypes.POINTER(ctypes.c_uint8)
    b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
    if epi in (0, 2, 3):
        out = np.ascontiguousarray(x, dtype=np.float32).copy() if epi in (2, 3) else np.empty((M, N), np.float32)
        st = lib.ace_mi_kernel_gemm_q(QTYPES[qtype], epi, variant, M, N, K, a.ctypes.data_as(u16p),
                                      w.ctypes.data_as(u8p), _fptr(b), _fptr(out), None)
    else:
        out = np.empty((M, N // 2), dtype=np.uint16)
        st = lib.ace_mi_kernel_gemm_q(QTYPES[qtype], epi, variant, M, N, K, a.ctypes.data_as(u16p),
                                      w.ctypes.data_as(u8p), _fptr(b), None, out.ctypes.data_as(u16p))
    if st != ACE_GGML_OK:
        raise RuntimeError(f"ace_mi_kernel_gemm_q failed (status={st})")
    return out


def kernel_gemm_a8(x: np.ndarray, w_blocks: np.ndarray, qtype: str, epi: int = 0, bias: Optional[np.ndarray] = None,
                   x0: Optional[np.ndarray] = None):
    """ggml-faithful quantized-activation GEMM (ACE_MI_QUANT_ACT=q8): x f32 [M][K] quantized on the device, then the
    integer-dot GEMM against ggml block rows w_blocks [N][nb][bb].  epi 0: acc (+ bias); 3: x0 + (acc + bias);
    7: silu(g) * u.  Returns (out, q int8 [M][K], s f32 [K/32][M], bsum f32 [K/32][M])."""
    lib = load_selftest_library()
    xa = np.ascontiguousarray(x, dtype=np.float32)
    w = np.ascontiguousarray(w_blocks, dtype=np.uint8)
    M, K = xa.shape
    N = w.shape[0]
    ncol = N // 2 if epi == 7 else N
    out = np.ascontiguousarray(x0, dtype=np.float32).copy() if epi == 3 else np.empty((M, ncol), np.float32)
    q = np.empty((M, K), np.int8)
    s = np.empty((K // 32, M), np.float32)
    bs = np.empty((K // 32, M), np.float32)
    b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
    st = lib.ace_mi_kernel_gemm_a8(QTYPES[qtype], epi, M, N, K, _fptr(xa), w.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                   _fptr(b), _fptr(out), q.ctypes.data_as(ctypes.POINTER(ctypes.c_int8)), _fptr(s),
                                   _fptr(bs))
    if st != ACE_GGML_OK:
        raise RuntimeError(f"ace_mi_kernel_gemm_a8 failed (status={st})")
    return out, q, s, bs


def bench_gemm_q(M: int, N: int, K: int, qtype: str, variant: int = -1, epi: int = 0, iters: int = 20) -> float:
    lib = load_selftest_library()
    ms = ctypes.c_float(0.0)
    st = lib.ace_mi_bench_gemm_q(QTYPES[qtype], epi, variant, M, N, K, iters, ctypes.byref(ms))
    if st != ACE_GGML_OK:
        raise RuntimeError(f"ace_mi_bench_gemm_q failed (status={st})")
    return float(ms.value)


def reference_noise(seed: int, n: int) -> np.ndarray:
    """x_T of the reference generator (std::mt19937 + std::normal_distribution<float>), host code."""
    out = np.empty(int(n), np.float32)
    if load_library().ace_mi_reference_noise(int(seed), int(n), _fptr(out)) != ACE_GGML_OK:
        raise RuntimeError("ace_mi_reference_noise failed")
    return out


def gemm_variant(variant: int) -> None:
    lib = load_library()
    if lib.ace_mi_gemm_variant(int(variant)) != ACE_GGML_OK:
        raise ValueError(variant)


WFMT = {"bf16": 0, "f16": 1, "q8_0": 2, "q4_k": 3, "q6_k": 4}  # WeightFormat of csrc/kernels.h
GEMM_FAMILIES = ("none", "gemm_kernel", "gemm8_kernel", "gemm_ws_kernel", "gemm_q_kernel", "gemm_qr_kernel",
                 "gemm_wsq_kernel")


def gemm_resolve(M: int, N: int, K: int, wfmt: str = "bf16", prep: bool = False, forced: int = -1, override: int = -1,
                 lib=None) -> int:
    """The variant launch_gemm would launch (csrc/gemm_variants.h): pure, no device.  `lib`: a loaded library that
    exports the entry, bound or not (default: the GPU self-test library)."""
    lib = _bind_gemm_variants(lib) if lib is not None else load_selftest_library()
    v = ctypes.c_int32(-1)
    st = lib.ace_mi_gemm_resolve(int(forced), int(override), int(M), int(N), int(K), WFMT[wfmt], int(bool(prep)), ctypes.byref(v))
    if st != ACE_GGML_OK:
        raise ValueError((M, N, K, wfmt))
    return v.value


def gemm_variant_row(vid: int, lib=None) -> Optional[dict]:
    """The row of base id `vid` in the variant table, or None: {"name", "dense", "quant" (family name, BM, BN, WM, WN,
    depth), "dense_split", "quant_split", "prep_sibling", "needs_n256"}."""
    lib = _bind_gemm_variants(lib) if lib is not None else load_selftest_library()
    f = (ctypes.c_int32 * 16)()
    name = ctypes.create_string_buffer(160)
    if lib.ace_mi_gemm_variant_row(int(vid), f, name, len(name)) != ACE_GGML_OK:
        return None
    kern = lambda k: (GEMM_FAMILIES[k[0]],) + tuple(k[1:])
    return {"name": name.value.decode(), "dense": kern(f[0:6]), "quant": kern(f[6:12]), "dense_split": f[12],
            "quant_split": f[13], "prep_sibling": f[14], "needs_n256": bool(f[15])}


def gemm_variant_arg_ok(variant: int, allow_unchecked: bool = False, lib=None) -> bool:
    lib = _bind_gemm_variants(lib) if lib is not None else load_selftest_library()
    return lib.ace_mi_gemm_variant_arg_ok(int(variant), int(allow_unchecked)) == ACE_GGML_OK


def rope_table(n: int, head_dim: int, theta: float, lib=None):
    """(cos, sin), each [n][head_dim / 2] float32: the RoPE table the engines build (csrc/runtime/devmem.h).  `lib`: a
    loaded library that exports the entry, bound or not (default: the GPU self-test library)."""
    lib = _bind_rope_table(lib) if lib is not None else load_selftest_library()
    cs, sn = (np.empty((n, head_dim // 2), np.float32) for _ in range(2))
    if lib.ace_mi_rope_table(int(n), int(head_dim), float(theta), _fptr(cs), _fptr(sn)) != ACE_GGML_OK:
        raise ValueError((n, head_dim, theta))
    return cs, sn


def rope_table_steps(steps, lib=None):
    """One table through ensure(n, head_dim, theta) for each triple of `steps`: (rows held after each call, cos, sin of
    the final table, each [rows[-1]][head_dim / 2] float32)."""
    lib = _bind_rope_table(lib) if lib is not None else load_selftest_library()
    n = np.array([s[0] for s in steps], np.int32)
    hd = np.array([s[1] for s in steps], np.int32)
    th = np.array([s[2] for s in steps], np.float32)
    rows = np.zeros(len(steps), np.int32)
    cs, sn = (np.empty((int(n.max()), int(hd[-1]) // 2), np.float32) for _ in range(2))
    if lib.ace_mi_rope_table_steps(len(steps), _iptr(n), _iptr(hd), _fptr(th), _iptr(rows), _fptr(cs), _fptr(sn)) != ACE_GGML_OK:
        raise ValueError(steps)
    return rows.tolist(), cs[:rows[-1]], sn[:rows[-1]]


def kernel_attn_kh(mode: int) -> None:
    """f8c attention kernel of this process: -1 environment / default policy, 0 attn2 (one wave per SIMD), 1 attn_kh."""
    if load_selftest_library().ace_mi_kernel_attn_kh(int(mode)) != ACE_GGML_OK:
        raise ValueError(mode)


ATTN_SHAPE_FIELDS = ("B", "Hq", "Hkv", "nq", "nk", "window", "causal", "has_part", "split", "pv_split", "f8", "out_f32")
ATTN_POLICY_FIELDS = ("ksplit_mode", "tail", "tail_min", "xcd_order", "kh", "n_cu")
ATTN_POLICY_DEFAULT = dict(ksplit_mode=0, tail=1, tail_min=16, xcd_order=1, kh=-1, n_cu=256)
ATTN_PLAN_FIELDS = ("ksplit", "split_from", "xcd_order", "n_blk", "grid", "kernel", "merge", "merge_grid")
ATTN_KERNELS = ("attn2", "attn_kh")
ATTN_MERGES = ("none", "uniform2", "uniform4", "tail")


def _attn_policy_words(policy: dict, unset: int):
    bad = set(policy) - set(ATTN_POLICY_FIELDS)
    if bad:
        raise ValueError(f"unknown attention policy fields {sorted(bad)}")
    return (ctypes.c_int32 * 6)(*[int(policy.get(n, unset if unset is not None else ATTN_POLICY_DEFAULT[n]))
                                  for n in ATTN_POLICY_FIELDS])


def kernel_attn_policy(**policy) -> None:
    """Override the attention launch policy of this process (csrc/attn_plan.h): ksplit_mode, tail, tail_min,
    xcd_order, kh, n_cu; a field left out (or -1) stays with the environment / the device, no field clears the
    override."""
    if load_selftest_library().ace_mi_kernel_attn_policy(_attn_policy_words(policy, -1)) != ACE_GGML_OK:
        raise ValueError(policy)


def attn_plan(shape, lib=None, **policy) -> dict:
    """The launch plan of an attention shape (ATTN_SHAPE_FIELDS, a dict or a sequence) under a policy (fields left out:
    ATTN_POLICY_DEFAULT, i.e. the defaults on a 256-CU device): pure, no device.  `lib` as for gemm_resolve."""
    lib = _bind_attn_plan(lib) if lib is not None else load_selftest_library()
    if isinstance(shape, dict):
        shape = [shape[n] for n in ATTN_SHAPE_FIELDS]
    out = (ctypes.c_int32 * 8)()
    if lib.ace_mi_attn_plan((ctypes.c_int32 * 12)(*[int(v) for v in shape]), _attn_policy_words(policy, None),
                            out) != ACE_GGML_OK:
        raise ValueError((list(shape), policy))
    plan = dict(zip(ATTN_PLAN_FIELDS, out))
    plan["kernel"], plan["merge"] = ATTN_KERNELS[plan["kernel"]], ATTN_MERGES[plan["merge"]]
    return plan


def attn_plan_block(ksplit: int, split_from: int, xcd_order: int, n_blk: int, x: int, lib=None):
    """Launch index x of a plan -> (logical block, key-range part, parts of the block, valid)."""
    lib = _bind_attn_plan(lib) if lib is not None else load_selftest_library()
    out = (ctypes.c_int32 * 4)()
    if lib.ace_mi_attn_plan_block(ksplit, split_from, xcd_order, n_blk, x, out) != ACE_GGML_OK:
        raise ValueError((ksplit, split_from, xcd_order, n_blk, x))
    return out[0], out[1], out[2], bool(out[3])


def attn_plan_tiles(nk: int, window: int, causal: bool, q0: int, qpb: int, part: int, parts: int, lib=None):
    """(first key tile, key tiles) of part `part` of `parts` for the queries [q0, q0 + qpb)."""
    lib = _bind_attn_plan(lib) if lib is not None else load_selftest_library()
    out = (ctypes.c_int32 * 2)()
    if lib.ace_mi_attn_plan_tiles(nk, window, int(bool(causal)), q0, qpb, part, parts, out) != ACE_GGML_OK:
        raise ValueError((nk, window, causal, q0, qpb, part, parts))
    return out[0], out[1]


def kernel_gemm_a8_mode(mode: int) -> None:
    """Q8_0 GEMM form of the q8 mode in this process: -1 environment / default (bf16 MFMA), 0 i8 MFMA, 1 bf16 MFMA."""
    if load_selftest_library().ace_mi_kernel_gemm_a8_mode(int(mode)) != ACE_GGML_OK:
        raise ValueError(mode)
