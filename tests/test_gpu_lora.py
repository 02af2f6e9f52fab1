"""PEFT LoRA adapters on the MI355X: the merge kernel (kernels/lora.hip) against numpy bit for bit through
ace_mi_kernel_lora_merge, and the engine's HIP path against merged checkpoints (helpers and the numpy restatement
of the kernel are those of tests/test_lora_cpu.py)."""
import numpy as np
import pytest

from test_lora_cpu import (adapter, base_ckpt, bridge, forward_pair, fwd, inputs, merge_cases, numpy_merge,
                           quantized_pair_errors, rel, target_sets)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ kernel
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("r", [1, 13, 64, 128])
@pytest.mark.parametrize("rows,cols", [(17, 40), (48, 256), (160, 2048)])
def test_merge_kernel_matches_numpy(rows, cols, r, fmt):
    """Every row map (plain at eff 0 and 0.37, offset with copy-through rows, the gate|up interleave, several jobs in
    one launch, in place), ld > cols on both sides: equal words everywhere, so the words beyond cols of each row and
    the rows outside the jobs are untouched."""
    from acestep_mi355x import capi
    for name, base, out0, jobs in merge_cases(rows, cols, r, fmt, seed=rows + r):
        got = capi.kernel_lora_merge(base, out0, cols, jobs, fmt=fmt)
        want = numpy_merge(base, out0, cols, jobs, fmt)
        np.testing.assert_array_equal(got, want, err_msg=name)
        if name == "plain eff=0.0":
            np.testing.assert_array_equal(got[:, :cols], base[:, :cols])  # eff = 0 reproduces the base
        if name == "plain eff=0.37":
            assert (got[:, :cols] != base[:, :cols]).mean() > 0.5  # and a real scale moves it


# ------------------------------------------------------------------ engine, HIP path
@pytest.mark.parametrize("targets,r,scale,dtype", [("no_v_up", 13, 0.37, "BF16"), ("all", 8, 1.0, "F16"),
                                                    ("self_qkvo", 1, 1.0, "BF16")])
def test_adapter_equals_merged_checkpoint(targets, r, scale, dtype):
    got, ref = forward_pair(None, base_ckpt(dtype), adapter(r=r, targets=target_sets()[targets], seed=r), scale,
                            inputs(T=40, L=7))
    np.testing.assert_array_equal(got, ref)


def test_full_width_layer_equals_merged_checkpoint():
    """The real 2048 / 6144 / 16 / 8 / 128 widths on one layer: grid sizes and the real w_gu / w_ckv_all shapes."""
    from acestep_mi355x.synthetic import make_config
    cfg = make_config(num_hidden_layers=1)
    base = base_ckpt("BF16", cfg=cfg)
    ad = adapter(cfg=cfg, r=16, targets=target_sets()["all"], seed=16)
    x = inputs(T=32, L=16, H=cfg["hidden_size"])
    got, ref = forward_pair(None, base, ad, 0.8, x)
    np.testing.assert_array_equal(got, ref)
    br = bridge(None, base)
    assert rel(fwd(br, x), got) > 1e-4  # the adapter is not ignored
    br.close()


def gpu_sample(br, x):
    """A 3-step sampling run with the cross-attention cache on device tensors; returns x0."""
    import torch
    h, c, e = (torch.from_numpy(a[None].copy()).cuda() for a in x)
    br.dit_sample_ex_device(1, h.shape[1], e.shape[1], h.data_ptr(), c.data_ptr(), e.data_ptr(), 0, 0, [1.0, 0.6, 0.3],
                            cache_cross=True)
    br.synchronize()
    return h[0].cpu().numpy()


def test_state_changes():
    x = inputs(T=40, L=7)
    X = adapter(targets=target_sets()["all"], seed=7, r=5)
    Y = adapter(targets=target_sets()["no_v_up"], seed=8, r=8)
    fresh = bridge(None, base_ckpt())
    fresh.load_lora(Y, 0.6)
    want = fwd(fresh, x)
    want_sample = gpu_sample(fresh, x)
    fresh.close()
    br = bridge(None, base_ckpt())
    plain = fwd(br, x)
    plain_sample = gpu_sample(br, x)
    br.load_lora(X, 0.0)  # scale 0: the base weights, adapter resident
    np.testing.assert_array_equal(fwd(br, x), plain)
    br.set_lora_scale(1.0)
    assert rel(fwd(br, x), plain) > 1e-4
    br.load_lora(Y, 0.2)  # replaces X
    br.set_lora_scale(0.6)  # rebuilt from the base
    np.testing.assert_array_equal(fwd(br, x), want)
    got_sample = gpu_sample(br, x)  # the cached cross K/V of the base run are not reused
    np.testing.assert_array_equal(got_sample, want_sample)
    assert rel(got_sample, plain_sample) > 1e-4
    br.unload_lora()
    np.testing.assert_array_equal(fwd(br, x), plain)
    np.testing.assert_array_equal(gpu_sample(br, x), plain_sample)
    br.close()


@pytest.mark.parametrize("staged", ["1", "0"])
def test_quantized_base(monkeypatch, staged):
    e0, e1 = quantized_pair_errors(None, monkeypatch, env=(("ACE_MI_QUANT_STAGED", staged),))
    print(f"quantized base (MI355X, ACE_MI_QUANT_STAGED={staged}): e0 = {e0:.3e}, with adapter = {e1:.3e}")
    assert e1 == 0.0 if e0 == 0.0 else e1 <= 2.0 * e0, (e0, e1)


def test_launch_sequence_is_unchanged():
    """Dense checkpoint: the kernel classes and launch counts of one forward are the same with an adapter."""
    x = inputs(T=40, L=7)
    br = bridge(None, base_ckpt())
    fwd(br, x)

    def profile():
        br.profile_enable(True)
        br.profile_reset()
        fwd(br, x)
        got = [(n, c) for n, _, c in br.profile_get()]
        br.profile_enable(False)
        return got

    before = profile()
    br.load_lora(adapter(targets=target_sets()["all"], seed=3))
    assert profile() == before and len(before) > 5
    br.close()
