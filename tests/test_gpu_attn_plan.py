"""Every attention grid layout (csrc/attn_plan.h) on the GPU at a few hundred rows: the policy override
(ace_mi_kernel_attn_policy) plans for an 8-CU device, so 10 blocks overfill the "chip" the way 376 blocks overfill
256 CUs at 240 s.  Each case first asks ace_mi_attn_plan, under the same policy, for the layout it means to run.

Shape: Hq 2 / Hkv 1 (64 queries per block), 600 queries (10 blocks, the last one 24 rows), 1100 keys (18 key tiles); the
key mask hides the whole first key-range half of every block (a part with m = -inf, l = 0) and 30 % of the rest.
Against the fp64 reference and per-mode bounds of tests/test_gpu_kernels.py."""
import numpy as np
import pytest

from test_gpu_kernels import MODES, _check_attn

pytestmark = pytest.mark.gpu

SCALE = 1.0 / np.sqrt(128.0)
# name -> (policy fields beside n_cu = 8, the plan they must give for 10 blocks)
LAYOUTS = {
    "tail": (dict(ksplit_mode=0, tail=1),  # 8 whole blocks + 2 x 2 halves, rounded up to 8
             dict(ksplit=2, split_from=8, grid=16, merge="tail", merge_grid=32)),
    "uniform2": (dict(ksplit_mode=2, tail=0),  # 20 parts, four empty workgroups
                 dict(ksplit=2, split_from=0, grid=24, merge="uniform2")),
    "unsplit": (dict(ksplit_mode=1, tail=1),  # six empty workgroups
                dict(ksplit=1, split_from=0, grid=16, merge="none", merge_grid=0)),
}
# name -> (operand mode of test_gpu_kernels.MODES, kh, the kernel that must run)
KERNELS = {"f8c-attn2": ("f8c", 0, "attn2"), "f8c-attn_kh": ("f8c", 1, "attn_kh"), "split": ("split", 0, "attn2")}


def _capi():
    from acestep_mi355x import capi
    return capi


def _inputs(B, hq, hkv, nq, nk):
    rng = np.random.default_rng(B * 1000 + hq + nq + nk)
    q = rng.standard_normal((B, nq, hq * 128)).astype(np.float32) * 2.0
    kv = rng.standard_normal((B, nk, 2 * hkv * 128)).astype(np.float32) * 0.3
    kmask = (rng.random((B, nk)) > 0.3).astype(np.int32)
    tiles = (nk + 63) // 64
    half = (tiles + 1) // 2 * 64  # the first of two key-range parts: ceil(tiles / 2) tiles
    kmask[:, :half] = 0
    kmask[:, half] = 1
    return q, kv, kmask


def _run(B, hq, hkv, nq, nk, layout, kernel):
    capi = _capi()
    policy, want = LAYOUTS[layout]
    mode, kh, want_kernel = KERNELS[kernel]
    q, kv, kmask = _inputs(B, hq, hkv, nq, nk)
    shape = dict(B=B, Hq=hq, Hkv=hkv, nq=nq, nk=nk, window=0, causal=0, has_part=1, out_f32=0,
                 split=int(MODES[mode].get("split", False)), pv_split=int(MODES[mode].get("pv_split", False)),
                 f8=int(MODES[mode].get("f8", False)))
    outs = []
    for xcd in (0, 1):
        full = dict(policy, tail_min=16, xcd_order=xcd, kh=kh, n_cu=8)  # every field: nothing left to the environment
        plan = capi.attn_plan(shape, **full)
        assert plan["n_blk"] == 10 and plan["kernel"] == want_kernel and plan["xcd_order"] == xcd, plan
        assert {k: plan[k] for k in want} == want, plan
        capi.kernel_attn_policy(**full)
        try:
            outs.append(capi.kernel_attention(q, kv, hq, hkv, window=0, kmask=kmask, scale=SCALE, **MODES[mode]))
        finally:
            capi.kernel_attn_policy()
    _check_attn(outs[1], q, kv, hq, hkv, 0, kmask, SCALE, mode)
    # a block's arithmetic does not depend on its launch index
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_attention_layouts_at_600_rows(layout, kernel):
    _run(1, 2, 1, 600, 1100, layout, kernel)


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_attention_tail_layout_four_heads_per_group(kernel):
    """n_rep 4 (32 queries per block): two items of 150 queries are 10 blocks, the last of each item 22 rows."""
    _run(2, 4, 1, 150, 1100, "tail", kernel)
