"""CPU checks of the causal-LM feature: the synthetic LM writer against the fixture's sha256, the hook object's protocol
with a fake bridge, and the LM engine (runtime/lm.cpp) on the host emulation of its kernels (tests/lmhostlib.py) through
cases (a)-(d) of tests/golden/lm_qwen3.npz."""
import numpy as np
import pytest

import lm_cases as lc


@pytest.mark.parametrize("variant", ["tied", "untied"])
def test_lm_writer_matches_fixture_sha(variant):
    assert lc.sha256(lc.checkpoint(variant)) == str(lc.fixture()[f"{variant}/sha256"])


def test_lm_writer_layout():
    from oracle.dit_oracle import read_safetensors
    import json
    import os
    for variant in ("tied", "untied"):
        d = lc.checkpoint(variant)
        names = set(read_safetensors(os.path.join(d, "model.safetensors")))
        assert "model.embed_tokens.weight" in names and "model.layers.1.mlp.down_proj.weight" in names
        assert ("lm_head.weight" in names) == (variant == "untied")
        with open(os.path.join(d, "config.json")) as f:
            assert json.load(f)["tie_word_embeddings"] == (variant == "tied")


class FakeBridge:
    VOCAB = 11

    def __init__(self):
        self.calls = []

    def lm_info(self):
        return dict(vocab_size=self.VOCAB, max_positions=64)

    def lm_begin(self, batch, capacity):
        self.calls.append(("begin", batch, capacity))

    def lm_forward(self, ids, mask):
        import torch
        self.calls.append(("forward", tuple(ids.shape), None if mask is None else tuple(mask.shape)))
        return torch.zeros((ids.shape[0], self.VOCAB))


def test_hook_protocol_with_fake_bridge():
    import torch
    from acestep_mi355x.hook import install_lm_backend

    class Handler:
        llm = None
        llm_backend = "vllm"
        device = "cpu"

    h, br = Handler(), FakeBridge()
    install_lm_backend(h, br, max_new_tokens=16)
    assert h.llm_backend == "pt" and h.llm.generation_config.use_cache is True and h.llm.eval() is h.llm
    assert isinstance(h.llm.device, torch.device)
    ids = torch.ones((2, 5), dtype=torch.long)
    mask = torch.ones((2, 5), dtype=torch.long)
    out = h.llm(input_ids=ids, attention_mask=mask, past_key_values=None, use_cache=True)
    assert tuple(out.logits.shape) == (2, 1, br.VOCAB) and out.logits[:, -1, :].shape == (2, br.VOCAB)
    assert br.calls == [("begin", 2, 21), ("forward", (2, 5), (2, 5))]
    past = out.past_key_values
    mask = torch.ones((2, 6), dtype=torch.long)
    out2 = h.llm(input_ids=ids[:, -1:], attention_mask=mask, past_key_values=past, use_cache=True)
    assert br.calls[-1] == ("forward", (2, 1), (2, 1)) and out2.past_key_values is past
    with pytest.raises(ValueError, match="one token"):
        h.llm(input_ids=ids[:, -2:], attention_mask=mask, past_key_values=past)
    h.llm(input_ids=ids, attention_mask=None, past_key_values=None)           # a new prefill: capacity clipped
    assert br.calls[-2:] == [("begin", 2, 21), ("forward", (2, 5), None)]
    with pytest.raises(ValueError, match="stale"):
        h.llm(input_ids=ids[:, -1:], past_key_values=past)
    with pytest.raises(NotImplementedError, match="_generate_with_constrained_decoding.*_generate_with_cfg_custom"):
        h.llm.generate(input_ids=ids)
    install_lm_backend(h, br, max_new_tokens=1000)
    h.llm(input_ids=ids)
    assert br.calls[-2] == ("begin", 2, 64)                                    # max_position_embeddings


def test_lm_runtime_under_asan_ubsan():
    """tests/host/lm_asan_driver.cpp, a stand-alone program, over the host-emulated kernels with ASan + UBSan."""
    import json
    import os
    import shutil
    import subprocess
    import tempfile
    from lmhostlib import CLANG, host_flags, lm_host_sources, ROOT
    if not os.path.exists(CLANG):
        pytest.skip("host clang++ not available")
    work = tempfile.mkdtemp(prefix="acemi_lm_asan_")
    nohead = os.path.join(work, "nohead")
    shutil.copytree(lc.checkpoint("tied"), nohead)
    with open(os.path.join(nohead, "config.json")) as f:
        cfg = json.load(f)
    cfg["tie_word_embeddings"] = False
    with open(os.path.join(nohead, "config.json"), "w") as f:
        json.dump(cfg, f)
    exe = os.path.join(work, "lm_asan_driver")
    subprocess.run([CLANG, "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-fno-sanitize-recover=undefined", *host_flags(), *lm_host_sources(),
                    os.path.join(ROOT, "tests", "host", "lm_asan_driver.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("ACE_GGML_QWEN_WEIGHT_QTYPE", None)
    r = subprocess.run([exe, lc.checkpoint("tied"), lc.checkpoint("untied"), lc.checkpoint("tied", model_prefix=False),
                        lc.checkpoint("tied", dtype="F32"), nohead], capture_output=True, text=True, timeout=600, env=env)
    print(r.stdout[-2000:], r.stderr[-6000:])
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stderr[-6000:]


@pytest.fixture(scope="module")
def host_bridges():
    from acestep_mi355x.capi import GGMLCAPIBridge
    from lmhostlib import build_lm_host_lib
    lib = build_lm_host_lib()
    made = {}

    def get(variant):
        if variant not in made:
            br = GGMLCAPIBridge(lib_path=lib)
            br.load_lm(lc.checkpoint(variant))
            made[variant] = br
        return made[variant]
    yield get
    for br in made.values():
        br.close()


@pytest.mark.parametrize("variant,case", [("tied", "a"), ("untied", "b"), ("tied", "c"), ("untied", "d")])
def test_host_emulated_lm_vs_fixture(host_bridges, variant, case):
    """The engine's control flow, cache indexing and rounding points on the CPU (each case in one variant, to keep the
    emulated GEMMs quick; the GPU suite runs every case in both)."""
    br = host_bridges(variant)
    info = br.lm_info()
    assert info["tied"] == (variant == "tied") and info["vocab_size"] == 1000 and info["head_dim"] == 128
    _, err, bound = lc.measure(br, variant, case, "cpu", "host")
    assert np.all(err <= bound), (variant, case, float(np.nanmax(err / bound)))


def test_host_emulated_lm_state_handling(host_bridges):
    import torch
    br = host_bridges("tied")
    z = lc.fixture()
    ids = torch.from_numpy(z["tied/a/ids"])
    br.lm_begin(1, 40)
    br.lm_forward(ids[:, :37])
    assert br.lm_info()["cache_len"] == 37
    with pytest.raises(RuntimeError, match="status=2"):
        br.lm_forward(ids[:, :2])               # a prefill onto a non-empty cache
    for i in range(37, 40):
        br.lm_forward(ids[:, i:i + 1])
    with pytest.raises(RuntimeError, match="capacity.*status=2"):
        br.lm_forward(ids[:, 40:41])
    assert br.lm_info()["cache_len"] == 40
    br.lm_reset()
    assert br.lm_info()["cache_len"] == 0
    for bad in ((0, 8), (9, 8), (1, 0), (1, 10 ** 6)):
        with pytest.raises(RuntimeError, match="status=2"):
            br.lm_begin(*bad)
