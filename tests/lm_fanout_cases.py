"""Shared by tests/test_lm_fanout_cpu.py (the LM host library) and tests/test_gpu_lm_fanout.py (the GPU): the cache
fan-out kernel (kernels/lm_fanout.hip / lm_fanout_host.h through ace_mi_kernel_lm_cache_fanout), the runtime entries
ace_mi_lm_fanout / ace_mi_lm_uniforms on the tiny synthetic checkpoint of lm_cases.py, and hook.install_lm_backend's
batch_codes switch with a fake handler.

Nothing here has a tolerance.  The kernel moves bits, so every comparison is of bytes.  The runtime property is that item
s of a batched loop gets the tokens, and a decode step the logits, of its one-item run: the prefill is the same call on
the same rows, the fan-out copies its cache, and a decode-step kernel computes a row from that row's operands alone, in
an order that does not depend on the number of rows -- so the comparison is equality too."""
import contextlib

import numpy as np

import lm_cases as lc
import lm_sample_cases as sc

# ------------------------------------------------------------------------------------------------------ the kernel
LAYERS = 2
K_FILL, V_FILL, M_FILL = 0xA5A5, 0x5A5A, -77          # the destination before the launch
SPECIAL = (0x7E00, 0xFE01, 0x7C01, 0x7C00, 0xFC00, 0x8000, 0x0001, 0x83FF)   # NaNs, +-Inf, -0, subnormals


def kernel_cases():
    """(G, S, hkv, n, cap_src): n 1 and 7 are below a 16-byte multiple of mask words, 257 crosses LM_SPLIT_KEYS and a
    16-position workgroup boundary by one; cap_dst = n + 5."""
    out = []
    for G, S in [(g, s) for g in (1, 2) for s in (1, 3, 4)] + [(1, 8)]:
        for hkv in (1, 2):
            for n in (1, 7, 64, 257):
                for cap_src in (n, n + 3):
                    out.append((G, S, hkv, n, cap_src))
    return out


def case_id(c):
    return "G{}_S{}_hkv{}_n{}_src{}".format(*c)


def kernel_inputs(G, S, hkv, n, cap_src, seed=0):
    rng = np.random.default_rng([seed, G, S, hkv, n, cap_src])
    cap_dst = n + 5
    shape = (LAYERS, G, hkv, cap_src, 128)
    k = rng.integers(0, 65536, shape, dtype=np.uint16)
    v = rng.integers(0, 65536, shape, dtype=np.uint16)
    for a, shift in ((k, 0), (v, 3)):                   # every special pattern in every row that is copied
        for j, bits in enumerate(SPECIAL):
            a[..., (shift + 13 * j) % 128] = bits
    mask = np.ones((G, cap_src), np.int32)
    if G == 2:
        mask[1, : n // 2] = 0                            # the left padding of the unconditional row
    mask[:, n:] = 9                                      # slots past the held positions: never copied
    dst_shape = (LAYERS, G * S, hkv, cap_dst, 128)
    return (k, v, mask, np.full(dst_shape, K_FILL, np.uint16), np.full(dst_shape, V_FILL, np.uint16),
            np.full((G * S, cap_dst), M_FILL, np.int32))


def run_kernel_case(case, lib):
    """positions [0, n) equal as bits, the sentinel intact in [n, cap_dst), the source unchanged"""
    from acestep_mi355x import capi
    G, S, hkv, n, cap_src = case
    k, v, m, kd, vd, md = kernel_inputs(*case)
    want_k, want_v, want_m = kd.copy(), vd.copy(), md.copy()
    for d in range(G * S):                               # the numpy index copy
        want_k[:, d, :, :n] = k[:, d // S, :, :n]
        want_v[:, d, :, :n] = v[:, d // S, :, :n]
        want_m[d, :n] = m[d // S, :n]
    ks, vs, ms, gk, gv, gm = capi.kernel_lm_cache_fanout(k, v, m, kd, vd, md, n, lib=lib)
    assert gk.tobytes() == want_k.tobytes() and gv.tobytes() == want_v.tobytes() and gm.tobytes() == want_m.tobytes()
    assert (gk[:, :, :, n:] == K_FILL).all() and (gv[:, :, :, n:] == V_FILL).all() and (gm[:, n:] == M_FILL).all()
    assert ks.tobytes() == k.tobytes() and vs.tobytes() == v.tobytes() and ms.tobytes() == m.tobytes()


def run_kernel_refusals(lib):
    import pytest
    from acestep_mi355x import capi
    k, v, m, kd, vd, md = kernel_inputs(1, 8, 1, 7, 7)
    for bad_n in (0, 8, -1):                             # nothing, and past the source
        with pytest.raises(RuntimeError, match="status=2"):
            capi.kernel_lm_cache_fanout(k, v, m, kd, vd, md, bad_n, lib=lib)
    k, v, m, kd, vd, md = kernel_inputs(1, 8, 1, 7, 20)
    with pytest.raises(RuntimeError, match="status=2"):  # past the destination (cap_dst 12)
        capi.kernel_lm_cache_fanout(k, v, m, kd, vd, md, 13, lib=lib)
    k3 = np.zeros((LAYERS, 3, 1, 7, 128), np.uint16)
    with pytest.raises(RuntimeError, match="status=2"):  # G = 3
        capi.kernel_lm_cache_fanout(k3, k3, np.ones((3, 7), np.int32), k3, k3, np.ones((3, 7), np.int32), 7, lib=lib)
    k2 = np.zeros((LAYERS, 2, 1, 7, 128), np.uint16)
    k10 = np.zeros((LAYERS, 10, 1, 7, 128), np.uint16)
    with pytest.raises(RuntimeError, match="status=2"):  # 10 sequences
        capi.kernel_lm_cache_fanout(k2, k2, np.ones((2, 7), np.int32), k10, k10, np.ones((10, 7), np.int32), 7, lib=lib)


# ------------------------------------------------------------------------------------------------------ the runtime
N_TOKENS = 24
SAMPLED = dict(sc.PARAMS, cfg_scale=2.0, repetition_penalty=1.1)       # top-k 8, top-p 0.9, both temperatures
ARGMAX = dict(cfg_scale=2.0, temperature=0.0)
SEEDS = (1234567890123, 99, 2 ** 64 - 1, 7)
# ace_mi_lm_uniforms: the first four 24-bit numerators (x >> 40) of std::mt19937_64(seed), computed with the C++
# library's generator, whose 10000th default-seeded output is the standard's 9981545732273789042
PINNED = {1234567890123: (13459040, 2951908, 262423, 4378149),
          2 ** 64 - 1: (434762, 12044561, 645046, 8624000)}


def cfg_prompt(n_prompt, device, seed=5):
    """ids, mask [2, n_prompt]: the unconditional row is shorter and left-padded"""
    import torch
    rng = np.random.default_rng(seed)
    ids = rng.integers(1, 1000, (2, n_prompt)).astype(np.int64)
    mask = np.ones((2, n_prompt), np.int64)
    pad = max(1, n_prompt // 3)
    ids[1, :pad] = 0
    mask[1, :pad] = 0
    return torch.from_numpy(ids).to(device), torch.from_numpy(mask).to(device)


def seen_map(ids, S, device):
    import torch
    seen = torch.zeros((S, 1000), dtype=torch.uint8, device=device)
    seen.scatter_(1, ids[:1].repeat(S, 1), 1)
    return seen


def run_equality(bridge, device, S, params, n_prompt=9, n=N_TOKENS):
    """prefill 2 rows, fan out to S pairs, one loop with column s = the stream of SEEDS[s]  ==  S one-item runs"""
    import torch
    ids, mask = cfg_prompt(n_prompt, device)
    cap = n_prompt + n
    penal = params.get("repetition_penalty", 1.0) != 1.0
    want, step_rows = [], None
    nxt = torch.full((2, 1), 321, dtype=torch.int64).to(device)
    for s in range(S):
        bridge.lm_begin(2, cap)
        logits = bridge.lm_forward(ids, mask)
        toks, n_out = bridge.lm_generate(logits, n, seen=seen_map(ids, 1, device) if penal else None, seed=SEEDS[s],
                                         **params)
        assert n_out == n
        want.append(toks.cpu().numpy()[0])
    bridge.lm_begin(2, cap)
    prompt_logits = bridge.lm_forward(ids, mask).cpu().numpy()
    step_rows = bridge.lm_forward(nxt).cpu().numpy()                    # the one-item run's decode step

    bridge.lm_begin(2, n_prompt)
    logits = bridge.lm_forward(ids, mask)
    wide = bridge.lm_fanout(S, cap, logits)
    info = bridge.lm_info()
    assert (info["batch"], info["capacity"], info["cache_len"]) == (2 * S, cap, n_prompt)
    assert tuple(wide.shape) == (2 * S, 1000)
    for r in range(2 * S):
        assert wide[r].cpu().numpy().tobytes() == prompt_logits[r // S].tobytes(), r
    u = np.stack([bridge.lm_uniforms(SEEDS[s], n) for s in range(S)], axis=1)
    got, n_out = bridge.lm_generate(wide, n, uniforms=torch.from_numpy(u), seen=seen_map(ids, S, device) if penal else None,
                                    **params)
    assert n_out == n and bridge.lm_info()["cache_len"] == n_prompt + n - 1
    got = got.cpu().numpy()
    for s in range(S):
        assert got[s].tolist() == want[s].tolist(), (s, got[s].tolist(), want[s].tolist())
    if params.get("temperature", 1.0) > 0:
        assert any(got[s].tolist() != got[0].tolist() for s in range(1, S))    # the items do differ

    # one decode step after the fan-out, the same token on all rows: rows s and s + S are the one-item run's 0 and 1
    bridge.lm_begin(2, n_prompt)
    wide = bridge.lm_fanout(S, cap, bridge.lm_forward(ids, mask))
    step = bridge.lm_forward(nxt.repeat(S, 1)).cpu().numpy()
    for s in range(S):
        assert step[s].tobytes() == step_rows[0].tobytes() and step[s + S].tobytes() == step_rows[1].tobytes(), s


def run_uniforms(bridge, device):
    import torch
    assert sc.mt_uniforms(5489, 10000, 1)[-1, 0] == np.float32((9981545732273789042 >> 40) * 2.0 ** -24)
    for seed, head in PINNED.items():
        u = bridge.lm_uniforms(seed, 40)
        assert u.dtype == np.float32 and u.shape == (40,)
        assert u[:4].tolist() == [np.float32(x * 2.0 ** -24) for x in head]
        assert u.tobytes() == sc.mt_uniforms(seed, 40, 1)[:, 0].tobytes()
        assert bridge.lm_uniforms(seed, 3).tobytes() == u[:3].tobytes()
    assert bridge.lm_uniforms(5, 0).shape == (0,)
    # ace_mi_lm_generate with the seed alone draws this stream
    params = dict(sc.PARAMS, seed=SEEDS[0])
    a, _ = bridge.lm_generate(sc.prefill(bridge, 1, 6, 32, device), 10, **params)
    u = torch.from_numpy(bridge.lm_uniforms(SEEDS[0], 10)[:, None].copy())
    b, _ = bridge.lm_generate(sc.prefill(bridge, 1, 6, 32, device), 10, uniforms=u, **params)
    assert a.cpu().numpy().tolist() == b.cpu().numpy().tolist()


def run_refusals(bridge, device):
    """every refusal leaves ace_mi_lm_get_info as it was, and the next decode step gives the logits it would have"""
    import pytest
    import torch
    max_pos = bridge.lm_info()["max_positions"]

    def start(B, n_prompt):
        bridge.lm_begin(B, 12)
        if n_prompt:
            ids, mask = cfg_prompt(n_prompt, device)
            ids, mask = (torch.cat([ids, ids[:1]])[:B], torch.cat([mask, mask[:1]])[:B])
            return bridge.lm_forward(ids, mask)
        return torch.zeros((B, 1000), dtype=torch.float32).to(device)

    def step(B):
        return bridge.lm_forward(torch.full((B, 1), 44, dtype=torch.int64).to(device)).cpu().numpy()

    for B, n_prompt, bad in ((2, 6, [(0, 12), (-1, 12), (5, 12), (2, 5), (2, max_pos + 1)]),
                             (3, 6, [(2, 12), (1, 12)]),           # G > 2
                             (2, 0, [(2, 12), (1, 12)])):          # an empty cache
        start(B, n_prompt)
        clean = step(B)
        for copies, cap in bad:
            logits = start(B, n_prompt)
            keep = logits.cpu().numpy().copy()
            before = bridge.lm_info()
            with pytest.raises(RuntimeError, match=r"lm fanout.*status=2"):
                bridge.lm_fanout(copies, cap, logits)
            with pytest.raises(RuntimeError, match=r"lm fanout.*status=2"):
                bridge.lm_fanout(copies, cap)
            assert bridge.lm_info() == before and logits.cpu().numpy().tobytes() == keep.tobytes()
            assert step(B).tobytes() == clean.tobytes(), (B, n_prompt, copies, cap)
    # copies == 1: the same capacity changes nothing, a larger one re-lays the cache and the run goes on unchanged
    start(2, 6)
    clean = [step(2) for _ in range(3)]
    logits = start(2, 6)
    before = bridge.lm_info()
    same = bridge.lm_fanout(1, 12, logits)
    assert bridge.lm_info() == before and same.cpu().numpy().tobytes() == logits.cpu().numpy().tobytes()
    assert step(2).tobytes() == clean[0].tobytes()
    assert bridge.lm_fanout(1, 40) is None
    info = bridge.lm_info()
    assert (info["batch"], info["capacity"], info["cache_len"]) == (2, 40, 7)
    assert step(2).tobytes() == clean[1].tobytes() and step(2).tobytes() == clean[2].tobytes()


def run_not_loaded(lib_path, device):
    import pytest
    import torch
    from acestep_mi355x.capi import GGMLCAPIBridge
    br = GGMLCAPIBridge(lib_path=lib_path)
    try:
        with pytest.raises(RuntimeError, match=r"lm not loaded \(status=1\)"):
            br.lm_fanout(2, 16)
        with pytest.raises(RuntimeError, match=r"lm not loaded \(status=1\)"):
            br.lm_fanout(2, 16, torch.zeros((1, 1000), dtype=torch.float32).to(device))
    finally:
        br.close()


# ------------------------------------------------------------------------------------------------------ the hook
class Tokenizer:
    """One id per character; a list is padded to its longest row on `padding_side`."""
    eos_token_id = 7
    pad_token_id = 0
    padding_side = "right"

    def __call__(self, texts, return_tensors="pt", padding=False, truncation=True):
        import torch
        rows = [[100 + ord(c) % 800 for c in t] for t in ([texts] if isinstance(texts, str) else texts)]
        width = max(len(r) for r in rows)
        ids = torch.zeros((len(rows), width), dtype=torch.long)
        mask = torch.zeros((len(rows), width), dtype=torch.long)
        for i, r in enumerate(rows):
            at = width - len(r) if self.padding_side == "left" else 0
            ids[i, at:at + len(r)] = torch.tensor(r)
            mask[i, at:at + len(r)] = 1
        return {"input_ids": ids, "attention_mask": mask}

    def decode(self, ids, skip_special_tokens=False):
        return " ".join(str(int(i)) for i in ids)


def make_handler(device, start_state="CODES_GENERATION"):
    """The stub handler of lm_sample_cases.make_stubs with the batch entry of the `pt` backend on top: `_run_pt` serves
    a list of prompts one after the other through `_run_pt_single`, which tokenises, sets the shared processor up, runs
    the CFG loop (cfg_scale > 1) or the constrained loop, and decodes what follows the prompt."""
    import torch
    base, Processor, _ = sc.make_stubs(device)

    class Handler(type(base)):
        llm_tokenizer = Tokenizer()
        max_model_len = 64 + 12                       # 12 new tokens at the most: the per-token fallbacks stay short

        def __init__(self):
            super().__init__()
            self.constrained_processor = None
            self.contexts = 0

        def _normalize_batch_input(self, prompts):
            return (prompts, True) if isinstance(prompts, list) else ([prompts], False)

        @contextlib.contextmanager
        def _load_model_context(self):
            self.contexts += 1
            yield

        def _setup_constrained_processor(self, use_constrained_decoding, constrained_decoding_debug, target_duration,
                                         user_metadata, stop_at_reasoning, skip_genres, skip_caption, skip_language,
                                         generation_phase, is_batch=False):
            if not use_constrained_decoding:
                return None
            proc = Processor()                            # the reset of the shared processor
            proc.state = type(proc.state)[start_state]
            self.constrained_processor = proc
            return proc

        def _build_unconditional_prompt(self, caption, lyrics, cot_text, negative_prompt, generation_phase, is_batch):
            return negative_prompt

        def _run_pt_single(self, formatted_prompt, temperature, cfg_scale, negative_prompt, top_k, top_p,
                           repetition_penalty, use_constrained_decoding, constrained_decoding_debug, target_duration,
                           user_metadata, stop_at_reasoning, skip_genres, skip_caption, skip_language, generation_phase,
                           caption, lyrics, cot_text):
            tok = self.llm_tokenizer
            proc = self._setup_constrained_processor(
                use_constrained_decoding=use_constrained_decoding, constrained_decoding_debug=constrained_decoding_debug,
                target_duration=target_duration, user_metadata=user_metadata, stop_at_reasoning=stop_at_reasoning,
                skip_genres=skip_genres, skip_caption=skip_caption, skip_language=skip_language,
                generation_phase=generation_phase, is_batch=False)
            new = min(int(max(10, min(600, target_duration)) * 5) + 500, self.max_model_len - 64)
            pad = tok.pad_token_id or tok.eos_token_id
            with self._load_model_context():
                if cfg_scale > 1.0:
                    side, tok.padding_side = tok.padding_side, "left"
                    enc = tok([formatted_prompt, self._build_unconditional_prompt(
                        caption=caption, lyrics=lyrics, cot_text=cot_text, negative_prompt=negative_prompt,
                        generation_phase=generation_phase, is_batch=False)], padding=True)
                    tok.padding_side = side
                    ids, am = enc["input_ids"].to(self.device), enc["attention_mask"].to(self.device)
                    out = self._generate_with_cfg_custom(ids, am, new, temperature, cfg_scale, top_k, top_p,
                                                         repetition_penalty, pad, None, proc)[0:1]
                else:
                    enc = tok(formatted_prompt)
                    ids, am = enc["input_ids"].to(self.device), enc["attention_mask"].to(self.device)
                    out = self._generate_with_constrained_decoding(ids, am, new, temperature, top_k, top_p,
                                                                   repetition_penalty, pad, None, proc)
            return tok.decode(out[0][ids.shape[1]:].cpu(), skip_special_tokens=False)

        def _run_pt(self, formatted_prompts, temperature, cfg_scale, negative_prompt, top_k, top_p, repetition_penalty,
                    use_constrained_decoding=True, constrained_decoding_debug=False, target_duration=None,
                    user_metadata=None, stop_at_reasoning=False, skip_genres=True, skip_caption=False,
                    skip_language=False, generation_phase="cot", caption="", lyrics="", cot_text="", seeds=None):
            prompts, is_batch = self._normalize_batch_input(formatted_prompts)
            texts = []
            with self._load_model_context():
                for i, p in enumerate(prompts):
                    if is_batch and seeds and i < len(seeds):
                        torch.manual_seed(seeds[i])
                    texts.append(self._run_pt_single(
                        p, temperature, cfg_scale, negative_prompt, top_k, top_p, repetition_penalty,
                        use_constrained_decoding, constrained_decoding_debug, target_duration,
                        None if is_batch else user_metadata, False if is_batch else stop_at_reasoning,
                        True if is_batch else skip_genres, True if is_batch else skip_caption,
                        True if is_batch else skip_language, generation_phase, caption, lyrics, cot_text))
            return texts if is_batch else texts[0]

    return Handler()


class Counted:
    """counts the prefills (forwards of more than one token) and the loops a bridge runs"""

    def __init__(self, bridge):
        self.bridge, self.prefills, self.loops, self.fanouts = bridge, 0, 0, 0

    def __enter__(self):
        fwd, gen, fan = self.bridge.lm_forward, self.bridge.lm_generate, self.bridge.lm_fanout

        def forward(ids, mask=None):
            self.prefills += int(ids.shape[1] > 1)
            return fwd(ids, mask)

        def generate(*a, **kw):
            self.loops += 1
            return gen(*a, **kw)

        def fanout(*a, **kw):
            self.fanouts += 1
            return fan(*a, **kw)
        self.bridge.lm_forward, self.bridge.lm_generate, self.bridge.lm_fanout = forward, generate, fanout
        return self

    def __exit__(self, *exc):
        del self.bridge.lm_forward, self.bridge.lm_generate, self.bridge.lm_fanout
        return False


PROMPT = "a song about rain"
CALL = dict(temperature=0.85, negative_prompt="NO", top_k=8, top_p=0.9, target_duration=30.0, generation_phase="codes")


def run_pt(bridge, device, batch_codes, prompts, cfg_scale, seeds, torch_seed=4, start_state="CODES_GENERATION",
           use_constrained_decoding=True):
    """(texts, prefills, loops, fanouts, torch's generator state after the call)"""
    import torch
    from acestep_mi355x.hook import install_lm_backend
    h = make_handler(device, start_state)
    install_lm_backend(h, bridge, max_new_tokens=32, device_codes=True, batch_codes=batch_codes)
    torch.manual_seed(torch_seed)
    with Counted(bridge) as c:
        out = h._run_pt(prompts, cfg_scale=cfg_scale, repetition_penalty=1.0 if cfg_scale > 1.0 else 1.1, seeds=seeds,
                        use_constrained_decoding=use_constrained_decoding, **CALL)
    return out, c.prefills, c.loops, c.fanouts, torch.get_rng_state()


def run_hook_equal(bridge, device, n_items, cfg_scale, seeds):
    """batch_codes=True returns what device_codes=True alone returns, from ceil(n / group) prefills"""
    import torch
    prompts = [PROMPT] * n_items
    want, prefills, loops, fanouts, state = run_pt(bridge, device, False, prompts, cfg_scale, seeds)
    assert (prefills, loops, fanouts) == (n_items, n_items, 0)
    got, prefills, loops, fanouts, state2 = run_pt(bridge, device, True, prompts, cfg_scale, seeds)
    groups = -(-n_items // (4 if cfg_scale > 1.0 else 8))
    assert (prefills, loops, fanouts) == (groups, groups, groups)
    assert isinstance(got, list) and got == want, (got, want)
    assert len(set(got)) > 1                                   # the items differ
    assert all(len(t.split()) == 7 and t.split()[-1] == "7" for t in got)      # 6 codes and the forced EOS
    assert torch.equal(state, state2)                          # the generator is left where the sequential run leaves it


def run_hook_fallbacks(bridge, device):
    import pytest
    from acestep_mi355x.hook import install_lm_backend
    for what, kw, prompts in (
            ("unequal prompts", {}, [PROMPT, PROMPT, PROMPT + "!"]),
            ("no processor", dict(use_constrained_decoding=False), [PROMPT] * 3),
            ("metadata state", dict(start_state="THINK_TAG"), [PROMPT] * 3),
            ("one prompt in a list", {}, [PROMPT]),
            ("a single prompt", {}, PROMPT)):
        n = len(prompts) if isinstance(prompts, list) else 1
        want, prefills, _, _, _ = run_pt(bridge, device, False, prompts, 2.0, None, **kw)
        got, prefills2, _, fanouts, _ = run_pt(bridge, device, True, prompts, 2.0, None, **kw)
        assert prefills == n and prefills2 == n and fanouts == 0, what
        assert type(got) is type(want) and got == want, what
    h = make_handler(device)
    with pytest.raises(ValueError, match="batch_codes"):
        install_lm_backend(h, bridge, max_new_tokens=32, batch_codes=True)
    assert h.llm is None
