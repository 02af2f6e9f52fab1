"""Cases of ace_mi_lm_extend / ace_mi_lm_truncate shared by tests/test_gpu_lm_extend.py and tests/test_lm_extend_cpu.py.
`delta` is tests/lm_score_cases.py route_delta: the rel-L2 tolerance between two routes to one position's logits; a
log-probability then moves by at most 2 delta |l|_2 and a rank by at most the number of logits that close to the
target's (lm_score_cases.run_engine's derivation)."""
import numpy as np

import lm_cases as lc
import lm_score_cases as sc


def run_extend_vs_steps(bridge, device, delta, B, P, n):
    """prefill P + one chunk of n against prefill P + n single-token steps: last logits and cache length"""
    import torch
    ids, mask = sc.batch(B, P + n, device)
    bridge.lm_begin(B, P + n)
    bridge.lm_forward(ids[:, :P], mask[:, :P])
    got = bridge.lm_extend(ids[:, P:], mask[:, P:]).cpu().numpy()
    assert bridge.lm_info()["cache_len"] == P + n
    bridge.lm_begin(B, P + n)
    ref = bridge.lm_forward(ids[:, :P], mask[:, :P])
    for t in range(P, P + n):
        ref = bridge.lm_forward(ids[:, t:t + 1], mask[:, t:t + 1])
    d = lc.rel_l2(got, ref.cpu().numpy().astype(np.float64))
    print(f"extend B {B} P {P} n {n}: rel_l2 against single steps {d} (bound {delta:.3e})")
    assert bridge.lm_info()["cache_len"] == P + n and (d <= delta).all()


def run_scoring(bridge, device, delta, B, P, T):
    """scoring a target of T tokens by truncate + extend against the engine's per-prefix logits, and against
    ace_mi_lm_score on prompt + target; then the same extend again gives the same bytes"""
    import torch
    n = P + T
    ids, mask = sc.batch(B, n, device)
    bridge.lm_begin(B, n)
    ref_lp, ref_rk = (v.cpu().numpy() for v in bridge.lm_score(ids, mask, P))
    bridge.lm_begin(B, n)
    bridge.lm_forward(ids[:, :P], mask[:, :P])
    bridge.lm_truncate(P - 1)
    lp, rk = bridge.lm_extend(ids[:, P - 1:], mask[:, P - 1:], score_from=1)
    assert bridge.lm_info()["cache_len"] == n and lp.shape == (B, T) and rk.dtype == torch.int32
    bridge.lm_truncate(P - 1)
    lp2, rk2 = bridge.lm_extend(ids[:, P - 1:], mask[:, P - 1:], score_from=1)
    assert lp.cpu().numpy().tobytes() == lp2.cpu().numpy().tobytes() and torch.equal(rk, rk2)
    lp, rk = lp.cpu().numpy(), rk.cpu().numpy()
    for p in range(P, n):
        l, t = sc.prefix_logits(bridge, ids, mask, p), ids[:, p].cpu().numpy()
        _, want_lp, want_rk = sc.reference(l, np.eye(l.shape[1]), t)
        e = delta * np.linalg.norm(l, axis=1)
        near = (np.abs(l - l[np.arange(B), t][:, None]) <= 2 * e[:, None]).sum(axis=1) - 1
        for name, a, b in (("prefixes", want_lp, want_rk), ("lm_score", ref_lp[:, p - P], ref_rk[:, p - P])):
            d_lp, d_rk = np.abs(lp[:, p - P] - a), np.abs(rk[:, p - P] - b)
            print(f"B {B} P {P} pos {p} vs {name}: |dlogprob| {d_lp} bound {2 * e} |drank| {d_rk} allowed {near}")
            assert (d_lp <= 2 * e).all() and (d_rk <= near).all()


def run_refusals(bridge, lib_path, device):
    import pytest
    ids, mask = sc.batch(2, 12, device)
    bad = r"lm extend.*status=2"
    bridge.lm_begin(2, 12)
    with pytest.raises(RuntimeError, match=bad):        # an empty cache
        bridge.lm_extend(ids[:, :4], mask[:, :4])
    bridge.lm_forward(ids[:, :6], mask[:, :6])
    with pytest.raises(RuntimeError, match=bad):        # beyond the capacity
        bridge.lm_extend(ids[:, 5:], mask[:, 5:])
    for score_from in (0, 4, -1):
        with pytest.raises(RuntimeError, match=bad):
            bridge.lm_extend(ids[:, 6:10], mask[:, 6:10], score_from=score_from)
    null = lambda *out: bridge.lib.ace_mi_lm_extend(bridge.ctx, ids.to(dtype=ids.dtype).data_ptr(), None, 1, 1, *out, None)
    assert null(None, None, None) == 2 and null(1, None, None) == 2 and null(None, 1, None) == 2   # no output; half a pair
    for length in (-1, 7):
        with pytest.raises(RuntimeError, match=r"lm truncate.*status=2"):
            bridge.lm_truncate(length)
    assert bridge.lm_info()["cache_len"] == 6
    bridge.lm_truncate(0)
    assert bridge.lm_info()["cache_len"] == 0 and bridge.lm_info()["capacity"] == 12
    for br in sc.open_bridge(lib_path, None):
        with pytest.raises(RuntimeError, match=r"lm not loaded \(status=1\)"):
            br.lm_extend(ids[:, :4], None)
    for br in sc.open_bridge(lib_path, lc.checkpoint("tied")):     # no ace_mi_lm_begin
        with pytest.raises(RuntimeError, match=bad):
            br.lm_extend(ids[:, :4], None)


def run_hook(bridge, device, delta):
    """reuse_score_prompt=True: one prefill for two targets on one prompt, a fresh one when the prompt changes; scores
    within run_scoring's tolerance of the keyword-off path (their difference: twice the bound of either to the truth)"""
    import types
    from acestep_mi355x import hook
    prefills = []
    forward = bridge.lm_forward
    bridge.lm_forward = lambda ids, mask=None: (prefills.append(tuple(ids.shape)), forward(ids, mask))[1]
    try:
        handlers = []
        for reuse in (False, True):
            h = types.SimpleNamespace(llm=None, llm_backend="vllm", llm_tokenizer=sc.Tokenizer(), device=device)
            ns = types.SimpleNamespace(_calculate_log_prob=None, _calculate_topk_recall=None)
            hook.install_lm_backend(h, bridge, scoring_module=ns, reuse_score_prompt=reuse)
            handlers.append((h, ns))
        (h0, off), (h1, on) = handlers
        prompt, other = "a prompt of some length", "another prompt, longer"
        cases = ((prompt, "bpm: 120"), (prompt, "key: C minor"), (other, "bpm: 90"))
        got = []
        for i, (pr, target) in enumerate(cases):      # the keyword-on wrappers first: they own the cache meanwhile
            del prefills[:]
            got.append(on._calculate_log_prob(h1, pr, target))
            assert prefills == ([] if i == 1 else [(1, len(pr))]), prefills
        for (pr, target), g in zip(cases, got):
            want = off._calculate_log_prob(h0, pr, target)
            full = sc.Tokenizer()(pr + target)["input_ids"].to(device)
            norm = max(float(np.linalg.norm(sc.prefix_logits(bridge, full, None, p))) for p in range(len(pr), full.shape[1]))
            print(f"hook reuse '{target}': log prob {g:.6f} keyword off {want:.6f} bound {4 * delta * norm:.3e}")
            assert abs(g - want) <= 4 * delta * norm
    finally:
        bridge.lm_forward = forward
