"""Shared by tests/test_gpu_lm_score.py (the product and self-test libraries on the GPU) and tests/test_lm_score_cpu.py
(the LM host library): teacher-forced scoring -- kernels/lm_score.hip through ace_mi_kernel_lm_score, the runtime entry
ace_mi_lm_score and hook.install_lm_backend's scoring_module keyword.

Kernel tolerance.  The reference is float64 on the exact 16-bit operand values.  With u = 2^-24, c = the longest f32
addition chain behind a logit (reported by the entry: one MFMA's 32 products, then one add per 32 values of H) and
A[m][j] = sum_k |x[m][k] w[j][k]|, a computed logit is within b[m][j] = c u A[m][j] of the exact one.  logprob =
l_t - logsumexp(l):
  * l_t contributes b[m][t]; logsumexp is 1-Lipschitz in the sup norm, so the logits contribute max_j b[m][j] to it;
  * the sum of exp: V positive terms, at most V additions behind any of them (per-lane, per-tile, per-split and merge
    sums together), relative error V u; every term is expf(l - max) with |l - max| <= R = max l - min l, whose argument
    carries one rounding (R u absolute = R u relative in the value) and expf itself at most 4 u; every tile, and the
    merge, rescales the running sum once more (another expf and a product: (R + 5) u each);
  * logf is within 4 u of |log s| <= log V, and the last two operations round at the size of their operands.
  tol[m] = b[m][t] + max_j b[m][j] + u (V + (tiles + 2)(R + 5) + 4 + 3 (|l_t| + |logsumexp|))
rank is exact: the test first asserts, on the reference alone, that no other logit lies within b[m][t] + b[m][j] of the
target's (head rows that are copies of the target's row excepted: those tie exactly and are ordered by index)."""
import numpy as np

BM, BN = 64, 128
U = 2.0 ** -24

# (M, V, H, splits, act_type 0 bf16 / 1 fp16): M around the 64-row block, V around the 128-column tile, 805 = 7 tiles
# (3 and 4 per split, the last one partial), H with one, several and a half k step (1056 = 16.5 x 64), splits 5 > the
# single tile of V = 127
CASES = ((1, 127, 64, 5, 0), (63, 129, 256, 1, 1), (65, 1000, 64, 2, 0), (131, 805, 256, 2, 1), (3, 1000, 1056, 0, 0),
         (65, 1000, 64, 0, 1))
# The (case, family) pairs that run, each with a seed for which the separation assertion of run_kernel_case holds
# (searched on the float64 reference alone).  131 rows x 805 columns under moving_max has no such seed below 400 (its
# bound grows with the +-80 products): that pair is left out, the family runs on the five other shapes.
SEEDS = {(0, "normal"): 1, (0, "moving_max"): 1, (0, "edges"): 1, (0, "duplicates"): 1,
         (1, "normal"): 1, (1, "moving_max"): 1, (1, "edges"): 1, (1, "duplicates"): 1,
         (2, "normal"): 1, (2, "moving_max"): 67, (2, "edges"): 1, (2, "duplicates"): 1,
         (3, "normal"): 2, (3, "edges"): 2, (3, "duplicates"): 13,
         (4, "normal"): 2, (4, "moving_max"): 1, (4, "edges"): 1, (4, "duplicates"): 1,
         (5, "normal"): 4, (5, "moving_max"): 103, (5, "edges"): 3, (5, "duplicates"): 1}


def kernel_params(n_cases=len(CASES)):
    return [k for k in SEEDS if k[0] < n_cases]


def param_id(k):
    c = CASES[k[0]]
    return "M%d-V%d-H%d-S%d-%s-%s" % (c[0], c[1], c[2], c[3], "f16" if c[4] else "bf16", k[1])


def to_bits(a, act_type):
    """(16-bit words, the float64 values they hold)"""
    if act_type == 1:
        h = np.asarray(a, np.float32).astype(np.float16)
        return h.view(np.uint16), h.astype(np.float64)
    from acestep_mi355x.synthetic import _bf16_bits
    bits = _bf16_bits(np.asarray(a, np.float32))
    return bits, (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def make_inputs(case, family, seed):
    """x [M][H], w [V][H], target [M], dup [M][V] bool (head rows that copy the target's)"""
    M, V, H, splits, _ = case
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M, H))
    w = rng.standard_normal((V, H)) * (3.0 / np.sqrt(H))
    target = rng.integers(0, V, M)
    if family == "moving_max":
        # feature 0 puts every logit near -80, features 1..3 lift one column to +80 for the rows with m % 3 == g: a
        # column of the first tile, of the last full tile and of the partial tile
        hot = (5, (V // BN - 1) * BN + 3 if V >= BN else 0, V - 1)
        x[:, :4] = 0.0
        w[:, :4] = 0.0
        x[:, 0] = 8.0
        w[:, 0] = -10.0
        for g in range(3):
            x[g::3, 1 + g] = 8.0
            w[hot[g], 1 + g] = 20.0
    if family == "edges":
        tiles = -(-V // BN)
        s = max(splits, 1)
        edge = (1 * tiles // s) * BN if s <= tiles else BN   # first column of split 1
        for i, t in enumerate((0, V - 1, BN - 1, BN, edge - 1, edge)):
            if i < M and 0 <= t < V:
                target[i] = t
    if family == "duplicates":
        target[:] = np.where(np.arange(M) % 2 == 0, V // 3, V - 2)
        for t in (V // 3, V - 2):
            w[t - 1] = w[t]
            w[t + 1] = w[t]
    dup = np.zeros((M, V), bool)
    if family == "duplicates":
        for m in range(M):
            dup[m, [target[m] - 1, target[m] + 1]] = True
    return x, w, target.astype(np.int32), dup


def reference(xv, wv, target):
    logits = xv @ wv.T
    rows = np.arange(len(target))
    lt = logits[rows, target]
    mx = logits.max(axis=1)
    lse = mx + np.log(np.exp(logits - mx[:, None]).sum(axis=1))
    cols = np.arange(logits.shape[1])[None, :]
    above = (logits > lt[:, None]) | ((logits == lt[:, None]) & (cols < target[:, None]))
    above[rows, target] = False
    return logits, lt - lse, above.sum(axis=1).astype(np.int32)


def run_kernel_case(param, lib):
    from acestep_mi355x import capi
    case, family, seed = CASES[param[0]], param[1], SEEDS[param]
    M, V, H, splits, act = case
    x, w, target, dup = make_inputs(case, family, seed)
    xb, xv = to_bits(x, act)
    wb, wv = to_bits(w, act)
    logits, ref_lp, ref_rank = reference(xv, wv, target)
    got_lp, got_rank, chain = capi.kernel_lm_score(xb, wb, target, splits, act, lib=lib)
    b = chain * U * (np.abs(xv) @ np.abs(wv).T)
    rows = np.arange(M)
    lt = logits[rows, target]
    gap = np.abs(logits - lt[:, None]) - (b + b[rows, target][:, None])
    gap[rows, target] = np.inf
    gap[dup] = np.inf
    assert gap.min() > 0, f"seed {seed}: a logit within the bound of the target's (margin {gap.min():.3e})"
    R = logits.max(axis=1) - logits.min(axis=1)
    lse = lt - ref_lp
    tol = b[rows, target] + b.max(axis=1) + U * (V + (-(-V // BN) + 2) * (R + 5) + 4 + 3 * (np.abs(lt) + np.abs(lse)))
    err = np.abs(got_lp.astype(np.float64) - ref_lp)
    print(f"{param_id(param)}: chain {chain} max err {err.max():.3e} max err/tol {(err / tol).max():.3f} "
          f"min tol {tol.min():.3e} ranks {ref_rank.min()}..{ref_rank.max()}")
    assert np.isfinite(got_lp).all() and (err <= tol).all()
    assert (got_rank == ref_rank).all()
    again = capi.kernel_lm_score(xb, wb, target, splits, act, lib=lib)
    assert again[0].tobytes() == got_lp.tobytes() and again[1].tobytes() == got_rank.tobytes()


def run_kernel_refusals(lib):
    """H % 32 != 0 is the launcher's refusal (status 1); ids outside [0, V) are clamped"""
    import pytest
    from acestep_mi355x import capi
    with pytest.raises(RuntimeError, match="status=1"):
        capi.kernel_lm_score(to_bits(np.ones((2, 48)), 0)[0], to_bits(np.ones((5, 48)), 0)[0], np.zeros(2, np.int32), lib=lib)
    x, w, _, _ = make_inputs((2, 200, 64, 1, 0), "normal", 3)
    xb, wb = to_bits(x, 0)[0], to_bits(w, 0)[0]
    clamped = capi.kernel_lm_score(xb, wb, np.array([0, 199], np.int32), 1, lib=lib)
    wild = capi.kernel_lm_score(xb, wb, np.array([-7, 2 ** 31 - 1], np.int32), 1, lib=lib)
    assert wild[0].tobytes() == clamped[0].tobytes() and wild[1].tobytes() == clamped[1].tobytes()


# ------------------------------------------------------------------------------------------------- the engine entry
def open_bridge(lib_path, model_dir):
    from acestep_mi355x.capi import GGMLCAPIBridge
    br = GGMLCAPIBridge(lib_path=lib_path)
    try:
        if model_dir:
            br.load_lm(model_dir)
        yield br
    finally:
        br.close()


def batch(B, n, device):
    """ids and a left-padded mask [B][n]: row b starts with 2 b padding columns"""
    import torch
    ids = np.random.default_rng(100 + B).integers(1, 1000, (B, n))
    mask = (np.arange(n)[None, :] >= 2 * np.arange(B)[:, None]).astype(np.int64)
    return torch.from_numpy(ids).to(device), torch.from_numpy(mask).to(device)


def route_delta(bridge, fixture_logits, device):
    """tests/lm_cases.py's tolerance for one position's logits reached by two routes -- 1.5 x the rel-L2 error of the
    engine's full-sequence route against the float64 fixture -- doubled; taken at the first call of fixture case a"""
    import torch
    import lm_cases as lc
    z = lc.fixture()
    ids, mask, prompt = z["tied/a/ids"], z["tied/a/mask"], int(z["tied/a/prompt"])
    bridge.lm_begin(1, prompt)
    got = bridge.lm_forward(torch.from_numpy(ids[:, :prompt].copy()).to(device),
                            torch.from_numpy(mask[:, :prompt].copy()).to(device)).cpu().numpy()
    return 2 * 1.5 * float(lc.rel_l2(got, fixture_logits[0]).max())


def prefix_logits(bridge, ids, mask, p):
    """the engine's own last-position logits of the prefix [0, p), float64 (a one-token prefix is the decode step)"""
    bridge.lm_begin(ids.shape[0], p)
    return bridge.lm_forward(ids[:, :p], None if mask is None else mask[:, :p]).cpu().numpy().astype(np.float64)


def run_engine(bridge, device, delta, B, score_from, n=12):
    """lm_score against lm_forward on every prefix.  Two logit vectors within rel-L2 `delta` differ by at most
    e = delta |l|_2 in any entry: the log-probability by at most 2 e, the rank by at most the number of reference
    logits within 2 e of the target's.  Then one decode step gives what it gives after a plain prefill."""
    import torch
    ids, mask = batch(B, n, device)
    nxt, one = torch.full((B, 1), 5).to(device), torch.ones((B, 1), dtype=torch.int64).to(device)
    bridge.lm_begin(B, n + 1)
    logprob, rank = bridge.lm_score(ids, mask, score_from)
    assert bridge.lm_info()["cache_len"] == n and logprob.shape == (B, n - score_from) and rank.dtype == torch.int32
    step = bridge.lm_forward(nxt, one).cpu().numpy()
    bridge.lm_begin(B, n + 1)
    bridge.lm_forward(ids, mask)
    assert bridge.lm_forward(nxt, one).cpu().numpy().tobytes() == step.tobytes()
    logprob, rank = logprob.cpu().numpy(), rank.cpu().numpy()
    for p in range(score_from, n):
        l, t = prefix_logits(bridge, ids, mask, p), ids[:, p].cpu().numpy()
        _, ref_lp, ref_rank = reference(l, np.eye(l.shape[1]), t)
        e = delta * np.linalg.norm(l, axis=1)
        near = (np.abs(l - l[np.arange(B), t][:, None]) <= 2 * e[:, None]).sum(axis=1) - 1
        d_lp, d_rank = np.abs(logprob[:, p - score_from] - ref_lp), np.abs(rank[:, p - score_from] - ref_rank)
        print(f"B {B} from {score_from} pos {p}: |dlogprob| {d_lp} bound {2 * e} |drank| {d_rank} allowed {near}")
        ok = mask[:, :p].cpu().numpy().any(axis=1)   # a prefix of padding alone predicts nothing (NaN on both routes)
        assert ok[0] and (d_lp <= 2 * e)[ok].all() and (d_rank <= near)[ok].all()


def run_refusals(bridge, lib_path, device):
    import pytest
    ids, mask = batch(2, 12, device)
    bridge.lm_begin(2, 12)
    for bad in (0, 12, -3):
        with pytest.raises(RuntimeError, match=r"lm score.*status=2"):
            bridge.lm_score(ids, mask, bad)
    assert bridge.lm_info()["cache_len"] == 0
    bridge.lm_score(ids, mask, 5)
    with pytest.raises(RuntimeError, match=r"lm score.*status=2"):   # a prefill on a cache that is not empty
        bridge.lm_score(ids, mask, 5)
    bridge.lm_begin(2, 8)
    with pytest.raises(RuntimeError, match=r"lm score.*status=2"):   # beyond the capacity
        bridge.lm_score(ids, mask, 5)
    for br in open_bridge(lib_path, None):
        with pytest.raises(RuntimeError, match=r"lm not loaded \(status=1\)"):
            br.lm_score(ids, None, 5)


# ------------------------------------------------------------------------------------------------------ the hook
class Tokenizer:
    """one id per character, no special tokens"""

    def __call__(self, text, return_tensors="pt", **kw):
        import torch
        ids = torch.tensor([[ord(c) % 997 + 1 for c in text]], dtype=torch.int64)
        return {"input_ids": ids, "attention_mask": torch.ones_like(ids)}


def run_hook(bridge, device, delta):
    """the replaced functions against the reference's formulas on per-prefix engine logits; topk = 500 so that some
    targets of the random model fall inside it.  The log-probability bound is run_engine's, averaged over the target."""
    import types
    import torch
    from acestep_mi355x import hook
    handler = types.SimpleNamespace(llm=None, llm_backend="vllm", llm_tokenizer=Tokenizer(), device=device)
    ns = types.SimpleNamespace(_calculate_log_prob=None, _calculate_topk_recall=None)
    hook.install_lm_backend(handler, bridge, scoring_module=ns)
    prompt, target, topk = "a prompt of some length", "bpm: 120", 500
    ids = Tokenizer()(prompt + target)["input_ids"].to(device)
    lps, ranks, bound, near = [], [], [], []
    for p in range(len(prompt), ids.shape[1]):
        l = torch.from_numpy(prefix_logits(bridge, ids, None, p))
        lps.append(torch.log_softmax(l, -1)[0, ids[0, p]].item())
        ranks.append(int((l[0] > l[0, ids[0, p]]).sum()))
        bound.append(2 * delta * float(l.norm()))
        near.append(int(((l[0] - l[0, ids[0, p]]).abs() <= bound[-1]).sum()) - 1)
    got = ns._calculate_log_prob(handler, prompt, target)
    avg, per_k = ns._calculate_topk_recall(handler, prompt, target, topk=topk)
    print(f"hook: log prob {got:.6f} reference {np.mean(lps):.6f} bound {np.mean(bound):.3e}; recall {avg:.4f} ranks {ranks}")
    assert abs(got - np.mean(lps)) <= np.mean(bound) and min(ranks) < topk
    r, d = np.array(ranks), np.array(near)   # a rank moves by at most `near` between the two routes (run_engine)
    weight = lambda q: np.where(q < topk, 1.0 - np.maximum(q, 0) / topk, 0.0).mean()
    assert all(np.mean(r + d < k) <= per_k[k] <= np.mean(r - d < k) for k in range(1, topk + 1))
    assert weight(r + d) - 1e-12 <= avg <= weight(r - d) + 1e-12
    # and exactly the reference's formulas on the engine's own scores of the same ids
    bridge.lm_begin(1, ids.shape[1])
    lp, rk = (v[0].cpu().numpy() for v in bridge.lm_score(ids, torch.ones_like(ids), len(prompt)))
    assert got == float(torch.from_numpy(lp).mean()) and per_k == {k: float(np.mean(rk < k)) for k in range(1, topk + 1)}
    assert abs(avg - weight(rk)) < 1e-12
    assert ns._calculate_log_prob(handler, prompt, "") == float("-inf")
    assert ns._calculate_topk_recall(handler, prompt, "") == (0.0, {})
