"""Shared by test_lm_sample_cpu.py (the host library) and test_gpu_lm_sample.py (the GPU): cases and numpy references
of the token-selection kernel (kernels/lm_sample.hip, ace_mi_kernel_lm_select) and of the engine loop
(ace_mi_lm_select / ace_mi_lm_generate).  The references are written from the definitions in include/acestep_mi355x.h:
steps 1-5 as numpy float32 operations (bit-exact), the top-p cut and the draw from float64 softmaxes.

Tolerance of everything that depends on a sum of exp values (which values the top-p cut keeps, which id a uniform
draws), in units of probability mass: eps = c * 2^-24 with

    c = 2 * (3 * A + ULP) + CHAIN_PART + CHAIN_TOTAL + 2

KERNEL.  A term is expf(x), x = fl(z / T) - fl(zmax / T) (T = 1 for top-p: x = fl(z - zmax)).  The rounding of zmax / T
is common to all terms and cancels in the normalisation; the rest of the argument error is at most (|z / T| + |x|) *
2^-24 <= 3 * A * 2^-24 with A = max |z / T| over the kept values, and expf itself is within ULP = 2 units of the last
place (the device library documents 1).  A relative error r of every term moves a normalised partial sum by at most
2 r (numerator and denominator).  Every f32 addition on the longest path behind a sum is 2^-24 relative on a partial
sum <= 1: CHAIN_PART additions behind the partial sum that is compared, CHAIN_TOTAL behind the total it is compared
with.  lm_select_chains reports three lengths for n candidates.  [0], behind a top-p mass and behind Z alike (PART =
TOTAL = [0]): the thread's run of ceil(n / 1024), 6 butterfly steps, the 15 additions of the 16 waves in order.  [1],
behind the draw's total: rows = ceil(ceil(n / 16) / 64) lane-column additions, 6 butterfly steps, 16 wave additions.
[2], behind a cumulative value of the draw: the base of the last wave (15 wave totals of depth rows + 6 each, added in
order), one carry addition per row already walked (rows - 1), the 6 scan steps inside the row folded into the row
total that the carry took, and the final carry + scan value: 2 * rows + 21.  For the draw PART = [2], TOTAL = [1].
The last 2: the product u * total (or top_p * Z) and the comparison against it.
EMULATION (the host library).  Terms and sums in double, every chain reported as 1: every error above is below the
kernel's, so the same formula with the reported chains bounds it too.
A and the chains come from the inputs and the mapping, never from an output."""
import numpy as np

NINF = np.float32(-np.inf)
ULP = 2


def eps_of(A, chain_part, chain_total):
    return (2.0 * (3.0 * float(A) + ULP) + chain_part + chain_total + 2.0) * 2.0 ** -24


# ---------------------------------------------------------------------------------------------- numpy references
def process(logits, vocab, cfg_scale=1.0, allowed=None, stop_id=-1, block_stop=False, force_stop=False,
            pre_temperature=0.0, repetition_penalty=1.0, seen=None, top_k=0):
    """Steps 1-5 in float32: per sampled sequence (ids [n] ascending candidates, z [n] f32, surv [n] bool)."""
    x = np.asarray(logits, np.float32)
    B = x.shape[0]
    S = B // 2 if cfg_scale > 1.0 else B
    out = []
    for s in range(S):
        if force_stop:
            ids = np.array([stop_id], np.int64)
        else:
            ids = np.arange(vocab, dtype=np.int64) if allowed is None else np.asarray(allowed, np.int64)
        z = x[s, ids].copy()
        if cfg_scale > 1.0:
            u = x[s + S, ids]
            with np.errstate(invalid="ignore"):
                z = (u + np.float32(cfg_scale) * (z - u)).astype(np.float32)
        z[np.isnan(z)] = NINF
        if block_stop and not force_stop and stop_id >= 0:
            z[ids == stop_id] = NINF
        if pre_temperature > 0:
            z = (z / np.float32(pre_temperature)).astype(np.float32)
        if seen is not None and repetition_penalty != 1.0:
            p = np.float32(repetition_penalty)
            hit = np.asarray(seen)[s, ids] != 0
            with np.errstate(invalid="ignore"):
                z = np.where(hit, np.where(z < 0, z * p, z / p), z).astype(np.float32)
        surv = z > NINF
        if 0 < top_k < len(z):
            kth = np.sort(z)[::-1][top_k - 1]
            surv &= z >= kth
        out.append((ids, z, surv))
    return out


def top_p_cut(z, surv, top_p):
    """Step 6 from the float64 softmax: (keep [n] bool, the smallest |mass_above(v) - top_p| over the distinct
    surviving values v, A = max |z| of the survivors)."""
    if not surv.any():
        return surv.copy(), np.inf, 0.0
    zs = z[surv].astype(np.float64)
    A = float(np.abs(zs).max())
    if not (0.0 < top_p < 1.0):
        return surv.copy(), np.inf, A
    vals, counts = np.unique(zs, return_counts=True)
    e = np.exp(vals - vals.max()) * counts
    q = e / e.sum()
    above = np.concatenate([np.cumsum(q[::-1])[::-1][1:], [0.0]])  # mass strictly greater than vals[i]
    above[-1] = 0.0
    keep_v = above <= float(np.float32(top_p))
    cut = vals[keep_v].min()
    gap = float(np.abs(above - float(np.float32(top_p))).min())
    return surv & (z.astype(np.float64) >= cut), gap, A


def expected_processed(vocab, ids, z, keep):
    row = np.full(vocab, NINF, np.float32)
    row[ids[keep]] = z[keep]
    return row


def draw_check(ids, z, keep, temperature, u, token, chains):
    """The sampled-token criterion: `token` is a kept id whose float64 CDF interval meets [u - eps, u + eps].  Returns
    the distance from u to the interval in units of eps (<= 1 passes; inf for an id that is not kept)."""
    kid = ids[keep]
    if token not in set(kid.tolist()):
        return np.inf
    a = z[keep].astype(np.float64) / float(np.float32(temperature))
    p = np.exp(a - a.max())
    p /= p.sum()
    c = np.cumsum(p)
    j = int(np.nonzero(kid == token)[0][0])
    lo, hi = (c[j - 1] if j else 0.0), (1.0 if j == len(kid) - 1 else c[j])
    u = float(u)
    dist = max(lo - u, u - hi, 0.0)
    return dist / eps_of(np.abs(a).max(), int(chains[2]), int(chains[1]))


def argmax_token(ids, z, keep):
    if not keep.any():
        return int(ids[0])
    m = z[keep].max()
    return int(ids[np.nonzero(keep & (z == m))[0][0]])


# ---------------------------------------------------------------------------------------------------- kernel cases
VOCABS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 4097)   # 1025 / 2049: just past one / two passes of 1024 threads
BIG_VOCAB = 151936
PAD = 5            # columns of NaN past every logits row, sentinel words past every output row


def allowed_shape(kind, vocab):
    """None | one id | a contiguous range plus one outlier below it (the EOS shape)"""
    if kind is None:
        return None
    if kind == "one":
        return np.array([vocab // 2], np.int32)
    n = int(kind)
    start = vocab - n - 3 if vocab - n - 3 > 1 else 2
    return np.concatenate([[start // 2], np.arange(start, start + n - 1)]).astype(np.int32)


def make_logits(seed, B, vocab, scale, shape="normal"):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, vocab)) * scale).astype(np.float32)
    if shape == "peaked":
        x = (x * 0.1).astype(np.float32)
        x[:, vocab // 3] += np.float32(30.0)
    elif shape == "flat":
        x[:] = np.float32(1.25)
    out = np.full((B, vocab + PAD), np.nan, np.float32)
    out[:, :vocab] = x
    return out


def toleranced_cases():
    """(name, dict) of the sampled cases: sizes x S x CFG x allowed shapes, top-k and top-p on and off.  The scale of
    the logits grows with the vocabulary so that the mass sits on few ids and the top-p precondition can hold."""
    cases = []
    i = 0
    for vocab in VOCABS:
        for B, cfg in ((1, 1.0), (2, 1.0), (2, 2.0), (4, 1.0), (4, 2.0), (8, 2.5)):   # S = 1, 2, 1, 4, 2, 4
            i += 1
            kinds = [None]
            if vocab >= 2:
                kinds.append("one")
            kinds += [k for k in (2, 65, 1025) if vocab >= k + 4]
            kind = kinds[i % len(kinds)]
            top_k = (0, 8, 50)[i % 3]
            top_p = (1.0, 0.9, 0.6)[(i // 2) % 3]
            cases.append((f"v{vocab}-B{B}-cfg{cfg}-a{kind}-k{top_k}-p{top_p}",
                          dict(seed=100 + i, B=B, vocab=vocab, cfg=cfg, kind=kind, top_k=top_k, top_p=top_p,
                               scale=3.0 + 0.5 * np.log2(vocab), pre=0.85, temp=0.85, pen=1.0 if i % 4 else 1.3)))
    for shape in ("peaked", "flat"):
        cases.append((f"{shape}-v1025", dict(seed=7, B=2, vocab=1025, cfg=1.0, kind=None, top_k=0,
                                             top_p=0.9 if shape == "peaked" else 0.6, scale=3.0, pre=0.0, temp=1.0,
                                             pen=1.0, shape=shape)))
    cases.append(("big", dict(seed=11, B=2, vocab=BIG_VOCAB, cfg=2.0, kind=None, top_k=50, top_p=0.9, scale=12.0,
                              pre=0.85, temp=0.85, pen=1.0)))
    cases.append(("big-allowed", dict(seed=12, B=1, vocab=BIG_VOCAB, cfg=1.0, kind=64001, top_k=0, top_p=0.9,
                                      scale=12.0, pre=0.85, temp=0.85, pen=1.1)))
    return cases


def run_toleranced(case, lib, uniforms=(0.0, 0.37, 1.0 - 2.0 ** -24)):
    """Runs one case for every uniform (and once as argmax); asserts the bit-exact and the toleranced properties,
    determinism and the untouched padding.  Returns the worst distance / eps."""
    from acestep_mi355x import capi
    c = dict(case)
    vocab, B, cfg = c["vocab"], c["B"], c["cfg"]
    S = B // 2 if cfg > 1.0 else B
    x = make_logits(c["seed"], B, vocab, c["scale"], c.get("shape", "normal"))
    allowed = allowed_shape(c["kind"], vocab)
    rng = np.random.default_rng(c["seed"] + 1)
    seen = np.zeros((S, vocab + PAD), np.uint8)
    seen[:, :vocab] = rng.random((S, vocab)) < 0.3
    seen[:, vocab:] = 9
    stop = int(allowed[0]) if allowed is not None and len(allowed) > 1 else -1
    kw = dict(cfg_scale=cfg, pre_temperature=c["pre"], repetition_penalty=c["pen"], top_k=c["top_k"], top_p=c["top_p"],
              allowed=allowed, stop_id=stop, block_stop=False, vocab=vocab, lib=lib)
    ref = process(x, vocab, cfg, allowed, stop, False, False, c["pre"], c["pen"], seen, c["top_k"])
    worst = 0.0
    for u in tuple(uniforms) + (None,):
        temp = c["temp"] if u is not None else 0.0
        run = lambda: capi.kernel_lm_select(
            x, temperature=temp, uniform=None if u is None else np.full(S, u, np.float32), seen=seen,
            tokens0=np.full(S * 3, -7, np.int32), token_stride=3, next_ids0=np.full(B + 2, -9, np.int32)[:B],
            done0=np.full(1 + S, 0, np.int32), processed0=np.full((S, vocab + PAD), 123.0, np.float32), **kw)
        r = run()
        r2 = run()
        for k in ("tokens", "seen", "next_ids", "done", "processed"):   # determinism, every output, bit for bit
            assert r[k].tobytes() == r2[k].tobytes(), k
        chains = r["chains"]
        tok = r["tokens"].reshape(S, 3)
        assert np.all(tok[:, 1:] == -7)
        assert np.all(r["processed"][:, vocab:] == 123.0) and np.all(r["seen"][:, vocab:] == 9)
        for s in range(S):
            ids, z, surv = ref[s]
            keep, gap, A = top_p_cut(z, surv, c["top_p"])
            if 0.0 < c["top_p"] < 1.0:   # the precondition of an exact comparison of the kept set
                e0 = eps_of(A, int(chains[0]), int(chains[0]))
                assert gap > e0, ("top-p precondition", gap, e0)
            want = expected_processed(vocab, ids, z, keep)
            assert r["processed"][s, :vocab].view(np.uint32).tolist() == want.view(np.uint32).tolist()
            t = int(tok[s, 0])
            if u is None:
                assert t == argmax_token(ids, z, keep)
            else:
                d = draw_check(ids, z, keep, c["temp"], u, t, chains)
                worst = max(worst, d)
                assert d <= 1.0, (s, u, t, d)
            assert r["next_ids"][s] == t and (cfg <= 1.0 or r["next_ids"][s + S] == t)
            changed = np.nonzero(r["seen"][s] != seen[s])[0]
            assert r["seen"][s, t] == 1 and set(changed.tolist()) <= {t}
            assert (r["done"][1 + s] != 0) == (t == stop)
        assert (r["done"][0] != 0) == bool(np.any(tok[:, 0] == stop))
    return worst


def select_np(lib, x, **kw):
    from acestep_mi355x import capi
    B = x.shape[0]
    S = B // 2 if kw.get("cfg_scale", 1.0) > 1.0 else B
    return capi.kernel_lm_select(x, processed0=np.zeros((S, x.shape[1]), np.float32), lib=lib, **kw)


def run_exact_properties(lib):
    """The bit-exact properties that need crafted rows."""
    rng = np.random.default_rng(3)
    V = 1025
    x = (rng.standard_normal((2, V)) * 4).astype(np.float32)
    am = np.argmax(x, axis=1)
    for u in (0.0, 0.5, 1.0 - 2.0 ** -24):   # top_k = 1: the argmax whatever u is
        r = select_np(lib, x, top_k=1, temperature=1.0, uniform=np.full(2, u, np.float32))
        assert r["tokens"].tolist() == am.tolist()
    a = select_np(lib, x, top_k=0, temperature=0.0)["processed"]        # top_k >= candidates: off
    for k in (V, V + 1, 10 ** 6):
        assert select_np(lib, x, top_k=k, temperature=0.0)["processed"].tobytes() == a.tobytes()
    # a tiny top_p leaves exactly the group of maxima
    y = x.copy()
    y[0, [5, 77, 1024]] = y[0].max() + np.float32(1.0)
    r = select_np(lib, y, top_p=1e-6, temperature=1.0, uniform=np.array([0.99, 0.0], np.float32))
    assert np.nonzero(np.isfinite(r["processed"][0]))[0].tolist() == [5, 77, 1024] and r["tokens"][0] == 1024
    assert np.nonzero(np.isfinite(r["processed"][1]))[0].tolist() == [int(am[1])]
    # all-equal logits with top_p = 0.6 keep all
    f = np.full((1, 65), 0.5, np.float32)
    r = select_np(lib, f, top_p=0.6, temperature=1.0, uniform=np.array([1.0 - 2.0 ** -24], np.float32))
    assert np.isfinite(r["processed"]).all() and r["tokens"][0] == 64
    # duplicates of the k-th value are all kept
    d = np.arange(64, dtype=np.float32)[None, :].copy()
    d[0, [3, 9, 40]] = 60.0                                             # 63, 62, 61, then 60 four times
    r = select_np(lib, d, top_k=4, temperature=0.0)
    assert np.nonzero(np.isfinite(r["processed"][0]))[0].tolist() == [3, 9, 40, 60, 61, 62, 63]
    # the penalty sign rule on negative, positive and zero logits (and -0)
    p = np.array([[-2.0, 3.0, 0.0, -0.0, 1.5, -1.5]], np.float32)
    seen = np.array([[1, 1, 1, 1, 0, 0]], np.uint8)
    r = select_np(lib, p, repetition_penalty=1.3, seen=seen, temperature=0.0)
    want = np.array([np.float32(-2.0) * np.float32(1.3), np.float32(3.0) / np.float32(1.3), 0.0, -0.0, 1.5, -1.5], np.float32)
    assert r["processed"][0].view(np.uint32).tolist() == want.view(np.uint32).tolist()
    assert r["tokens"][0] == 1 and r["seen"][0].tolist() == [1, 1, 1, 1, 0, 0]
    # min_tokens blocks stop_id, force_stop leaves only it; done only on stop; a stopped sequence keeps emitting it
    s = np.zeros((2, 9), np.float32)
    s[:, 4] = 50.0
    r = select_np(lib, s, stop_id=4, block_stop=True, temperature=0.0, done0=np.zeros(3, np.int32))
    assert r["tokens"].tolist() == [0, 0] and r["done"].tolist() == [0, 0, 0] and np.isinf(r["processed"][:, 4]).all()
    r = select_np(lib, s, stop_id=4, temperature=0.0, done0=np.zeros(3, np.int32), n_emitted=6)
    assert r["tokens"].tolist() == [4, 4] and r["done"].tolist() == [7, 1, 1]
    s[:, 4] = -50.0
    r = select_np(lib, s, stop_id=4, force_stop=True, temperature=1.0, uniform=np.array([0.3, 0.9], np.float32),
                  done0=np.array([3, 0, 0], np.int32), n_emitted=6)
    assert r["tokens"].tolist() == [4, 4] and r["done"].tolist() == [3, 1, 1]
    assert np.nonzero(np.isfinite(r["processed"]))[1].tolist() == [4, 4]
    r = select_np(lib, s, stop_id=4, temperature=0.0, done0=np.array([2, 0, 1], np.int32), n_emitted=6)
    assert r["tokens"].tolist() == [0, 4] and r["done"].tolist() == [2, 0, 1]
    # NaN counts as -inf; a CFG pair fills both rows of next_ids
    n = np.array([[1.0, np.nan, 0.5], [0.0, 9.0, 0.25]], np.float32)
    r = select_np(lib, n, cfg_scale=2.0, temperature=0.0, next_ids0=np.array([-1, -1], np.int32))
    assert r["tokens"].tolist()[:1] == [0] and r["next_ids"].tolist() == [0, 0] and np.isinf(r["processed"][0, 1])
    mix = np.float32(0.0) + np.float32(2.0) * (np.float32(1.0) - np.float32(0.0))
    assert r["processed"][0, 0] == mix


# ---------------------------------------------------------------------------------------------------- engine cases
PARAMS = dict(top_k=8, top_p=0.9, pre_temperature=0.85, temperature=0.85)


def prefill(bridge, B, n_prompt, capacity, device, seed=5, vocab=1000):
    import torch
    ids = torch.from_numpy(np.random.default_rng(seed).integers(0, vocab, (1, n_prompt)).astype(np.int64))
    ids = ids.repeat(B, 1)
    if B > 1:
        ids[B // 2:, : n_prompt // 2] = 3          # the unconditional half differs
    bridge.lm_begin(B, capacity)
    return bridge.lm_forward(ids.to(device))


def compose(bridge, logits, n_max, uniforms, device, stop_id=-1, min_tokens=0, check=None, **params):
    """The loop through the public entries: lm_select, then lm_forward of the token on every row.  Returns (tokens
    [S][n], logits of every step, n_out by the reference's torch.any rule)."""
    import torch
    B = logits.shape[0]
    S = B // 2 if params.get("cfg_scale", 1.0) > 1.0 else B
    toks, logs = [], []
    n_out = n_max
    for t in range(n_max):
        logs.append(logits.cpu().numpy().copy())
        tok = bridge.lm_select(logits, uniforms=uniforms[t].to(device), n_emitted=t, stop_id=stop_id,
                               min_tokens=min_tokens, **params)
        toks.append(tok.cpu().numpy().copy())
        if check is not None:
            check(t, logs[-1], toks[-1])
        if stop_id >= 0 and (toks[-1] == stop_id).any():
            n_out = t + 1
            break
        if t + 1 < n_max:
            logits = bridge.lm_forward(tok.to(torch.int64).repeat(B // S)[:, None])
    return np.stack(toks, axis=1), logs, n_out


def kernel_criterion(params, allowed, chain_of):
    """check(t, logits, tokens) for compose(): the chosen token passes the kernel-level criterion on these logits."""
    def check(t, logits, tokens):
        cfg = params.get("cfg_scale", 1.0)
        ref = process(logits, logits.shape[1], cfg, allowed, -1, False, False, params.get("pre_temperature", 0.0), 1.0,
                      None, params.get("top_k", 0))
        for s, (ids, z, surv) in enumerate(ref):
            keep, gap, A = top_p_cut(z, surv, params.get("top_p", 1.0))
            n = len(ids)
            assert gap > eps_of(A, chain_of(n)[0], chain_of(n)[0]), ("top-p precondition", t, gap)
            d = draw_check(ids, z, keep, params["temperature"], check.u[t][s], int(tokens[s]), chain_of(n))
            assert d <= 1.0, (t, s, d)
    return check


def mt_uniforms(seed, n, S):
    """The documented stream of ace_mi_lm_generate: std::mt19937_64(seed), value = (x >> 40) * 2^-24, order [t][s]."""
    N, M, R = 312, 156, 31
    A, U, D, Sx, Bm, T, C, L, F = (0xB5026F5AA96619E9, 29, 0x5555555555555555, 17, 0x71D67FFFEDA60000, 37,
                                  0xFFF7EEE000000000, 43, 6364136223846793005)
    mask = (1 << 64) - 1
    mt = [seed & mask]
    for i in range(1, N):
        mt.append((F * (mt[-1] ^ (mt[-1] >> 62)) + i) & mask)
    out = []
    idx = N
    for _ in range(n * S):
        if idx >= N:
            for i in range(N):
                x = (mt[i] & ~((1 << R) - 1) & mask) | (mt[(i + 1) % N] & ((1 << R) - 1))
                xa = x >> 1
                if x & 1:
                    xa ^= A
                mt[i] = mt[(i + M) % N] ^ xa
            idx = 0
        y = mt[idx]
        idx += 1
        y ^= (y >> U) & D
        y ^= (y << Sx) & Bm
        y ^= (y << T) & C
        y ^= y >> L
        out.append(np.float32((y >> 40) * 2.0 ** -24))
    return np.array(out, np.float32).reshape(n, S)


_CHAINS = {}


def chain_source(lib):
    """n_cand -> the three chain lengths of the implementation behind `lib` (None: the GPU self-test library)."""
    from acestep_mi355x import capi

    def chain_of(n):
        key = (id(lib), n)
        if key not in _CHAINS:
            _CHAINS[key] = capi.kernel_lm_select(np.zeros((1, n), np.float32), temperature=0.0, lib=lib)["chains"].tolist()
        return _CHAINS[key]
    return chain_of


def run_composition(bridge, device, chain_of, B, cfg, n_prompt, capacity, n=12, seed=21):
    """lm_generate with explicit uniforms == the loop of lm_forward + lm_select, tokens and logits bit for bit; every
    chosen token passes the kernel-level criterion on the logits the engine returned."""
    import torch
    S = B // 2 if cfg > 1.0 else B
    params = dict(PARAMS, cfg_scale=cfg)
    u = torch.from_numpy(np.random.default_rng(seed).random((n, S)).astype(np.float32))
    check = kernel_criterion(params, None, chain_of)
    check.u = u.numpy()
    logits = prefill(bridge, B, n_prompt, capacity, device)
    want, logs, _ = compose(bridge, logits, n, u, device, check=check, **params)
    assert bridge.lm_info()["cache_len"] == n_prompt + n - 1
    logits = prefill(bridge, B, n_prompt, capacity, device)
    got, n_out = bridge.lm_generate(logits, n, uniforms=u, **params)
    assert n_out == n and bridge.lm_info()["cache_len"] == n_prompt + n - 1
    assert got.cpu().numpy().tolist() == want.tolist()
    # the scratch logits hold the last step's: the input of the last selection
    assert logits.cpu().numpy().tobytes() == logs[-1].tobytes()
    return want


def run_stop(bridge, device):
    import torch
    stop, code, n_max, n_prompt = 7, 500, 40, 9
    params = dict(allowed_ids=[stop, code], temperature=50.0, stop_id=stop, min_tokens=5)
    u = np.full((n_max, 1), 0.9, np.float32)
    u[2] = 0.1      # stop is blocked here: the code is the only candidate
    u[8] = 0.1      # the first stop
    u[20] = 0.1
    u = torch.from_numpy(u)
    logits = prefill(bridge, 1, n_prompt, 64, device)
    want, _, n_ref = compose(bridge, logits, n_max, u, device, **params)
    assert n_ref < n_max and n_ref % 16 != 0 and n_ref == 9, n_ref      # the reference itself stops early, off a poll
    assert want[0].tolist() == [code] * 8 + [stop]
    logits = prefill(bridge, 1, n_prompt, 64, device)
    got, n_out = bridge.lm_generate(logits, n_max, uniforms=u, **params)
    assert n_out == n_ref and got.cpu().numpy()[:, :n_out].tolist() == want.tolist()
    # the loop notices a stop at the next multiple of 16 tokens; the tokens before that one were fed back
    assert bridge.lm_info()["cache_len"] == n_prompt + min(n_max, 16 * -(-n_out // 16)) - 1
    # the duration-constrained case: min_tokens == n_max, the stop token is never a candidate
    logits = prefill(bridge, 1, n_prompt, 64, device)
    got, n_out = bridge.lm_generate(logits, 20, uniforms=u[:20], **dict(params, min_tokens=20))
    assert n_out == 20 and got.cpu().numpy().tolist() == [[code] * 20]
    assert bridge.lm_info()["cache_len"] == n_prompt + 19


def run_seeded(bridge, device):
    import torch
    # the restatement itself, anchored: the C++ standard fixes the 10000th output of std::mt19937_64 seeded with 5489
    assert mt_uniforms(5489, 10000, 1)[-1, 0] == np.float32((9981545732273789042 >> 40) * 2.0 ** -24)
    params = dict(PARAMS, cfg_scale=2.0, seed=1234567890123)
    runs = []
    for _ in range(2):
        logits = prefill(bridge, 4, 6, 32, device)
        got, n_out = bridge.lm_generate(logits, 10, **params)
        runs.append(got.cpu().numpy())
        assert n_out == 10
    assert runs[0].tolist() == runs[1].tolist()
    u = torch.from_numpy(mt_uniforms(params["seed"], 10, 2))
    logits = prefill(bridge, 4, 6, 32, device)
    got, _ = bridge.lm_generate(logits, 10, uniforms=u, **params)
    assert got.cpu().numpy().tolist() == runs[0].tolist()
    other, _ = bridge.lm_generate(prefill(bridge, 4, 6, 32, device), 10, **dict(params, seed=99))
    assert other.cpu().numpy().tolist() != runs[0].tolist()


def run_errors(bridge, device):
    import pytest
    import torch
    nxt = torch.tensor([[11]], dtype=torch.int64).to(device)
    logits = prefill(bridge, 1, 6, 16, device)
    clean = bridge.lm_forward(nxt).cpu().numpy()
    bad = [dict(n_max=12), dict(n_max=0), dict(n_max=-3), dict(n_max=2, allowed_ids=[]), dict(n_max=2, stop_id=1000),
           dict(n_max=2, allowed_ids=[5], stop_id=5, min_tokens=1), dict(n_max=2, cfg_scale=2.0)]
    logits = prefill(bridge, 1, 6, 16, device)
    keep = logits.cpu().numpy().copy()
    for kw in bad:
        kw = dict(kw)
        n_max = kw.pop("n_max")
        with pytest.raises(RuntimeError, match="status=2"):
            bridge.lm_generate(logits, n_max, seed=1, **kw)
        assert bridge.lm_info()["cache_len"] == 6
    for kw in (dict(allowed_ids=[]), dict(stop_id=1000), dict(allowed_ids=[5], stop_id=5, min_tokens=1),
               dict(cfg_scale=2.0), dict(force_stop=True)):
        with pytest.raises(RuntimeError, match="status=2"):
            bridge.lm_select(logits, uniforms=torch.zeros(1), **kw)
        assert bridge.lm_info()["cache_len"] == 6
    assert logits.cpu().numpy().tobytes() == keep.tobytes()
    assert bridge.lm_forward(nxt).cpu().numpy().tobytes() == clean.tobytes()
    got, n_out = bridge.lm_generate(prefill(bridge, 1, 6, 16, device), 11, seed=1)    # exactly fills the cache
    assert n_out == 11 and bridge.lm_info()["cache_len"] == 16


# ------------------------------------------------------------------------------------------------------ hook stubs
def make_stubs(device, target=6, eos=7, allowed=range(100, 164), mask=True):
    import enum
    import torch

    class State(enum.Enum):
        THINK_TAG = 1
        CODES_GENERATION = 2
        COMPLETED = 3

    class Processor:
        def __init__(self):
            self.enabled = True
            self.state = State.CODES_GENERATION
            self.codes_count = 0
            self.target_codes = target
            self.eos_token_id = eos
            self.codes_temperature = 0.9
            self.non_audio_code_mask = None
            if mask:
                m = torch.full((1, 1000), float("-inf"))
                m[0, list(allowed)] = 0
                m[0, eos] = 0
                self.non_audio_code_mask = m

        def __call__(self, ids, scores):
            if not self.enabled:
                return scores
            scores = scores.clone()
            if self.non_audio_code_mask is not None:
                scores = scores + self.non_audio_code_mask.to(scores.device)
            if self.target_codes is not None:
                if self.codes_count < self.target_codes:
                    scores[:, self.eos_token_id] = float("-inf")
                else:
                    keep = scores[:, self.eos_token_id].clone()
                    scores.fill_(float("-inf"))
                    scores[:, self.eos_token_id] = keep
            return scores / self.codes_temperature

        def update_state(self, token):
            if self.enabled and self.state == State.CODES_GENERATION:
                self.codes_count += 1

    class Tokenizer:
        eos_token_id = eos

    class Handler:
        llm = None
        llm_backend = "vllm"
        llm_tokenizer = Tokenizer()

        def __init__(self):
            self.device = device

        def _apply_top_k_filter(self, logits, top_k):
            if not top_k:
                return logits
            ranked = torch.sort(logits, dim=-1).values                   # ascending: the k-th largest sits k from the end
            floor = ranked[:, logits.shape[-1] - min(int(top_k), logits.shape[-1])].unsqueeze(-1)
            return torch.where(logits >= floor, logits, torch.full_like(logits, float("-inf")))

        def _apply_top_p_filter(self, logits, top_p):
            return logits

        def _sample_tokens(self, logits, temperature):
            if temperature > 0:
                return torch.multinomial(torch.softmax(logits.float() / temperature, dim=-1), 1).squeeze(1)
            return torch.argmax(logits, dim=-1)

    class Streamer:
        def __init__(self):
            self.n, self.ended = 0, False

        def put(self, x):
            self.n += 1

        def end(self):
            self.ended = True

    return Handler(), Processor, Streamer


def run_hook(bridge, device):
    import torch
    from acestep_mi355x.hook import install_lm_backend
    calls = []
    real = bridge.lm_generate

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    bridge.lm_generate = counted
    try:
        allowed = set(range(100, 164))
        prompt = torch.from_numpy(np.random.default_rng(2).integers(0, 1000, (1, 7)).astype(np.int64)).to(device)
        for cfg in (None, 2.0):
            h, Processor, Streamer = make_stubs(device)
            install_lm_backend(h, bridge, max_new_tokens=32, device_codes=True)
            ids = prompt if cfg is None else torch.cat([prompt, prompt.flip(1)], dim=0)
            proc = Processor()
            del calls[:]
            torch.manual_seed(4)
            if cfg is None:
                out = h._generate_with_constrained_decoding(ids, None, 32, 0.85, 8, 0.9, 1.1, 0, None, proc)
            else:
                out = h._generate_with_cfg_custom(ids, torch.ones_like(ids), 32, 0.85, cfg, 8, 0.9, 1.0, 0, None, proc)
            assert len(calls) == 1 and tuple(out.shape) == (ids.shape[0], 7 + 6 + 1) and out.dtype == ids.dtype
            gen = out[:, 7:].cpu().numpy()
            assert set(gen[:, :6].ravel().tolist()) <= allowed and gen[:, 6].tolist() == [7] * ids.shape[0]
            assert np.array_equal(out[:, :7].cpu().numpy(), ids.cpu().numpy()) and (gen == gen[0]).all()
            assert proc.codes_count == 6 and proc.state.name == "COMPLETED"
            torch.manual_seed(4)
            proc2 = Processor()
            again = h._generate_with_constrained_decoding(ids, None, 32, 0.85, 8, 0.9, 1.1, 0, None, proc2) if cfg is None \
                else h._generate_with_cfg_custom(ids, torch.ones_like(ids), 32, 0.85, cfg, 8, 0.9, 1.0, 0, None, proc2)
            assert torch.equal(out, again)                      # the torch seed picks the engine's stream
        # the fallbacks stay on the per-token path
        h, Processor, Streamer = make_stubs(device)
        install_lm_backend(h, bridge, max_new_tokens=32, device_codes=True)
        for what in ("no target", "no mask", "streamer", "no processor", "other state", "disabled"):
            proc, st = Processor(), None
            if what == "no target":
                proc.target_codes = None
            elif what == "no mask":
                proc.non_audio_code_mask = None
            elif what == "streamer":
                st = Streamer()
            elif what == "no processor":
                proc = None
            elif what == "disabled":
                proc.enabled = False
            else:
                proc.state = type(proc.state).THINK_TAG
            del calls[:]
            out = h._generate_with_constrained_decoding(prompt, None, 4 if what != "streamer" else 32, 0.0, None, None,
                                                        1.0, 0, st, proc)
            assert not calls, what
            if what == "streamer":
                assert tuple(out.shape) == (1, 14) and out[0, -1].item() == 7 and st.n == 7 and st.ended
                assert set(out[0, 7:13].tolist()) <= allowed and proc.codes_count == 7
            else:
                assert 8 <= out.shape[1] <= 11, what
        # the CFG loop with a scale that does not mix stays per token: the reference duplicates the batch all the same
        pair = torch.cat([prompt, prompt.flip(1)], dim=0)
        proc = Processor()
        del calls[:]
        out = h._generate_with_cfg_custom(pair, None, 32, 0.0, 1.0, None, None, 1.0, 0, None, proc)
        assert not calls and tuple(out.shape) == (2, 14) and out[:, -1].tolist() == [7, 7] and proc.codes_count == 7
        assert set(out[0, 7:13].tolist()) <= allowed and torch.equal(out[0, 7:], out[1, 7:])
        h2, _, _ = make_stubs(device)
        install_lm_backend(h2, bridge, max_new_tokens=32)           # the default leaves the handler's loops alone
        assert not hasattr(h2, "_generate_with_cfg_custom")
    finally:
        del bridge.lm_generate


def run_not_loaded(lib_path, device):
    """both entries before ace_mi_load_lm: ACE_GGML_ERR with the message the other LM entries give"""
    import pytest
    import torch
    from acestep_mi355x.capi import GGMLCAPIBridge
    br = GGMLCAPIBridge(lib_path=lib_path)
    try:
        logits = torch.zeros((1, 1000), dtype=torch.float32).to(device)
        with pytest.raises(RuntimeError, match=r"lm not loaded \(status=1\)"):
            br.lm_select(logits, uniforms=torch.zeros(1))
        with pytest.raises(RuntimeError, match=r"lm not loaded \(status=1\)"):
            br.lm_generate(logits, 2, seed=1)
    finally:
        br.close()
