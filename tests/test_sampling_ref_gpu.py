"""Device sampling (sampling.hip) against bit-level host references: single Gumbel variates
read back from the slot, whole seeded draws against argmax(l / T + G_ref) in float64
(tests/_philox.py), top-k / top-p threshold sets at their edges, vocabulary shards,
device-resident parameters, and the repeat-penalty / finalizer edge cases."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from _philox import N_MAX, draw_n, gumbel_ref
from _sampling_ref import expected_set, key_to_float, order_keys, split_slot
from cake_amd.ops import reference as R

pytestmark = pytest.mark.gpu

DEFAULT_SEED = 299792458
HI_SEED = (7 << 32) | 5
V_LLAMA = 128256
G_TOL = 1e-3  # an error eps in G changes a token's odds by e^eps: below 0.1 %

# (step, index) of the default seed at V_LLAMA whose 24-bit variate n is 2^24 - 1
# (u rounded to 1.0 and G to +inf before gumbel() clamped u), from a CPU scan of steps 0-699
HITS = [(165, 15064), (255, 84910), (478, 18028), (599, 56489)]
# further extremes of the same kind of scan: (seed, step, index, n)
EXTREMES = [(DEFAULT_SEED, 689, 65021, N_MAX), (DEFAULT_SEED, 149, 79986, 0),
            (DEFAULT_SEED, 383, 1442, 0), (DEFAULT_SEED, 634, 118718, 0),
            (1234, 32, 128157, N_MAX), (1234, 80, 66359, 0), (HI_SEED, 25, 43167, 0)]


def _i32(v, dev):
    return torch.tensor(v if isinstance(v, (list, tuple)) else [v], dtype=torch.int32, device=dev)


def _randn3(n, seed, dev="cpu"):
    """randn * 3 from a generator of its own: the suite's global RNG state stays as it was
    (later tests draw their inputs from it)."""
    return (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 3).to(dev)


def _state(dev, max_hist, step=0, guard=0):
    """slot, hist (max_hist usable entries), hist_len, tok, pos, thr of one decode state."""
    return dict(slot=torch.zeros(1, dtype=torch.int64, device=dev),
                hist=torch.zeros(max_hist + guard, dtype=torch.int32, device=dev)[:max_hist],
                hist_len=_i32(step, dev), tok=_i32(-1, dev), pos=_i32(step, dev),
                thr=torch.zeros(1, dtype=torch.int32, device=dev))


# ---------------------------------------------------------------------------
# a. single device Gumbel variates
# ---------------------------------------------------------------------------

def _triples():
    rng = np.random.default_rng(2024)
    t = [(int(i), int(s), int(seed)) for i, s, seed in zip(
        rng.integers(0, 2 ** 31 - 1, 240), rng.integers(0, 2 ** 31 - 1, 240),
        rng.integers(0, 2 ** 64, 240, dtype=np.uint64))]
    for seed in (DEFAULT_SEED, 1234, HI_SEED, 2 ** 64 - 1):
        t += [(i, s, seed) for i in (0, 1, V_LLAMA - 1, 2 ** 31 - 2) for s in (0, 1, 2 ** 20)]
    t += [(i, s, DEFAULT_SEED) for s, i in HITS]
    t += [(i, s, seed) for seed, s, i, _ in EXTREMES]
    # one step's scan: its largest and smallest n, the draws next to G = 0 (u = 1/e, where
    # the outer log's argument is next to 1), and the u closest to 1/2
    for seed, step in ((DEFAULT_SEED, 0), (HI_SEED, 3)):
        n = draw_n(np.arange(V_LLAMA), step, seed)
        g = gumbel_ref(np.arange(V_LLAMA), step, seed)
        picks = [n.argmax(), n.argmin(), np.abs(n - 2 ** 23).argmin(), *np.argsort(np.abs(g))[:4]]
        t += [(int(i), step, seed) for i in picks]
    return t


def test_device_gumbel_values(cuda):
    """select_shard on the one-element shard [0.0] at offset i with temperature 1 leaves
    ordered(0 + G_i) << 32 | ~i in the slot: the device's Gumbel variate of the Philox
    counter (i, step) and key seed, bit for bit.  Every one is finite, within 1e-3 of
    -log(-log(u)) in float64 (u as the kernel forms it), and carries its own index."""
    from cake_amd.ops import hip as K
    triples = _triples()
    for seed, s, i, n in EXTREMES:
        assert int(draw_n(i, s, seed)) == n
    for s, i in HITS:
        assert int(draw_n(i, s, DEFAULT_SEED)) == N_MAX
    m = len(triples)
    assert m >= 300
    logit = torch.zeros(1, device=cuda)
    hist = torch.zeros(1, dtype=torch.int32, device=cuda)
    steps = _i32([s for _, s, _ in triples], cuda)
    slots = torch.zeros(m, dtype=torch.int64, device=cuda)
    for j, (i, _, seed) in enumerate(triples):
        K.select_shard(logit, i, hist, steps[j:j + 1], 0, 1.0, 1.0, seed, slots[j:j + 1])
    torch.cuda.synchronize()
    assert float(logit) == 0.0
    hi, idx = split_slot(slots)
    g_dev = np.array([key_to_float(k) for k in hi], dtype=np.float64)
    g_ref = np.array([float(gumbel_ref(i, s, seed)) for i, s, seed in triples])
    assert np.isfinite(g_ref).all()
    err = np.abs(g_dev - g_ref)
    worst = int(np.nanargmax(np.where(np.isfinite(err), err, np.inf)))
    print(f"\nmax |G_dev - G_ref| = {err[worst]:.3e} at (i, step, seed) = {triples[worst]}, "
          f"G_ref = {g_ref[worst]:.6f}; G range [{g_ref.min():.3f}, {g_ref.max():.3f}]")
    bad = [(triples[j], g_dev[j], g_ref[j]) for j in range(m)
           if not (np.isfinite(g_dev[j]) and err[j] <= G_TOL)]
    assert not bad, bad[:8]
    assert idx.tolist() == [i for i, _, _ in triples]


# ---------------------------------------------------------------------------
# b. whole draws
# ---------------------------------------------------------------------------

def _draw(K, logits, cfg, steps, first_step=0):
    """steps device draws through select_token in a plain loop; the history length is the
    Philox step, so every draw is a fresh one.  Returns the drawn tokens."""
    st = _state(logits.device, first_step + steps, step=first_step)
    for _ in range(steps):
        K.select_token(logits, st["slot"], st["hist"], st["hist_len"], st["tok"], st["pos"], cfg,
                       st["thr"])
    torch.cuda.synchronize()
    assert int(st["hist_len"]) == first_step + steps
    return st["hist"][first_step:].cpu().numpy().astype(np.int64)


def _check_draws(logits, T, seed, toks, keep=None, first_step=0):
    """Every token against argmax(l / T + G_ref) in float64 (over keep, if given).  The
    device's score l * (1 / T) + G is off by at most eps = 1e-3 (the G bound) +
    max|l| / T * 2^-22 (f32 rounding of 1 / T, of the product and of the sum), so it can
    prefer d to the reference's r only when score_r - score_d < 2 eps: such steps are
    excused and counted; any other mismatch fails.  Returns the excused share."""
    l64 = logits.cpu().numpy().astype(np.float64)
    V = l64.size
    idx = np.arange(V) if keep is None else np.nonzero(keep.numpy())[0]
    base = l64[idx] / T
    bound = 2 * (G_TOL + float(np.abs(l64[np.isfinite(l64)]).max()) / T * 2.0 ** -22)

    def one(j):
        sc = base + gumbel_ref(idx, first_step + j, seed)
        r = int(np.argmax(sc))
        margin = float(sc[r] - np.delete(sc, r).max())  # the reference's top-two margin
        d = np.nonzero(idx == toks[j])[0]
        if d.size == 0:
            return j, int(idx[r]), margin, np.inf  # outside the set
        return j, int(idx[r]), margin, float(sc[r] - sc[d[0]])

    with ThreadPoolExecutor(8) as ex:  # numpy releases the GIL in the Philox rounds
        res = list(ex.map(one, range(len(toks))))
    excused, wrong = 0, []
    for j, r, margin, gap in res:
        if toks[j] == r:
            continue
        if margin < bound and gap < bound:
            excused += 1
        else:
            wrong.append((first_step + j, int(toks[j]), r, margin, gap))
    assert not wrong, (wrong[:8], bound)
    return excused / len(toks)


def test_draws_match_reference_small_vocab(cuda):
    from cake_amd.models.sampling import SamplingConfig
    from cake_amd.ops import hip as K
    V, T, seed, n = 1000, 0.8, 1234, 2000
    logits = _randn3(V, 3, cuda)
    toks = _draw(K, logits, SamplingConfig(temperature=T, seed=seed), n)
    share = _check_draws(logits, T, seed, toks)
    print(f"\nexcused share V={V}: {share:.4f}")
    assert share <= 0.02
    assert len(set(toks.tolist())) > 50  # draws, not one token


def test_draws_match_reference_llama_vocab(cuda):
    """Default seed, steps 0-299: steps 165 and 255 hold the counters whose u rounded to
    1.0 (G = +inf: the token won whatever its logit).  Their logits are -30 here, so they
    must never be drawn."""
    from cake_amd.models.sampling import SamplingConfig
    from cake_amd.ops import hip as K
    V, T, n = V_LLAMA, 1.0, 300
    logits = _randn3(V, 4, cuda)
    logits[15064] = -30.0
    logits[84910] = -30.0
    cfg = SamplingConfig(temperature=T)
    assert cfg.seed == DEFAULT_SEED
    toks = _draw(K, logits, cfg, n)
    assert 15064 not in toks.tolist() and 84910 not in toks.tolist(), \
        (int(toks[165]), int(toks[255]))
    share = _check_draws(logits, T, cfg.seed, toks)
    print(f"\nexcused share V={V}: {share:.4f}")
    assert share <= 0.02


def test_draws_match_reference_top_k_top_p(cuda):
    from cake_amd.models.sampling import SamplingConfig
    from cake_amd.ops import hip as K
    V, T, seed, n = 1000, 0.8, 1234, 400
    logits = _randn3(V, 5, cuda)
    cfg = SamplingConfig(temperature=T, top_k=40, top_p=0.9, seed=seed)
    toks = _draw(K, logits, cfg, n, first_step=7)
    keep = expected_set(logits.cpu(), T, 40, 0.9)
    assert 1 < int(keep.sum()) <= 40
    assert keep[torch.from_numpy(toks)].all()
    share = _check_draws(logits, T, seed, toks, keep=keep, first_step=7)
    print(f"\nexcused share top-k/top-p: {share:.4f}")
    assert share <= 0.02
    assert len(set(toks.tolist())) > 3


# ---------------------------------------------------------------------------
# c. threshold sets at the edges
# ---------------------------------------------------------------------------

def _logits(kind, V):
    g = torch.Generator().manual_seed(V * 7 + len(kind))
    x = torch.randn(V, generator=g) * 3
    if kind == "ties":  # multiples of 0.25: dense ties (+ 0.0: no -0.0, whose key is below +0.0's)
        return torch.round(x * 4) / 4 + 0.0
    if kind == "equal":
        return torch.full((V,), 1.5)
    if kind == "neginf":
        x[torch.randperm(V, generator=g)[:V // 4]] = float("-inf")
        return x
    if kind == "negative":
        return -x.abs() - 1.0
    if kind == "huge":
        return torch.where(x > 0, torch.tensor(1e4), torch.tensor(-1e4))
    assert kind == "randn"
    return x


def _mid_p(logits, T, k, p0):
    """A top-p next to p0 that sits on no rounding boundary: the midpoint of the two
    consecutive distinct-value cumulative masses (float64, descending, over the host's
    top-k tokens, full-vocabulary probabilities) that enclose p0."""
    probs = torch.softmax(logits.double() / T, 0)
    vals = logits
    if k:
        top = torch.topk(logits, k).indices
        probs, vals = probs[top], logits[top]
    uv, inv = torch.unique(vals, return_inverse=True)  # ascending
    mass = torch.zeros(uv.numel(), dtype=torch.float64).index_add_(0, inv, probs).flip(0)
    cum = torch.cumsum(mass, 0)
    cum = cum[torch.cat([torch.tensor([True]), cum[1:] > cum[:-1]])]  # distinct masses
    j = int(torch.searchsorted(cum, torch.tensor(p0, dtype=torch.float64), right=True))
    j = min(j, cum.numel() - 1)
    lo = float(cum[j - 1]) if j else 0.0
    p = float(np.float32(0.5 * (lo + min(float(cum[j]), 1.0))))
    assert lo < p < float(cum[j]) and 0.0 < p < 1.0, (lo, p, float(cum[j]))
    return p


def _threshold_case(K, dev, logits, T, k, p0):
    p = _mid_p(logits, T, k, p0) if p0 is not None else None
    thr = torch.zeros(1, dtype=torch.int32, device=dev)
    K.sample_threshold(logits.to(dev), T, k, p, thr)
    got = torch.from_numpy(order_keys(logits) >= (int(thr.item()) & 0xFFFFFFFF))
    host = expected_set(logits, T, k, p)
    exp = logits >= logits[host].min()  # closure over ties with the last kept token
    if torch.equal(got, exp):
        return None
    return dict(T=T, k=k, p=p, got=int(got.sum()), exp=int(exp.sum()), host=int(host.sum()))


def _kp_cases(V):
    ks = sorted({k for k in (1, V - 1, V) if k >= 1})
    return [(k, None) for k in ks] + [(None, p) for p in (1e-6, 0.5, 0.999)] + \
        [(min(40, V), 0.5), (min(40, V), 0.999)]


@pytest.mark.parametrize("T", [0.05, 0.8, 5.0])
@pytest.mark.parametrize("kind", ["ties", "equal", "neginf", "negative", "huge"])
def test_threshold_set_edges(cuda, kind, T):
    """The device keeps every token whose logit ties with the last kept one, so the
    expected set is the closure {i : l_i >= l_J}, J being the last (lowest) token the
    float64 host rule (expected_set) keeps; without ties that is the host set itself.
    k in {1, V - 1, V}, p next to {1e-6, 0.5, 0.999} (see _mid_p), and both."""
    from cake_amd.ops import hip as K
    logits = _logits(kind, 4096)
    bad = [c for c in (_threshold_case(K, cuda, logits, T, k, p) for k, p in _kp_cases(4096)) if c]
    assert not bad, bad


@pytest.mark.parametrize("V", [1, 2, 1023, 1024, 1025, 4096])
def test_threshold_set_vocab_sizes(cuda, V):
    """Around the 1024-thread workgroup of the threshold kernel, same closure rule."""
    from cake_amd.ops import hip as K
    bad = []
    for kind in ("randn", "ties"):
        logits = _logits(kind, V)
        bad += [dict(c, kind=kind) for c in
                (_threshold_case(K, cuda, logits, 0.8, k, p) for k, p in _kp_cases(V)) if c]
    assert not bad, bad


# ---------------------------------------------------------------------------
# d. vocabulary shards
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("T", [0.0, 0.7])
def test_shards_equal_full_vector(cuda, T):
    """Three uneven shards into one slot leave the key of the whole vector's argmax /
    Gumbel-max (global Philox counter), and the shards' penalties (history ids at every
    shard's off - 1, off, off + V - 1, off + V, repeated, and beyond the vocabulary) add
    up to apply_repeat_penalty of the full vector."""
    from cake_amd.ops import hip as K
    V, seed, pen = 5000, HI_SEED, 1.3
    bounds = [0, 1000, 1001, V]
    full = _randn3(V, 9)
    full[999] = 0.0    # penalised zero stays +0.0
    full[1000] = -2.0  # the one-token shard, penalised negative logit
    ids = [0, 999, 1000, 1001, V - 1, V, V + 7, 2 ** 31 - 1, 999, 1000, 1000, 0, 2500, V - 1, 1]
    hist = torch.zeros(64, dtype=torch.int32, device=cuda)
    hist[:len(ids)] = torch.tensor(ids, dtype=torch.int32)
    hist_len = _i32(len(ids), cuda)
    last_n = len(ids) - 1  # the leading 0 is outside the window, the later 0 inside
    ref = R.apply_repeat_penalty(full, pen, ids[-last_n:])
    assert not torch.equal(ref, full)
    slot = torch.zeros(1, dtype=torch.int64, device=cuda)
    shards = [full[a:b].clone().to(cuda) for a, b in zip(bounds, bounds[1:])]
    for sh, off in zip(shards, bounds):
        K.select_shard(sh, off, hist, hist_len, last_n, pen, T, seed, slot)
    got = torch.cat(shards).cpu()
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
    whole = torch.zeros(1, dtype=torch.int64, device=cuda)
    if T > 0:
        K.gumbel_argmax(ref.to(cuda), T, seed, hist_len, whole)
    else:
        K.argmax(ref.to(cuda), whole)
    assert int(slot) == int(whole) and int(slot) != 0
    key, idx = split_slot(slot)
    assert 0 <= int(idx[0]) < V
    if T > 0:
        sc = ref.double().numpy() / T + gumbel_ref(np.arange(V), len(ids), seed)
        eps = G_TOL + float(ref.abs().max()) / T * 2.0 ** -22  # as in _check_draws
        assert sc.max() - sc[int(idx[0])] < 2 * eps
        assert abs(key_to_float(key[0]) - sc[int(idx[0])]) < eps
    else:
        assert int(idx[0]) == int(torch.argmax(ref))


# ---------------------------------------------------------------------------
# e. device-resident parameters
# ---------------------------------------------------------------------------

def _configs():
    from cake_amd.models.sampling import SamplingConfig as S
    return {"greedy": S(temperature=0.0), "none": S(temperature=None),
            "temperature": S(temperature=0.7, seed=11),
            "k": S(temperature=0.9, top_k=12, seed=12),
            "p": S(temperature=1.2, top_p=0.85, seed=13),
            "kp": S(temperature=0.8, top_k=40, top_p=0.9, seed=14),
            "seed_hi": S(temperature=1.0, seed=(3 << 32) | 9),
            "seed_hi_kp": S(temperature=0.6, top_k=30, top_p=0.95, seed=2 ** 64 - 3)}


@pytest.mark.parametrize("name", list(_configs()))
def test_device_params_match_launch_arguments(cuda, name):
    """select_token(params=...) reads temperature / top_k / top_p / seed on the device:
    same threshold and same tokens as the launch-argument path, step after step."""
    from cake_amd.ops import hip as K
    cfg = _configs()[name]
    logits = _randn3(5000, 21, cuda)
    params = K.sample_params_tensor(cfg, cuda)
    a, b = _state(cuda, 64, step=17), _state(cuda, 64, step=17)
    for step in range(6):
        K.select_token(logits, a["slot"], a["hist"], a["hist_len"], a["tok"], a["pos"], cfg,
                       a["thr"])
        K.select_token(logits, b["slot"], b["hist"], b["hist_len"], b["tok"], b["pos"], None,
                       b["thr"], params=params)
        for f in ("tok", "thr", "hist", "hist_len", "pos", "slot"):
            assert torch.equal(a[f], b[f]), (step, f, a[f][:24], b[f][:24])
    toks = a["hist"][17:23].tolist()
    if cfg.greedy:
        assert toks == [int(torch.argmax(logits))] * 6 and int(b["thr"]) == 0
    else:
        assert len(set(toks)) > 1
        keep = expected_set(logits.cpu(), cfg.temperature, cfg.top_k, cfg.top_p)
        assert keep[toks].all()
        if cfg.top_k or cfg.top_p:
            got = order_keys(logits) >= (int(b["thr"]) & 0xFFFFFFFF)
            assert torch.equal(torch.from_numpy(got), keep)


# ---------------------------------------------------------------------------
# f. repeat penalty and finalizer edges
# ---------------------------------------------------------------------------

def _penalty_case(K, dev, logits, ids, last_n, pen):
    hist = torch.zeros(max(len(ids), 1) + 8, dtype=torch.int32, device=dev)
    if ids:
        hist[:len(ids)] = torch.tensor(ids, dtype=torch.int32)
    dev_logits = logits.clone().to(dev)
    K.repeat_penalty(dev_logits, hist, _i32(len(ids), dev), last_n, pen)
    ref = R.apply_repeat_penalty(logits, pen, ids[max(0, len(ids) - last_n):])
    assert torch.equal(dev_logits.cpu().view(torch.int32), ref.view(torch.int32))
    return ref


def test_repeat_penalty_window_edges(cuda):
    """A window wider than the kernel's 256 threads over a history full of repeats (each
    unique token is penalised once), tokens only outside the window, a window longer than
    the history, an empty history, and penalised logits of +0.0, -0.0 and below zero."""
    from cake_amd.ops import hip as K
    V, pen = 1000, 1.3
    logits = _randn3(V, 13)
    logits[3], logits[4], logits[5] = 0.0, -0.0, -2.5
    g = torch.Generator().manual_seed(1)
    ids = list(range(900, 1000))                              # outside the 600 window
    ids += torch.randint(0, 40, (500,), generator=g).tolist()  # heavy duplication
    ids += [3, 4, 5, 3, 4, 5] + torch.randint(0, 700, (94,), generator=g).tolist()
    assert len(ids) == 700
    ref = _penalty_case(K, cuda, logits, ids, 600, pen)
    assert torch.equal(ref[900:], logits[900:]) and not torch.equal(ref[:40], logits[:40])
    assert float(ref[5]) == pytest.approx(-2.5 * 1.3) and float(ref[3]) == 0.0
    assert ref.view(torch.int32)[3] == 0 and ref.view(torch.int32)[4] == -2 ** 31  # +0.0, -0.0
    # the same token in every one of 600 places is still penalised once
    once = _penalty_case(K, cuda, logits, [7] * 700, 600, pen)
    assert float(once[7]) == float(R.apply_repeat_penalty(logits, pen, [7])[7])
    # last_n > hist_len: the whole history, nothing before it
    _penalty_case(K, cuda, logits, ids[:10], 600, pen)
    _penalty_case(K, cuda, logits, ids[100:400], 10 ** 6, pen)
    # empty history: untouched
    assert torch.equal(_penalty_case(K, cuda, logits, [], 600, pen), logits)


@pytest.mark.parametrize("push", [False, True])
def test_full_history_is_not_overrun(cuda, push):
    """hist_len == hist.numel(): tok and pos still update, the history and its length stay,
    and the element after the history is not written."""
    from cake_amd.ops import hip as K
    n = 16
    st = _state(cuda, n, step=n, guard=1)
    backing = st["hist"]._base if st["hist"]._base is not None else st["hist"]
    assert backing.numel() == n + 1 and st["hist"].numel() == n
    backing.copy_(torch.arange(100, 100 + n + 1, dtype=torch.int32))
    before = backing.clone()
    if push:
        K.push_token(_i32(42, cuda), st["tok"], st["hist"], st["hist_len"], st["pos"])
    else:
        key = (0xBF800000 << 32) | (0xFFFFFFFF - 42)  # ordered(1.0f) << 32 | ~42
        st["slot"].fill_(key - 2 ** 64)
        K.finalize_token(st["slot"], st["tok"], st["hist"], st["hist_len"], st["pos"])
        assert int(st["slot"]) == 0
    assert int(st["tok"]) == 42 and int(st["pos"]) == n + 1
    assert int(st["hist_len"]) == n
    assert torch.equal(backing, before)
    # one below full: the last entry is written, then the guard holds
    st["hist_len"].fill_(n - 1)
    if push:
        K.push_token(_i32(43, cuda), st["tok"], st["hist"], st["hist_len"], st["pos"])
    else:
        st["slot"].fill_((0xBF800000 << 32 | (0xFFFFFFFF - 43)) - 2 ** 64)
        K.finalize_token(st["slot"], st["tok"], st["hist"], st["hist_len"], st["pos"])
    assert int(st["hist_len"]) == n and int(backing[n - 1]) == 43 and int(st["tok"]) == 43
    assert int(backing[n]) == 100 + n and torch.equal(backing[:n - 1], before[:n - 1])
