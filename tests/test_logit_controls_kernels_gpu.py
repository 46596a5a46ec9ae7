"""cake_logit_controls (logit_controls.hip) through ops/hip.py against ops/reference.py's
logit_controls_ref.

Judged bit for bit: the adjusted row, the count table (the histogram of generated), the
counted word, the key of the adjusted row's maximum and the min_p cut key.  No element is
excluded; the words around the row are checked untouched."""
import numpy as np
import pytest
import torch

from _philox import gumbel_ref
from cake_amd.ops.reference import logit_controls_ref, ordered_key

pytestmark = pytest.mark.gpu

VS = [1, 3, 255, 256, 257, 1000, 4099]
PAD = 777.0


def _bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _row(V: int, seed: int) -> np.ndarray:
    """Random logits on a 1/64 grid (products and sums with the dyadic penalties below are
    still rounded by the kernel: the oracle is float32, not exact arithmetic)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(V, generator=g) * 3).to(torch.float32).numpy()


def _generated(V: int, n: int, seed: int) -> list[int]:
    """n tokens with repeats, id 0 and id V - 1 among them."""
    if n == 0:
        return []
    rng = np.random.default_rng(seed)
    pool = np.unique(np.concatenate([[0, V - 1], rng.integers(0, V, size=max(1, n // 3))]))
    out = rng.choice(pool, size=n).tolist()
    out[0] = 0
    out[-1] = V - 1
    return [int(t) for t in out]


class State:
    """Device state of one generation: history = prompt + generated, table, blocks."""

    def __init__(self, dev, V, prompt, cap=512, off=0):
        self.dev, self.V, self.off = dev, V, off
        self.gen0 = len(prompt)
        self.hist = torch.zeros(cap, dtype=torch.int32, device=dev)
        self.hist[:len(prompt)] = torch.tensor(prompt, dtype=torch.int32)
        self.hl = torch.tensor([len(prompt)], dtype=torch.int32, device=dev)
        self.cnt = torch.zeros(V, dtype=torch.int32, device=dev)
        self.state = torch.zeros(68, dtype=torch.int32, device=dev)
        self.state[1] = self.gen0
        self.buf = torch.full((V + off + 8,), PAD, dtype=torch.float32, device=dev)
        self.params = None

    def set_params(self, presence=0.0, frequency=0.0, bias=None, min_p=None, temperature=0.0):
        from cake_amd.ops import hip
        self.params = hip.pack_logit_controls(presence, frequency, bias, min_p, temperature,
                                              self.gen0).to(self.dev)

    def push(self, toks):
        n = int(self.hl)
        self.hist[n:n + len(toks)] = torch.tensor(toks, dtype=torch.int32)
        self.hl.fill_(n + len(toks))

    def run(self, x: np.ndarray, mb: int = 0) -> np.ndarray:
        from cake_amd.ops import hip
        self.buf.fill_(PAD)
        row = self.buf[self.off:self.off + self.V]
        row.copy_(torch.from_numpy(x))
        hip.logit_controls(row, self.hist, self.hl, self.cnt, self.params, self.state, mb)
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        assert (b[:self.off] == PAD).all() and (b[self.off + self.V:] == PAD).all()
        return b[self.off:self.off + self.V].copy()


def _judge(st: State, got: np.ndarray, x, generated, what, **kw):
    ref, cut = logit_controls_ref(x, generated, kw.get("presence", 0.0), kw.get("frequency", 0.0),
                                  kw.get("bias"), kw.get("min_p"), kw.get("temperature", 0.0))
    ref = ref.numpy()
    assert np.array_equal(_bits(got), _bits(ref)), (what, np.nonzero(_bits(got) != _bits(ref))[0][:8])
    cnt = st.cnt.cpu().numpy()
    assert np.array_equal(cnt, np.bincount(np.asarray(generated, dtype=np.int64),
                                           minlength=st.V)), what
    s = st.state.cpu().numpy().view(np.uint32)
    assert s[0] == 0, what                                   # the ticket is left re-armed
    assert s[1] == st.gen0 + len(generated), what            # counted
    assert s[2] == (0 if cut is None else cut), (what, hex(s[2]), cut)
    assert s[3] == ordered_key(ref).max(), what
    return ref, cut


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("V", VS)
def test_rows(cuda, V, off):
    """Every row length on an aligned row and one offset by an element: empty, one-token and
    37-token histories, presence + frequency with a bias list of counted and uncounted ids."""
    x = _row(V, V)
    for n in (0, 1, 37):
        gen = _generated(V, n, V + n)
        ids = sorted({0, V - 1, V // 2, V // 3})
        bias = {i: (4.0 if j % 2 else -3.5) for j, i in enumerate(ids)}
        kw = dict(presence=0.25, frequency=0.5, bias=bias, min_p=0.2, temperature=0.8)
        st = State(cuda, V, [V - 1, 0, 0], off=off)     # prompt tokens that generated repeats
        st.set_params(**kw)
        st.push(gen)
        got = st.run(x)
        _judge(st, got, x, gen, f"V {V} off {off} n {n}", **kw)


def test_llama_vocab(cuda):
    V = 128256
    x = _row(V, 7)
    gen = _generated(V, 37, 11)
    rng = np.random.default_rng(5)
    ids = list(dict.fromkeys([0, V - 1, gen[5]] + rng.choice(V, size=300, replace=False).tolist()))
    bias = {int(i): float(np.float32(rng.uniform(-100, 100))) for i in ids[:300]}
    kw = dict(presence=-0.5, frequency=1.25, bias=bias, min_p=0.05, temperature=1.3)
    for mb in (0, 3):   # the default grid (one piece per workgroup) and slices of many pieces
        st = State(cuda, V, [5, 6, 7, gen[0]])
        st.set_params(**kw)
        st.push(gen)
        _judge(st, st.run(x, mb), x, gen, f"llama vocab max_blocks {mb}", **kw)


@pytest.mark.parametrize("kw", [dict(presence=0.75), dict(frequency=0.3), dict(presence=-1.5, frequency=-0.1),
                                dict(presence=2.0, frequency=2.0), dict()],
                         ids=["presence", "frequency", "negative", "max", "neutral"])
@pytest.mark.parametrize("n_bias", [0, 1, 300])
def test_penalties_and_bias(cuda, kw, n_bias):
    V = 1000
    x = _row(V, 3)
    gen = _generated(V, 37, 4)
    rng = np.random.default_rng(n_bias)
    ids = [gen[3]] + [int(i) for i in rng.permutation(V) if i != gen[3]]   # a counted id first
    bias = {i: float(np.float32(rng.uniform(-100, 100))) for i in ids[:n_bias]}
    st = State(cuda, V, [1, 2])
    st.set_params(bias=bias, **kw)
    st.push(gen)
    _judge(st, st.run(x), x, gen, f"{kw} n_bias {n_bias}", bias=bias, **kw)


def test_successive_calls_and_reset(cuda):
    """hist_len growing by 1 per call and once by 5 on one table equals the one-shot oracle at
    every call; a call without new entries (the engine's warm step) counts nothing twice; a
    second generation starts from a cleared table."""
    V = 257
    kw = dict(presence=0.5, frequency=0.25, bias={0: 1.0, 256: -2.0})
    gen = _generated(V, 16, 9)
    st = State(cuda, V, [256, 3])
    st.set_params(**kw)
    done = 0
    for step, grow in enumerate([0, 1, 1, 0, 1, 5, 1, 1, 0, 6]):
        st.push(gen[done:done + grow])
        done += grow
        x = _row(V, 100 + step)
        _judge(st, st.run(x), x, gen[:done], f"call {step}", **kw)
    assert done == len(gen)
    # second generation: another prompt length, the caller clears the table and sets counted
    st2_gen = _generated(V, 5, 10)
    st.hl.fill_(4)
    st.gen0 = 4
    st.cnt.zero_()
    st.state[1] = 4
    st.set_params(**kw)
    st.push(st2_gen)
    x = _row(V, 200)
    _judge(st, st.run(x), x, st2_gen, "second generation", **kw)


def test_back_to_back_launches(cuda):
    """Four launches on one stream with no host reset or synchronisation in between: the ticket
    and maximum words are left clean by every launch."""
    from cake_amd.ops import hip
    V = 4099
    kw = dict(presence=0.25, frequency=0.5, bias={7: 3.0}, min_p=0.3, temperature=0.7)
    gen = _generated(V, 8, 2)
    st = State(cuda, V, [1])
    st.set_params(**kw)
    rows = [_row(V, 300 + i) for i in range(4)]
    bufs = [torch.from_numpy(r).to(cuda) for r in rows]
    hls = [torch.tensor([1 + 2 * (i + 1)], dtype=torch.int32, device=cuda) for i in range(4)]
    st.hist[1:9] = torch.tensor(gen, dtype=torch.int32)
    states = []
    for i in range(4):
        hip.logit_controls(bufs[i], st.hist, hls[i], st.cnt, st.params, st.state)
        states.append(st.state.clone())       # stream-ordered copy
    torch.cuda.synchronize()
    for i in range(4):
        g = gen[:2 * (i + 1)]
        ref, cut = logit_controls_ref(rows[i], g, 0.25, 0.5, {7: 3.0}, 0.3, 0.7)
        assert np.array_equal(_bits(bufs[i].cpu().numpy()), _bits(ref.numpy())), i
        s = states[i].cpu().numpy().view(np.uint32)
        assert (s[0], s[1], s[2]) == (0, 1 + len(g), cut), i
    assert np.array_equal(st.cnt.cpu().numpy(), np.bincount(gen, minlength=V))


def test_min_p_cut(cuda):
    """Elements exactly at the cut are kept, one ulp below dropped; min_p = 1 keeps exactly the
    maxima (also a maximum of -0.0, whose cut +0.0 is clamped to the maximum's key); greedy and
    min_p off produce no restriction."""
    from cake_amd.ops.reference import min_p_offset
    V, T, mp = 1000, 0.5, 0.25
    d = np.float32(min_p_offset(T, mp))
    x = np.full(V, -20.0, dtype=np.float32)
    x[17] = 6.0
    cut = np.float32(np.float32(6.0) + d)
    x[100], x[999] = cut, cut
    x[101] = np.nextafter(cut, np.float32(-np.inf))
    x[0] = np.nextafter(cut, np.float32(np.inf))
    st = State(cuda, V, [1])
    st.set_params(min_p=mp, temperature=T)
    _, key = _judge(st, st.run(x), x, [], "cut", min_p=mp, temperature=T)
    keep = ordered_key(x) >= key
    assert sorted(np.nonzero(keep)[0].tolist()) == [0, 17, 100, 999]
    # the cut follows the adjusted row: a bias moves the maximum
    st.set_params(min_p=mp, temperature=T, bias={500: 40.0})
    _judge(st, st.run(x), x, [], "cut after bias", min_p=mp, temperature=T, bias={500: 40.0})
    for name, row in (("ties", np.where(np.arange(V) % 250 == 3, 2.5, -1.0).astype(np.float32)),
                      ("negative zero", np.where(np.arange(V) == 9, -0.0, -1.0).astype(np.float32)),
                      ("both zeros", np.where(np.arange(V) < 2, [0.0, -0.0] * (V // 2), -1.0)
                       .astype(np.float32))):
        st.set_params(min_p=1.0, temperature=T)
        _, key = _judge(st, st.run(row), row, [], name, min_p=1.0, temperature=T)
        assert np.array_equal(ordered_key(row) >= key, ordered_key(row) == ordered_key(row).max()), name
    for kw in (dict(min_p=mp, temperature=0.0), dict(min_p=None, temperature=T),
               dict(min_p=0.0, temperature=T)):
        st.set_params(**kw)
        _, key = _judge(st, st.run(x), x, [], str(kw), **kw)
        assert key is None


@pytest.mark.parametrize("seed", [1, 1234, 299792458])
def test_min_p_draw(cuda, seed):
    """cake_gumbel_argmax fed the produced cut key draws argmax(x / T + G) over the oracle's
    set (float64 reference; a step whose top two reference scores are closer than the device's
    score error 2 (1e-3 + max|x| / T 2^-22) may pick either of them).  Also merged with a
    top-k threshold: the larger key."""
    from cake_amd.ops import hip
    V, T, mp = 4099, 0.8, 0.1
    x = _row(V, 21)
    st = State(cuda, V, [1, 2, 3])
    st.set_params(min_p=mp, temperature=T)
    got = st.run(x)
    ref, cut = logit_controls_ref(x, [], min_p=mp, temperature=T)
    assert np.array_equal(_bits(got), _bits(x)) and st.state.cpu().numpy().view(np.uint32)[2] == cut
    keep = np.nonzero(ordered_key(x) >= cut)[0]
    assert 1 < keep.size < V
    slot = torch.zeros(1, dtype=torch.int64, device=cuda)
    row = torch.from_numpy(x).to(cuda)
    bound = 2 * (1e-3 + float(np.abs(x).max()) / T * 2.0 ** -22)
    for step in range(8):
        slot.zero_()
        hl = torch.tensor([step], dtype=torch.int32, device=cuda)
        hip.gumbel_argmax(row, T, seed, hl, slot, st.state[2:3])
        tok = 0xFFFFFFFF - (int(slot.cpu().numpy().view(np.uint64)[0]) & 0xFFFFFFFF)
        sc = x[keep].astype(np.float64) / T + gumbel_ref(keep, step, seed)
        order = np.argsort(-sc)
        assert tok in keep, (step, tok)
        if sc[order[0]] - sc[order[1]] >= bound:
            assert tok == keep[order[0]], (step, tok, keep[order[0]])
        else:
            assert tok in (keep[order[0]], keep[order[1]]), (step, tok)
    # merged with top-k: the effective threshold is the larger key
    thr = torch.zeros(1, dtype=torch.int32, device=cuda)
    for k in (3, 2000):
        hip.sample_threshold(row, T, k, None, thr)
        kthr = int(thr.cpu().numpy().view(np.uint32)[0])
        hip.logit_controls_merge_thr(thr, st.state[2:3])
        assert int(thr.cpu().numpy().view(np.uint32)[0]) == max(kthr, cut), k
