"""cake_lse_rows / cake_lse_finish (score.hip) through ops/hip.py against the float64
reference of tests/_score.py.

Judged by: the target logit and the argmax logit bit-equal to the input, the argmax id equal
to the float64 argmax (lowest id at ties), |lse - ref64| <= 2^-24 (|ref64| + 128).  No
element is excluded."""
import numpy as np
import pytest
import torch

import _score as S

pytestmark = pytest.mark.gpu


def _bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class State:
    def __init__(self, T, dev):
        self.run_max = torch.empty(T, dtype=torch.float32, device=dev)
        self.run_sum = torch.empty(T, dtype=torch.float64, device=dev)
        self.tgt = torch.empty(T, dtype=torch.float32, device=dev)
        self.key = torch.empty(T, dtype=torch.int64, device=dev)
        self.lse = torch.empty(T, dtype=torch.float32, device=dev)
        self.top = torch.empty(T, dtype=torch.int32, device=dev)
        self.topv = torch.empty(T, dtype=torch.float32, device=dev)


def _run(dev, x: np.ndarray, target: np.ndarray, chunks, pad: int = 0, state: State = None):
    """The launch sequence over `chunks` in the order given; `pad` extra columns per row make
    ld larger than the chunk.  Returns numpy (lse, tgt, top, topv)."""
    from cake_amd.ops import hip
    T, V = x.shape
    buf = torch.full((T, V + pad), 12345.0, dtype=torch.float32, device=dev)
    buf[:, :V] = torch.from_numpy(x).to(dev)
    s = state or State(T, dev)
    tg = torch.from_numpy(np.asarray(target, dtype=np.int32)).to(dev)
    for i, (v0, vc) in enumerate(chunks):
        hip.lse_rows(buf[:, v0:v0 + vc], v0, i == 0, tg, s.run_max, s.run_sum, s.tgt, s.key)
    hip.lse_finish(s.run_max, s.run_sum, s.key, s.lse, s.top, s.topv)
    torch.cuda.synchronize()
    return s.lse.cpu().numpy(), s.tgt.cpu().numpy(), s.top.cpu().numpy(), s.topv.cpu().numpy()


def _judge(x, target, got, what):
    lse, tgt, top, topv = got
    T = x.shape[0]
    rl, rt, rtop, rmax = S.lse_ref(x.astype(np.float64), target)
    has = np.asarray(target) >= 0
    assert np.array_equal(_bits(tgt[has]), _bits(rt[has].astype(np.float32))), what
    assert np.isnan(tgt[~has]).all(), what
    assert np.array_equal(top.astype(np.int64), rtop), what
    assert np.array_equal(_bits(topv), _bits(x[np.arange(T), rtop])), what
    fin = np.isfinite(rl)
    err = np.abs(lse[fin].astype(np.float64) - rl[fin])
    worst = float((err / S.lse_bound(rl[fin])).max()) if fin.any() else 0.0
    print(f"{what}: lse error / bound, worst row: {worst:.3f}")
    assert (err <= S.lse_bound(rl[fin])).all(), (what, worst)
    assert np.array_equal(lse[~fin], rl[~fin].astype(np.float32)), what   # -inf rows
    assert not np.isnan(lse).any() and not np.isnan(topv).any(), what


# every (T, V, chunking) but those whose chunk exceeds V
GRID = [(T, V, c) for T in S.TS for V in S.VS for c in S.CHUNKINGS
        if S.chunks_of(V, c) is not None]


@pytest.mark.parametrize("T,V,chunking", GRID)
def test_grid(cuda, T, V, chunking):
    chunks = S.chunks_of(V, chunking)
    pad = 3 if chunking == "strided" else 0   # an odd ld: every row base aligned differently
    target = S.random_targets(T, V)
    for family in S.FAMILIES:
        x = S.family_logits(family, T, V)
        _judge(x, target, _run(cuda, x, target, chunks, pad), f"{family} T{T} V{V} {chunking}")


@pytest.mark.parametrize("V,w", [(1000, 256), (2052, 513), (8705, 513)])
def test_ties_across_chunks(cuda, V, w):
    """The row maximum planted at two ids in different chunks, and at ids 0 and V - 1: the
    lower id wins in either launch order (v0 defines the index, not the order)."""
    T = 4
    x = S.family_logits("normal", T, V, seed=5)
    big = np.float32(x.max() + 3)
    pairs = [(w - 1, w), (3, V - 2), (0, V - 1), (w + 1, 2 * w + 1)]
    for t, (a, b) in enumerate(pairs):
        x[t, a] = x[t, b] = big
    target = np.full(T, -1, dtype=np.int32)
    chunks = S.chunks_of(V, "c256" if w == 256 else "c513")
    for order in (chunks, chunks[::-1]):
        got = _run(cuda, x, target, order)
        assert got[2].tolist() == [a for a, _ in pairs]
        _judge(x, target, got, f"ties V{V} w{w}")


def test_targets_at_chunk_edges_reverse_order(cuda):
    V, w = 2052, 513
    chunks = S.chunks_of(V, "c513")[::-1]
    target = np.array([0, V - 1, w - 1, w, -1, 2 * w - 1, 2 * w], dtype=np.int32)
    x = S.family_logits("x30", len(target), V, seed=9)
    got = _run(cuda, x, target, chunks)
    _judge(x, target, got, "targets at chunk edges, chunks reversed")
    assert np.isnan(got[1][4])


@pytest.mark.parametrize("chunking", ["one", "c256"])
def test_minus_inf_rows(cuda, chunking):
    """Half a row -inf, a whole row -inf (lse -inf, top 0, nothing NaN), and a row whose
    first chunks are all -inf."""
    V = 1000
    x = S.family_logits("normal", 3, V, seed=2)
    x[0, ::2] = -np.inf
    x[1, :] = -np.inf
    x[2, :600] = -np.inf
    target = np.array([1, -1, 700], dtype=np.int32)
    got = _run(cuda, x, target, S.chunks_of(V, chunking))
    _judge(x, target, got, f"-inf rows {chunking}")
    assert got[0][1] == -np.inf and got[2][1] == 0 and got[3][1] == -np.inf


def test_first_resets_used_state(cuda):
    """A second launch sequence with first = 1 on used state must not see the old state."""
    T, V = 3, 1000
    st = State(T, cuda)
    chunks = S.chunks_of(V, "c256")
    hot = (S.family_logits("normal", T, V, seed=3) + np.float32(500)).astype(np.float32)
    t1 = np.array([5, 999, 300], dtype=np.int32)
    _judge(hot, t1, _run(cuda, hot, t1, chunks, state=st), "first run")
    x = S.family_logits("normal", T, V, seed=4)
    t2 = np.array([-1, 2, -1], dtype=np.int32)
    got = _run(cuda, x, t2, chunks, state=st)
    _judge(x, t2, got, "second run on used state")


def test_rejects_bad_arguments(cuda):
    from cake_amd.ops import hip
    st = State(2, cuda)
    x = torch.zeros(2, 8, dtype=torch.float32, device=cuda)
    tg = torch.zeros(2, dtype=torch.int32, device=cuda)
    with pytest.raises(ValueError):
        hip.lse_rows(x.t(), 0, True, tg, st.run_max, st.run_sum, st.tgt, st.key)
    with pytest.raises(Exception):
        hip.lse_rows(x, -1, True, tg, st.run_max, st.run_sum, st.tgt, st.key)
