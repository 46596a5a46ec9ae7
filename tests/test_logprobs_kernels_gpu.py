"""cake_logprob_topk (logprob.hip) through ops/hip.py against ops/reference.py's
logprob_topk_ref.

Judged by: ids equal to the oracle's (descending logit, the lower id first at ties), the
token's logit and every top logit bit-equal to the input, |lse - ref64| <= 2^-24 (|ref64| +
128) (the bound of the score kernel).  No element is excluded."""
import numpy as np
import pytest
import torch

import _score as S
from cake_amd.ops.reference import logprob_topk_ref

pytestmark = pytest.mark.gpu

VS = [1, 2, 19, 20, 21, 255, 257, 1000, 8705, 128256]
KS = [0, 1, 5, 20]
BLOCKS = [1, 2, 7, 0]
W = 48
CANARY = 0x5A5A5A5A


def _bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Bufs:
    def __init__(self, dev, V, max_rec=4):
        from cake_amd.ops import hip
        self.rec = torch.full((max_rec, W), CANARY, dtype=torch.int32, device=dev)
        self.ws = torch.zeros(max(1, hip.logprob_ws_bytes(V) // 8), dtype=torch.int64, device=dev)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self.tok = torch.zeros(1, dtype=torch.int32, device=dev)
        self.hl = torch.zeros(1, dtype=torch.int32, device=dev)


def _launch(b: Bufs, xdev, tok, idx, K, mb=0):
    from cake_amd.ops import hip
    b.tok.fill_(tok)
    b.hl.fill_(idx + 1)
    hip.logprob_topk(xdev, b.tok, b.hl, K, b.rec, b.ws, b.ticket, mb)


def _decode(row: np.ndarray) -> dict:
    """One 48-word record (int32) as a dict."""
    u = row.view(np.uint32)
    return {"id": int(row[0]), "logit": u[1:2].view(np.float32)[0], "lse": u[2:3].view(np.float32)[0],
            "K": int(row[3]), "top_ids": row[4:24].copy(), "top_logits": u[24:44].view(np.float32).copy(),
            "pad": row[44:48].copy()}


def _judge(x: np.ndarray, tok: int, K: int, r: dict, what: str) -> float:
    ref = logprob_topk_ref(torch.from_numpy(x), tok, K)
    assert r["id"] == tok and r["K"] == K and (r["pad"] == 0).all(), what
    assert _bits(r["logit"])[()] == _bits(x[tok])[()], what
    assert np.array_equal(r["top_ids"][:K], ref["top_ids"].numpy()), what
    assert np.array_equal(_bits(r["top_logits"][:K]), _bits(ref["top_logits"].numpy())), what
    assert (r["top_ids"][K:] == -1).all() and np.isneginf(r["top_logits"][K:]).all(), what
    n = min(K, x.size)
    assert np.array_equal(_bits(r["top_logits"][:n]), _bits(x[r["top_ids"][:n]])), what
    lse = ref["lse"]
    assert not np.isnan(r["lse"]), what
    if np.isneginf(lse):
        assert np.isneginf(r["lse"]), what
        return 0.0
    ratio = abs(float(r["lse"]) - lse) / float(S.lse_bound(np.float64(lse)))
    assert ratio <= 1.0, (what, ratio, float(r["lse"]), lse)
    return ratio


def _one(dev, x: np.ndarray, tok: int, K: int, mb: int = 0, what: str = "", off: int = 0) -> dict:
    """Launch on a copy of x placed `off` floats past an aligned base; judge; return the record."""
    V = x.size
    buf = torch.full((V + off + 8,), 777.0, dtype=torch.float32, device=dev)
    buf[off:off + V] = torch.from_numpy(x).to(dev)
    b = Bufs(dev, V)
    _launch(b, buf[off:off + V], tok, 1, K, mb)
    torch.cuda.synchronize()
    rec = b.rec.cpu().numpy()
    assert (rec[[0, 2, 3]].view(np.uint32) == CANARY).all(), what   # the neighbours untouched
    assert int(b.ticket.item()) == 0, what                            # re-armed
    r = _decode(rec[1])
    r["ratio"] = _judge(x, tok, K, r, what)
    return r


@pytest.mark.parametrize("V", VS)
def test_grid(cuda, V):
    worst = 0.0
    for fi, family in enumerate(S.FAMILIES):
        x = S.family_logits(family, 1, V, seed=11)[0]
        toks = [0, V - 1, int(np.argmax(x)), (7 * V) // 13]
        for K in KS:
            for mb in BLOCKS:
                tok = toks[(fi + K + mb) % 4]
                r = _one(cuda, x, tok, K, mb, f"{family} V{V} K{K} blocks{mb} tok{tok}")
                worst = max(worst, r["ratio"])
    print(f"V{V}: lse error / bound, worst case: {worst:.3f}")


@pytest.mark.parametrize("mb", BLOCKS)
def test_top20_inside_one_slice(cuda, mb):
    """The 20 largest logits all within ids [100, 120): a slice that keeps one candidate (or
    fewer than K) loses them."""
    V = 128256
    x = S.family_logits("normal", 1, V, seed=3)[0]
    order = np.random.default_rng(5).permutation(20)
    x[100:120] = (np.float32(x.max()) + 1 + order).astype(np.float32)
    r = _one(cuda, x, 5000, 20, mb, f"top 20 in [100, 120) blocks{mb}")
    assert sorted(r["top_ids"].tolist()) == list(range(100, 120))
    assert 5000 not in r["top_ids"]          # a tok outside the top K


@pytest.mark.parametrize("V", [21, 8705, 128256])
def test_ties(cuda, V):
    """All-equal row: ids 0..K-1.  40 equal maxima at random ids plus ids 0 and V - 1: the
    lowest ids first."""
    x = np.full(V, 1.5, dtype=np.float32)
    for K in KS:
        r = _one(cuda, x, V - 1, K, 0, f"all equal V{V} K{K}")
        assert r["top_ids"][:min(K, V)].tolist() == list(range(min(K, V)))
    if V < 100:
        return
    x = S.family_logits("x30", 1, V, seed=8)[0]
    ids = np.unique(np.concatenate([np.random.default_rng(V).integers(0, V, 40), [0, V - 1]]))
    x[ids] = np.float32(x.max()) + 2
    for mb in BLOCKS:
        r = _one(cuda, x, 0, 20, mb, f"40 equal maxima V{V} blocks{mb}")
        assert r["top_ids"].tolist() == ids[:20].tolist()


@pytest.mark.parametrize("V", [21, 1000, 128256])
def test_minus_inf(cuda, V):
    """All but m < K entries -inf (the rest of the top K are -inf logits, lowest ids first), and
    an all -inf row (lse -inf, nothing NaN)."""
    x = np.full(V, -np.inf, dtype=np.float32)
    keep = [V - 1, 3, V // 2]
    x[keep] = np.array([0.5, -2.0, 7.25], dtype=np.float32)
    for K in (5, 20):
        r = _one(cuda, x, V // 2, K, 0, f"3 finite V{V} K{K}")
        assert r["top_ids"][:3].tolist() == [V // 2, V - 1, 3]
        r = _one(cuda, x, 0, K, 2, f"3 finite, tok -inf V{V} K{K}")
        assert np.isneginf(r["logit"])
    x[:] = -np.inf
    for mb in (0, 1):
        r = _one(cuda, x, V - 1, 20, mb, f"all -inf V{V} blocks{mb}")
        assert np.isneginf(r["lse"]) and r["top_ids"][:min(20, V)].tolist() == list(range(min(20, V)))


@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("V", [19, 257, 8705])
def test_misaligned_base(cuda, V, off):
    x = S.family_logits("offset", 1, V, seed=off)[0]
    for mb in (0, 2):
        _one(cuda, x, V - 1, 20, mb, f"base + {off} floats V{V} blocks{mb}", off=off)


def test_index_out_of_range_writes_nothing(cuda):
    V = 1000
    x = torch.from_numpy(S.family_logits("normal", 1, V)[0]).to(cuda)
    b = Bufs(cuda, V, max_rec=3)
    for idx in (-1, 3, 1000, -5):
        _launch(b, x, 1, idx, 5)
    torch.cuda.synchronize()
    assert (b.rec.cpu().numpy().view(np.uint32) == CANARY).all()
    assert int(b.ticket.item()) == 0
    _launch(b, x, 1, 2, 5)          # and the state is good for a launch in range
    torch.cuda.synchronize()
    rec = b.rec.cpu().numpy()
    assert (rec[:2].view(np.uint32) == CANARY).all()
    _judge(x.cpu().numpy(), 1, 5, _decode(rec[2]), "after out-of-range launches")


def test_bad_arguments(cuda):
    from cake_amd.ops import hip
    from cake_amd.ops._lib import KernelError, kernels
    V = 64
    x = torch.zeros(V, dtype=torch.float32, device=cuda)
    b = Bufs(cuda, V)
    for K in (-1, 21):
        with pytest.raises(KernelError):
            hip.logprob_topk(x, b.tok, b.hl, K, b.rec, b.ws, b.ticket)
    with pytest.raises(ValueError):
        hip.logprob_topk(x[::2], b.tok, b.hl, 1, b.rec, b.ws, b.ticket)
    L = kernels()
    args = lambda **kw: [kw.get("x", x.data_ptr()), kw.get("V", V), b.tok.data_ptr(),
                         kw.get("hl", b.hl.data_ptr()), 1, kw.get("rec", b.rec.data_ptr()), 4,
                         kw.get("ws", b.ws.data_ptr()), b.ticket.data_ptr(), 0, None]
    inval = 1   # hipErrorInvalidValue
    assert L.cake_logprob_topk(*args(V=0)) == inval
    assert L.cake_logprob_topk(*args(x=None)) == inval
    assert L.cake_logprob_topk(*args(hl=None)) == inval
    assert L.cake_logprob_topk(*args(rec=None)) == inval
    assert L.cake_logprob_topk(*args(ws=None)) == inval
    assert L.cake_logprob_topk(*args(x=x.data_ptr() + 2)) == inval    # not 4-byte aligned
    torch.cuda.synchronize()
    assert (b.rec.cpu().numpy().view(np.uint32) == CANARY).all()      # nothing was launched
    assert hip.logprob_ws_bytes(128256) > 0 and hip.logprob_ws_bytes(0) == 0


def test_back_to_back_launches(cuda):
    """Two launches on different rows with nothing between them: the workspace and the ticket
    of the first must not leak into the second."""
    V = 128256
    xa = S.family_logits("normal", 1, V, seed=1)[0]
    xb = (S.family_logits("dominant", 1, V, seed=2)[0] + np.float32(40)).astype(np.float32)
    da, db = (torch.from_numpy(a).to(cuda) for a in (xa, xb))
    b = Bufs(cuda, V)
    _launch(b, da, 11, 0, 20)
    b2_tok, b2_hl = b.tok.clone(), b.hl.clone()
    b2_tok.fill_(V - 1)
    b2_hl.fill_(3)
    from cake_amd.ops import hip
    hip.logprob_topk(db, b2_tok, b2_hl, 20, b.rec, b.ws, b.ticket)
    torch.cuda.synchronize()
    rec = b.rec.cpu().numpy()
    _judge(xa, 11, 20, _decode(rec[0]), "first of two")
    _judge(xb, V - 1, 20, _decode(rec[2]), "second of two")


def test_graph_replay(cuda):
    """One captured launch replayed three times with the logits and hist_len changed between
    the replays: each record matches its own row (a ticket or workspace left dirty shows)."""
    from cake_amd.ops import hip
    V = 8705
    rows = [S.family_logits(f, 1, V, seed=20 + i)[0] for i, f in enumerate(["normal", "x30", "offset"])]
    x = torch.zeros(V, dtype=torch.float32, device=cuda)
    b = Bufs(cuda, V)
    x.copy_(torch.from_numpy(rows[0]))
    b.tok.fill_(0)
    b.hl.fill_(5)            # warm-up launch, at an index past the array
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        hip.logprob_topk(x, b.tok, b.hl, 20, b.rec, b.ws, b.ticket, 7)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        hip.logprob_topk(x, b.tok, b.hl, 20, b.rec, b.ws, b.ticket, 7)
    toks = [5, V - 1, 4000]
    for i, row in enumerate(rows):
        x.copy_(torch.from_numpy(row))
        b.tok.fill_(toks[i])
        b.hl.fill_(i + 1)
        g.replay()
    torch.cuda.synchronize()
    rec = b.rec.cpu().numpy()
    for i, row in enumerate(rows):
        _judge(row, toks[i], 20, _decode(rec[i]), f"replay {i}")
    assert (rec[3].view(np.uint32) == CANARY).all()


def test_deterministic(cuda):
    """The same input launched 20 times gives identical record bytes (the merge is by slice
    index, not by arrival)."""
    V = 128256
    xn = S.family_logits("x30", 1, V, seed=6)[0]
    x = torch.from_numpy(xn).to(cuda)
    b = Bufs(cuda, V, max_rec=20)
    b.tok.fill_(77)
    from cake_amd.ops import hip
    for i in range(20):
        b.hl.fill_(i + 1)
        hip.logprob_topk(x, b.tok, b.hl, 20, b.rec, b.ws, b.ticket)
    torch.cuda.synchronize()
    rec = b.rec.cpu().numpy()
    assert all(np.array_equal(rec[0], rec[i]) for i in range(1, 20))
    _judge(xn, 77, 20, _decode(rec[0]), "20 launches")
