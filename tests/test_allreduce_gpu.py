"""The one-shot collectives of allreduce.hip (ar_sum, ar_max_key, ar_gather) against the
host model of tests/_allreduce.py, bit for bit.

Part A runs ONE rank's kernel with emulated peers: plain int64 device tensors stand for the
rank's inbox and the peers' inboxes, the model fills the inbox with the peers' granules of
the expected tag before the launch (a collective whose inbox is full never waits), and
afterwards every peer buffer must hold exactly the rank's rows and nothing else, the result
must be the model's, and the tag counter must have advanced.  A layout bug ends in the
error word after the 2 s bound, not in a wait.

Part B runs live ranks (processes sharing cuda:0 over the IPC inboxes): bursts of sums, key
maxima and gathers without a host sync, skewed ranks, a captured graph replayed three
times; every rank's results equal the model and all ranks report the same digest."""
import ctypes as C
import os
import socket
import time

import pytest
import torch

import _allreduce as A

pytestmark = pytest.mark.gpu

TIMEOUT_S = 2.0


def _assert_bits(got, want, what):
    """Bit equality of two tensors of one 4- or 8-byte dtype, with a message that says where."""
    got, want = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    assert got.shape == want.shape and got.dtype == want.dtype, what
    view = torch.int32 if got.element_size() == 4 else torch.int64
    g, w = got.view(view), want.view(view)
    if not torch.equal(g, w):
        bad = (g != w).nonzero().flatten()
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {g.numel()} words differ, first at {i}: "
                             f"got {got.flatten()[i].item()!r} ({g.flatten()[i].item():#x}), want "
                             f"{want.flatten()[i].item()!r} ({w.flatten()[i].item():#x})")


class OneRank:
    """One rank's channel on plain device tensors; the peers exist as buffers and a model."""

    def __init__(self, dev, kind, world, rank, n, seq0=0):
        self.dev, self.kind, self.world, self.rank, self.n = dev, kind, world, rank, n
        self.seq0, self.k = seq0, 0
        words = A.inbox_words(kind, world, n)
        self.inbox = torch.empty(words, dtype=torch.int64, device=dev)
        self.peers = {r: torch.full((words,), A.PEER_FILL, dtype=torch.int64, device=dev)
                      for r in range(world) if r != rank}
        self.model = {r: torch.full((words,), A.PEER_FILL, dtype=torch.int64) for r in self.peers}
        self.ptrs = (C.c_void_p * 8)()
        for r, t in self.peers.items():
            self.ptrs[r] = t.data_ptr()
        self.seq = torch.tensor([A.as_i32(seq0), 0], dtype=torch.int32, device=dev)
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)

    def args(self, timeout_s=TIMEOUT_S):
        return (self.ptrs, self.inbox.data_ptr(), self.seq, self.err, self.rank, self.world,
                timeout_s)

    def begin(self, rows, spoil=None):
        """Fill the inbox for the next tag: the peers' rows, the stale sentinel (tag - 2)
        everywhere else.  spoil: an inbox index that keeps the stale word."""
        self.tag = A.next_tag(self.seq0 + self.k)
        ib = torch.full((self.inbox.numel(),), A.sentinel(self.tag), dtype=torch.int64)
        A.prefill_inbox(self.kind, ib, rows, self.rank, self.world, self.n, self.tag)
        if spoil is not None:
            ib[spoil] = A.sentinel(self.tag)
        self.filled = ib
        self.inbox.copy_(ib)
        return self.tag

    def end(self, words, off=0, err=0, what=""):
        """After the launch: the pushes are exact and nothing else was written, the inbox is
        untouched, the tag advanced, the ticket is back at 0."""
        torch.cuda.synchronize()
        what = f"{what} tag {self.tag:#x}"
        s, g = A.expected_push(self.kind, words, self.rank, self.world, self.n, self.tag, off)
        for r, buf in self.peers.items():
            self.model[r][s:s + g.numel()] = g
            _assert_bits(buf, self.model[r], f"{what}: inbox of peer {r}")
        _assert_bits(self.inbox, self.filled, f"{what}: own inbox")
        assert self.seq.tolist() == [A.as_i32(self.tag), 0], (what, self.seq.tolist())
        assert int(self.err.item()) == err, what
        self.k += 1


def _run_sum(dev, world, rank, P, out0, mode, seq0=0):
    """P [rounds, world, n]: consecutive launches on the same buffers."""
    from cake_amd.ops import hip as K
    n = P.shape[2]
    ch = OneRank(dev, "sum", world, rank, n, seq0)
    running = out0.clone()
    out = out0.to(dev)
    banks = []
    for k in range(P.shape[0]):
        what = f"ar_sum world {world} rank {rank} n {n} {mode} round {k}"
        tag = ch.begin({r: A.bits(P[k, r]) for r in range(world)})
        banks.append(A.bank_of("sum", world, n, tag))
        partial = P[k, rank].clone().to(dev)
        if mode == "in_place":
            K.ar_sum(partial, partial, False, *ch.args())
            ch.end(A.bits(P[k, rank]), what=what)
            _assert_bits(partial, A.sum_ref(P[k]), what + ": out (aliasing partial)")
            continue
        K.ar_sum(partial, out, mode == "accumulate", *ch.args())
        ch.end(A.bits(P[k, rank]), what=what)
        running = A.sum_ref(P[k], running if mode == "accumulate" else None)
        _assert_bits(out, running, what + ": out")
        _assert_bits(partial, P[k, rank], what + ": partial")
    if len(banks) == 3:
        assert banks[0] != banks[1] and banks[2] == banks[0]


@pytest.mark.parametrize("mode", ["set", "accumulate", "in_place"])
@pytest.mark.parametrize("world,rank,n", A.sum_cases())
def test_ar_sum_one_rank(cuda, world, rank, n, mode):
    """out (+)= the ascending-rank f32 sum, bit for bit, three launches on alternating banks.
    On ranks >= 2 of a world >= 3 a kernel that adds its own partial first fails here
    (test_allreduce_cpu.py::test_data_tells_the_two_orders_apart)."""
    P, out0 = A.sum_inputs(world, n)
    _run_sum(cuda, world, rank, P, out0, mode)


@pytest.mark.parametrize("mode", ["set", "accumulate", "in_place"])
@pytest.mark.parametrize("world,rank,n", [(2, 1, 257), (3, 2, 255), (8, 4, 257), (5, 0, 1)])
def test_ar_sum_tag_wrap(cuda, world, rank, n, mode):
    """seq0 = 0xFFFFFFFE (int32 -2): the tags run 0xFFFFFFFF, 0, 1."""
    P, out0 = A.sum_inputs(world, n)
    _run_sum(cuda, world, rank, P, out0, mode, seq0=A.WRAP_SEQ0)


@pytest.mark.parametrize("mode", ["set", "accumulate"])
@pytest.mark.parametrize("world", A.WORLDS)
def test_ar_sum_special_values(cuda, world, mode):
    """inf + finite, -0.0 from every rank stays -0.0 (also accumulated onto -0.0), an exact
    denormal sum, overflow to inf."""
    P = A.special_sum_rows(world)[None]
    out0 = torch.full((P.shape[2],), -0.0)
    for rank in A.ranks_of(world):
        _run_sum(cuda, world, rank, P, out0, mode)


def test_ar_sum_stale_word_raises_error_word(cuda):
    """One peer word still carries the stale tag of its bank: the kernel gives up after its
    bound, raises the error word and still advances the tag (the sequence is not lost)."""
    from cake_amd.ops import hip as K
    world, rank, n = 3, 1, 257
    P, _ = A.sum_inputs(world, n)
    ch = OneRank(cuda, "sum", world, rank, n)
    tag = ch.begin({r: A.bits(P[0, r]) for r in range(world)},
                   spoil=A.row_start("sum", world, n, A.next_tag(0), 2) + 100)
    partial = P[0, rank].clone().to(cuda)
    out = torch.zeros(n, device=cuda)
    K.ar_sum(partial, out, False, *ch.args(timeout_s=0.05))
    ch.end(A.bits(P[0, rank]), err=1, what="stale word")
    assert ch.seq.tolist() == [tag, 0]
    want = A.sum_ref(P[0])
    keep = torch.arange(n) != 100          # every other element is still the sum
    _assert_bits(out.cpu()[keep], want[keep], "stale word: the other elements")


@pytest.mark.parametrize("seq0", [0, A.WRAP_SEQ0])
@pytest.mark.parametrize("world,rank", [(w, r) for w in A.WORLDS for r in A.ranks_of(w)])
def test_ar_max_key_one_rank(cuda, world, rank, seq0):
    """slot <- the unsigned 64-bit maximum; two exact words pushed to every peer."""
    from cake_amd.ops import hip as K
    ch = OneRank(cuda, "key", world, rank, 2, seq0)
    for name, keys in A.key_rounds(world, rank):
        what = f"ar_max_key world {world} rank {rank}: {name}"
        ch.begin({r: A.key_words(keys[r]) for r in range(world)})
        slot = torch.tensor([A.as_i64(keys[rank])], dtype=torch.int64, device=cuda)
        K.ar_max_key(slot, *ch.args())
        ch.end(A.key_words(keys[rank]), what=what)
        assert int(slot.item()) == A.as_i64(A.key_ref(keys)), \
            (what, hex(int(slot.item()) & (2 ** 64 - 1)), hex(A.key_ref(keys)))


@pytest.mark.parametrize("V", A.GATHER_V)
@pytest.mark.parametrize("world,rank", [(w, r) for w in A.WORLDS for r in A.ranks_of(w)])
def test_ar_gather_one_rank(cuda, world, rank, V):
    """full is bit-equal to the concatenation of uneven shards holding NaN payloads, signed
    zeros, infinities and denormals; three launches on alternating banks."""
    from cake_amd.ops import hip as K
    V = world if V is None else V
    data = A.with_specials(A.recipe(world, V, rounds=3)[:, 0].contiguous())
    rng = A.shard_ranges(V, world)
    a, b = rng[rank]
    ch = OneRank(cuda, "gather", world, rank, V)
    for k in range(3):
        what = f"ar_gather world {world} rank {rank} V {V} round {k}"
        shards = [data[k, lo:hi].contiguous() for lo, hi in rng]
        ch.begin({r: (A.bits(shards[r]), rng[r][0]) for r in range(world)})
        shard = shards[rank].to(cuda)
        full = torch.full((V,), 12345.0, device=cuda)
        K.ar_gather(shard, a, full, *ch.args())
        ch.end(A.bits(shards[rank]), off=a, what=what)
        _assert_bits(full, A.gather_ref(shards), what + ": full")
        _assert_bits(shard, shards[rank], what + ": shard")


# ---------------------------------------------------------------------------
# part B: live ranks
# ---------------------------------------------------------------------------

LIVE_N = 4101
LIVE_EAGER = 33     # rounds launched one by one
LIVE_GRAPH = 8      # rounds captured in one graph
LIVE_REPLAYS = 3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _live_inputs(world):
    T = LIVE_EAGER + LIVE_GRAPH
    V = 1000 * world + 3
    P = A.recipe(world, LIVE_N, rounds=T)
    keys = A.random_keys(world, T)
    vocab = A.with_specials(A.recipe(world, V, rounds=T)[:, 0].contiguous())
    return P, keys, vocab


def _live_model(world, P, keys, vocab):
    """What every rank must hold after each round, in issue order: the eager rounds, then the
    graph's rounds once per replay (out keeps accumulating across them)."""
    order = list(range(LIVE_EAGER)) + list(range(LIVE_EAGER, LIVE_EAGER + LIVE_GRAPH)) * LIVE_REPLAYS
    out = torch.zeros(LIVE_N)
    sums = []
    for t in order:
        if t % 3 == 0:                      # in place: out is not touched
            sums.append(A.sum_ref(P[t]))
        else:
            out = A.sum_ref(P[t], out if t % 2 == 1 else None)
            sums.append(out)
    maxes = [A.as_i64(A.key_ref(keys[t])) for t in order]
    return (torch.stack(sums), torch.tensor(maxes, dtype=torch.int64),
            torch.stack([vocab[t] for t in order]))


def _live_body(comm, rank, world, rep):
    import hashlib
    dev = "cuda:0"
    n, T, E, G = LIVE_N, LIVE_EAGER + LIVE_GRAPH, LIVE_EAGER, LIVE_GRAPH
    V = 1000 * world + 3
    P, keys, vocab = _live_inputs(world)
    a, b = A.shard_ranges(V, world)[rank]
    Pd = P[:, rank].contiguous().to(dev)
    Kd = torch.tensor([A.as_i64(k[rank]) for k in keys], dtype=torch.int64).to(dev)
    Sd = vocab[:, a:b].contiguous().to(dev)
    out, buf = torch.zeros(n, device=dev), torch.empty(n, device=dev)
    slot = torch.zeros(1, dtype=torch.int64, device=dev)
    full = torch.empty(V, device=dev)
    rows = E + G * LIVE_REPLAYS
    res_sum = torch.zeros(rows, n, device=dev)
    res_key = torch.zeros(rows, dtype=torch.int64, device=dev)
    res_full = torch.zeros(rows, V, device=dev)
    step_sum = torch.zeros(T, n, device=dev)       # the graph's rounds write rows E..T
    step_key = torch.zeros(T, dtype=torch.int64, device=dev)
    step_full = torch.zeros(T, V, device=dev)
    chans = [comm.sum_ch, comm.key_ch, comm.gather_ch]
    start = [int(ch["seq"][0].item()) for ch in chans]

    def body(t):
        if t % 3 == 0:
            buf.copy_(Pd[t])
            comm.sum_(buf, buf, accumulate=False)
            step_sum[t].copy_(buf)
        else:
            comm.sum_(Pd[t], out, accumulate=t % 2 == 1)
            step_sum[t].copy_(out)
        slot.copy_(Kd[t:t + 1])
        comm.max_key_(slot)
        step_key[t:t + 1].copy_(slot)
        comm.gather_(Sd[t], a, full)
        step_full[t].copy_(full)

    comm.barrier()
    t0 = time.perf_counter()
    for t in range(E):
        if t % 5 == 2:
            time.sleep(rank * 0.002)    # the fast ranks run one collective ahead
        body(t)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for t in range(E, T):
            body(t)
    res_sum[:E].copy_(step_sum[:E])
    res_key[:E].copy_(step_key[:E])
    res_full[:E].copy_(step_full[:E])
    for i in range(LIVE_REPLAYS):
        g.replay()
        lo = E + i * G
        res_sum[lo:lo + G].copy_(step_sum[E:])
        res_key[lo:lo + G].copy_(step_key[E:])
        res_full[lo:lo + G].copy_(step_full[E:])
    torch.cuda.synchronize()
    rep["burst_s"] = time.perf_counter() - t0
    got = [res_sum.cpu().view(torch.int32), res_key.cpu(), res_full.cpu().view(torch.int32)]
    want_sum, want_key, want_full = _live_model(world, P, keys, vocab)
    want = [want_sum.view(torch.int32), want_key, want_full.view(torch.int32)]
    for name, x, y in zip(("sum", "key", "gather"), got, want):
        bad = (x != y).reshape(rows, -1)
        if bool(bad.any()):
            first = int(bad.any(1).nonzero()[0])
            rep["problems"].append(f"{name}: {int(bad.sum())} words differ from the model, "
                                   f"first in issue {first} ({int(bad[first].sum())} words)")
    rep["errors"] = comm.errors()
    rep["seq"] = [int(ch["seq"][0].item()) - s for ch, s in zip(chans, start)]
    h = hashlib.sha256()
    for x in got:
        h.update(x.contiguous().numpy().tobytes())
    rep["digest"] = h.hexdigest()
    rep["us"] = comm.measure_us(50)


def _live_worker(rank, world, port, q):
    import torch.distributed as dist
    from cake_amd.parallel.tensor_parallel import AllReduce
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      HSA_ENABLE_IPC_MODE_LEGACY="0", CAKE_HOP_TIMEOUT="20")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    rep = {"rank": rank, "problems": [], "mode": None}
    try:
        torch.cuda.set_device(0)
        comm = AllReduce(rank, world, "cuda:0", n=LIVE_N, n_gather=1000 * world + 3)
        rep["mode"] = comm.mode
        if comm.mode == "ipc":
            _live_body(comm, rank, world, rep)
        q.put(rep)
        comm.close()
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [3, 8])
def test_live_ranks_hold_identical_bits(cuda, world):
    """world processes on cuda:0: 33 skewed rounds of sum / key max / gather and three replays
    of an 8-round graph, one synchronize; every rank equals the model bit for bit, and the
    ranks' digests are identical (the sum is rank-invariant: replicas, not neighbours)."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_live_worker, args=(r, world, port, q)) for r in range(world)]
    t0 = time.perf_counter()
    for p in ps:
        p.start()
    got = {}
    try:
        for _ in range(world):
            rep = q.get(timeout=150)
            got[rep["rank"]] = rep
        for p in ps:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in ps:  # a failed rank leaves its peers blocked in a collective
            if p.is_alive():
                p.kill()
    issued = LIVE_EAGER + LIVE_GRAPH * LIVE_REPLAYS
    print(f"live world {world}: {time.perf_counter() - t0:.1f} s wall, burst "
          f"{max(r.get('burst_s', 0) for r in got.values()):.2f} s, all-reduce "
          f"{got[0].get('us')} us")
    assert sorted(got) == list(range(world))
    for r in range(world):
        assert got[r]["mode"] == "ipc", (r, got[r]["mode"])   # no silent fallback
        assert not got[r]["problems"], (r, got[r]["problems"])
        assert got[r]["errors"] == 0, r
        assert got[r]["seq"] == [issued] * 3, (r, got[r]["seq"])
    assert len({got[r]["digest"] for r in range(world)}) == 1, \
        {r: got[r]["digest"][:12] for r in range(world)}
