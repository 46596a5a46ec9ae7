"""Host model of the one-shot collectives of allreduce.hip (ar_sum, ar_max_key, ar_gather).

A collective of tag t pushes 8-byte granules `bits_u32 | t << 32` (held here in int64, two's
complement) into every peer's inbox and reads the peers' granules from its own:

  sum     bank = (t & 1) * world * n; rank r's word i sits at bank + r * n + i
  key     the same with n = 2: lane 0 the low word of the u64 key, lane 1 the high word
  gather  bank = (t & 1) * n; the word of global index j sits at bank + j

with t = (seq0 + 1) mod 2^32, seq0 the channel's tag counter before the launch.  A kernel
never waits when its inbox already holds the peers' granules of tag t, so one rank's kernel
can be run alone against inboxes filled by `prefill_inbox` and its stores compared with
`expected_push`.

The references are what every rank must hold afterwards: `sum_ref` adds the partials in f32
in ASCENDING RANK ORDER (((p0 + p1) + p2) + ...), the same on every rank, so the ranks'
results are bit-identical; `own_first_ref` is the order of the kernel before that was
fixed (the own partial first, then the peers ascending), which differs from it on ranks
>= 2 of a world >= 3.

Plain torch on the CPU; the GPU tests move the inputs over.
"""
from __future__ import annotations

import torch

MASK32 = 0xFFFFFFFF
KINDS = ("sum", "key", "gather")

WORLDS = [2, 3, 5, 8]
SUM_N = [1, 255, 257]
SUM_N_STRIDE = 64 * 256 + 5          # the 64-block grid's stride loop with a ragged second pass
SUM_N_STRIDE_WORLDS = [2, 8]
GATHER_V = [None, 2049, 20011]       # None: V = world (one element per shard); 20011 > 64 * 256
WRAP_SEQ0 = 0xFFFFFFFE               # three rounds from here carry the tags 0xFFFFFFFF, 0, 1


def ranks_of(world: int) -> list[int]:
    """Rank 0, a middle rank and the last one."""
    return sorted({0, world // 2, world - 1})


def sum_cases() -> list[tuple[int, int, int]]:
    """(world, rank, n) of the one-rank ar_sum test."""
    out = [(w, r, n) for w in WORLDS for r in ranks_of(w) for n in SUM_N]
    out += [(w, r, SUM_N_STRIDE) for w in SUM_N_STRIDE_WORLDS for r in ranks_of(w)]
    return out


# ---------------------------------------------------------------------------
# granules and layout
# ---------------------------------------------------------------------------

def next_tag(seq0: int) -> int:
    return (int(seq0) + 1) & MASK32


def as_i32(u: int) -> int:
    """The int32 that holds the 32 bits of u (the tag counter is an int32 tensor)."""
    u = int(u) & MASK32
    return u - (1 << 32) if u >= 1 << 31 else u


def as_i64(u: int) -> int:
    """The int64 that holds the 64 bits of u."""
    u = int(u) & 0xFFFFFFFFFFFFFFFF
    return u - (1 << 64) if u >= 1 << 63 else u


def granules(words: torch.Tensor, tag: int) -> torch.Tensor:
    """int32 words (bit patterns) -> int64 granules words_u32 | tag << 32."""
    assert words.dtype == torch.int32
    return (words.to(torch.int64) & MASK32) + as_i64((int(tag) & MASK32) << 32)


def words_of(g: torch.Tensor) -> torch.Tensor:
    """Low 32 bits of int64 granules, as int32."""
    lo = g & MASK32
    return torch.where(lo >= 1 << 31, lo - (1 << 32), lo).to(torch.int32)


def tags_of(g: torch.Tensor) -> torch.Tensor:
    """High 32 bits of int64 granules, as non-negative int64."""
    return (g >> 32) & MASK32


def bits(x: torch.Tensor) -> torch.Tensor:
    """f32 -> its int32 bit patterns."""
    assert x.dtype == torch.float32
    return x.contiguous().view(torch.int32)


def key_words(key: int) -> torch.Tensor:
    """u64 key -> int32 [low word, high word]."""
    key = int(key) & 0xFFFFFFFFFFFFFFFF
    return torch.tensor([as_i32(key), as_i32(key >> 32)], dtype=torch.int32)


def key_of_words(w: torch.Tensor) -> int:
    return (int(w[0]) & MASK32) | ((int(w[1]) & MASK32) << 32)


def inbox_words(kind: str, world: int, n: int) -> int:
    """Granules of one rank's inbox: two parity banks."""
    return {"sum": 2 * world * n, "key": 2 * world * 2, "gather": 2 * n}[kind]


def bank_of(kind: str, world: int, n: int, tag: int) -> int:
    per_bank = inbox_words(kind, world, n) // 2
    return (int(tag) & 1) * per_bank


def row_start(kind: str, world: int, n: int, tag: int, rank: int, off: int = 0) -> int:
    """First granule of `rank`'s row in any inbox; off is the rank's global offset (gather)."""
    if kind == "gather":
        return bank_of(kind, world, n, tag) + off
    width = 2 if kind == "key" else n
    return bank_of(kind, world, n, tag) + rank * width


def sentinel(tag: int) -> int:
    """The stale granule of the same bank: tag - 2, a word no test data holds."""
    return as_i64(((int(tag) - 2) & MASK32) << 32 | 0x7FA5C3E1)


PEER_FILL = as_i64(0x6B6B6B6B_5A5A5A5A)   # what a peer's inbox holds where nothing is pushed


def expected_push(kind: str, words: torch.Tensor, rank: int, world: int, n: int, tag: int,
                  off: int = 0) -> tuple[int, torch.Tensor]:
    """(start, granules): what `rank` must write into every peer's inbox.  words: the int32
    bit patterns of its partial (sum), key_words (key) or shard (gather, at offset off)."""
    return row_start(kind, world, n, tag, rank, off), granules(words, tag)


def prefill_inbox(kind: str, inbox: torch.Tensor, rows: dict, rank: int, world: int, n: int,
                  tag: int) -> torch.Tensor:
    """Write the peers' rows of tag `tag` into rank's inbox (int64, in place).
    rows: {r: words} or, for the gather, {r: (words, off)}; rank's own row is left out."""
    assert inbox.numel() == inbox_words(kind, world, n)
    for r, w in rows.items():
        if r == rank:
            continue
        w, off = w if isinstance(w, tuple) else (w, 0)
        s, g = expected_push(kind, w, r, world, n, tag, off)
        inbox[s:s + g.numel()] = g
    return inbox


def pull(kind: str, inbox: torch.Tensor, r: int, world: int, n: int, tag: int, count: int,
         off: int = 0) -> torch.Tensor:
    """Rank r's `count` words of tag `tag` read back from an inbox; raises on another tag."""
    s = row_start(kind, world, n, tag, r, off)
    g = inbox[s:s + count]
    if not bool((tags_of(g) == (int(tag) & MASK32)).all()):
        raise AssertionError(f"{kind}: rank {r}'s row does not carry tag {tag:#x}")
    return words_of(g)


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------

def sum_ref(partials: torch.Tensor, out0: torch.Tensor | None = None) -> torch.Tensor:
    """f32 sum over dim 0 of partials [world, n], sequentially in ascending rank order;
    with accumulate, out0 + that sum (one more f32 add)."""
    assert partials.dtype == torch.float32
    s = partials[0].clone()
    for r in range(1, partials.shape[0]):
        s = s + partials[r]
    return s if out0 is None else out0 + s


def own_first_ref(partials: torch.Tensor, rank: int, out0: torch.Tensor | None = None):
    """The order before the fix: the rank's own partial, then the peers ascending."""
    s = partials[rank].clone()
    for r in range(partials.shape[0]):
        if r != rank:
            s = s + partials[r]
    return s if out0 is None else out0 + s


def key_ref(keys) -> int:
    """Unsigned 64-bit maximum of the ranks' keys (python ints or an int64 tensor)."""
    if isinstance(keys, torch.Tensor):
        keys = keys.tolist()
    return max(int(k) & 0xFFFFFFFFFFFFFFFF for k in keys)


def shard_ranges(V: int, world: int) -> list[tuple[int, int]]:
    """Uneven contiguous shards: V // world each, the last takes the remainder."""
    q = V // world
    assert q >= 1
    return [(r * q, V if r == world - 1 else (r + 1) * q) for r in range(world)]


def gather_ref(shards) -> torch.Tensor:
    return torch.cat(list(shards))


# ---------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------

def recipe(world: int, n: int, rounds: int | None = None) -> torch.Tensor:
    """randn * 10**randint(-3, 4), f32 [world, n] ([rounds, world, n]), from
    torch.Generator().manual_seed(1000 * world + n): every rank can rebuild every rank's
    input.  Magnitudes from 1e-3 to 1e3 make the f32 sum depend on its order."""
    g = torch.Generator().manual_seed(1000 * world + n)
    shape = (world, n) if rounds is None else (rounds, world, n)
    x = torch.randn(shape, generator=g)
    e = torch.randint(-3, 4, shape, generator=g)
    return x * torch.pow(10.0, e.double()).float()


def sum_inputs(world: int, n: int) -> tuple[torch.Tensor, torch.Tensor]:
    """Three rounds of partials [3, world, n] and an initial `out` [n] for the accumulate
    mode of the one-rank ar_sum test."""
    x = recipe(world, n, rounds=4)
    return x[:3].contiguous(), x[3, 0].contiguous()


def key_rounds(world: int, rank: int) -> list[tuple[str, list[int]]]:
    """(name, keys[world]) for the one-rank ar_max_key test, run as consecutive rounds."""
    top, ones = 1 << 63, (1 << 64) - 1
    out = []
    for m in range(world):       # the maximum at each rank in turn, the own rank included
        out.append((f"max at rank {m}", [1000 + r + ((1 << 40) if r == m else 0)
                                         for r in range(world)]))
    for m in sorted({0, rank, world - 1}):
        # bit 63 beats everything below it: the int64 view of that key is negative
        ks = [top - 1 - r for r in range(world)]
        ks[m] = top | 5
        out.append((f"bit 63 at rank {m}", ks))
    out.append(("bit 63 everywhere", [top | (7 * r + 1) for r in range(world)]))
    # one word differs, its bit 31 set (a sign-extended word would spoil the other one)
    lows = [0x12345678_00000000 | (0x80000000 + 7 * r) for r in range(world)]
    highs = [((0x80000000 + 3 * r) << 32) | 0xCAFEBABE for r in range(world)]
    out += [("low word only, ascending", lows), ("low word only, descending", lows[::-1]),
            ("high word only, ascending", highs), ("high word only, descending", highs[::-1])]
    out.append(("all equal", [0xDEADBEEF_12345678] * world))
    out.append(("all zero", [0] * world))
    for m in sorted({0, rank, world - 1}):
        ks = [0] * world
        ks[m] = ones
        out.append((f"2^64 - 1 at rank {m}", ks))
    out.append(("all 2^64 - 1", [ones] * world))
    return out


def random_keys(world: int, rounds: int) -> list[list[int]]:
    """u64 keys [rounds][world] over the whole 64-bit range."""
    g = torch.Generator().manual_seed(77 * world + rounds)
    lo = torch.randint(0, 1 << 32, (rounds, world), generator=g)
    hi = torch.randint(0, 1 << 32, (rounds, world), generator=g)
    return [[int(l) | (int(h) << 32) for l, h in zip(ls, hs)]
            for ls, hs in zip(lo.tolist(), hi.tolist())]


# NaNs with distinct payloads (quiet and signalling, both signs), zeros, infinities, denormals
SPECIAL_BITS = [0x7FC00001, 0x7F800001, 0xFFC12345, 0xFFBFFFFF, 0x7FFFFFFF, 0x00000000,
                0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x00400000]


def with_specials(x: torch.Tensor) -> torch.Tensor:
    """x (f32, any shape) with every third element of its last dim replaced by the special
    patterns in turn, the first element included."""
    w = bits(x).clone()
    idx = torch.arange(0, w.shape[-1], 3)
    sp = torch.tensor([as_i32(b) for b in SPECIAL_BITS], dtype=torch.int32)
    w[..., idx] = sp[(idx // 3) % sp.numel()]
    return w.view(torch.float32)


def special_sum_rows(world: int) -> torch.Tensor:
    """partials [world, 8] whose sums are special: +inf + finite, -inf + finite, -0.0 from
    every rank (stays -0.0), +0.0 from one rank among -0.0 (+0.0), +inf from two ranks, a
    denormal from every rank (an exact denormal sum), an overflow to +inf, and cancellation
    to +0.0.  No row makes a NaN: the bits of a generated NaN are the adder's choice."""
    inf = float("inf")
    p = torch.zeros(world, 8)
    last = world - 1
    p[:, 0] = 1.5
    p[last, 0] = inf
    p[:, 1] = -2.5
    p[0, 1] = -inf
    p[:, 2] = -0.0
    p[:, 3] = -0.0
    p[last, 3] = 0.0
    p[:, 4] = 1.0
    p[0, 4] = inf
    p[last, 4] = inf
    p[:, 5] = torch.tensor([1], dtype=torch.int32).view(torch.float32)
    p[:, 6] = 3.0e38
    p[:, 7] = 0.0
    p[0, 7] = 7.25
    p[last, 7] = -7.25
    return p
