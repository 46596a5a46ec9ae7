"""The host model of the all-reduce kernels (tests/_allreduce.py) checked against itself:
the granule layout round-trips, the parity banks are disjoint across the tag wrap, the test
data tells the ascending-rank sum from the own-partial-first sum, and the f32 reference
stays within the sequential-summation bound of a float64 sum."""
import pytest
import torch

import _allreduce as A


def _gather_inputs(world, V):
    full = A.with_specials(A.recipe(world, V)[0])
    rng = A.shard_ranges(V, world)
    return full, rng, [full[a:b] for a, b in rng]


@pytest.mark.parametrize("world", A.WORLDS)
@pytest.mark.parametrize("seq0", [0, 1, A.WRAP_SEQ0, A.WRAP_SEQ0 + 1])
def test_model_round_trip(world, seq0):
    """Every rank pushes its rows into every peer's inbox; every rank then pulls the peers'
    rows back and reduces: the direct references, on every rank."""
    n, V = 37, 10 * world + 3
    tag = A.next_tag(seq0)
    P = A.recipe(world, n)
    keys = A.random_keys(world, 1)[0]
    full, rng, shards = _gather_inputs(world, V)
    inbox = {k: [torch.full((A.inbox_words(k, world, m),), A.sentinel(tag), dtype=torch.int64)
                 for _ in range(world)] for k, m in (("sum", n), ("key", 2), ("gather", V))}
    for r in range(world):               # the pushes, one row at a time
        for d in range(world):
            if d == r:
                continue
            for kind, m, w, off in (("sum", n, A.bits(P[r]), 0), ("key", 2, A.key_words(keys[r]), 0),
                                    ("gather", V, A.bits(shards[r]), rng[r][0])):
                s, g = A.expected_push(kind, w, r, world, m, tag, off)
                assert A.bank_of(kind, world, m, tag) <= s
                assert s + g.numel() <= A.bank_of(kind, world, m, tag) + A.inbox_words(kind, world, m) // 2
                inbox[kind][d][s:s + g.numel()] = g
    for d in range(world):               # prefill_inbox builds the same inbox in one call
        for kind, m, rows in (("sum", n, {r: A.bits(P[r]) for r in range(world)}),
                              ("key", 2, {r: A.key_words(keys[r]) for r in range(world)}),
                              ("gather", V, {r: (A.bits(shards[r]), rng[r][0]) for r in range(world)})):
            ib = torch.full((A.inbox_words(kind, world, m),), A.sentinel(tag), dtype=torch.int64)
            assert torch.equal(A.prefill_inbox(kind, ib, rows, d, world, m, tag), inbox[kind][d])
    want_sum, want_key = A.sum_ref(P), A.key_ref(keys)
    for d in range(world):
        rows = [A.bits(P[d]) if r == d else A.pull("sum", inbox["sum"][d], r, world, n, tag, n)
                for r in range(world)]
        got = A.sum_ref(torch.stack(rows).view(torch.float32))
        assert torch.equal(A.bits(got), A.bits(want_sum))
        ks = [keys[d] if r == d else
              A.key_of_words(A.pull("key", inbox["key"][d], r, world, 2, tag, 2)) for r in range(world)]
        assert ks == keys and A.key_ref(ks) == want_key
        parts = [A.bits(shards[d]) if r == d else
                 A.pull("gather", inbox["gather"][d], r, world, V, tag, rng[r][1] - rng[r][0], rng[r][0])
                 for r in range(world)]
        assert torch.equal(A.gather_ref(parts), A.bits(full))
        # nothing landed in rank d's own row or in the other bank
        for kind, m in (("sum", n), ("key", 2), ("gather", V)):
            other = A.bank_of(kind, world, m, tag + 1)
            half = A.inbox_words(kind, world, m) // 2
            assert bool((inbox[kind][d][other:other + half] == A.sentinel(tag)).all())
        with pytest.raises(AssertionError):
            A.pull("sum", inbox["sum"][d], d, world, n, tag, n)


def test_granule_words_and_tags():
    w = torch.tensor([0, 1, -1, -(1 << 31), (1 << 31) - 1, 0x12345678], dtype=torch.int32)
    for tag in (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF):
        g = A.granules(w, tag)
        assert g.dtype == torch.int64
        assert torch.equal(A.words_of(g), w)
        assert A.tags_of(g).tolist() == [tag] * w.numel()
        for gi, wi in zip(g.tolist(), w.tolist()):
            assert gi & 0xFFFFFFFFFFFFFFFF == (wi & A.MASK32) | (tag << 32)
    for key in (0, 1, (1 << 64) - 1, 1 << 63, 0x0123456789ABCDEF, 0xFEDCBA9876543210):
        assert A.key_of_words(A.key_words(key)) == key
    assert A.tags_of(torch.tensor([A.sentinel(1)])).item() == 0xFFFFFFFF
    assert A.tags_of(torch.tensor([A.sentinel(0)])).item() == 0xFFFFFFFE


@pytest.mark.parametrize("kind,world,n", [("sum", 2, 1), ("sum", 8, 16389), ("key", 5, 2),
                                          ("gather", 3, 20011)])
def test_banks_of_consecutive_tags_are_disjoint(kind, world, n):
    """Also across the wrap 0xFFFFFFFF -> 0: the tag's parity flips there as anywhere."""
    half = A.inbox_words(kind, world, n) // 2
    for seq0 in (0, 1, 2, 0x7FFFFFFE, 0x7FFFFFFF, A.WRAP_SEQ0 - 1, A.WRAP_SEQ0, 0xFFFFFFFF):
        t0, t1, t2 = A.next_tag(seq0), A.next_tag(seq0 + 1), A.next_tag(seq0 + 2)
        assert t1 == (t0 + 1) & A.MASK32
        b0, b1, b2 = (A.bank_of(kind, world, n, t) for t in (t0, t1, t2))
        assert {b0, b1} == {0, half} and b2 == b0
        # the stale word of a bank carries the tag of two collectives ago
        assert A.tags_of(torch.tensor([A.sentinel(t2)])).item() == t0
    assert [A.next_tag(A.WRAP_SEQ0 + k) for k in range(3)] == [0xFFFFFFFF, 0, 1]
    assert A.as_i32(A.WRAP_SEQ0) == -2


def test_key_ref_is_unsigned():
    top = 1 << 63
    assert A.key_ref([top, top - 1]) == top
    assert A.key_ref(torch.tensor([A.as_i64(top), A.as_i64(top - 1)])) == top
    assert A.key_ref([0, (1 << 64) - 1, 5]) == (1 << 64) - 1
    assert A.as_i64(top) < 0


def test_key_rounds_cover_the_compare():
    for world in A.WORLDS:
        for rank in A.ranks_of(world):
            rounds = dict(A.key_rounds(world, rank))
            assert all(len(ks) == world and all(0 <= k < 1 << 64 for k in ks)
                       for ks in rounds.values())
            for m in range(world):       # the maximum sits at every rank once, unique
                ks = rounds[f"max at rank {m}"]
                assert ks.index(max(ks)) == m and ks.count(max(ks)) == 1
            ks = rounds[f"bit 63 at rank {rank}"]
            # a signed compare picks another key than the unsigned one
            assert max(ks, key=A.as_i64) != A.key_ref(ks) == ks[rank]
            for name in ("low word only, ascending", "low word only, descending"):
                assert len({k >> 32 for k in rounds[name]}) == 1 and len(set(rounds[name])) == world
            for name in ("high word only, ascending", "high word only, descending"):
                assert len({k & A.MASK32 for k in rounds[name]}) == 1
                assert len(set(rounds[name])) == world
            assert A.key_ref(rounds["all zero"]) == 0
            assert A.key_ref(rounds[f"2^64 - 1 at rank {rank}"]) == (1 << 64) - 1


def test_recipe_is_reproducible_and_wide():
    a, b = A.recipe(5, 257), A.recipe(5, 257)
    assert torch.equal(A.bits(a), A.bits(b)) and a.shape == (5, 257)
    big = A.recipe(8, 16389)
    assert float(big.abs().max()) > 1e3 and float(big.abs().min()) < 1e-4
    assert torch.isfinite(big).all()
    r = A.recipe(3, 255, rounds=4)
    assert r.shape == (4, 3, 255) and not torch.equal(r[0], r[1])


_DISCRIMINATING = [(w, n) for w in A.WORLDS if w >= 3 for n in A.SUM_N + [A.SUM_N_STRIDE]
                   if n >= 255 and (n != A.SUM_N_STRIDE or w in A.SUM_N_STRIDE_WORLDS)]


@pytest.mark.parametrize("world,n", _DISCRIMINATING + [(3, 4101), (8, 4101)])
def test_data_tells_the_two_orders_apart(world, n):
    """For every (world >= 3, n >= 255) case the GPU tests run, the own-partial-first sum
    differs bitwise from the ascending-rank sum on every tested rank >= 2 (never on ranks 0
    and 1, where the two orders are the same additions): the GPU test fails on a kernel that
    sums its own partial first."""
    rounds, out0 = A.sum_inputs(world, n)       # what test_ar_sum_one_rank runs
    for P in [*rounds, A.recipe(world, n)]:
        want = A.bits(A.sum_ref(P))
        for r in range(world):
            diff = int((A.bits(A.own_first_ref(P, r)) != want).sum())
            if r < 2:
                assert diff == 0
            elif r in A.ranks_of(world):
                assert diff > 0, (world, n, r)
                acc = A.bits(A.own_first_ref(P, r, out0)) != A.bits(A.sum_ref(P, out0))
                assert int(acc.sum()) > 0, (world, n, r)
        assert any(int((A.bits(A.own_first_ref(P, r)) != want).sum()) for r in range(2, world))


@pytest.mark.parametrize("world,n", sorted({(w, n) for w, _, n in A.sum_cases()}))
def test_sum_ref_within_the_sequential_bound_of_float64(world, n):
    """|sum_ref - sum_f64| <= (world - 1) 2^-24 sum|p|, the bound of sequential summation."""
    P = A.recipe(world, n)
    exact = P.double().sum(0)
    bound = (world - 1) * 2.0 ** -24 * P.double().abs().sum(0)
    err = (A.sum_ref(P).double() - exact).abs()
    assert bool((err <= bound).all()), float((err / bound).max())


def test_special_sum_rows():
    for world in A.WORLDS:
        s = A.sum_ref(A.special_sum_rows(world))
        inf = float("inf")
        assert s[0] == inf and s[1] == -inf and s[4] == inf and s[6] == inf
        assert A.bits(s)[2].item() == A.as_i32(0x80000000)      # -0.0 from every rank
        assert A.bits(s)[3].item() == 0 and A.bits(s)[7].item() == 0
        assert A.bits(s)[5].item() == world                     # world denormal steps
        assert not torch.isnan(s).any()


def test_shard_ranges_and_specials():
    for world in A.WORLDS:
        for V in (world, 2049, 20011, 1000 * world + 3):
            rng = A.shard_ranges(V, world)
            assert rng[0][0] == 0 and rng[-1][1] == V
            assert all(a[1] == b[0] for a, b in zip(rng, rng[1:]))
            assert all(b - a >= 1 for a, b in rng)
            if V % world:
                assert rng[-1][1] - rng[-1][0] > rng[0][1] - rng[0][0]
    x = A.with_specials(A.recipe(2, 100)[0])
    w = A.bits(x)
    for i, b in enumerate(A.SPECIAL_BITS):
        assert w[3 * i].item() == A.as_i32(b)
    assert len({b for b in A.SPECIAL_BITS if (b & 0x7F800000) == 0x7F800000 and b & 0x7FFFFF}) >= 4
