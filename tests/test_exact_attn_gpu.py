"""Decode attention (attn_core.h / attn_core2.h, the head-parallel kernel), MFMA flash
attention and attn512 on block-code inputs (tests/_exact.py): each query's softmax mass
sits exactly on the visible keys of one 16-key block, V is one-hot, so the output is 1/n
in n known columns and exactly 0 elsewhere.  One key dropped or counted twice at a split,
block or tile edge, a causal mask off by one, or a wrong kv head changes n or lights a
zero column -- errors of |v| / Tk that the Gaussian tests' tolerance cannot see."""
import ctypes
import functools
import math

import pytest
import torch

import _exact as X

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]


@pytest.fixture(params=[(1, 320), (2, 320), (2, 0)], ids=["core1", "core2", "core2-split"])
def attn_impl(request, cuda):
    """Both decode-attention cores; core 2 also with its one-split range off, so short
    contexts take the split + merge path too (as tests/test_kernels_gpu.py)."""
    from cake_amd.ops import hip as K_
    impl, single = request.param
    prev, prev_single = K_._ATTN_IMPL[0], K_._ATTN_SINGLE[0]
    K_.attn_set_impl(impl)
    K_.attn_set_single_max(single)
    yield impl
    K_.attn_set_impl(prev)
    K_.attn_set_single_max(prev_single)


@functools.lru_cache(maxsize=48)
def _cache(nkv, hd, Tk, S, phase, dt):
    return X.decode_case(nkv, hd, Tk, S, phase, dt, device="cuda")


class _Decode:
    """One set of decode buffers (workspace, tickets) kept across every launch of a test:
    each launch finds the previous launch's partials (other targets, other lengths)."""

    def __init__(self, nh, nkv, hd, dt, dev):
        from cake_amd.ops import hip as K_
        self.K, self.nh, self.nkv, self.hd, self.dt = K_, nh, nkv, hd, dt
        self.part = torch.zeros(K_.attn_workspace_numel(nh, hd, 0), device=dev)
        self.tickets = torch.zeros(2 * nkv + 2, dtype=torch.int32, device=dev)
        self.out = torch.empty(nh * hd, device=dev, dtype=dt)

    def run(self, bc, what, heads=None):
        p = torch.tensor([bc.live - 1], dtype=torch.int32, device=bc.device)
        for launch, t in enumerate(X.decode_targets(bc, self.nh)):
            q, expect, n, _ = X.block_code_queries(bc, t, X.ATTN_C[self.hd])
            self.out.fill_(float("nan"))
            qf = q.float().reshape(-1)
            if heads is None:
                self.K.attn_decode(qf, bc.k, bc.v, p, 1 / math.sqrt(self.hd), self.part,
                                   self.tickets, self.out)
            else:
                self.K.attn_decode_heads(qf, bc.k, bc.v, p, 1 / math.sqrt(self.hd), self.out,
                                         waves=heads[0], prefetch=heads[1])
            X.assert_block_code_output(self.out.view(self.nh, 1, self.hd), expect, n,
                                       f"{what} launch {launch}")
        assert not self.K.attn_error(self.tickets)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nh,nkv,hd", X.DECODE_SHAPES)
@pytest.mark.parametrize("min_keys", [64, 256])
def test_exact_attn_decode(cuda, attn_impl, dt, nh, nkv, hd, min_keys):
    """Every live length x block phase: blocks sit on and across every 16- / 64-key and
    split edge; every live block is some head's target; the heads of one kv head aim at
    different blocks (GQA mapping); the dead cache rows are NaN."""
    from cake_amd.ops import hip as K_
    d = _Decode(nh, nkv, hd, dt, cuda)
    K_.attn_set_min_keys(min_keys)
    try:
        for Tk, S in X.DECODE_TKS:
            for phase in (0, 8):
                d.run(_cache(nkv, hd, Tk, S, phase, dt), f"Tk {Tk} phase {phase}")
    finally:
        K_.attn_set_min_keys(64)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nh,nkv,hd", [(32, 8, 128), (8, 8, 64)])
@pytest.mark.parametrize("cap,target,prefetch", [(8, 16, 0), (16, 64, 0), (0, 4, 0), (0, 64, 0),
                                                 (0, 16, 1), (0, 16, 2)])
def test_exact_attn_decode_core2_settings(cuda, dt, nh, nkv, hd, cap, target, prefetch):
    """Core 2 under the knobs that change which keys a workgroup walks: a split cap below
    the split count the length wants (8 against 16 at Tk 2047; 16 against 64 at Tk 8190
    with a 64-split target), 4 and 64 target splits, 1 and 2 key blocks in flight."""
    from cake_amd.ops import hip as K_
    prev, prev_single = K_._ATTN_IMPL[0], K_._ATTN_SINGLE[0]
    d = _Decode(nh, nkv, hd, dt, cuda)
    try:
        K_.attn_set_impl(2)
        K_.attn_set_single_max(320)
        K_.attn_set_target_splits(target)
        K_.attn_set_prefetch(prefetch)
        if cap:
            assert K_.attn_splits(8190) > cap and (target > 16 or K_.attn_splits(2047) > cap)
        for Tk, S in [(65, 2048), (321, 2048), (1000, 2048), (2047, 2048), (8190, 8192)]:
            for phase in (0, 8):
                bc = _cache(nkv, hd, Tk, S, phase, dt)
                if cap:
                    with K_.attn_split_cap(cap):
                        d.run(bc, f"Tk {Tk} phase {phase}")
                else:
                    d.run(bc, f"Tk {Tk} phase {phase}")
    finally:
        K_.attn_set_target_splits(16)
        K_.attn_set_prefetch(0)
        K_.attn_set_impl(prev)
        K_.attn_set_single_max(prev_single)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nh,nkv,hd", X.DECODE_SHAPES)
@pytest.mark.parametrize("waves,prefetch", [(1, 2), (2, 2), (4, 2), (8, 2), (16, 2), (4, 4),
                                            (16, 4)])
def test_exact_attn_decode_heads(cuda, dt, nh, nkv, hd, waves, prefetch):
    """The head-parallel short-context kernel (one workgroup per query head) on the same
    caches: block edges (16 / 17 keys), a ragged tail, 601 keys walked by one workgroup."""
    d = _Decode(nh, nkv, hd, dt, cuda)
    for Tk in X.HEADS_TKS:
        for phase in (0, 8):
            d.run(_cache(nkv, hd, Tk, X.HEADS_S, phase, dt), f"Tk {Tk} phase {phase}",
                  heads=(waves, prefetch))


# ---------------------------------------------------------------------------
# flash attention
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=8)
def _flash_case(shape, phase, dt):
    return X.flash_case(*shape, phase, dt, device="cuda")


def _flash_run(shape, dt, what, launch=None):
    from cake_amd.ops import hip as K
    B, H, Hkv, N, M, D, causal, pos0 = shape
    for phase in (0, 8):
        q, k, v, expect, n = _flash_case(shape, phase, dt)
        out = torch.full((B, N, H, D), float("nan"), device=q.device, dtype=dt).transpose(1, 2)
        if launch is None:
            K.flash_attn(q, k, v, out, 1 / math.sqrt(D), causal, pos0)
        else:
            launch(q, k, v, out)
        X.assert_block_code_output(out, expect, n, f"{what} phase {phase}")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", X.FLASH_SHAPES)
@pytest.mark.parametrize("impl", [1, 2])
def test_exact_flash_attn(cuda, dt, shape, impl):
    """Both flash kernels: GQA, ragged rows and keys, padded head dims (40, 80, 160), causal
    with and without an offset.  Causal even rows aim at the block of their own diagonal
    key, so `key > qpos` against `key >= qpos` changes n."""
    from cake_amd.ops import hip as K
    K.flash_set_impl(impl)
    try:
        _flash_run(shape, dt, f"impl {impl}")
    finally:
        K.flash_set_impl(2)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", [s for s in X.FLASH_SHAPES if s[6]])
@pytest.mark.parametrize("pair_min", [1, 0])
def test_exact_flash_causal_pairing(cuda, dt, shape, pair_min):
    """Causal q-tile pairing forced on and off."""
    from cake_amd.ops import hip as K
    K.flash_set_pair_min(pair_min)
    try:
        _flash_run(shape, dt, f"pair_min {pair_min}")
    finally:
        K.flash_set_pair_min(512)


# Waves per workgroup of the 32x32x16 kernel.  The grids of FLASH_SHAPES are small, so auto
# (the tests above) picks 1 or 2 waves at every entry; production shapes run 4.  An override
# below the kernel's minimum (1 wave at D > 64) falls back to auto by design.
FLASH_NW = [1, 2, 4]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", X.FLASH_SHAPES)
@pytest.mark.parametrize("nw", FLASH_NW)
def test_exact_flash_attn_waves(cuda, dt, shape, nw):
    """test_exact_flash_attn's cases (auto = nw 0 there) with 1, 2 and 4 waves forced: the
    4-wave kernel, 128 query rows per workgroup, under the exact-arithmetic check."""
    from cake_amd.ops import hip as K
    K.flash_set_impl(2)
    K.flash_set_nw(nw)
    try:
        _flash_run(shape, dt, f"nw {nw}")
    finally:
        K.flash_set_nw(0)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", [s for s in X.FLASH_SHAPES if s[6]])
@pytest.mark.parametrize("pair_min", [1, 0])
@pytest.mark.parametrize("nw", FLASH_NW)
def test_exact_flash_causal_pairing_waves(cuda, dt, shape, pair_min, nw):
    """Causal q-tile pairing forced on and off at each tile size (32 nw query rows)."""
    from cake_amd.ops import hip as K
    K.flash_set_pair_min(pair_min)
    K.flash_set_nw(nw)
    try:
        _flash_run(shape, dt, f"pair_min {pair_min} nw {nw}")
    finally:
        K.flash_set_nw(0)
        K.flash_set_pair_min(512)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", X.FLASH_KSPLIT_SHAPES)
@pytest.mark.parametrize("ksplit", [2, 4])
def test_exact_flash_key_split(cuda, dt, shape, ksplit):
    """The non-causal key split (f32 partial rows + merge) forced to 2 and 4 splits at
    ragged key counts (M 513: a last split of one key; M 1000)."""
    from cake_amd.ops import hip as K
    K.flash_set_ksplit(ksplit)
    try:
        _flash_run(shape, dt, f"ksplit {ksplit}")
    finally:
        K.flash_set_ksplit(0)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", X.FLASH_FORCED_SPLIT_SHAPES)
@pytest.mark.parametrize("ksplit", [2, 4])
@pytest.mark.parametrize("pair_min", [1, 0])
def test_exact_flash_causal_forced_key_split(cuda, dt, shape, ksplit, pair_min):
    """The opt-in causal key split, paired and unpaired tiles."""
    from cake_amd.ops import hip as K
    B, H, Hkv, N, M, D, causal, pos0 = shape
    lib = K.kernels()
    ws = torch.empty(4 * B * H * N * (D + 1), device=cuda)

    def launch(q, k, v, out):
        st = [x for t in (q, k, v, out) for x in t.stride()[:3]]
        arr = (ctypes.c_longlong * 12)(*st)
        K.check(lib.cake_flash_attn_ws(K._dt(q), K._p(q), K._p(k), K._p(v), K._p(out), B, H, Hkv,
                                       N, M, D, ctypes.cast(arr, ctypes.c_void_p),
                                       1 / math.sqrt(D), 1, pos0, K._p(ws), ws.numel() * 4,
                                       K._stream()), "flash")
        torch.cuda.synchronize()
    K.flash_set_pair_min(pair_min)
    lib.cake_flash_set_ksplit(ksplit)
    try:
        _flash_run(shape, dt, f"ksplit {ksplit} pair_min {pair_min}", launch)
    finally:
        K.flash_set_pair_min(512)
        lib.cake_flash_set_ksplit(0)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,N,M", X.ATTN512_SHAPES)
def test_exact_attn512(cuda, dt, B, N, M):
    """Head-dim-512 attention (VAE mid-block): a key count below one tile and a ragged one."""
    from cake_amd.ops import hip as K
    q, k, v, expect, n = X.attn512_case(B, N, M, dt, device="cuda")
    out = torch.full((B, N, 512), float("nan"), device=cuda, dtype=dt)
    K.attn512(q, k, v, out, 1 / math.sqrt(512))
    X.assert_block_code_output(out, expect, n, "attn512")
