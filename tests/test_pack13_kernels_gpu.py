"""The lossless 13-bit bf16 packing on the device (pack13.hip, gemv_p13*.hip): the round trip
is bit-exact, the raw rows are those of the numpy rule (tests/_pack13.py), and every P13
decode kernel writes the same bits as its 16-bit twin (torch.equal on every output buffer),
for every instantiated (U, prefetch), with raw rows in a wave's first pair and in a later one."""
import itertools

import numpy as np
import pytest
import torch

import _pack13 as P

pytestmark = pytest.mark.gpu

EPS = 1e-5
TILE = P.TILE
HIP_INVALID = 1  # hipErrorInvalidValue


def _bits(t):
    return t.contiguous().view(torch.int16)


def _np_bits(t):
    return _bits(t).cpu().numpy().view(np.uint16)


def _force_raw(w, r):
    """Row r becomes a plain normal row with one value at its top * 2^-40: 20 h steps under
    the row's largest."""
    w[r] = (w[1].float() * 1.5).to(torch.bfloat16)
    w[r, 5] = (w[r].float().abs().max() * 2.0 ** -40).to(torch.bfloat16)


def _special_row(K, g):
    """Representable with every special: +-0, denormals, +-Inf, NaN payloads, and the full
    span of 15 codes (h = 113 .. 127: magnitudes 2^99 and up)."""
    e = torch.randint(226, 255, (K,), generator=g)            # exponents of h = 113 .. 127
    m = torch.randint(0, 128, (K,), generator=g)
    s = torch.randint(0, 2, (K,), generator=g)
    b = ((s << 15) | (e << 7) | m).numpy().astype(np.uint16)
    b[:15] = [(226 + 2 * i) << 7 for i in range(15)]           # one value per code
    b[15:23] = [0x0000, 0x8000, 0x0001, 0x807F, 0x7F80, 0xFF80, 0x7FC1, 0xFFFF]
    b[23:27] = [0x7F81, 0xFFAA, 0x0040, 0x8001]                # signalling NaNs, denormals
    return b


def _matrix(N, K, seed, raw_at=(), specials=False, dev="cuda"):
    """randn * 0.02 rows; when N allows row 2 all zero, 3 with top < 15 (negative base) and
    (`specials`) 0 the specials; `raw_at` rows forced raw."""
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(N, K, generator=g) * 0.02).to(torch.bfloat16)
    if N >= 5:
        if specials:
            w[0] = torch.from_numpy(_special_row(K, g).view(np.int16)).view(torch.bfloat16)
        w[2] = 0
        w[2, 7] = -0.0
        w[3] = (torch.randn(K, generator=g) * 2.0 ** -105).to(torch.bfloat16)
    for r in raw_at:
        _force_raw(w, r)
    return w.to(dev)


@pytest.mark.parametrize("N,K,raw_at", [(6, TILE, (4,)), (5, 2 * TILE, (4,)),
                                         (130, 4096, (4, 77, 129))])
def test_round_trip_and_raw_rule(cuda, N, K, raw_at):
    from cake_amd.ops import hip as K_
    w = _matrix(N, K, 100 + N, raw_at, specials=True)
    bits = _np_bits(w)
    want_raw = P.raw_rows(bits)
    assert not want_raw[:4].any() and want_raw[list(raw_at)].all()
    assert int(P.row_top(bits)[3]) < 15 and int(P.row_top(bits)[0]) == 127
    m = K_.pack13_rows(w)
    assert m.nraw == int(want_raw.sum())
    assert m.planes.numel() + (4 * N + 15) // 16 * 16 + m.nraw * K * 2 == K_.pack13_bytes(N, K, m.nraw)
    assert np.array_equal(m.hdr.cpu().numpy(), P.headers(bits, want_raw))
    # the planes of the packed rows are the reference's, a raw row's are zero
    planes = m.planes.cpu().numpy()
    ref = P.pack_planes(bits[~want_raw])
    assert np.array_equal(planes[~want_raw], ref)
    assert not planes[want_raw].any()
    assert torch.equal(_bits(m.raw), _bits(w[torch.from_numpy(want_raw).to(cuda)]))
    out = torch.full_like(w, 7.0)
    K_.unpack13_rows(m, out)
    assert torch.equal(_bits(out), _bits(w))


def test_pairing_kinds(cuda):
    """A raw row takes its partner with it: (i, i + hd / 2) of a head, (j, j + N / 2)."""
    from cake_amd.ops import hip as K_
    w = _matrix(64, TILE, 7, raw_at=(3, 40))
    bits = _np_bits(w)
    for kind, hd, pairs in (("adjacent", 0, {3, 2, 40, 41}), ("head_halves", 16, {3, 11, 40, 32}),
                            ("gate_up", 0, {3, 35, 40, 8})):
        want = P.raw_rows(bits, kind, hd)
        assert set(np.flatnonzero(want)) == pairs
        m = K_.pack13_rows(w, kind, hd)
        assert np.array_equal(m.hdr.cpu().numpy(), P.headers(bits, want))
        out = torch.empty_like(w)
        K_.unpack13_rows(m, out)
        assert torch.equal(_bits(out), _bits(w))


# ---- bit equality with the 16-bit kernels ------------------------------------------------

# the 16-bit kernels' defaults (gemv.hip; the library has no getter for them)
W16_DEFAULTS = {"qkv": (2, 4, 1024), "swiglu": (2, 4, 512), "x16": (4, 4, 1024),
                "norm_f32": (4, 4, 256), "x16s": (4, 4, 1024)}


@pytest.fixture
def tuning(cuda):
    from cake_amd.ops import hip as K_
    prev = {k: K_.get_gemv_p13_tuning(k) for k in K_.GEMV_P13_KINDS}
    yield K_
    for k, (U, pf, mb) in prev.items():
        K_.set_gemv_p13_tuning(k, U=U, prefetch=pf, max_blocks=mb)
    for k, (U, pf, mb) in W16_DEFAULTS.items():
        K_.set_gemv_tuning(k, U=U, prefetch=pf, max_blocks=mb)


def _set_all(K_, U, pf, mb):
    """(U, prefetch) of every P13 kind, and the grid cap of both formats: the twins are
    compared launch for launch, a pair taking the same place (a wave's first pair or a later
    one) in both — the 16-bit kernel's own (U, prefetch) do not change its results."""
    for k in K_.GEMV_P13_KINDS:
        K_.set_gemv_p13_tuning(k, U=U, prefetch=pf, max_blocks=mb)
        assert K_.get_gemv_p13_tuning(k) == (U, pf, mb)
    for k, (u16, pf16, _) in W16_DEFAULTS.items():
        K_.set_gemv_tuning(k, U=u16, prefetch=pf16, max_blocks=mb)


_cache = {}


def _inputs(K, cuda):
    key = K
    if key not in _cache:
        g = torch.Generator().manual_seed(K)
        _cache[key] = dict(resid=(torch.randn(K, generator=g) * 3).to(cuda),
                           nw=(1 + 0.1 * torch.randn(K, generator=g)).to(torch.bfloat16).to(cuda),
                           x16=torch.randn(K, generator=g).to(torch.bfloat16).to(cuda))
    return _cache[key]


def _check_x16_and_head(K_, K, N, raw_at, cuda):
    """gemv_x16 (accumulate and plain), gemv_norm_f32 and head_select over one matrix."""
    p = _inputs(K, cuda)
    w = _matrix(N, K, 31 * N + K, raw_at)
    m = K_.pack13_rows(w)
    assert m.nraw >= len(raw_at)
    for acc in (True, False):
        a = torch.full((N + 4,), 0.5, device=cuda)
        b = a.clone()
        K_.gemv(p["x16"], w, a[:N], acc)
        K_.gemv_p13(p["x16"], m, b[:N], acc)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), ("x16", acc)
    a, b = torch.full((N + 4,), 7.0, device=cuda), torch.full((N + 4,), 7.0, device=cuda)
    K_.norm_gemv_f32(p["resid"], p["nw"], EPS, w, a[:N])
    K_.norm_gemv_f32_p13(p["resid"], p["nw"], EPS, m, b[:N])
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "norm_f32"
    g = torch.Generator().manual_seed(N)
    table = (torch.randn(N, K, generator=g) * 2.0).to(torch.bfloat16).to(cuda)
    hist0 = torch.randint(0, N, (300,), generator=g, dtype=torch.int32)
    for penalty in (1.0, 1.1):
        sa, sb = _state(N, hist0, p["resid"], cuda), _state(N, hist0, p["resid"], cuda)
        for step in range(2):
            K_.head_select(sa["resid"], p["nw"], EPS, w, sa["logits"], sa["hist"], sa["hist_len"],
                           128, penalty, sa["slot"], sa["ticket"], sa["tok"], sa["pos"], embed=table)
            K_.head_select_p13(sb["resid"], p["nw"], EPS, m, sb["logits"], sb["hist"],
                               sb["hist_len"], 128, penalty, sb["slot"], sb["ticket"], sb["tok"],
                               sb["pos"], embed=table)
            for k in sa:  # token, history, pos, the logits and the gathered next row
                assert torch.equal(_raw(sa[k]), _raw(sb[k])), ("head_select", penalty, step, k)
            assert int(sb["hist_len"]) == 301 + step and int(sb["slot"]) == 0


def _raw(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _state(N, hist0, resid0, cuda):
    hist = torch.zeros(400, dtype=torch.int32, device=cuda)
    hist[:300] = hist0.to(cuda)
    return dict(hist=hist, hist_len=torch.tensor([300], dtype=torch.int32, device=cuda),
                tok=torch.zeros(1, dtype=torch.int32, device=cuda),
                pos=torch.tensor([299], dtype=torch.int32, device=cuda),
                slot=torch.zeros(1, dtype=torch.int64, device=cuda),
                ticket=torch.zeros(1, dtype=torch.int32, device=cuda),
                logits=torch.zeros(N, device=cuda), resid=resid0.clone())


def _check_swiglu(K_, K, I, raw_at, cuda):
    p = _inputs(K, cuda)
    w = _matrix(2 * I, K, 17 * I + K, raw_at)  # gate | up
    m = K_.pack13_rows(w, "gate_up")
    a = torch.full((I + 4,), 3.0, dtype=torch.bfloat16, device=cuda)
    b = a.clone()
    K_.swiglu(p["resid"], p["nw"], EPS, w[:I], w[I:], a[:I])
    K_.swiglu_p13(p["resid"], p["nw"], EPS, m.rows(0, I), m.rows(I, 2 * I), b[:I])
    assert torch.equal(_bits(a), _bits(b)), "swiglu"


def _check_qkv(K_, K, raw_at, cuda, nh=4, nkv=2, hd=16, S=64):
    p = _inputs(K, cuda)
    nq, nk = nh * hd, nkv * hd
    w = _matrix(nq + 2 * nk, K, 13 * K + nh, raw_at)  # q | k | v
    m = K_.pack13_rows(w, "head_halves", hd)
    inv_freq = (1.0 / (500000.0 ** (torch.arange(0, hd, 2).float() / hd))).to(cuda)
    for kv_fmt, pos in itertools.product((0, 1), (0, 37)):
        cdt = torch.uint8 if kv_fmt == 1 else torch.bfloat16
        out = []
        for packed in (False, True):
            q = torch.full((nq,), 9.0, device=cuda)
            kc = torch.zeros(nkv, S, hd, device=cuda).to(cdt)
            vc = torch.zeros(nkv, S, hd, device=cuda).to(cdt)
            pt = torch.tensor([pos], dtype=torch.int32, device=cuda)
            if packed:
                K_.qkv_rope_p13(p["resid"], p["nw"], EPS, m.rows(0, nq), m.rows(nq, nq + nk),
                                m.rows(nq + nk, nq + 2 * nk), inv_freq, pt, q, kc, vc, kv_fmt=kv_fmt)
            else:
                K_.qkv_rope(p["resid"], p["nw"], EPS, w[:nq], w[nq:nq + nk], w[nq + nk:], inv_freq,
                            pt, q, kc, vc, kv_fmt=kv_fmt)
            out.append((q.view(torch.int32), kc.view(torch.uint8), vc.view(torch.uint8)))
        for name, a, b in zip(("q", "kcache", "vcache"), *out):
            assert torch.equal(a, b), ("qkv_rope", kv_fmt, pos, name)
        assert int(out[1][1].count_nonzero()) > 0


# N = 5: one workgroup with an idle wave and a clamped last pair; 37: odd, several
# workgroups; 150 under a grid cap of 3: twelve waves walk 75 pairs (raw rows 8 and 9 are
# pair 4 — the first of wave 0 of workgroup 1 — and row 100 is pair 50: a later pair)
@pytest.mark.parametrize("K", [TILE, 4096])
@pytest.mark.parametrize("N,mb,raw_at", [(5, 1024, (4,)), (37, 1024, (8, 30)), (150, 3, (8, 100))])
def test_bit_equal_to_w16(tuning, cuda, K, N, mb, raw_at):
    K_ = tuning
    U, pf, _ = K_.get_gemv_p13_tuning("x16")
    _set_all(K_, U, pf, mb)
    _check_x16_and_head(K_, K, N, raw_at, cuda)
    _check_swiglu(K_, K, N, raw_at + (N + 1,), cuda)
    if N != 5:
        _check_qkv(K_, K, (0, 100), cuda)  # pairs (0, 8) and (100, 108): first and later
    torch.cuda.synchronize()


@pytest.mark.parametrize("U,pf", list(itertools.product((1, 2, 3), (0, 1, 2))))
def test_every_tuning_is_bit_equal(tuning, cuda, U, pf):
    """Every instantiated (U, prefetch), K = 3 tiles (U = 2 leaves a tail tile, prefetch 2 a
    one-tile main loop), under a grid cap of 3 and without one."""
    K_ = tuning
    assert (U in K_.GEMV_P13_U) and (pf in K_.GEMV_P13_PF)
    for mb in (3, 1024):
        _set_all(K_, U, pf, mb)
        _check_x16_and_head(K_, 3 * TILE, 61, (0, 50), cuda)
        _check_swiglu(K_, 3 * TILE, 61, (0, 111), cuda)
        _check_qkv(K_, 3 * TILE, (0, 100), cuda)
    torch.cuda.synchronize()


def test_tuning_refusals_and_defaults(tuning, cuda):
    from cake_amd.ops._lib import KernelError
    K_ = tuning
    for kind in K_.GEMV_P13_KINDS:
        U, pf, mb = K_.get_gemv_p13_tuning(kind)
        assert U in K_.GEMV_P13_U and pf in K_.GEMV_P13_PF and mb >= 1
    for bad in (dict(U=4), dict(prefetch=4), dict(max_blocks=0)):
        with pytest.raises(KernelError):
            K_.set_gemv_p13_tuning("x16", **bad)


def test_refusals(cuda):
    """K not a multiple of the tile, f16, and null planes: hipErrorInvalidValue, nothing run."""
    from cake_amd.ops import hip as K_
    from cake_amd.ops._lib import kernels
    L = kernels()
    st = torch.cuda.current_stream().cuda_stream
    N, K = 8, TILE
    w = _matrix(N, K, 3)
    m = K_.pack13_rows(w)
    x = torch.zeros(K, dtype=torch.bfloat16, device=cuda)
    resid, nw = torch.zeros(K, device=cuda), torch.ones(K, dtype=torch.bfloat16, device=cuda)
    out, act = torch.full((N,), 5.0, device=cuda), torch.zeros(N, dtype=torch.bfloat16, device=cuda)
    pl, hd, _ = m.args()
    p = lambda t: t.data_ptr()  # noqa: E731
    for dt, k, planes, hdr in ((0, K + 1024, pl, hd), (0, 1024, pl, hd), (1, K, pl, hd),
                               (0, K, None, hd), (0, K, pl, None)):
        assert L.cake_gemv_x16_p13(dt, p(x), planes, hdr, None, k, N, p(out), 0, st) == HIP_INVALID
        assert L.cake_gemv_norm_f32_p13(dt, p(resid), p(nw), EPS, planes, hdr, None, k, N, p(out),
                                        st) == HIP_INVALID
        assert L.cake_swiglu_p13(dt, p(resid), p(nw), EPS, planes, planes, hdr, hdr, None, None,
                                 k, N // 2, p(act), st) == HIP_INVALID
    assert L.cake_pack13_rows(0, p(w), N, 1024, 0, None, None, None, 0, st) == -HIP_INVALID
    assert L.cake_pack13_rows(0, p(w), N, K, 0, pl, None, None, 0, st) == -HIP_INVALID
    assert L.cake_pack13_rows(1, p(w), N, K, 3, None, None, None, 0, st) == -HIP_INVALID
    assert L.cake_unpack13_rows(None, hd, None, N, K, p(w), st) == HIP_INVALID
    assert K_.pack13_bytes(N, 1024, 0) == -1 and K_.pack13_bytes(N, K + 8, 0) == -1
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())
