"""FP8 (e4m3) KV cache kernels: decode attention over code caches (bit-equal to the 16-bit
kernel on the codes' values, and exact on block-code caches), the KV write of the three
fused QKV GEMVs, and the prefill write / read.  Oracle: reference.quant_kv_fp8."""
import functools
import math

import pytest
import torch

import _exact as X
import _kv8 as KV
from cake_amd.ops import reference as R

pytestmark = pytest.mark.gpu

DTYPES = KV.DTYPES
TKS = [1, 15, 16, 17, 63, 65, 320, 321, 1000, 2047]
S = 2048


@pytest.fixture
def core2(cuda):
    """Core 2 (the only core with an fp8 twin), settings restored afterwards."""
    from cake_amd.ops import hip as K_
    prev, prev_single = K_._ATTN_IMPL[0], K_._ATTN_SINGLE[0]
    K_.attn_set_impl(2)
    yield K_
    K_.attn_set_impl(prev)
    K_.attn_set_single_max(prev_single)


class _Buffers:
    def __init__(self, K_, nh, nkv, hd, dt, dev):
        self.part = torch.zeros(K_.attn_workspace_numel(nh, hd, 0), device=dev)
        self.tickets = torch.zeros(2 * nkv + 2, dtype=torch.int32, device=dev)
        self.out = torch.empty(nh * hd, device=dev, dtype=dt)


# ---------------------------------------------------------------------------
# decode attention
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=4)
def _gauss(nkv, hd):
    k8, v8 = KV.gaussian_codes(nkv, S, hd, seed=100 + nkv + hd)
    return k8.cuda(), v8.cuda()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nh,nkv,hd", [(8, 2, 64), (8, 8, 64), (32, 8, 128), (64, 8, 128)])
def test_attn_decode_kv8_equals_16bit_twin(cuda, core2, dt, nh, nkv, hd):
    """Same source, same split walk, exact widening: the output over the code caches is the
    16-bit kernel's output over caches holding the codes' values, bit for bit — at every
    live length, in the one-split and the split + merge range, capped and uncapped.  Dead
    rows hold the NaN code / NaN.  Each kernel keeps its own workspace and tickets."""
    K_ = core2
    base_k, base_v = _gauss(nkv, hd)
    b8, b16 = _Buffers(K_, nh, nkv, hd, dt, cuda), _Buffers(K_, nh, nkv, hd, dt, cuda)
    torch.manual_seed(7)
    scale = 1 / math.sqrt(hd)
    for Tk in TKS:
        k8, v8 = KV.with_dead_rows(base_k, Tk), KV.with_dead_rows(base_v, Tk)
        k16, v16 = KV.widen_codes(k8, dt), KV.widen_codes(v8, dt)
        assert bool(torch.isnan(v16[:, Tk:].float()).all())
        q = torch.randn(nh * hd, device=cuda)
        p = torch.tensor([Tk - 1], dtype=torch.int32, device=cuda)
        for single in (320, 0):
            K_.attn_set_single_max(single)
            for cap in (0, 8):
                b8.out.fill_(float("nan"))
                b16.out.fill_(float("nan"))
                with K_.attn_split_cap(cap):
                    K_.attn_decode_kv8(q, k8, v8, p, scale, b8.part, b8.tickets, b8.out)
                    K_.attn_decode(q, k16, v16, p, scale, b16.part, b16.tickets, b16.out)
                what = f"Tk {Tk} single {single} cap {cap}"
                assert bool(torch.isfinite(b16.out.float()).all()), what
                assert torch.equal(b8.out.view(torch.int16), b16.out.view(torch.int16)), what
    assert not K_.attn_error(b8.tickets) and not K_.attn_error(b16.tickets)


@functools.lru_cache(maxsize=48)
def _block_cache(nkv, hd, Tk, phase, dt):
    bc = X.decode_case(nkv, hd, Tk, S, phase, dt, device="cuda")
    return bc, KV.block_code_codes(bc)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nh,nkv,hd", X.DECODE_SHAPES)
@pytest.mark.parametrize("single", [320, 0])
def test_attn_decode_kv8_closed_form(cuda, core2, dt, nh, nkv, hd, single):
    """Block-code caches as codes: 1/n in the n columns of the target block's visible keys,
    exactly 0 elsewhere.  Successive launches on one workspace aim at other blocks, so a
    merge that picked up the previous launch's partials lights a zero column."""
    K_ = core2
    K_.attn_set_single_max(single)
    b = _Buffers(K_, nh, nkv, hd, dt, cuda)
    for Tk in TKS:
        for phase in (0, 8):
            bc, (k8, v8) = _block_cache(nkv, hd, Tk, phase, dt)
            p = torch.tensor([Tk - 1], dtype=torch.int32, device=cuda)
            for launch, t in enumerate(X.decode_targets(bc, nh)):
                q, expect, n, _ = X.block_code_queries(bc, t, X.ATTN_C[hd])
                b.out.fill_(float("nan"))
                K_.attn_decode_kv8(q.float().reshape(-1), k8, v8, p, 1 / math.sqrt(hd), b.part,
                                   b.tickets, b.out)
                X.assert_block_code_output(b.out.view(nh, 1, hd), expect, n,
                                           f"Tk {Tk} phase {phase} launch {launch}")
    assert not K_.attn_error(b.tickets)


def test_attn_decode_kv8_refuses_core_1(cuda, core2):
    from cake_amd.ops._lib import KernelError
    K_ = core2
    k8 = torch.zeros(2, 64, 64, dtype=torch.uint8, device=cuda)
    b = _Buffers(K_, 8, 2, 64, torch.bfloat16, cuda)
    p = torch.zeros(1, dtype=torch.int32, device=cuda)
    K_.attn_set_impl(1)
    with pytest.raises(KernelError):
        K_.attn_decode_kv8(torch.zeros(8 * 64, device=cuda), k8, k8.clone(), p, 0.125, b.part,
                           b.tickets, b.out)


# ---------------------------------------------------------------------------
# the KV write of the fused QKV GEMVs
# ---------------------------------------------------------------------------

FILL8 = 0x55


def _qkv_weights(variant, dt, nh, nkv, hd, H, dev):
    """(launch(pos, q_out, kc, vc, kv_fmt), ) over weights whose K and V matrices are the
    first nkv * hd rows of Q (scales included): K's and V's f32 dot products are then the
    kernel's own q dot products."""
    from cake_amd.ops import hip as K_
    n = nkv * hd
    w = (torch.randn(nh * hd, H, device=dev) * 0.05).to(dt)
    resid = torch.randn(H, device=dev)
    nw = (1 + 0.1 * torch.randn(H, device=dev)).to(dt)
    invf = R.inv_freq(hd, 500000.0).to(dev)
    if variant == "w16":
        wk = w[:n].clone()

        def launch(p, q, kc, vc, kv_fmt):
            K_.qkv_rope(resid, nw, 1e-5, w, wk, wk.clone(), invf, p, q, kc, vc, kv_fmt=kv_fmt)
    elif variant == "w8":
        codes, scale = R.quant_rows_fp8(w.cpu())
        codes, scale = codes.to(dev), scale.to(dev)
        ck, sk = codes[:n].clone(), scale[:n].clone()

        def launch(p, q, kc, vc, kv_fmt):
            K_.qkv_rope_w8(resid, nw, 1e-5, codes, ck, ck.clone(), scale, sk, sk.clone(), invf, p,
                           q, kc, vc, kv_fmt=kv_fmt)
    else:
        codes, e8 = R.quant_rows_mxfp4(w.cpu())
        codes, e8 = codes.to(dev), e8.to(dev)
        ck, ek = codes[:n].clone(), e8[:n].clone()

        def launch(p, q, kc, vc, kv_fmt):
            K_.qkv_rope_w4(resid, nw, 1e-5, codes, ck, ck.clone(), e8, ek, ek.clone(), invf, p,
                           q, kc, vc, kv_fmt=kv_fmt)
    return launch


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("variant", ["w16", "w8", "w4"])
@pytest.mark.parametrize("H,nh,nkv,hd", [(256, 4, 1, 64), (1024, 8, 8, 128), (4096, 32, 8, 128)])
def test_qkv_kv_write_is_the_oracle_of_the_kernels_own_f32(cuda, dt, variant, H, nh, nkv, hd):
    torch.manual_seed(31)
    Sq, n = 1024, nkv * hd
    launch = _qkv_weights(variant, dt, nh, nkv, hd, H, cuda)

    def run(pos, kv_fmt):
        p = torch.tensor([pos], dtype=torch.int32, device=cuda)
        q = torch.full((nh * hd,), float("nan"), device=cuda)
        if kv_fmt == 1:
            kc = torch.full((nkv, Sq, hd), FILL8, dtype=torch.uint8, device=cuda)
        else:
            kc = torch.full((nkv, Sq, hd), 7.0, dtype=dt, device=cuda)
        vc = kc.clone()
        launch(p, q, kc, vc, kv_fmt)
        return q, kc, vc

    v_row0 = None
    for pos in (0, 5, 777):
        q0, _, _ = run(pos, 0)
        q1, k8, v8 = run(pos, 1)
        q2, k16, v16 = run(pos, 2)
        assert bool(torch.isfinite(q0).all())
        assert torch.equal(q1, q0) and torch.equal(q2, q0), f"pos {pos}: q_out changed"
        want = R.quant_kv_fp8(q0[:n].cpu()).view(nkv, hd).to(cuda)
        got = k8[:, pos]
        print(f"{variant} pos {pos}: K codes off {int((got != want).sum())} of {n}, "
              f"max code steps {int(KV.code_steps(got, want).max())}")
        assert torch.equal(got, want), f"pos {pos}: K codes"
        if pos == 0:  # RoPE at position 0 is the identity: V's f32 values are q_out's
            assert torch.equal(v8[:, 0], want), "V codes at pos 0"
            v_row0 = v8[:, 0].clone()
        else:         # V does not depend on the position
            assert torch.equal(v8[:, pos], v_row0), f"pos {pos}: V codes"
        for c8 in (k8, v8):  # every other row keeps its fill byte
            rest = torch.cat([c8[:, :pos], c8[:, pos + 1:]], dim=1)
            assert bool((rest == FILL8).all()), f"pos {pos}: a row other than pos was written"
        # kv_fmt 2: the codes' values as 16 bits, other rows untouched
        assert torch.equal(k16[:, pos], KV.widen_codes(got, dt))
        assert torch.equal(v16[:, pos], KV.widen_codes(v8[:, pos], dt))
        rest = torch.cat([k16[:, :pos], k16[:, pos + 1:], v16[:, :pos], v16[:, pos + 1:]], dim=1)
        assert bool((rest == 7.0).all())


# ---------------------------------------------------------------------------
# prefill write and read
# ---------------------------------------------------------------------------

ROPE_SHAPES = [(8, 2, 128, False), (4, 1, 64, False), (4, 2, 64, True)]  # nh, nkv, hd, scalar


def _rope_inputs(T, nh, nkv, hd, dt, scalar, dev):
    """q, k, v as column slices of one fused projection output; `scalar`: a row stride that
    is no multiple of 8 elements, which takes the scalar fallback kernel."""
    ncol = (nh + 2 * nkv) * hd
    ld = ncol + (4 if scalar else 0)
    qkv = torch.randn(T, ld, device=dev).to(dt)
    return (qkv[:, :nh * hd], qkv[:, nh * hd:(nh + nkv) * hd], qkv[:, (nh + nkv) * hd:ncol])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nh,nkv,hd,scalar", ROPE_SHAPES)
@pytest.mark.parametrize("T", [1, 7, 130])
@pytest.mark.parametrize("pos0", [0, 33])
def test_rope_kv_fp8_write_and_dequant(cuda, dt, nh, nkv, hd, scalar, T, pos0):
    from cake_amd.ops import hip as K_
    torch.manual_seed(T + pos0)
    Sp = 256
    q, k, v = _rope_inputs(T, nh, nkv, hd, dt, scalar, cuda)
    invf = R.inv_freq(hd, 500000.0).to(cuda)
    rows = slice(pos0, pos0 + T)
    # the 16-bit kernel's q is what the twins must leave in q
    qv = torch.empty(T, q.stride(0), device=cuda, dtype=dt)[:, :nh * hd]
    qv.copy_(q)
    K_.rope_kv(qv, k, v, invf, pos0, torch.zeros(nkv, Sp, hd, device=cuda, dtype=dt),
               torch.zeros(nkv, Sp, hd, device=cuda, dtype=dt))

    def run(kv_fmt):
        buf = torch.empty(T, q.stride(0), device=cuda, dtype=dt)
        qq = buf[:, :nh * hd]
        qq.copy_(q)
        if kv_fmt == 1:
            kc = torch.full((nkv, Sp, hd), FILL8, dtype=torch.uint8, device=cuda)
        else:
            kc = torch.full((nkv, Sp, hd), 7.0, dtype=dt, device=cuda)
        vc = kc.clone()
        K_.rope_kv(qq, k, v, invf, pos0, kc, vc, kv_fmt=kv_fmt)
        return qq, kc, vc

    q1, k8, v8 = run(1)
    q2, k16, v16 = run(2)
    # q is still roped in place in 16 bits: the f32 rotation rounded once (the 16-bit kernel
    # may fuse a multiply-add, so it can differ in the last bit), the same in both formats
    assert torch.equal(q1, q2)
    assert int(X.ulp_distance(q1.contiguous(), qv.contiguous()).max()) <= 1
    # V: quant of the 16-bit value widened to f32 — exact
    want_v = R.quant_kv_fp8(v.float().cpu()).view(T, nkv, hd).transpose(0, 1).to(cuda)
    assert torch.equal(v8[:, rows], want_v)
    # K: quant of the f32 rotation; one code step allowed within one f32 ulp of a boundary
    qr, kr = KV.rope_reference_f32(q.reshape(T, nh, hd), k.reshape(T, nkv, hd), invf, pos0)
    q_off = int((q1.reshape(T, nh, hd) != qr.to(dt)).sum())
    print(f"q elements off the rounded f32 reference: {q_off} of {qr.numel()}")
    assert q_off <= 1e-3 * qr.numel()
    kr = kr.transpose(0, 1).contiguous().cpu()
    want_k = R.quant_kv_fp8(kr)
    got_k = k8[:, rows].cpu()
    steps = KV.code_steps(got_k, want_k)
    off = steps > 0
    excused = off & (steps == 1) & KV.near_boundary(kr)
    share = float(off.float().mean())
    print(f"K codes: {int(off.sum())} of {off.numel()} off ({share:.2e}), {int(excused.sum())} "
          f"within an ulp of a boundary, max steps {int(steps.max())}")
    assert bool((off == excused).all()), "a K code off without a rounding boundary next to it"
    assert share <= 1e-3
    # rows outside [pos0, pos0 + T) keep the fill
    for c8 in (k8, v8):
        assert bool((c8[:, :pos0] == FILL8).all()) and bool((c8[:, pos0 + T:] == FILL8).all())
    # kv_fmt 2 == the values of kv_fmt 1's codes
    assert torch.equal(k16[:, rows], KV.widen_codes(k8[:, rows], dt))
    assert torch.equal(v16[:, rows], KV.widen_codes(v8[:, rows], dt))
    assert bool((k16[:, :pos0] == 7.0).all()) and bool((k16[:, pos0 + T:] == 7.0).all())
    assert bool((v16[:, :pos0] == 7.0).all()) and bool((v16[:, pos0 + T:] == 7.0).all())
    # the prefill read: rows [0, Tk) widened exactly, rows >= Tk of the scratch untouched
    Tk = pos0 + T
    s_k = torch.full((nkv, Sp, hd), 3.0, dtype=dt, device=cuda)
    s_v = torch.full((nkv, Sp, hd), 3.0, dtype=dt, device=cuda)
    K_.dequant_kv_fp8(k8, v8, Tk, s_k, s_v)
    assert torch.equal(s_k[:, :Tk], KV.widen_codes(k8[:, :Tk], dt))
    assert torch.equal(s_v[:, :Tk], KV.widen_codes(v8[:, :Tk], dt))
    assert bool((s_k[:, Tk:] == 3.0).all()) and bool((s_v[:, Tk:] == 3.0).all())


@pytest.mark.parametrize("dt", DTYPES)
def test_dequant_kv_fp8_every_code(cuda, dt):
    """All 256 codes through the prefill read (NaN codes give NaN), several kv heads."""
    from cake_amd.ops import hip as K_
    nkv, Sp, hd = 3, 40, 64
    g = torch.Generator().manual_seed(3)
    k8 = torch.randint(0, 256, (nkv, Sp, hd), generator=g, dtype=torch.int32).to(torch.uint8)
    k8.view(-1)[:256] = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    v8 = k8.flip(1).contiguous()
    k8, v8 = k8.cuda(), v8.cuda()
    s_k = torch.full((nkv, Sp, hd), 3.0, dtype=dt, device=cuda)
    s_v = s_k.clone()
    K_.dequant_kv_fp8(k8, v8, 37, s_k, s_v)
    for got, codes in ((s_k, k8), (s_v, v8)):
        want = KV.widen_codes(codes[:, :37], dt)
        assert torch.equal(torch.isnan(got[:, :37].float()), torch.isnan(want.float()))
        assert torch.equal(torch.nan_to_num(got[:, :37].float()), torch.nan_to_num(want.float()))
        assert bool((got[:, 37:] == 3.0).all())
