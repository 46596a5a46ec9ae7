"""The exact-arithmetic builders (tests/_exact.py) on the CPU, at every shape the GPU tests
use: operands representable, partial sums below 2^24, attention score gaps above 110,
closed-form expectation == f32 reference (each asserted inside the builders: a case that
falls short raises), and the integer GEMM outputs really exercise the 16-bit rounding."""
import math

import pytest
import torch

import _exact as X

DTYPES = [torch.bfloat16, torch.float16]


def test_int_operands_representable_or_raise():
    for dt, top in X.EXACT_INT.items():
        t = X.int_operands((64, 64), -top, top, dt, 0)
        assert torch.equal(t.double(), t.double().round()) and float(t.abs().max()) <= top
        with pytest.raises(AssertionError):
            X.int_operands((4096,), -2 * top - 1, 2 * top + 1, dt, 0)
    t = X.int_operands((1000,), -8, 8, torch.bfloat16, 1, scale=1 / 8, sparsity=0.5)
    assert torch.equal((t.double() * 8).round(), t.double() * 8)
    assert 0.4 < float((t == 0).float().mean()) < 0.7
    with pytest.raises(ValueError):
        X.int_operands((4,), -1, 1, torch.bfloat16, 0, scale=0.3)


def test_exact_linear_refuses_inexact_operands():
    x = X.int_operands((4, 1024), -256, 256, torch.bfloat16, 0)
    w = X.int_operands((4, 1024), -256, 256, torch.bfloat16, 1)
    with pytest.raises(AssertionError):      # 1024 * 256 * 256 = 2^26 units
        X.exact_linear(x, w)
    with pytest.raises(AssertionError):      # not a multiple of the unit
        X.exact_linear(torch.full((1, 8), 0.5), torch.ones(1, 8))


def test_ulp_distance():
    for dt in DTYPES:
        a = torch.tensor([1.0, -1.0, 0.0, 3.0], dtype=dt)
        up = torch.nextafter(a.float(), torch.full((4,), 9.0)).to(dt)  # f32 step: rounds back
        assert int(X.ulp_distance(a, up).max()) == 0
        bits = a.view(torch.int16) + torch.tensor([1, 1, 1, 2], dtype=torch.int16)
        assert X.ulp_distance(a, bits.view(dt)).tolist() == [1, 1, 1, 2]
        assert int(X.ulp_distance(torch.tensor([0.0], dtype=dt), torch.tensor([-0.0], dtype=dt))) == 0


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M,N,K,splits", X.GEMM_SHAPES + [s + (2,) for s in X.PAIR_SHAPES])
def test_gemm_cases(dt, M, N, K, splits):
    c = X.gemm_case(M, N, K, dt)
    assert float(c["x"].abs().max()) <= 8 and K * 64 + 1128 < 2 ** 24
    if dt == torch.bfloat16 and K >= 320:
        # the outputs exercise the rounding: many are not representable, some are exact ties
        for name in ("y", "yb", "ybr16"):
            frac, ties = X.rounding_coverage(c[name], dt)
            assert frac >= 0.25 and ties >= 1, (name, frac, ties)
    a = X.act_case(M, N, K, dt)
    assert float(a["yb"].abs().max()) <= X.ACT_LIMIT
    assert float((a["yb"] != 0).float().mean()) >= 0.5
    for name in ("silu", "quick_gelu", "gelu", "swiglu", "geglu"):
        # the yardstick itself: f32 torch, rounded, against the float64 value, rounded
        # (both GELUs far below zero are y (1 + erf / tanh) / 2 with the sum cancelling in
        # f32: there the yardstick is coarse, and act_allowance() widens the bound only there)
        d = X.ulp_distance(a["f32"][name].to(dt), a[name].to(dt))
        if name in ("gelu", "geglu"):
            d = d[a["pre"][name] >= -3]
        assert int(d.max()) <= 1, (name, int(d.max()))
        lim = X.act_allowance(a, name, dt)
        assert int(lim.min()) == 1 and lim.shape == a[name].shape


def test_rounding_coverage_counts_ties():
    ref = torch.tensor([257.0, 258.0, 256.0, 259.0])     # bf16 step 2 above 256
    frac, ties = X.rounding_coverage(ref, torch.bfloat16)
    assert frac == 0.5 and ties == 2


@pytest.mark.parametrize("dt", DTYPES)
def test_gemv_cases(dt):
    for K in X.GEMV_KS:
        for N in X.GEMV_NS:
            c = X.gemv_case(K, N, dt)
            assert c["y"].shape == (N,) and c["yacc"].dtype == torch.float32
    from cake_amd.ops import reference as R
    for K in X.GEMV_FMT_KS:
        for N in X.GEMV_NS:
            c = X.gemv_fmt_case("w8", K, N, dt)   # raises unless exact
            assert torch.equal(R.dequant_rows_fp8(*c["quant"]), c["w"])
            assert c["quant"][1].unique().numel() > (1 if N > 1 else 0)
            c = X.gemv_fmt_case("w4", K, N, dt)
            assert torch.equal(R.dequant_rows_mxfp4(*c["quant"]), c["w"])
            assert (c["quant"][1].min(), c["quant"][1].max()) == (125, 129) or N * K // 32 < 64
            assert float(c["x"].abs().max()) == (8 if K <= 4096 else 6)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", X.CONV_SHAPES + [X.CONV_HALO_SHAPE, X.CONV_OUT_NCHW]
                         + X.CONV_SMALL_IC)
def test_conv_cases(dt, shape):
    c = X.conv_case(*shape, dt)
    x = c["x"].float()
    assert float(x[:, 0].abs().min()) >= 24 and float(x[:, :, -1].abs().min()) >= 24
    if shape[1] > 2 and shape[2] > 2:
        assert float(x[:, 1:-1, 1:-1].abs().max()) <= 4
    if dt == torch.bfloat16:
        frac, _ = X.rounding_coverage(c["full"], dt)
        assert frac >= 0.25, frac


@pytest.mark.parametrize("dt", DTYPES)
def test_conv1x1_cases(dt):
    for shape in X.CONV1X1_SMALL:
        X.conv1x1_case(*shape, dt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nh,nkv,hd", X.DECODE_SHAPES)
def test_decode_cases(dt, nh, nkv, hd):
    for Tk, S in X.DECODE_TKS + [(t, X.HEADS_S) for t in X.HEADS_TKS]:
        for phase in (0, 8):
            bc = X.decode_case(nkv, hd, Tk, S, phase, dt)
            assert torch.isnan(bc.v[:, Tk:].float()).all() and torch.isfinite(bc.v[:, :Tk].float()).all()
            assert torch.equal(bc.k.float().abs(), torch.ones_like(bc.k.float()))
            seen = set()
            prev = None
            for t in X.decode_targets(bc, nh):
                q, e, n, gap = X.block_code_queries(bc, t, X.ATTN_C[hd])
                assert gap >= X.MIN_GAP
                seen.update(t.view(-1).tolist())
                g = t.view(nkv, nh // nkv)
                if bc.live_blocks >= nh // nkv:     # heads of one kv head differ
                    assert all(len(set(row.tolist())) == nh // nkv for row in g)
                if bc.live_blocks > 1 and prev is not None:
                    assert not torch.equal(t, prev)
                prev = t
                # 1/n in n columns, 0 elsewhere
                assert torch.equal((e != 0).sum(-1), n)
                want = (1.0 / n.double()).float()[..., None].expand_as(e)
                assert torch.equal(e[e != 0], want[e != 0])
            assert seen == set(range(bc.live_blocks))


def test_block_code_raises_on_small_gap():
    t = torch.zeros(1, 1, dtype=torch.long)
    with pytest.raises(AssertionError, match="gap"):      # c too small for the gap
        X.block_code_attention(D=64, keys=2048, targets=t, c=2.0, dtype=torch.bfloat16)
    with pytest.raises(AssertionError, match="no visible key"):
        X.block_code_attention(D=64, keys=64, live=16, targets=t + 2, c=64.0, dtype=torch.bfloat16)


@pytest.mark.parametrize("D,keys,c,gap", [(64, 2048, 32.0, 110), (128, 8192, 32.0, 150),
                                          (40, 1024, 64.0, 150), (80, 300, 32.0, 150),
                                          (160, 300, 16.0, 150), (512, 4096, 16.0, 250)])
def test_block_code_settings(D, keys, c, gap):
    """Every block of the context as a target at once: the worst gap of the setting."""
    nb = keys // 16
    q, k, v, e, n, g, bc = X.block_code_attention(D=D, keys=keys, targets=torch.arange(nb)[None, :],
                                                  c=c, dtype=torch.bfloat16)
    assert g >= gap and int(n.min()) == 16 and torch.equal(e[e != 0], torch.full((nb * 16,), 1 / 16))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", X.FLASH_SHAPES + X.FLASH_KSPLIT_SHAPES)
def test_flash_cases(dt, shape):
    B, H, Hkv, N, M, D, causal, pos0 = shape
    for phase in (0, 8):
        q, k, v, e, n = X.flash_case(*shape, phase, dt)
        assert q.shape == (B, H, N, D) and k.shape == (B, Hkv, M, D) and e.shape == (B, H, N, D)
        assert torch.isfinite(v.float()).all()
        assert int(n.min()) >= 1 and int(n.max()) <= 16
        if causal:   # the diagonal rows see only part of their block
            assert int((n[:, :, ::2] < 16).sum()) > N // 4
            assert math.isclose(float(e[0, 0, 0].sum()), 1.0)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,N,M", X.ATTN512_SHAPES)
def test_attn512_cases(dt, B, N, M):
    q, k, v, e, n = X.attn512_case(B, N, M, dt)
    assert q.shape == (B, N, 512) and k.shape == (B, M, 512) and e.shape == (B, N, 512)
    assert torch.equal((e != 0).sum(-1), n)
