"""FP8 (e4m3) weight-only kernels (quant_fp8.hip, gemv_w8*.hip) against the plain-torch
oracle: ops/reference.py quant_rows_fp8 / dequant_rows_fp8, and f32 torch math on the
dequantised weights with the tolerances tests/test_kernels_gpu.py uses for each kernel's
16-bit twin (the accumulation is f32 in both)."""
import math

import pytest
import torch

from _fp8 import grid_matrix, half_spacing
from cake_amd.ops import reference as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
QUANT_SHAPES = [(5, 16), (257, 512), (64, 2064)]


def _tol(dt):
    return dict(atol=3e-2, rtol=3e-2) if dt == torch.bfloat16 else dict(atol=1e-2, rtol=1e-2)


def _rand(*shape, dt=torch.float32, std=1.0, dev="cuda"):
    return (torch.randn(*shape, device=dev) * std).to(dt)


def _quant(w16):
    """Oracle codes and scales of a device matrix, on the device."""
    codes, scale = R.quant_rows_fp8(w16.cpu())
    return codes.cuda(), scale.cuda()


def _w8(N, K, dt, std=0.02):
    """A drawn 16-bit matrix as (codes, scale, dequantised f32)."""
    codes, scale = _quant(_rand(N, K, dt=dt, std=std))
    return codes, scale, R.dequant_rows_fp8(codes, scale)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,K", QUANT_SHAPES)
def test_quant_rows_fp8(cuda, dt, N, K):
    from cake_amd.ops import hip as K_
    torch.manual_seed(20)
    w = _rand(N, K, dt=dt, std=0.02)
    w[0] = 0  # an all-zero row
    w[N - 1] = 0
    w[N - 1, K // 3] = -0.011  # a single non-zero
    w8 = torch.full((N, K), 0x7F, dtype=torch.uint8, device=cuda)
    scale = torch.full((N,), float("nan"), device=cuda)
    K_.quant_rows_fp8(w, w8, scale)
    rc, rs = R.quant_rows_fp8(w.cpu())
    assert torch.equal(scale.cpu(), rs)
    assert float(scale[0]) == 1.0 and int(w8[0].sum()) == 0
    assert int(((w8 & 0x7F) == 0x7F).sum()) == 0  # never the NaN code
    v = w.float().cpu() / rs[:, None]
    err = (v - w8.cpu().view(torch.float8_e4m3fn).float()).abs()
    ratio = float((err / half_spacing(v)).max())
    print(f"quant N={N} K={K} {dt}: max |v-q| / half-spacing {ratio}, "
          f"codes != torch: {int((w8.cpu() != rc).sum())}")
    assert bool((err <= half_spacing(v)).all()), ratio


@pytest.mark.parametrize("N,K", QUANT_SHAPES)
def test_quant_rows_fp8_grid_is_bit_equal(cuda, N, K):
    from cake_amd.ops import hip as K_
    w, codes, scale = grid_matrix(N, K, torch.Generator().manual_seed(21))
    w8 = torch.empty((N, K), dtype=torch.uint8, device=cuda)
    s = torch.empty(N, device=cuda)
    K_.quant_rows_fp8(w.cuda(), w8, s)
    assert torch.equal(s.cpu(), scale)
    assert torch.equal(w8.cpu(), codes)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,K", QUANT_SHAPES)
def test_dequant_rows_fp8(cuda, dt, N, K):
    from cake_amd.ops import hip as K_
    torch.manual_seed(22)
    codes, scale = _quant(_rand(N, K, dt=torch.bfloat16, std=0.02))
    out = torch.empty((N, K), dtype=dt, device=cuda)
    K_.dequant_rows_fp8(codes, scale, out)
    ref = R.dequant_rows_fp8(codes.cpu(), scale.cpu()).to(dt)
    assert torch.equal(out.cpu().view(torch.int16), ref.view(torch.int16))


# K = 512: 32 chunks, only the tail loop; 2064: 129 chunks, one full pass at U = 1 + a
# one-chunk tail; 4096: the whole row in the prefetch registers; N = 257: an odd last
# pair (the clamped second row must not be written); N = 6: fewer pairs than waves
GEMV_SHAPES = [(512, 257), (2064, 257), (4096, 257), (4096, 6), (512, 6)]


def _gemv_case(K_, cuda, dt, K, N):
    x = _rand(K, dt=dt)
    codes, scale, wd = _w8(N, K, dt)
    tol = dict(atol=2e-3 * math.sqrt(K / 256), rtol=1e-3)
    guard = torch.full((N + 8,), 7.0, device=cuda)  # rows past N stay untouched
    out = guard[:N]
    out.copy_(torch.randn(N, device=cuda))
    ref = out + wd @ x.float()
    K_.gemv_w8(x, codes, scale, out, accumulate=True)
    torch.testing.assert_close(out, ref, **tol)
    out2 = guard[:N]
    K_.gemv_w8(x, codes, scale, out2, accumulate=False)
    torch.testing.assert_close(out2, wd @ x.float(), **tol)
    assert bool((guard[N:] == 7.0).all())


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("K,N", GEMV_SHAPES)
def test_gemv_w8(cuda, dt, K, N):
    from cake_amd.ops import hip as K_
    torch.manual_seed(23)
    _gemv_case(K_, cuda, dt, K, N)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("K,I", [(512, 1000), (4096, 72)])
def test_swiglu_w8(cuda, dt, K, I):
    from cake_amd.ops import hip as K_
    torch.manual_seed(24)
    resid = torch.randn(K, device=cuda)
    nw = (1 + 0.1 * torch.randn(K, device=cuda)).to(dt)
    cg, sg, wg = _w8(I, K, dt, std=0.05)
    cu, su, wu = _w8(I, K, dt, std=0.05)
    act = torch.empty(I, device=cuda, dtype=dt)
    K_.swiglu_w8(resid, nw, 1e-5, cg, cu, sg, su, act)
    x = R.rms_norm(resid, nw, 1e-5)
    torch.testing.assert_close(act.float(), R.silu_mul(wg @ x, wu @ x), **_tol(dt))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("H,nh,nkv,hd", [(512, 8, 2, 64), (2048, 4, 1, 128)])
@pytest.mark.parametrize("pos", [0, 37])
def test_qkv_rope_w8(cuda, dt, H, nh, nkv, hd, pos):
    """Three different scale vectors (q, k and v rows are drawn with different spreads):
    a kernel reading q's scale for k fails."""
    from cake_amd.ops import hip as K_
    torch.manual_seed(25)
    S = 64
    resid = torch.randn(H, device=cuda)
    nw = (1 + 0.1 * torch.randn(H, device=cuda)).to(dt)
    (cq, sq, wq), (ck, sk, wk), (cv, sv, wv) = (
        _w8(n * hd, H, dt, std=std) for n, std in ((nh, 0.05), (nkv, 0.11), (nkv, 0.02)))
    assert not torch.equal(sq[:nkv * hd], sk) and not torch.equal(sk, sv)
    invf = R.inv_freq(hd, 500000.0).to(cuda)
    kc = torch.zeros(nkv, S, hd, device=cuda, dtype=dt)
    vc = torch.zeros_like(kc)
    q = torch.empty(nh * hd, device=cuda)
    p = torch.tensor([pos], dtype=torch.int32, device=cuda)
    K_.qkv_rope_w8(resid, nw, 1e-5, cq, ck, cv, sq, sk, sv, invf, p, q, kc, vc)
    x = R.rms_norm(resid, nw, 1e-5)
    posv = torch.tensor([pos], device=cuda)
    qr = R.rope((wq @ x).view(1, nh, hd), posv, invf).view(-1)
    kr = R.rope((wk @ x).view(1, nkv, hd), posv, invf).view(nkv, hd)
    vr = (wv @ x).view(nkv, hd)
    torch.testing.assert_close(q, qr, atol=2e-3, rtol=2e-3)
    torch.testing.assert_close(kc[:, pos].float(), kr, **_tol(dt))
    torch.testing.assert_close(vc[:, pos].float(), vr, **_tol(dt))
    assert kc[:, :pos].abs().sum() == 0 and kc[:, pos + 1:].abs().sum() == 0
    assert vc[:, :pos].abs().sum() == 0 and vc[:, pos + 1:].abs().sum() == 0


@pytest.fixture
def w8_tuning(cuda):
    from cake_amd.ops import hip as K_
    prev = {k: K_.get_gemv_w8_tuning(k) for k in K_.GEMV_W8_KINDS}
    yield K_
    for k, (U, pf, mb) in prev.items():
        K_.set_gemv_w8_tuning(k, U=U, prefetch=pf, max_blocks=mb)


@pytest.mark.parametrize("U,pf,mb", [(1, 0, 1024), (1, 2, 3), (2, 4, 1024), (4, 2, 1024),
                                     (4, 4, 3)])
def test_gemv_w8_tuning_loop(w8_tuning, cuda, U, pf, mb):
    """Every (U, prefetch) instantiation and a grid cap of 3 (many pairs per wave), on the
    gemv shapes plus one swiglu and one qkv case."""
    K_ = w8_tuning
    for kind in K_.GEMV_W8_KINDS:
        K_.set_gemv_w8_tuning(kind, U=U, prefetch=pf, max_blocks=mb)
        assert K_.get_gemv_w8_tuning(kind) == (U, pf, mb)
    torch.manual_seed(26)
    dt = torch.bfloat16
    for K, N in [(2064, 257), (4096, 100), (512, 6), (14336, 66)]:
        _gemv_case(K_, cuda, dt, K, N)
    K, I = 4096, 200
    resid = torch.randn(K, device=cuda)
    nw = (1 + 0.1 * torch.randn(K, device=cuda)).to(dt)
    x = R.rms_norm(resid, nw, 1e-5)
    cg, sg, wg = _w8(I, K, dt, std=0.05)
    cu, su, wu = _w8(I, K, dt, std=0.05)
    act = torch.empty(I, device=cuda, dtype=dt)
    K_.swiglu_w8(resid, nw, 1e-5, cg, cu, sg, su, act)
    torch.testing.assert_close(act.float(), R.silu_mul(wg @ x, wu @ x), **_tol(dt))
    nh, nkv, hd, pos = 4, 1, 128, 9
    (cq, sq, wq), (ck, sk, wk), (cv, sv, wv) = (
        _w8(n * hd, K, dt, std=std) for n, std in ((nh, 0.05), (nkv, 0.11), (nkv, 0.02)))
    invf = R.inv_freq(hd, 500000.0).to(cuda)
    kc = torch.zeros(nkv, 16, hd, device=cuda, dtype=dt)
    vc = torch.zeros_like(kc)
    q = torch.empty(nh * hd, device=cuda)
    K_.qkv_rope_w8(resid, nw, 1e-5, cq, ck, cv, sq, sk, sv, invf,
                   torch.tensor([pos], dtype=torch.int32, device=cuda), q, kc, vc)
    posv = torch.tensor([pos], device=cuda)
    torch.testing.assert_close(q, R.rope((wq @ x).view(1, nh, hd), posv, invf).view(-1),
                               atol=2e-3, rtol=2e-3)
    torch.testing.assert_close(kc[:, pos].float(),
                               R.rope((wk @ x).view(1, nkv, hd), posv, invf).view(nkv, hd),
                               **_tol(dt))
    torch.testing.assert_close(vc[:, pos].float(), (wv @ x).view(nkv, hd), **_tol(dt))
    with pytest.raises(RuntimeError):
        K_.set_gemv_w8_tuning("x16", U=8, prefetch=4)


def test_gemv_w8_scale_is_applied_per_row(cuda):
    """Scaling row n's scale by 2^+-3 scales output n by exactly that factor (a power of
    two commutes with every rounding): an ignored or mis-indexed scale fails."""
    from cake_amd.ops import hip as K_
    torch.manual_seed(27)
    dt = torch.bfloat16
    for K, N in [(512, 257), (4096, 6)]:
        x = _rand(K, dt=dt)
        codes, scale, _ = _w8(N, K, dt)
        f = torch.where(torch.arange(N, device=cuda) % 2 == 0, 8.0, 0.125)
        f[N // 2] = 1.0
        a = torch.empty(N, device=cuda)
        b = torch.empty(N, device=cuda)
        K_.gemv_w8(x, codes, scale, a, accumulate=False)
        K_.gemv_w8(x, codes, scale * f, b, accumulate=False)
        assert bool((a != 0).all())
        assert torch.equal(b, a * f)


def test_w8_bad_shape_is_refused(cuda):
    """K % 16 != 0: every launcher returns the error and writes nothing."""
    from cake_amd.ops import hip as K_
    from cake_amd.ops._lib import KernelError
    dt = torch.bfloat16
    K, N = 24, 8
    x = _rand(K, dt=dt)
    codes = torch.zeros((N, K), dtype=torch.uint8, device=cuda)
    scale = torch.ones(N, device=cuda)
    out = torch.full((N,), 3.0, device=cuda)
    with pytest.raises(KernelError):
        K_.gemv_w8(x, codes, scale, out, accumulate=False)
    w16 = _rand(N, K, dt=dt)
    w8 = torch.full((N, K), 0x11, dtype=torch.uint8, device=cuda)
    s = torch.full((N,), 5.0, device=cuda)
    with pytest.raises(KernelError):
        K_.quant_rows_fp8(w16, w8, s)
    o16 = torch.full((N, K), 2.0, dtype=dt, device=cuda)
    with pytest.raises(KernelError):
        K_.dequant_rows_fp8(codes, scale, o16)
    resid = torch.randn(K, device=cuda)
    nw = torch.ones(K, dtype=dt, device=cuda)
    act = torch.full((N,), 4.0, dtype=dt, device=cuda)
    with pytest.raises(KernelError):
        K_.swiglu_w8(resid, nw, 1e-5, codes, codes, scale, scale, act)
    hd = 8
    kc = torch.zeros(1, 4, hd, dtype=dt, device=cuda)
    vc = torch.zeros_like(kc)
    q = torch.full((hd,), 6.0, device=cuda)
    with pytest.raises(KernelError):
        K_.qkv_rope_w8(resid, nw, 1e-5, codes, codes, codes, scale, scale, scale,
                       R.inv_freq(hd, 500000.0).to(cuda),
                       torch.zeros(1, dtype=torch.int32, device=cuda), q, kc, vc)
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and bool((w8 == 0x11).all()) and bool((s == 5.0).all())
    assert bool((o16 == 2.0).all()) and bool((act == 4.0).all()) and bool((q == 6.0).all())
    assert int(kc.abs().sum()) == 0 and int(vc.abs().sum()) == 0
