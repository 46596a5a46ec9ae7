"""MXFP4 weight-only kernels (quant_mxfp4.hip, gemv_w4*.hip) against the plain-torch oracle:
ops/reference.py quant_rows_mxfp4 / dequant_rows_mxfp4 bit for bit, and f32 torch math on the
dequantised weights with the tolerances tests/test_fp8_kernels_gpu.py uses for the fp8 twins
(the accumulation is f32 in both)."""
import math

import pytest
import torch

from _mxfp4 import grid_matrix
from cake_amd.ops import reference as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
QUANT_SHAPES = [(5, 32), (257, 512), (64, 2080)]


def _tol(dt):
    return dict(atol=3e-2, rtol=3e-2) if dt == torch.bfloat16 else dict(atol=1e-2, rtol=1e-2)


def _rand(*shape, dt=torch.float32, std=1.0, dev="cuda"):
    return (torch.randn(*shape, device=dev) * std).to(dt)


def _quant(w16):
    """Oracle codes and scale bytes of a device matrix, on the device."""
    codes, e8 = R.quant_rows_mxfp4(w16.cpu())
    return codes.cuda(), e8.cuda()


def _w4(N, K, dt, std=0.02):
    """A drawn 16-bit matrix as (codes, scale bytes, dequantised f32)."""
    codes, e8 = _quant(_rand(N, K, dt=dt, std=std))
    return codes, e8, R.dequant_rows_mxfp4(codes, e8)


def _nibbles(codes):
    c = codes.to(torch.int64)
    return torch.stack((c & 15, c >> 4), dim=2).reshape(codes.shape[0], -1)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,K", QUANT_SHAPES)
def test_quant_rows_mxfp4(cuda, dt, N, K):
    from cake_amd.ops import hip as K_
    torch.manual_seed(30)
    w = _rand(N, K, dt=dt, std=0.02)
    w[0] = 0  # an all-zero row
    w[N - 1] = 0
    w[N - 1, K // 3] = -0.011  # a single non-zero
    w[1, :32] = w[1, :32].clamp(-0.03, 0.03)
    w[1, 5] = -0.03125  # a block whose amax sits exactly on a power of two
    w[2, K - 32:] = w[2, K - 32:].clamp(-0.0625, 0.0625)
    w[2, K - 1] = 0.0625
    w4 = torch.full((N, K // 2), 0xA5, dtype=torch.uint8, device=cuda)
    e8 = torch.full((N, K // 32), 0xFF, dtype=torch.uint8, device=cuda)
    K_.quant_rows_mxfp4(w, w4, e8)
    rc, rs = R.quant_rows_mxfp4(w.cpu())
    assert int(rs[1, 0]) == 127 - 5 - 2 and int(rs[2, -1]) == 127 - 4 - 2
    assert torch.equal(e8.cpu(), rs)
    assert bool((e8[0] == 127).all()) and int(w4[0].sum()) == 0
    assert int((e8 == 0xFF).sum()) == 0
    got, ref = _nibbles(w4.cpu()), _nibbles(rc)
    assert torch.equal(got & 7, ref & 7)
    nz = (ref & 7) != 0
    assert torch.equal(got[nz], ref[nz])  # signs wherever the magnitude is non-zero
    print(f"quant N={N} K={K} {dt}: codes != oracle {int((got != ref).sum())} (signed zeros)")


@pytest.mark.parametrize("N,K", QUANT_SHAPES)
def test_quant_rows_mxfp4_grid_is_bit_equal(cuda, N, K):
    from cake_amd.ops import hip as K_
    w, codes, scales = grid_matrix(N, K, torch.Generator().manual_seed(31))
    w4 = torch.empty((N, K // 2), dtype=torch.uint8, device=cuda)
    e8 = torch.empty((N, K // 32), dtype=torch.uint8, device=cuda)
    K_.quant_rows_mxfp4(w.cuda(), w4, e8)
    assert torch.equal(e8.cpu(), scales)
    assert torch.equal(w4.cpu(), codes)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,K", QUANT_SHAPES)
def test_dequant_rows_mxfp4(cuda, dt, N, K):
    """Bit-equal to the oracle: this is the check on the hardware convert's nibble order,
    values and scale (drawn codes, and a grid matrix holding every code with -0)."""
    from cake_amd.ops import hip as K_
    torch.manual_seed(32)
    drawn = _quant(_rand(N, K, dt=torch.bfloat16, std=0.02))
    _, gc, gs = grid_matrix(N, K, torch.Generator().manual_seed(33))
    for codes, e8 in (drawn, (gc.cuda(), gs.cuda())):
        out = torch.empty((N, K), dtype=dt, device=cuda)
        K_.dequant_rows_mxfp4(codes, e8, out)
        ref = R.dequant_rows_mxfp4(codes.cpu(), e8.cpu()).to(dt)
        assert torch.equal(out.cpu().view(torch.int16), ref.view(torch.int16))


# K = 512: 16 chunks, lanes 16-63 idle, only the tail loop; 2080: 65 chunks, one full pass
# at U = 1 + a one-chunk tail; 8192: the whole row in the deepest prefetch; N = 257: an odd
# last pair (the clamped second row must not be written); N = 6: fewer pairs than waves
GEMV_SHAPES = [(512, 257), (2080, 257), (8192, 257), (8192, 6), (512, 6)]


def _gemv_case(K_, cuda, dt, K, N):
    x = _rand(K, dt=dt)
    codes, e8, wd = _w4(N, K, dt)
    tol = dict(atol=2e-3 * math.sqrt(K / 256), rtol=1e-3)
    guard = torch.full((N + 8,), 7.0, device=cuda)  # rows past N stay untouched
    out = guard[:N]
    out.copy_(torch.randn(N, device=cuda))
    ref = out + wd @ x.float()
    K_.gemv_w4(x, codes, e8, out, accumulate=True)
    torch.testing.assert_close(out, ref, **tol)
    out2 = guard[:N]
    K_.gemv_w4(x, codes, e8, out2, accumulate=False)
    torch.testing.assert_close(out2, wd @ x.float(), **tol)
    assert bool((guard[N:] == 7.0).all())


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("K,N", GEMV_SHAPES)
def test_gemv_w4(cuda, dt, K, N):
    from cake_amd.ops import hip as K_
    torch.manual_seed(34)
    _gemv_case(K_, cuda, dt, K, N)


def _swiglu_case(K_, cuda, dt, K, I):
    resid = torch.randn(K, device=cuda)
    nw = (1 + 0.1 * torch.randn(K, device=cuda)).to(dt)
    cg, eg, wg = _w4(I, K, dt, std=0.05)
    cu, eu, wu = _w4(I, K, dt, std=0.05)
    act = torch.empty(I, device=cuda, dtype=dt)
    K_.swiglu_w4(resid, nw, 1e-5, cg, cu, eg, eu, act)
    x = R.rms_norm(resid, nw, 1e-5)
    torch.testing.assert_close(act.float(), R.silu_mul(wg @ x, wu @ x), **_tol(dt))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("K,I", [(512, 1000), (4096, 72)])
def test_swiglu_w4(cuda, dt, K, I):
    from cake_amd.ops import hip as K_
    torch.manual_seed(35)
    _swiglu_case(K_, cuda, dt, K, I)


def _qkv_case(K_, cuda, dt, H, nh, nkv, hd, pos, S=64):
    resid = torch.randn(H, device=cuda)
    nw = (1 + 0.1 * torch.randn(H, device=cuda)).to(dt)
    (cq, eq, wq), (ck, ek, wk), (cv, ev, wv) = (
        _w4(n * hd, H, dt, std=std) for n, std in ((nh, 0.05), (nkv, 0.4), (nkv, 0.006)))
    # the three scale arrays differ: a kernel reading q's scales for k fails
    assert not torch.equal(eq[:nkv * hd], ek) and not torch.equal(ek, ev)
    invf = R.inv_freq(hd, 500000.0).to(cuda)
    kc = torch.zeros(nkv, S, hd, device=cuda, dtype=dt)
    vc = torch.zeros_like(kc)
    q = torch.empty(nh * hd, device=cuda)
    p = torch.tensor([pos], dtype=torch.int32, device=cuda)
    K_.qkv_rope_w4(resid, nw, 1e-5, cq, ck, cv, eq, ek, ev, invf, p, q, kc, vc)
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


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("H,nh,nkv,hd", [(512, 8, 2, 64), (2048, 4, 1, 128)])
@pytest.mark.parametrize("pos", [0, 37])
def test_qkv_rope_w4(cuda, dt, H, nh, nkv, hd, pos):
    from cake_amd.ops import hip as K_
    torch.manual_seed(36)
    _qkv_case(K_, cuda, dt, H, nh, nkv, hd, pos)


@pytest.fixture
def w4_tuning(cuda):
    from cake_amd.ops import hip as K_
    prev = {k: K_.get_gemv_w4_tuning(k) for k in K_.GEMV_W4_KINDS}
    yield K_
    for k, (U, pf, mb) in prev.items():
        K_.set_gemv_w4_tuning(k, U=U, prefetch=pf, max_blocks=mb)


def test_gemv_w4_every_tuning(w4_tuning, cuda):
    """Every (U, prefetch) the dispatcher accepts, at a full grid and at a cap of 3 blocks
    (many pairs per wave), on the (2080, 257) and (8192, 6) gemv shapes (K = 8192 runs
    prefetch depth 4 and 2, K = 2080 falls back to none) plus a swiglu and a qkv case at
    K = 8192: every (U, prefetch) instantiation of the three kernels executes."""
    K_ = w4_tuning
    torch.manual_seed(37)
    dt = torch.bfloat16
    for U in (1, 2, 4):
        for pf in (0, 2, 4):
            for mb in (1024, 3):
                for kind in K_.GEMV_W4_KINDS:
                    K_.set_gemv_w4_tuning(kind, U=U, prefetch=pf, max_blocks=mb)
                    assert K_.get_gemv_w4_tuning(kind) == (U, pf, mb)
                _gemv_case(K_, cuda, dt, 2080, 257)
                _gemv_case(K_, cuda, dt, 8192, 6)
                if mb == 3:
                    _swiglu_case(K_, cuda, dt, 8192, 40)
                    _qkv_case(K_, cuda, dt, 8192, 2, 1, 64, 9, S=16)
    with pytest.raises(RuntimeError):
        K_.set_gemv_w4_tuning("x16", U=8, prefetch=4)
    with pytest.raises(RuntimeError):
        K_.set_gemv_w4_tuning("x16", U=2, prefetch=1)


def test_gemv_w4_block_scale_is_applied_per_block(cuda):
    """Raising one block's scale byte by 3 adds exactly 7 x that block's contribution (a
    power of two commutes with every rounding of the products): an ignored or mis-indexed
    block scale fails.  x is zero outside the probed block, so the sum is that block alone."""
    from cake_amd.ops import hip as K_
    torch.manual_seed(38)
    dt = torch.bfloat16
    for K, N, blk in [(512, 257, 5), (8192, 6, 200), (8192, 6, 64)]:
        codes, e8, _ = _w4(N, K, dt)
        x = torch.zeros(K, dtype=dt, device=cuda)
        x[blk * 32:(blk + 1) * 32] = _rand(32, dt=dt)
        a = torch.empty(N, device=cuda)
        b = torch.empty(N, device=cuda)
        K_.gemv_w4(x, codes, e8, a, accumulate=False)
        e2 = e8.clone()
        e2[:, blk] += 3
        e2[:, (blk + 1) % (K // 32)] -= 2  # a neighbour's scale must not matter
        K_.gemv_w4(x, codes, e2, b, accumulate=False)
        assert bool((a != 0).any())
        assert torch.equal(b, a * 8)


def test_w4_bad_shape_is_refused(cuda):
    """K % 32 != 0 (and K < 32): every launcher returns the error and writes nothing."""
    from cake_amd.ops import hip as K_
    from cake_amd.ops._lib import KernelError
    dt = torch.bfloat16
    K, N = 48, 8
    x = _rand(K, dt=dt)
    codes = torch.zeros((N, K // 2), dtype=torch.uint8, device=cuda)
    e8 = torch.full((N, K // 32), 127, dtype=torch.uint8, device=cuda)
    out = torch.full((N,), 3.0, device=cuda)
    with pytest.raises(KernelError):
        K_.gemv_w4(x, codes, e8, out, accumulate=False)
    w16 = _rand(N, K, dt=dt)
    w4 = torch.full((N, K // 2), 0x11, dtype=torch.uint8, device=cuda)
    s = torch.full((N, K // 32), 5, dtype=torch.uint8, device=cuda)
    with pytest.raises(KernelError):
        K_.quant_rows_mxfp4(w16, w4, s)
    with pytest.raises(KernelError):
        K_.quant_rows_mxfp4(_rand(N, 16, dt=dt), torch.zeros((N, 8), dtype=torch.uint8, device=cuda),
                            torch.zeros((N, 0), dtype=torch.uint8, device=cuda))
    o16 = torch.full((N, K), 2.0, dtype=dt, device=cuda)
    with pytest.raises(KernelError):
        K_.dequant_rows_mxfp4(codes, e8, o16)
    resid = torch.randn(K, device=cuda)
    nw = torch.ones(K, dtype=dt, device=cuda)
    act = torch.full((N,), 4.0, dtype=dt, device=cuda)
    with pytest.raises(KernelError):
        K_.swiglu_w4(resid, nw, 1e-5, codes, codes, e8, e8, act)
    hd = 8
    kc = torch.zeros(1, 4, hd, dtype=dt, device=cuda)
    vc = torch.zeros_like(kc)
    q = torch.full((hd,), 6.0, device=cuda)
    with pytest.raises(KernelError):
        K_.qkv_rope_w4(resid, nw, 1e-5, codes, codes, codes, e8, e8, e8,
                       R.inv_freq(hd, 500000.0).to(cuda),
                       torch.zeros(1, dtype=torch.int32, device=cuda), q, kc, vc)
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and bool((w4 == 0x11).all()) and bool((s == 5).all())
    assert bool((o16 == 2.0).all()) and bool((act == 4.0).all()) and bool((q == 6.0).all())
    assert int(kc.abs().sum()) == 0 and int(vc.abs().sum()) == 0
