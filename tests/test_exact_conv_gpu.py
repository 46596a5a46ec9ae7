"""Implicit-GEMM convolution (conv2d.hip) on integer operands (tests/_exact.py conv_case):
bit-equal to float64 F.conv2d.  The border pixels of x are large, so a padded tap that
reads a wrapped or neighbouring pixel instead of zero, a tap dropped at a split-K edge or
a pixel written to the wrong place cannot hide inside a tolerance."""
import functools

import pytest
import torch

import _exact as X

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
CFG_SPLITS = [(None, None), (0, 1), (3, 1), (1, 3), (2, 2), (4, 1), (5, 2), (6, 1), (7, 3),
              (8, 1), (9, 1), (10, 1), (11, 1), (12, 1), (13, 1)]


@functools.lru_cache(maxsize=None)
def _case(shape, dt):
    c = X.conv_case(*shape, dt)
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in c.items()}


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        bad = got != want
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} differ, first at {i}: "
                             f"got {float(got[i])}, want {float(want[i])}")


# the halo kernels (cfg 8-13) are stride-1 only
CONV_CASES = [(s, cfg, sp) for s in X.CONV_SHAPES for cfg, sp in CFG_SPLITS
              if not (cfg is not None and cfg >= 8 and s[6] != 1)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape,cfg,splits", CONV_CASES)
def test_exact_conv2d_nhwc(cuda, dt, shape, cfg, splits):
    """Every tile config (register-staged, LDS-DMA, halo) with its split counts: bias only,
    and bias + per-sample f32 bias + residual."""
    from cake_amd.ops import hip as K
    stride = shape[6]
    c = _case(shape, dt)
    kw = dict(stride=stride, pad=c["pad"], up=c["up"], cfg=cfg, splits=splits)
    _same(K.conv2d_nhwc(c["x"], c["wp"], c["b"], **kw), c["yb"].to(dt), "bias")
    _same(K.conv2d_nhwc(c["x"], c["wp"], **kw), c["y"].to(dt), "plain")
    _same(K.conv2d_nhwc(c["x"], c["wp"], c["b"], bias2=c["b2"], resid=c["r"], **kw),
          c["full"].to(dt), "bias + bias2 + resid")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("cfg,tile", [(8, (8, 16)), (8, (16, 8)), (8, (10, 12)), (8, (12, 10)),
                                      (10, (8, 8)), (10, (4, 16)), (10, (16, 4)),
                                      (12, (16, 16)), (12, (8, 32)), (13, (32, 8))])
def test_exact_conv2d_halo_tiles(cuda, dt, cfg, tile):
    """Every spatial tile shape of the halo kernels, with partial edge tiles."""
    from cake_amd.ops import hip as K
    c = _case(X.CONV_HALO_SHAPE, dt)
    _same(K.conv2d_nhwc(c["x"], c["wp"], c["b"], cfg=cfg, tile=tile), c["yb"].to(dt), "bias")
    _same(K.conv2d_nhwc(c["x"], c["wp"], c["b"], bias2=c["b2"], resid=c["r"], cfg=cfg, tile=tile),
          c["full"].to(dt), "bias + bias2 + resid")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", X.CONV_SMALL_IC)
def test_exact_conv2d_small_ic(cuda, dt, shape):
    """The direct 3x3 kernel for IC 3 / 4, stride 1 and 2, NHWC and planar (NCHW in, NCHW
    out)."""
    from cake_amd.ops import hip as K
    c = _case(shape, dt)
    stride = shape[6]
    _same(K.conv2d_nhwc(c["x"], c["wp"], c["b"], stride=stride), c["yb"].to(dt), "bias")
    _same(K.conv2d_nhwc(c["x"], c["wp"], c["b"], stride=stride, bias2=c["b2"], resid=c["r"]),
          c["full"].to(dt), "bias + bias2 + resid")
    y = K.conv2d_nhwc(c["x"].permute(0, 3, 1, 2).contiguous(), c["wp"], c["b"], stride=stride,
                      in_nchw=True, out_nchw=True)
    _same(y, c["yb"].to(dt).permute(0, 3, 1, 2).contiguous(), "NCHW in and out")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("cfg,splits", [(0, 1), (4, 2), (1, 3), (8, 1)])
def test_exact_conv2d_out_nchw(cuda, dt, cfg, splits):
    """conv_out-like (IC 320 -> OC 4) written straight into NCHW planes, incl. split-K."""
    from cake_amd.ops import hip as K
    c = _case(X.CONV_OUT_NCHW, dt)
    y = K.conv2d_nhwc(c["x"], c["wp"], c["b"], cfg=cfg, splits=splits, out_nchw=True)
    _same(y, c["yb"].to(dt).permute(0, 3, 1, 2).contiguous(), "out_nchw")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", X.CONV1X1_SMALL)
@pytest.mark.parametrize("layout", [0, 1, 2, 3])
def test_exact_conv1x1_small(cuda, dt, shape, layout):
    """The few-channel 1x1 conv in every input / output layout."""
    from cake_amd.ops import hip as K
    c = X.conv1x1_case(*shape, dt)
    x, w, b, ref = c["x"].cuda(), c["w"].cuda(), c["b"].cuda(), c["yb"].cuda().to(dt)
    in_nchw, out_nchw = bool(layout & 1), bool(layout & 2)
    xi = x.permute(0, 3, 1, 2).contiguous() if in_nchw else x
    y = K.conv1x1_small(xi, w, b, in_nchw=in_nchw, out_nchw=out_nchw)
    _same(y, ref.permute(0, 3, 1, 2).contiguous() if out_nchw else ref, f"layout {layout}")
