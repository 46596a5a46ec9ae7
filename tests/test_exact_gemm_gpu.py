"""MFMA GEMM (gemm.hip, every tile config) and the decode GEMV on integer operands whose
products and partial sums are exact in f32 (tests/_exact.py): the result is known to the
bit, so one k element dropped, read twice or misindexed, or an epilogue that truncates
instead of rounding to nearest even, fails -- where the Gaussian tests' tolerance hides
it.  Activation epilogues: exact pre-activation, float64 activation, within 1 ulp."""
import functools

import pytest
import torch

import _exact as X

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
CFGS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25,
        26, 27]


@functools.lru_cache(maxsize=None)
def _gemm_case(M, N, K, dt):
    return X.gemm_case(M, N, K, dt, device="cuda")


@functools.lru_cache(maxsize=None)
def _act_case(M, N, K, dt):
    return X.act_case(M, N, K, dt, device="cuda")


def _same(got, want, what):
    if not torch.equal(got, want):
        bad = got != want
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} differ, first at {i}: "
                             f"got {float(got[i])}, want {float(want[i])}")


def _refused(G, cfg, K):
    return cfg in G.K64_ONLY and K % 64 != 0


def test_cfg_list_is_complete(cuda):
    from cake_amd.ops import gemm as G
    assert sorted(G.CFG_TILES) == CFGS


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("M,N,K,splits", X.GEMM_SHAPES)
def test_exact_linear_epilogues(cuda, dt, cfg, M, N, K, splits):
    """store (+ bias), store32, resid32 and add16, bit-equal.  add16 is ONE rounding of the
    f32 sum y + bias + resid."""
    from cake_amd.ops import gemm as G
    c = _gemm_case(M, N, K, dt)
    x, w, b = c["x"], c["w"], c["b"]
    kw = dict(cfg=cfg, splits=splits)
    if _refused(G, cfg, K):  # refused, not wrong
        from cake_amd.ops._lib import KernelError
        with pytest.raises(KernelError):
            G.linear(x, w, b, **kw)
        return
    _same(G.linear(x, w, b, **kw), c["yb"].to(dt), "store + bias")
    _same(G.linear(x, w, **kw), c["y"].to(dt), "store")
    o32 = torch.full((M, N), float("nan"), device=cuda)
    G.linear(x, w, b, epi="store32", resid=o32, **kw)
    _same(o32, c["yb"], "store32 + bias")
    o32.fill_(float("nan"))
    G.linear(x, w, epi="store32", resid=o32, **kw)
    _same(o32, c["y"], "store32")
    r = c["r32"].clone()
    G.linear(x, w, b, epi="resid32", resid=r, **kw)
    _same(r, c["ybr32"], "resid32 + bias")
    r = c["r32"].clone()
    G.linear(x, w, epi="resid32", resid=r, **kw)
    _same(r, c["yr32"], "resid32")
    _same(G.linear(x, w, b, epi="add16", resid=c["r16"], **kw), c["ybr16"].to(dt), "add16")


def _act_check(got, case, name, dt):
    d = X.ulp_distance(got, case[name].to(dt))
    lim = X.act_allowance(case, name, dt)
    print(f"{name} {dt}: kernel vs float64 {int(d.max())} ulp, f32 torch vs float64 "
          f"{int(lim.max()) - 1} ulp")
    bad = d > lim
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{name}: {int(bad.sum())} outputs beyond their bound, first at {i}: "
                             f"operand {float(case['pre'][name][i])}, got {float(got[i])}, want "
                             f"{float(case[name][i])} ({int(d[i])} ulp, allowed {int(lim[i])})")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("M,N,K,splits", X.GEMM_SHAPES)
def test_exact_linear_activations(cuda, dt, cfg, M, N, K, splits):
    """silu / quick_gelu / gelu / swiglu / geglu on an exact pre-activation (|y| <= 16)
    against the float64 activation rounded to the dtype: 1 ulp, plus the f32-torch
    yardstick's own distance where that is not 0 (X.act_allowance)."""
    from cake_amd.ops import gemm as G
    from cake_amd.ops._lib import KernelError
    c = _act_case(M, N, K, dt)
    x, w, b = c["x"], c["w"], c["b"]
    kw = dict(cfg=cfg, splits=splits)
    if _refused(G, cfg, K):
        with pytest.raises(KernelError):
            G.linear(x, w, b, epi="silu", **kw)
        return
    for name in ("silu", "quick_gelu", "gelu"):
        _act_check(G.linear(x, w, b, epi=name, **kw), c, name, dt)
    if cfg in G.NO_GATED and splits == 1:
        # 80-column wave tiles: the in-kernel gated epilogue is refused, not wrong (split-K
        # runs it in the finalize launch, which gates any tile's partial rows)
        with pytest.raises(KernelError):
            G.linear(x, c["w2"], epi="swiglu", **kw)
        return
    _act_check(G.linear(x, c["w2"], epi="swiglu", **kw), c, "swiglu", dt)
    _act_check(G.linear(x, c["w2"], c["b2"], epi="geglu", **kw), c, "geglu", dt)


@pytest.mark.parametrize("dt", DTYPES)
def test_exact_strided_views(cuda, dt):
    """q|k|v column slices as inputs (row stride 3 x 320), 3-D token tensors, and an output
    written into a column slice whose neighbouring columns stay untouched."""
    from cake_amd.ops import gemm as G
    qkv = X.int_operands((2, 50, 3 * 320), -8, 8, dt, 11, device="cuda")
    w = X.int_operands((640, 320), -8, 8, dt, 12, device="cuda")
    b = X.int_operands((640,), -32, 32, dt, 13, device="cuda")
    for s in range(3):
        v = qkv[..., 320 * s:320 * (s + 1)]
        ref = X.exact_linear(v.reshape(-1, 320), w, b)
        _same(G.linear(v, w, b), ref.to(dt).view(2, 50, 640), f"slice {s}")
        for col in (0, 640, 1280):
            out = torch.full((100, 3 * 640), 7.0, device=cuda, dtype=dt)
            G.linear(v.reshape(100, 320), w, b, out=out[:, col:col + 640])
            _same(out[:, col:col + 640], ref.to(dt), f"slice {s} -> columns {col}")
            keep = torch.ones(3 * 640, dtype=torch.bool, device=cuda)
            keep[col:col + 640] = False
            assert bool((out[:, keep] == 7.0).all()), "neighbouring columns written"
        o32 = torch.full((100, 640 + 8), 7.0, device=cuda)
        G.linear(v.reshape(100, 320), w, b, epi="store32", resid=o32[:, :640])
        _same(o32[:, :640], ref, "strided f32 output")
        assert bool((o32[:, 640:] == 7.0).all())


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("cfg", [22, 23, 24, 25, 26, 27])
@pytest.mark.parametrize("M,N,K", X.PAIR_SHAPES)
def test_exact_four_wave_split_pair(cuda, dt, cfg, M, N, K):
    """The in-kernel split-K pair of the four-wave tiles (gemm_4w.h) at the smallest shapes
    that take it: one or two 256-wide tiles, one 64-element k step (K 128) or two (K 256)
    per half.  Bit-equal, three calls in a row (the tile counters re-arm)."""
    from cake_amd.ops import gemm as G
    bm, bn = G.CFG_TILES[cfg]
    ntiles = -(-M // bm) * -(-N // bn)
    assert int(G._lib().cake_gemm_ws_floats(cfg, 2, M, N, K, 0)) == ntiles * bm * bn, \
        "this shape does not take the in-kernel pair"
    c = _gemm_case(M, N, K, dt)
    for it in range(3):
        _same(G.linear(c["x"], c["w"], c["b"], cfg=cfg, splits=2), c["yb"].to(dt), f"store, call {it}")
        r = c["r32"].clone()
        G.linear(c["x"], c["w"], epi="resid32", resid=r, cfg=cfg, splits=2)
        _same(r, c["yr32"], f"resid32, call {it}")
        _same(G.linear(c["x"], c["w"], c["b"], epi="add16", resid=c["r16"], cfg=cfg, splits=2),
              c["ybr16"].to(dt), f"add16, call {it}")


GEMV_DEFAULTS = {"qkv": (2, 4, 1024), "swiglu": (2, 4, 512), "x16": (4, 4, 1024),
                 "norm_f32": (4, 4, 256), "x16s": (4, 4, 1024)}


@pytest.fixture
def gemv_tuning():
    from cake_amd.ops import hip as K_
    yield K_
    for kind, (u, pf, mb) in GEMV_DEFAULTS.items():
        K_.set_gemv_tuning(kind, U=u, prefetch=pf, max_blocks=mb)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("max_blocks", [None, 3])
@pytest.mark.parametrize("K", X.GEMV_KS)
def test_exact_gemv(cuda, gemv_tuning, dt, max_blocks, K):
    """Decode GEMV (f32 out [+]= W x), bit-equal: the plain and split x prologues (K 1792 /
    2048 / 3584 / 4096 / 14336), one 8-element k group (K 8), idle waves (N 1, 6), a ragged
    row count (257); default launch geometry and a grid capped at 3 blocks."""
    K_ = gemv_tuning
    if max_blocks is not None:
        for kind, (u, pf, _) in GEMV_DEFAULTS.items():
            K_.set_gemv_tuning(kind, U=u, prefetch=pf, max_blocks=max_blocks)
    for N in X.GEMV_NS:
        c = X.gemv_case(K, N, dt, device="cuda")
        out = c["out0"].clone()
        K_.gemv(c["x"], c["w"], out, accumulate=True)
        _same(out, c["yacc"], f"accumulate, N {N}")
        out = torch.full((N,), float("nan"), device=cuda)
        K_.gemv(c["x"], c["w"], out, accumulate=False)
        _same(out, c["y"], f"plain, N {N}")


@pytest.fixture
def quant_gemv_tuning():
    from cake_amd.ops import hip as K_
    prev8 = {k: K_.get_gemv_w8_tuning(k) for k in K_.GEMV_W8_KINDS}
    prev4 = {k: K_.get_gemv_w4_tuning(k) for k in K_.GEMV_W4_KINDS}
    yield K_
    for k, (U, pf, mb) in prev8.items():
        K_.set_gemv_w8_tuning(k, U=U, prefetch=pf, max_blocks=mb)
    for k, (U, pf, mb) in prev4.items():
        K_.set_gemv_w4_tuning(k, U=U, prefetch=pf, max_blocks=mb)


@functools.lru_cache(maxsize=None)
def _gemv_fmt_case(fmt, K, N, dt):
    return X.gemv_fmt_case(fmt, K, N, dt, device="cuda")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("max_blocks", [None, 3])
@pytest.mark.parametrize("K", X.GEMV_FMT_KS)
@pytest.mark.parametrize("fmt", ["w8", "w4"])
def test_exact_gemv_formats(cuda, quant_gemv_tuning, fmt, dt, max_blocks, K):
    """The fp8 and MXFP4 decode GEMVs (f32 out [+]= dequant(W) x), bit-equal to exact_linear
    on the dequantised weights: integer x, fp8 codes that are integers with power-of-two
    row scales, every e2m1 code with e8m0 bytes 125 .. 129 varying per 32-block
    (_exact.gemv_fmt_case).  K 32 is one MXFP4 chunk (most of the wave idle in the tail
    loop), 2048 / 4096 / 14336 the split x prologues (14336 the largest 16-bit one); idle
    waves (N 1, 6), a ragged row count (257); default launch geometry and a grid capped at
    3 blocks, where waves loop to pairs other than their first (the scales that are not
    preloaded)."""
    K_ = quant_gemv_tuning
    get, put, run = {"w8": (K_.get_gemv_w8_tuning, K_.set_gemv_w8_tuning, K_.gemv_w8),
                     "w4": (K_.get_gemv_w4_tuning, K_.set_gemv_w4_tuning, K_.gemv_w4)}[fmt]
    if max_blocks is not None:
        u, pf, _ = get("x16")
        put("x16", U=u, prefetch=pf, max_blocks=max_blocks)
    for N in X.GEMV_NS:
        c = _gemv_fmt_case(fmt, K, N, dt)
        out = c["out0"].clone()
        run(c["x"], *c["quant"], out, accumulate=True)
        _same(out, c["yacc"], f"{fmt} accumulate, N {N}")
        out = torch.full((N,), float("nan"), device=cuda)
        run(c["x"], *c["quant"], out, accumulate=False)
        _same(out, c["y"], f"{fmt} plain, N {N}")
