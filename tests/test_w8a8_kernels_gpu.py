"""cake_gemm_w8a8 (gemm_w8a8.hip): the fp8 x fp8 MFMA GEMM of the quantised prefill.

One-hot rows pin the lane-to-k map and the neutral hardware block scale; integer codes with
power-of-two scales give results known to the bit for every tile shape and epilogue; random
codes over the whole format are judged by the rule of tests/_w8a8.py, whose constant a
single-instruction probe checks against the hardware's own summation."""
import functools

import pytest
import torch

import _exact as X
import _ulp as U
import _w8a8 as W

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
CFGS = [0, 1]
HIP_INVALID = "hipError 1"


def _dev(c, dev):
    return {k: v.to(dev) if torch.is_tensor(v) else v for k, v in c.items()}


@functools.lru_cache(maxsize=None)
def _exact(M, N, K):
    return _dev(W.exact_case(M, N, K), "cuda")


@functools.lru_cache(maxsize=None)
def _gated(M, N, K):
    return _dev(W.gated_case(M, N, K), "cuda")


def _same(got, want, what):
    if not torch.equal(got, want):
        bad = got != want
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} differ, first at {i}: "
                             f"got {float(got[i])}, want {float(want[i])}")


def test_cfg_list_is_complete(cuda):
    from cake_amd.ops import hip as K
    assert K.gemm_w8a8_num_cfgs() == len(CFGS)


@pytest.mark.parametrize("cfg", [-1] + CFGS)
def test_one_hot_rows_pin_the_k_map_and_the_unit_scale(cuda, cfg):
    """C[m, n] == sa[m] * sw[n] * B[n, m], bit for bit: row m of A is 1.0 at k = m only."""
    from cake_amd.ops import hip as K
    c = _dev(W.one_hot_case(), cuda)
    out = torch.zeros(256, 256, device=cuda)
    K.gemm_w8a8(c["a8"], c["sa"], c["w8"], c["sw"], out, "resid32", cfg=cfg)
    _same(out, c["want"], f"one-hot, cfg {cfg}")
    # and with the roles swapped (B one-hot): the two operands share the map
    out.zero_()
    K.gemm_w8a8(c["w8"], c["sw"], c["a8"], c["sa"], out, "resid32", cfg=cfg)
    _same(out, c["want"].T.contiguous(), f"one-hot transposed, cfg {cfg}")


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("K_", W.KS)
@pytest.mark.parametrize("N", W.NS)
@pytest.mark.parametrize("M", W.MS)
def test_exact_store_and_resid32(cuda, M, N, K_, cfg):
    """Integer codes, power-of-two scales: the float64 result rounded once (store, both
    dtypes) and the exact f32 sum with an integer residual (resid32)."""
    from cake_amd.ops import hip as K
    c = _exact(M, N, K_)
    for dt in DTYPES:
        out = torch.full((M, N), float("nan"), device=cuda, dtype=dt)
        K.gemm_w8a8(c["a8"], c["sa"], c["w8"], c["sw"], out, "store", cfg=cfg)
        _same(out, c["want"].to(dt), f"store {dt}")
    r = c["r32"].clone()
    K.gemm_w8a8(c["a8"], c["sa"], c["w8"], c["sw"], r, "resid32", cfg=cfg)
    _same(r, c["want_r"].float(), "resid32")
    # a strided output with an odd row stride (the scalar store path): the columns behind N
    # stay as they were
    wide = torch.full((M, N + 3), 7.0, device=cuda, dtype=torch.bfloat16)
    K.gemm_w8a8(c["a8"], c["sa"], c["w8"], c["sw"], wide[:, :N], "store", cfg=cfg)
    _same(wide[:, :N], c["want"].to(torch.bfloat16), "strided store")
    assert bool((wide[:, N:] == 7.0).all())


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("K_", W.KS)
@pytest.mark.parametrize("N", W.NS)
@pytest.mark.parametrize("M", W.MS)
def test_exact_swiglu(cuda, M, N, K_, cfg):
    """Exact pre-activations (|y| <= 16), float64 silu(gate) * up rounded to the dtype: 1 ulp,
    plus the f32-torch yardstick's own distance where that is not 0 (X.act_allowance)."""
    from cake_amd.ops import hip as K
    c = _gated(M, N, K_)
    for dt in DTYPES:
        out = torch.full((M, N), float("nan"), device=cuda, dtype=dt)
        K.gemm_w8a8(c["a8"], c["sa"], c["w8"], c["sw"], out, "swiglu", cfg=cfg)
        case = {"swiglu": c["want"], "f32": {"swiglu": c["f32"]}, "pre": {"swiglu": c["pre"]}}
        d = X.ulp_distance(out, c["want"].to(dt))
        lim = X.act_allowance(case, "swiglu", dt)
        bad = d > lim
        if bad.any():
            i = tuple(bad.nonzero()[0].tolist())
            raise AssertionError(f"swiglu {dt}: {int(bad.sum())} outputs beyond their bound, first "
                                 f"at {i}: got {float(out[i])}, want {float(c['want'][i])} "
                                 f"({int(d[i])} ulp, allowed {int(lim[i])})")


def _probe_ratio(cuda) -> float:
    """One 16 x 16 x 128 tile (one instruction per output block) with unit scales against
    float64: the worst |got - ref| / (2^-24 sum |a||b|)."""
    from cake_amd.ops import hip as K
    worst = 0.0
    for seed in range(64):
        g = torch.Generator().manual_seed(50 + seed)
        a8, w8 = W.random_codes((16, 128), g), W.random_codes((16, 128), g)
        one = torch.ones(16)
        ref = W.R.gemm_w8a8_ref(a8, one, w8, one)
        A = W.values_of(a8).abs() @ W.values_of(w8).abs().T
        out = torch.zeros(16, 16, device=cuda)
        K.gemm_w8a8(a8.to(cuda), one.to(cuda), w8.to(cuda), one.to(cuda), out, "resid32", cfg=1)
        ratio = (out.cpu().double() - ref).abs() / (W.EPS24 * A)
        worst = max(worst, float(ratio.max()))
    return worst


def test_single_instruction_probe(cuda):
    """The instruction's own sum of 128 products against float64.  Measured on an MI355X:
    2581.448 * 2^-24 * sum|a||b| at worst over these 64 tiles, far above the f32-chain constant
    K + 2 = 130, so the random rule uses twice that ratio as its constant (W.RULE_K); this
    test keeps the measurement from drifting."""
    worst = _probe_ratio(cuda)
    print(f"single 16x16x128 instruction: worst |err| / (2^-24 sum|a||b|) = {worst:.3f}")
    assert worst <= W.PROBE_WORST


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("M,N,K_", [(17, 48, 128), (129, 144, 384), (257, 272, 1152)])
def test_random_codes_over_the_whole_format(cuda, M, N, K_, cfg):
    """All 254 non-NaN codes (subnormals, +-448), random f32 scales:
    |got - ref64| <= 0.5 ulp16(ref64) + C 2^-24 sa sw sum|a||b|; f32 outputs drop the ulp16
    term.  C = W.RULE_K = 5162.9, twice the single-instruction probe's worst ratio, in place
    of K + 2: the hardware's own sum exceeds the f32-chain bound (tests/_w8a8.py).  Measured:
    the f32 output is within 1803 (K = 128), 1080 (K = 384) and 693 (K = 1152) on every cfg."""
    from cake_amd.ops import hip as K
    c = W.random_case(M, N, K_)
    d = _dev(c, cuda)
    k = W.rule_k(K_)
    for dt in DTYPES:
        out = torch.full((M, N), float("nan"), device=cuda, dtype=dt)
        K.gemm_w8a8(d["a8"], d["sa"], d["w8"], d["sw"], out, "store", cfg=cfg)
        assert torch.isfinite(out).all()
        need = U.min_k(out, c["ref"], c["A"])
        print(f"store {dt} cfg {cfg} {M}x{N}x{K_}: passes from k = {need} (allowed {k})")
        U.assert_rule(out, c["ref"], c["A"], f"store {dt}", k=k)
    r = torch.zeros(M, N, device=cuda)
    K.gemm_w8a8(d["a8"], d["sa"], d["w8"], d["sw"], r, "resid32", cfg=cfg)
    err = (r.cpu().double() - c["ref"]).abs()
    ratio = float((err / (W.EPS24 * c["A"])).max())
    print(f"resid32 cfg {cfg} {M}x{N}x{K_}: worst |err| / (2^-24 A) = {ratio:.3f} (allowed {k})")
    assert bool((err <= k * W.EPS24 * c["A"]).all())


def test_planner_covers_the_cus(cuda):
    from cake_amd.ops import hip as K
    assert K.gemm_w8a8_plan(512, 6144, 4096) == 1      # 8B q|k|v at 512 tokens: 64 x 64 tiles
    assert K.gemm_w8a8_plan(512, 4096, 4096) == 1      # o
    assert K.gemm_w8a8_plan(2048, 28672, 4096) == 0    # gate|up at 2048 tokens: 128 x 128
    assert K.gemm_w8a8_plan(512, 10240, 8192) == 0     # 70B q|k|v at 512 tokens: 320 tiles
    assert K.gemm_w8a8_plan(1, 16, 128) == 1


def test_refusals_leave_the_output_untouched(cuda):
    """K = 192, lda = 8, a misaligned base and an unknown cfg: hipErrorInvalidValue before any
    launch."""
    from cake_amd.ops import hip as K
    from cake_amd.ops._lib import KernelError
    c = _exact(17, 48, 384)
    out = torch.full((17, 48), 3.0, device=cuda, dtype=torch.bfloat16)
    args = (c["a8"], c["sa"], c["w8"], c["sw"])

    def refused(a8, sa, w8, sw, **kw):
        with pytest.raises(KernelError, match=HIP_INVALID):
            K.gemm_w8a8(a8, sa, w8, sw, out, **kw)
        torch.cuda.synchronize()
        assert bool((out == 3.0).all())

    refused(c["a8"][:, :192], c["sa"], c["w8"][:, :192], c["sw"])              # K = 192
    flat = torch.zeros(17 * 8 + 384, device=cuda, dtype=torch.uint8)
    refused(flat.as_strided((17, 384), (8, 1)), c["sa"], c["w8"], c["sw"])       # lda = 8
    buf = torch.zeros(17 * 384 + 16, device=cuda, dtype=torch.uint8)
    refused(buf[1:1 + 17 * 384].view(17, 384), c["sa"], c["w8"], c["sw"])         # base + 1
    wbuf = torch.zeros(48 * 384 + 16, device=cuda, dtype=torch.uint8)
    refused(c["a8"], c["sa"], wbuf[8:8 + 48 * 384].view(48, 384), c["sw"])        # base + 8
    refused(*args, cfg=2)
    refused(*args, cfg=99)
    # gated: N % 16
    w24 = c["w8"][:40]
    out20 = torch.full((17, 20), 3.0, device=cuda, dtype=torch.bfloat16)
    with pytest.raises(KernelError, match=HIP_INVALID):
        K.gemm_w8a8(c["a8"], c["sa"], w24, c["sw"][:40], out20, "swiglu")
    assert bool((out20 == 3.0).all())
    with pytest.raises(ValueError):
        K.gemm_w8a8(*args, out, "geglu")
