"""RMSNorm, LayerNorm, GEGLU and the three GroupNorm entry points against float64 under the
rule of tests/_ulp.py, at the shapes where their launchers change path, on random,
eps-visible and exact-statistics inputs, and over a sweep of mean / std ratios."""
import pytest
import torch

import _ulp as U

pytestmark = pytest.mark.gpu
DT_IDS = ["bf16", "f16"]
dtypes = pytest.mark.parametrize("dt", U.DTYPES, ids=DT_IDS)


def _check(got, c, what):
    """The rule; on exact-statistics inputs also at most 1 ulp (the count of elements that
    are not bit-equal is printed)."""
    got = got.cpu()
    assert torch.isfinite(got.float()).all(), f"{what}: non-finite output"
    U.assert_rule(got, c["ref"], c["A"], what)
    if c["kind"] == "exact":
        d = U.ulp_distance(got, c["ref"].to(got.dtype))
        print(f"{what}: {int((d != 0).sum())} of {d.numel()} elements not bit-equal")
        assert int(d.max()) <= 1, f"{what}: {int(d.max())} ulp on exact statistics"


def _nan_like(shape, dt, dev):
    return torch.full(tuple(shape), float("nan"), dtype=dt, device=dev)


def _off2(t, dev):
    """A contiguous device copy of `t` that starts 2 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=dev)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 2 and v.is_contiguous()
    return v


@dtypes
@pytest.mark.parametrize("H", U.RMS_H)
@pytest.mark.parametrize("reg", [1, 0])
def test_rmsnorm(cuda, dt, H, reg):
    from cake_amd.ops import hip as K
    from cake_amd.ops._lib import kernels
    kernels().cake_rmsnorm_set_reg(reg)
    try:
        for name, c in U.rms_cases(H, dt):
            assert (c["w"] < 0).any()
            out = _nan_like(c["x"].shape, dt, cuda)
            K.rmsnorm(c["x"].to(cuda), c["w"].to(cuda), c["eps"], out)
            _check(out, c, f"rmsnorm reg {reg} H {H} {name}")
    finally:
        kernels().cake_rmsnorm_set_reg(1)


@dtypes
@pytest.mark.parametrize("C", U.LN_C)
@pytest.mark.parametrize("rows", U.LN_ROWS)
def test_layer_norm(cuda, dt, rows, C):
    from cake_amd.ops import hip as K
    for name, c in U.ln_cases(rows, C, dt):
        out = _nan_like(c["x"].shape, dt, cuda)
        K.layer_norm(c["x"].to(cuda), c["gamma"].to(cuda), c["beta"].to(cuda), c["eps"], out)
        _check(out, c, f"layer_norm {rows}x{C} {name}")


@dtypes
@pytest.mark.parametrize("which", ["x", "out", "gamma", "beta"])
def test_layer_norm_misaligned(cuda, dt, which):
    """C = 512 with one operand 2 bytes off a 16-byte boundary: the block kernel."""
    from cake_amd.ops import hip as K
    for name, c in U.ln_cases(5, 512, dt):
        t = dict(x=c["x"].to(cuda), gamma=c["gamma"].to(cuda), beta=c["beta"].to(cuda),
                 out=_nan_like(c["x"].shape, dt, cuda))
        t[which] = _off2(t[which], cuda)
        K.layer_norm(t["x"], t["gamma"], t["beta"], c["eps"], t["out"])
        _check(t["out"], c, f"layer_norm 5x512 {which} misaligned {name}")


@dtypes
@pytest.mark.parametrize("Fh", U.GEGLU_F)
@pytest.mark.parametrize("misaligned", [False, True])
def test_geglu(cuda, dt, Fh, misaligned):
    from cake_amd.ops import hip as K
    c = U.geglu_case(Fh, dt)
    h = _off2(c["h"], cuda) if misaligned else c["h"].to(cuda)
    out = _nan_like((U.GEGLU_ROWS, Fh), dt, cuda)
    K.geglu(h, out)
    U.assert_rule(out, c["ref"], c["A"], f"geglu F {Fh} misaligned {misaligned}")


@dtypes
def test_geglu_gate_sweep(cuda, dt):
    """Every finite 16-bit pattern as the gate, the other operand 1 and 3."""
    from cake_amd.ops import hip as K
    gate, other = U.gate_sweep(dt)
    h = torch.cat([other, gate], -1)
    ref, A = U.geglu_ref(h)
    out = _nan_like(gate.shape, dt, cuda)
    K.geglu(h.to(cuda), out)
    U.assert_rule(out, ref, A, "geglu gate sweep")


@dtypes
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("shape", U.GN_NCHW, ids=str)
def test_group_norm(cuda, dt, shape, silu):
    from cake_amd.ops import hip as K
    for name, c in U.gn_nchw_cases(shape, dt, silu):
        out = _nan_like(c["x"].shape, dt, cuda)
        K.group_norm(c["x"].to(cuda), c["gamma"].to(cuda), c["beta"].to(cuda), shape[4], c["eps"],
                     silu, out)
        _check(out, c, f"group_norm {shape} silu {silu} {name}")


@dtypes
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("shape", U.GN_NHWC, ids=str)
def test_group_norm_nhwc(cuda, dt, shape, silu):
    """Each case is launched twice: the second launch runs on the tickets the first re-armed."""
    from cake_amd.ops import hip as K
    for name, c in U.gn_nhwc_cases(shape, dt, silu):
        x, g, b = c["x"].to(cuda), c["gamma"].to(cuda), c["beta"].to(cuda)
        assert x.dim() == 4 and x.shape[1] * x.shape[2] == shape[1]
        outs = []
        for _ in range(2):
            out = _nan_like(x.shape, dt, cuda)
            K.group_norm_nhwc(x, g, b, shape[3], c["eps"], silu, out)
            outs.append(out)
        _check(outs[0], c, f"group_norm_nhwc {shape} silu {silu} {name}")
        assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), \
            f"group_norm_nhwc {shape} {name}: the second launch differs"


@dtypes
@pytest.mark.parametrize("cat", [False, True])
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("shape", U.GN_TWO, ids=str)
def test_group_norm_two_source(cuda, dt, shape, silu, cat):
    from cake_amd.ops import hip as K
    N, HW, Cx, Cs, G = shape
    for name, c in U.gn_two_cases(shape, dt, silu):
        full = c["x"].to(cuda)
        x, skip = full[..., :Cx].contiguous(), full[..., Cx:].contiguous()
        out = _nan_like(full.shape, dt, cuda)
        cat_out = _nan_like(full.shape, dt, cuda) if cat else None
        K.group_norm_nhwc(x, c["gamma"].to(cuda), c["beta"].to(cuda), G, c["eps"], silu, out,
                          skip=skip, cat_out=cat_out)
        _check(out, c, f"two-source {shape} silu {silu} cat {cat} {name}")
        if cat:
            assert torch.equal(cat_out.view(torch.int16), torch.cat([x, skip], -1).view(torch.int16))


def _run_cond(family, c, cuda):
    from cake_amd.ops import hip as K
    x, g, b = c["x"].to(cuda), c["gamma"].to(cuda), c["beta"].to(cuda)
    out = _nan_like(x.shape, x.dtype, cuda)
    if family == "layer_norm":
        K.layer_norm(x, g, b, c["eps"], out)
    elif family == "group_norm":
        K.group_norm(x, g, b, c["G"], c["eps"], False, out)
    elif family == "group_norm_nhwc":
        K.group_norm_nhwc(x, g, b, c["G"], c["eps"], False, out)
    else:
        Cx = x.shape[-1] // 8 // 2 * 8 + 8       # a source boundary inside a group where C allows
        K.group_norm_nhwc(x[..., :Cx].contiguous(), g, b, c["G"], c["eps"], False, out,
                          skip=x[..., Cx:].contiguous())
    return out


@dtypes
@pytest.mark.parametrize("shape", U.COND_NHWC, ids=str)
@pytest.mark.parametrize("family", U.COND_FAMILIES)
def test_conditioning(cuda, dt, family, shape, record_property):
    """mean / std from 0 to 400: the same rule (its A term carries |mean| rstd).  Prints,
    per point, the kernel's and the f32 yardstick's largest ulp distance over |ref| > 0.25."""
    if family in ("group_norm_nhwc", "two_source") and shape[2] // shape[3] < 4:
        from cake_amd.ops import hip as K
        assert not K.group_norm_nhwc_supported(shape[2], shape[3])   # hence G = C / 8 below
    failed = []
    for mean, std in U.COND:
        c = U.cond_case(family, shape, mean, std, dt)
        out = _run_cond(family, c, cuda).cpu()
        ku, yu = U.max_ulp(out, c["ref"]), U.max_ulp(U.yardstick(family, c, c["G"]), c["ref"])
        bad = int(U.violations(out, c["ref"], c["A"]).sum())
        line = (f"cond {family} {DT_IDS[U.DTYPES.index(dt)]} {shape} mean {mean:g} std {std:g}: "
                f"kernel {ku} ulp, yardstick {yu} ulp, {bad} outside the rule")
        print(line)
        record_property(f"mean {mean:g} std {std:g}", dict(kernel_ulp=ku, yardstick_ulp=yu, bad=bad))
        assert torch.isfinite(out.float()).all(), line
        if bad:
            failed.append(line)
    assert not failed, "\n".join(failed)
