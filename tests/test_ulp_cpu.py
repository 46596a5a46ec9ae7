"""CPU checks of tests/_ulp.py: every builder at every shape of the GPU tests, the float64
references against independent formulations, and the measurement of the rule's K on the f32
yardstick (printed with -s; pinned in _ulp.py)."""
import math

import pytest
import torch

import _exact as X
import _ulp as U

DT_IDS = ["bf16", "f16"]


def _every_norm_case(dt):
    """(family, name, case, yardstick output) of every norm case of the GPU tests."""
    for H in U.RMS_H:
        for name, c in U.rms_cases(H, dt):
            y = U.rmsnorm_ref(c["x"], c["w"], c["eps"], torch.float32)[0].to(dt)
            yield "rmsnorm", f"H {H} {name}", c, y
    for rows in U.LN_ROWS:
        for C in U.LN_C:
            for name, c in U.ln_cases(rows, C, dt):
                yield "layer_norm", f"{rows}x{C} {name}", c, U.yardstick("layer_norm", c)
    for silu in (False, True):
        for s in U.GN_NCHW:
            for name, c in U.gn_nchw_cases(s, dt, silu):
                yield "group_norm", f"{s} silu {silu} {name}", c, U.yardstick("group_norm", c, s[4], silu)
        for s in U.GN_NHWC:
            for name, c in U.gn_nhwc_cases(s, dt, silu):
                yield "group_norm_nhwc", f"{s} silu {silu} {name}", c, \
                    U.yardstick("group_norm_nhwc", c, s[3], silu)
        for s in U.GN_TWO:
            for name, c in U.gn_two_cases(s, dt, silu):
                yield "two_source", f"{s} silu {silu} {name}", c, U.yardstick("two_source", c, s[4], silu)
    for fam in U.COND_FAMILIES:
        for s in U.COND_NHWC:
            for mean, std in U.COND:
                c = U.cond_case(fam, s, mean, std, dt)
                yield "cond " + fam, f"{s} mean {mean} std {std}", c, U.yardstick(fam, c, c["G"])


def _every_glue_case(dt):
    for Fh in U.GEGLU_F:
        c = U.geglu_case(Fh, dt)
        yield "geglu", f"F {Fh}", c, U.geglu_ref(c["h"], torch.float32)[0].to(dt)
    gate, other = U.gate_sweep(dt)
    h = torch.cat([other, gate], -1)
    ref, A = U.geglu_ref(h)
    yield "geglu", "gate sweep", dict(ref=ref, A=A), U.geglu_ref(h, torch.float32)[0].to(dt)
    ref, A = U.silu_mul_ref(gate, other)
    yield "silu_mul", "gate sweep", dict(ref=ref, A=A), U.silu_mul_ref(gate, other, torch.float32)[0].to(dt)
    for hd in U.ROPE_HD + U.ROPE_SCALAR_HD:
        f = U.inv_freq(hd)
        for T in U.ROPE_T:
            for p in U.ROPE_POS0:
                pos0 = U.ROPE_S - T if p is None else p
                x = U.rope_inputs(T, 2, 1, hd, dt, pos0 + T + hd)[:, :2 * hd]
                ref, A = U.rope_ref(x, 2, hd, pos0, f)
                yield "rope", f"hd {hd} T {T} pos0 {pos0}", dict(ref=ref, A=A), \
                    U.rope_ref(x, 2, hd, pos0, f, torch.float32)[0].to(dt)
    yield from U.sd_glue_cases(dt)


@pytest.mark.parametrize("dt", U.DTYPES, ids=DT_IDS)
def test_yardstick_k(dt):
    """Builds every case (the builders assert their own conditions), runs the f32 yardstick
    through the rule and measures the k it needs: the largest over all cases is
    _ulp.YARDSTICK_K in at least one dtype and never above it."""
    worst = {}
    n = 0
    for fam, name, c, y in list(_every_norm_case(dt)) + list(_every_glue_case(dt)):
        n += 1
        assert torch.isfinite(c["ref"]).all(), (fam, name)
        k = U.min_k(y, c["ref"], c["A"])
        if k > worst.get(fam, (-1.0, ""))[0]:
            worst[fam] = (k, name)
    for fam, (k, name) in sorted(worst.items()):
        print(f"yardstick {DT_IDS[U.DTYPES.index(dt)]} {fam:22s} k = {k:<8g} at {name}")
    print(f"{n} cases; K = {U.K}")
    top = max(k for k, _ in worst.values())
    assert top <= U.YARDSTICK_K, worst
    test_yardstick_k.top = max(getattr(test_yardstick_k, "top", 0.0), top)


def test_k_is_the_smallest():
    """Runs after test_yardstick_k's two dtypes: their worst k is exactly YARDSTICK_K."""
    top = getattr(test_yardstick_k, "top", None)
    if top is None:
        top = 0.0
        for dt in U.DTYPES:
            for fam, name, c, y in list(_every_norm_case(dt)) + list(_every_glue_case(dt)):
                top = max(top, U.min_k(y, c["ref"], c["A"]))
    assert top == U.YARDSTICK_K and U.K == 2 * U.YARDSTICK_K


@pytest.mark.parametrize("dt", U.DTYPES, ids=DT_IDS)
def test_builders(dt):
    # exact statistics: distinct means, outputs +-gamma + beta, a miscounted element shows
    L = U.NHWC(2, 17, 256, 32)
    c = U.norm_case(L, "exact", dt, ref_fn=lambda x, g, b, e: U.group_norm_nhwc_ref(x, g, b, 32, e, False))
    xx = c["x"].double().reshape(2, 17, 32, 8)
    m = xx.mean((1, 3))
    assert m.unique().numel() == 64 and torch.equal(m, m.round())
    dev = (xx - m[:, None, :, None]).abs()
    assert set(dev.unique().tolist()) <= {1.0, 2.0, 4.0}
    want = torch.sign(xx - m[:, None, :, None]) * c["gamma"].double().view(1, 1, 32, 8) \
        + c["beta"].double().view(1, 1, 32, 8)
    assert torch.equal(want.reshape(c["ref"].shape), c["ref"]) and c["eps"] == 0.0
    # one element counted into the neighbouring group moves the result by many ulp
    x2 = c["x"].clone().reshape(2, 17, 256)
    x2[0, 0, 7], x2[0, 0, 8] = c["x"].reshape(2, 17, 256)[0, 0, 8], c["x"].reshape(2, 17, 256)[0, 0, 7]
    y2 = U.group_norm_nhwc_ref(x2.reshape(c["x"].shape), c["gamma"], c["beta"], 32, 1e-12, False)[0]
    assert int(X.ulp_distance(y2.to(dt), c["ref"].to(dt)).max()) > 8
    with pytest.raises(AssertionError, match="even group size"):
        U.exact_x(U.NCHW(1, 32, 1, 1, 32), dt, 0)
    with pytest.raises(AssertionError, match="distinct means"):
        U.exact_x(U.Rows(1200, 8), dt, 0)
    with pytest.raises(AssertionError, match="badly chosen"):
        U.norm_case(U.Rows(4, 512), "random", dt, mean=256.0, ref_fn=U.layer_norm_ref, cap=True)
    # eps-visible: each kind of group is there, constant groups give beta
    L = U.Rows(5, 512)
    for phase, eps in U.EPSVIS_RUNS:
        c = U.norm_case(L, "epsvis", dt, eps=eps, phase=phase, ref_fn=U.layer_norm_ref)
        var = c["x"].double().var(-1, unbiased=False)
        kind = (torch.arange(5) + phase) % 4
        assert (var[kind == 0] < 2e-6).all() and (var[kind == 0] > 0).all()
        assert (var[(kind == 1) | (kind == 2)] == 0).all() and (var[kind == 3] > 0.5).all()
        assert (c["x"][kind == 1] != 0).all() and (c["x"][kind == 2] == 0).all()
        for r in ((kind == 1) | (kind == 2)).nonzero().flatten().tolist():
            assert torch.equal(c["ref"][r], c["beta"].double())
    # random: negative gammas, the layouts agree on what a group is
    g, b = U.affine(64, dt, 3)
    assert (g < 0).any() and (g > 0).any()
    grp = torch.arange(2 * 4 * 6, dtype=torch.float64).reshape(8, 6)       # 2 images x 4 groups
    assert torch.equal(U.NCHW(2, 8, 1, 3, 4).place(grp)[1, 2:4].reshape(-1), grp[5])
    assert torch.equal(U.NHWC(2, 3, 8, 4).place(grp)[1, :, :, 2:4].reshape(-1), grp[5])
    # the gate sweep holds every finite pattern once per operand
    gate, other = U.gate_sweep(dt)
    n = 65536 - 2 * (2 ** U.MANT[dt])
    assert U.all_patterns(dt).numel() == n and gate[0].view(torch.int16).unique().numel() == n
    assert other[0, 0] == 1 and other[1, 0] == 3


def test_ulp16_and_rule():
    for dt in U.DTYPES:
        p = U.all_patterns(dt)
        p = p[p > 0].sort().values
        gap = (p[1:].double() - p[:-1].double())
        assert torch.equal(U.ulp16(p[:-1].double(), dt), gap)          # spacing above each value
        mid = (p[:-1].double() + p[1:].double()) / 2
        z = torch.zeros_like(mid)
        assert not U.violations(p[:-1], mid, z, 0.0).any()              # half an ulp passes
        assert U.violations(p[:-1][:-1], mid[1:], z[1:], 0.0).all()     # 1.5 ulp does not
        # the A term buys exactly k * 2^-24 * A
        one = torch.ones(1, dtype=torch.float64)
        got = torch.tensor([1.0], dtype=dt)
        u = 2.0 ** -U.MANT[dt]
        assert not U.violations(got, one + 0.5 * u + 8 * U.EPS24 * 3 - 1e-12, 3 * one, 8).any()
        assert U.violations(got, one + 0.5 * u + 8 * U.EPS24 * 3 + 1e-9, 3 * one, 8).any()
        nan = torch.tensor([float("nan"), float("inf")], dtype=torch.float64)
        assert not U.violations(nan.to(dt), nan, torch.zeros(2, dtype=torch.float64)).any()
        assert U.violations(torch.zeros(2, dtype=dt), nan, torch.zeros(2, dtype=torch.float64)).all()


def test_references_against_independent_forms():
    dt = torch.float16
    g, b = U.affine(320, dt, 1)
    x = U.random_x(U.NHWC(2, 35, 320, 32), 3.0, 2.0, dt, 2)
    for silu in (False, True):
        ref, _ = U.group_norm_nhwc_ref(x, g, b, 32, 1e-5, silu)
        t = torch.nn.functional.group_norm(x.double().movedim(-1, 1), 32, g.double(), b.double(), 1e-5)
        t = torch.nn.functional.silu(t) if silu else t
        torch.testing.assert_close(ref, t.movedim(1, -1), rtol=1e-12, atol=1e-13)
        two, _ = U.group_norm_nhwc_ref(x[..., :88], g, b, 32, 1e-5, silu, skip=x[..., 88:])
        assert torch.equal(two, ref)
    xc = x.movedim(-1, 1).contiguous()
    ref, _ = U.group_norm_nchw_ref(xc, g, b, 32, 1e-5, False)
    # Welford against two-pass
    v = xc.double().reshape(2, 32, -1)
    mean = torch.zeros(2, 32, dtype=torch.float64)
    m2 = torch.zeros_like(mean)
    for i in range(v.shape[-1]):
        d = v[..., i] - mean
        mean = mean + d / (i + 1)
        m2 = m2 + d * (v[..., i] - mean)
    y = (v - mean[..., None]) / torch.sqrt(m2 / v.shape[-1] + 1e-5)[..., None]
    y = y.reshape(xc.shape) * g.double().view(1, -1, 1, 1) + b.double().view(1, -1, 1, 1)
    torch.testing.assert_close(ref, y, rtol=1e-12, atol=1e-13)
    rows = U.random_x(U.Rows(5, 320), 64.0, 1.0, dt, 3)
    ref, _ = U.layer_norm_ref(rows, g, b, 1e-5)
    torch.testing.assert_close(ref, torch.nn.functional.layer_norm(rows.double(), (320,), g.double(),
                                                                   b.double(), 1e-5), rtol=1e-11, atol=1e-12)
    xf = torch.randn(3, 320, dtype=torch.float64).float()
    ref, _ = U.rmsnorm_ref(xf, g, 1e-5)
    alt = xf.double() / torch.sqrt(xf.double().pow(2).sum(-1, keepdim=True) / 320 + 1e-5) * g.double()
    torch.testing.assert_close(ref, alt, rtol=1e-13, atol=0)
    # GEGLU: the tanh form where it does not cancel; SiLU: x / (1 + exp(-x))
    h = torch.linspace(-3, 8, 4096, dtype=torch.float64).to(dt).repeat(2)[None]
    torch.testing.assert_close(U.geglu_ref(h)[0], h[:, :4096].double() * X.act_f64("gelu_tanh", h[:, 4096:]),
                               rtol=1e-11, atol=0)
    gate, other = U.gate_sweep(dt)
    torch.testing.assert_close(U.silu_mul_ref(gate, other)[0],
                               gate.double() / (1 + torch.exp(-gate.double())) * other.double(),
                               rtol=1e-13, atol=0)
    # RoPE: complex multiplication by exp(i angle), the angle formed in f32
    f = U.inv_freq(64)
    xq = U.rope_inputs(7, 2, 1, 64, dt, 5)[:, :128]
    ref, A = U.rope_ref(xq, 2, 64, 131065, f)
    ang = (torch.arange(131065, 131072, dtype=torch.float32)[:, None] * f[None]).double()
    z = torch.complex(xq.double().view(7, 2, 64)[..., :32], xq.double().view(7, 2, 64)[..., 32:]) \
        * torch.polar(torch.ones_like(ang), ang)[:, None]
    torch.testing.assert_close(ref.view(7, 2, 64), torch.cat([z.real, z.imag], -1), rtol=1e-12, atol=1e-14)
    assert torch.equal(U.rope_ref(xq[:1], 2, 64, 0, f)[0], xq[:1].double())   # position 0: identity
    # to_rgb8
    img = torch.tensor([-2.0, -1.0, 0.0, 1.0, 2.0, float("inf"), float("-inf"), 0.00390625,
                        -0.00390625], dtype=dt)
    img = img.repeat(3).reshape(1, 3, 3, 3)
    assert U.to_rgb8_ref(img, True).flatten()[:9].tolist() == [0, 0, 127, 255, 255, 255, 0, 127, 127]
    assert torch.equal(U.to_rgb8_ref(img, False), U.to_rgb8_ref(img.permute(0, 2, 3, 1), True))
