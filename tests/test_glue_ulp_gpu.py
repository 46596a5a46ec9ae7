"""RoPE + KV-cache write, the decode QKV epilogue at the last Llama-3.1 position, SiLU * up,
the residual add, the embedding gather, the 16-bit casts and the RGB8 store: against float64
under the rule of tests/_ulp.py, or bit for bit where the operation is exact."""

import pytest
import torch

import _ulp as U

pytestmark = pytest.mark.gpu
DT_IDS = ["bf16", "f16"]
dtypes = pytest.mark.parametrize("dt", U.DTYPES, ids=DT_IDS)
SENTINEL = 0x5A5A                      # a finite value in both dtypes
INVALID = 1                            # hipErrorInvalidValue
CAP = 4096 * 256                       # items one trip of a capped elementwise grid covers


def _bits(t):
    return t.contiguous().view(torch.int16)


def _sentinel(shape, dt, dev):
    return torch.full(tuple(shape), SENTINEL, dtype=torch.int16, device=dev).view(dt)


def _off2(t, dev):
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=dev)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 2
    return v


# ---------------------------------------------------------------------------
# rope_kv
# ---------------------------------------------------------------------------

def _rope_once(cuda, dt, fused_cpu, nh, nkv, hd, pos0, kc, vc, *, fused: bool, misalign=False):
    """Runs rope_kv on a copy of the fused projection; checks q, the written cache rows and
    V, then puts the sentinel back into the rows it wrote."""
    from cake_amd.ops import hip as K
    T = fused_cpu.shape[0]
    nq, nk = nh * hd, nkv * hd
    f = _off2(fused_cpu, cuda) if misalign else fused_cpu.to(cuda)
    if fused:
        q, k, v = f[:, :nq], f[:, nq:nq + nk], f[:, nq + nk:]
    else:
        q, k, v = ((_off2(t.contiguous(), cuda) if misalign else t.contiguous())
                   for t in (f[:, :nq], f[:, nq:nq + nk], f[:, nq + nk:]))
    invf = U.inv_freq(hd)
    K.rope_kv(q, k, v, invf.to(cuda), pos0, kc, vc)
    what = f"rope_kv hd {hd} T {T} pos0 {pos0} fused {fused} misaligned {misalign}"
    qref, qA = U.rope_ref(fused_cpu[:, :nq], nh, hd, pos0, invf)
    kref, kA = U.rope_ref(fused_cpu[:, nq:nq + nk], nkv, hd, pos0, invf)
    U.assert_rule(q, qref, qA, what + " q")
    krows = kc[:, pos0:pos0 + T].transpose(0, 1).reshape(T, nk)
    U.assert_rule(krows, kref, kA, what + " k")
    vrows = vc[:, pos0:pos0 + T].transpose(0, 1).reshape(T, nk)
    assert torch.equal(_bits(vrows).cpu(), _bits(fused_cpu[:, nq + nk:])), what + " v"
    assert torch.equal(_bits(k).cpu(), _bits(fused_cpu[:, nq:nq + nk])), what + ": k changed"
    if pos0 == 0 and T == 1:       # angle 0: the identity, bit for bit
        assert torch.equal(_bits(q).cpu(), _bits(fused_cpu[:, :nq])), what + " q at 0"
        assert torch.equal(_bits(krows).cpu(), _bits(fused_cpu[:, nq:nq + nk])), what + " k at 0"
    kc[:, pos0:pos0 + T] = _sentinel((1,), dt, cuda)
    vc[:, pos0:pos0 + T] = _sentinel((1,), dt, cuda)


def _untouched(kc, vc, what):
    for name, c in (("k", kc), ("v", vc)):
        assert bool((c.view(torch.int16) == SENTINEL).all()), f"{what}: {name} cache rows overwritten"


@dtypes
@pytest.mark.parametrize("hd", U.ROPE_HD)
def test_rope_kv_long_positions(cuda, dt, hd):
    """Positions up to 131071 in a 131072-row cache, fused and separate q / k / v."""
    nh, nkv, S = 2, 1, U.ROPE_S
    kc, vc = _sentinel((nkv, S, hd), dt, cuda), _sentinel((nkv, S, hd), dt, cuda)
    for T in U.ROPE_T:
        for p in U.ROPE_POS0:
            pos0 = S - T if p is None else p
            x = U.rope_inputs(T, nh, nkv, hd, dt, pos0 + T + hd)
            for fused in (True, False):
                _rope_once(cuda, dt, x, nh, nkv, hd, pos0, kc, vc, fused=fused)
    _untouched(kc, vc, f"rope_kv hd {hd}")


@dtypes
@pytest.mark.parametrize("hd,misalign", [(24, False), (40, False), (64, True)])
def test_rope_kv_scalar_kernel(cuda, dt, hd, misalign):
    """Head sizes that are no multiple of 16, and hd = 64 on a view 2 bytes off alignment."""
    nh, nkv, S = 2, 1, 4200
    kc, vc = _sentinel((nkv, S, hd), dt, cuda), _sentinel((nkv, S, hd), dt, cuda)
    for T in U.ROPE_T:
        for pos0 in (0, 1, 4095, S - T):
            x = U.rope_inputs(T, nh, nkv, hd, dt, pos0 + T + hd)
            for fused in (True, False):
                _rope_once(cuda, dt, x, nh, nkv, hd, pos0, kc, vc, fused=fused, misalign=misalign)
    _untouched(kc, vc, f"rope_kv scalar hd {hd}")


@dtypes
@pytest.mark.parametrize("pos0,T", [(60, 5), (64, 1), (-1, 1), (-3, 7), (2 ** 31 - 2, 7)])
def test_rope_kv_rejects_rows_outside_the_cache(cuda, dt, pos0, T):
    """The C entry point itself (the engine calls it without the Python wrapper's check)."""
    from cake_amd.ops._lib import kernels
    nh, nkv, hd, S = 2, 1, 64, 64
    kc, vc = _sentinel((nkv + 2, S, hd), dt, cuda), _sentinel((nkv + 2, S, hd), dt, cuda)
    x = U.rope_inputs(T, nh, nkv, hd, dt, 1).to(cuda)
    before = x.clone()
    ld = x.shape[1]
    q, k, v = x[:, :nh * hd], x[:, nh * hd:(nh + nkv) * hd], x[:, (nh + nkv) * hd:]
    rc = kernels().cake_rope_kv(U.DTYPES.index(dt), q.data_ptr(), k.data_ptr(), v.data_ptr(), ld, ld,
                                T, nh, nkv, hd, U.inv_freq(hd).to(cuda).data_ptr(), pos0, S,
                                kc[1:].data_ptr(), vc[1:].data_ptr(),
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == INVALID
    assert torch.equal(_bits(x), _bits(before))
    _untouched(kc, vc, "rejected rope_kv")


@dtypes
def test_qkv_rope_last_position(cuda, dt):
    """The decode epilogue at position 131071: K's cache row against the float64 rotation of
    the f32 projection; allowance: the rule plus test_qkv_rope's GEMV term (2e-3 + 2e-3 |ref|)."""
    from cake_amd.ops import hip as K
    from cake_amd.ops import reference as R
    H, nh, nkv, hd, S = 256, 2, 1, 128, U.ROPE_S
    pos = S - 1
    g = torch.Generator().manual_seed(11)
    resid = torch.randn(H, generator=g)
    nw = (1 + 0.1 * torch.randn(H, generator=g)).to(dt)
    wq, wk, wv = ((0.05 * torch.randn(n * hd, H, generator=g)).to(dt) for n in (nh, nkv, nkv))
    invf = U.inv_freq(hd)
    kc, vc = _sentinel((nkv, S, hd), dt, cuda), _sentinel((nkv, S, hd), dt, cuda)
    q = torch.empty(nh * hd, device=cuda)
    K.qkv_rope(resid.to(cuda), nw.to(cuda), 1e-5, wq.to(cuda), wk.to(cuda), wv.to(cuda),
               invf.to(cuda), torch.tensor([pos], dtype=torch.int32, device=cuda), q, kc, vc)
    x = R.rms_norm(resid, nw, 1e-5)
    ang = (torch.tensor([float(pos)]) * invf).double()                    # the f32 product
    c, s = torch.cos(ang), torch.sin(ang)

    def rot(w):
        y = (w.float() @ x).double().view(-1, hd)
        a, b = y[:, :hd // 2], y[:, hd // 2:]
        return torch.cat([a * c - b * s, a * s + b * c], -1), (a.abs() + b.abs()).repeat(1, 2)
    kref, kA = rot(wk)
    got = kc[:, pos].cpu()
    err = (got.double() - kref).abs()
    allow = U.allowance(kref, kA, dt) + 2e-3 + 2e-3 * kref.abs()
    assert bool((err <= allow).all()), f"K row: worst excess {float((err - allow).max()):.3e}"
    qref, _ = rot(wq)
    torch.testing.assert_close(q.cpu().double().view(nh, hd), qref, atol=2e-3, rtol=2e-3)
    vref = (wv.float() @ x).double().view(nkv, hd)
    verr = (vc[:, pos].cpu().double() - vref).abs()
    assert bool((verr <= 0.5 * U.ulp16(vref, dt) + 2e-3 + 2e-3 * vref.abs()).all())
    kc[:, pos] = _sentinel((1,), dt, cuda)
    vc[:, pos] = _sentinel((1,), dt, cuda)
    _untouched(kc, vc, "qkv_rope")


# ---------------------------------------------------------------------------
# silu_mul, silu_mul_rows, add_resid, embed
# ---------------------------------------------------------------------------

@dtypes
def test_silu_mul_gate_sweep(cuda, dt):
    from cake_amd.ops import hip as K
    gate, other = U.gate_sweep(dt)
    ref, A = U.silu_mul_ref(gate, other)
    out = torch.full(gate.shape, float("nan"), dtype=dt, device=cuda)
    K.silu_mul(gate.to(cuda), other.to(cuda), out)
    U.assert_rule(out, ref, A, "silu_mul gate sweep")
    out = torch.full(gate.shape, float("nan"), dtype=dt, device=cuda)
    K.silu_mul_rows(torch.cat([gate, other], -1).to(cuda), out)
    U.assert_rule(out, ref, A, "silu_mul_rows gate sweep")


def _past_cap(n, dt, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g).mul(2.0).to(dt)


@dtypes
def test_silu_mul_past_the_grid_cap(cuda, dt):
    """4096 x 256 items and a partial second trip (silu_mul_rows: items of 8 elements)."""
    from cake_amd.ops import hip as K
    n = CAP + 1000
    g, u = _past_cap(n, dt, 1), _past_cap(n, dt, 2)
    ref, A = U.silu_mul_ref(g, u)
    out = torch.full((n + 64,), float("nan"), dtype=dt, device=cuda)
    K.silu_mul(g.to(cuda), u.to(cuda), out[:n])
    U.assert_rule(out[:n], ref, A, "silu_mul past the cap")
    assert bool(out[n:].isnan().all())
    T, I = 8, (CAP + 1000)                     # T * I / 8 = CAP + 1000 items
    gu = _past_cap(T * 2 * I, dt, 3).view(T, 2 * I)
    ref, A = U.silu_mul_ref(gu[:, :I], gu[:, I:])
    out = torch.full((T + 1, I), float("nan"), dtype=dt, device=cuda)
    K.silu_mul_rows(gu.to(cuda), out[:T])
    U.assert_rule(out[:T], ref, A, "silu_mul_rows past the cap")
    assert bool(out[T:].isnan().all())


@dtypes
@pytest.mark.parametrize("vec", [True, False])
def test_add_resid_bit_equal(cuda, dt, vec):
    """Every 16-bit pattern of y (NaN included) on a random f32 residual; past the grid cap
    with a partial last trip.  vec: add_resid8 (n % 8 == 0, aligned); else the scalar kernel
    (odd n, y two bytes off)."""
    from cake_amd.ops import hip as K
    pats = U.all_patterns(dt, finite=False)
    n = (8 if vec else 1) * (CAP + 1000) + (0 if vec else 1)
    y = pats.repeat(-(-n // 65536))[:n].clone()
    resid = torch.randn(n, generator=torch.Generator().manual_seed(4)) * 3
    want = resid + y.float()
    r = resid.to(cuda)
    K.add_resid(r, y.to(cuda) if vec else _off2(y, cuda))
    got = r.cpu()
    nan = want.isnan()
    assert torch.equal(got.isnan(), nan)
    assert torch.equal(got[~nan].view(torch.int32), want[~nan].view(torch.int32))


@dtypes
def test_embed_bit_equal(cuda, dt):
    from cake_amd.ops import hip as K
    H = 64
    table = U.all_patterns(dt, finite=False).view(-1, H)           # [1024, 64]: every pattern
    tok = torch.cat([torch.arange(1024), torch.tensor([0, 1023, 5, 5, 1023])]).int()
    out = torch.full((tok.numel(), H), float("nan"), device=cuda)
    K.embed(table.to(cuda), tok.to(cuda), out)
    want = table[tok.long()].float()
    nan = want.isnan()
    assert torch.equal(out.cpu().isnan(), nan)
    assert torch.equal(out.cpu()[~nan].view(torch.int32), want[~nan].view(torch.int32))


# ---------------------------------------------------------------------------
# stores and conversions
# ---------------------------------------------------------------------------

SRC = [torch.bfloat16, torch.float16, torch.float32]


def _cast16(src, dst_kind, cuda):
    from cake_amd.ops._lib import kernels
    fn = kernels().cake_cast16
    s = src.to(cuda)
    out = torch.full((src.numel() + 16,), SENTINEL, dtype=torch.int16, device=cuda)
    rc = fn(SRC.index(src.dtype), dst_kind, s.data_ptr(), out.data_ptr(), src.numel(),
            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out


def _f32_probes(dst) -> torch.Tensor:
    """For every finite value of `dst` and its upper neighbour: their midpoint and its two
    f32 neighbours (both signs); f32 subnormals, the f32 and dst extremes, values that
    overflow dst, infinities and NaN."""
    p = U.all_patterns(dst)
    p = p[p >= 0].sort().values.double()
    mid = ((p[:-1] + p[1:]) / 2).float()
    assert torch.equal(mid.double(), (p[:-1] + p[1:]) / 2)            # exact in f32
    inf = torch.full_like(mid, float("inf"))
    pos = torch.cat([mid, torch.nextafter(mid, inf), torch.nextafter(mid, -inf), p.float()])
    top = float(p[-1])
    extra = torch.tensor([1e-45, 3e-45, 1.1754942e-38, 1.17549435e-38, 3.4028235e38, top,
                          float("inf"), float("nan")], dtype=torch.float32)
    # the overflow threshold of dst (its largest value plus half an ulp) and its f32 neighbours
    half = (p[-1] + U.ulp16(p[-1], dst) / 2).float()
    edge = torch.stack([half, torch.nextafter(half, inf[0]), torch.nextafter(half, -inf[0])])
    pos = torch.cat([pos, extra, edge])
    return torch.cat([pos, -pos])


@pytest.mark.parametrize("dst", U.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("src", SRC, ids=["bf16", "f16", "f32"])
def test_cast16_bit_equal(cuda, src, dst):
    """from_f32's round-to-nearest-even, on which every kernel's store rests: bit-equal to
    torch's CPU conversion, NaN for NaN; past the grid cap; an f32 destination is refused."""
    x = _f32_probes(dst) if src == torch.float32 else U.all_patterns(src, finite=False)
    n = CAP + 1000
    x = torch.cat([x, x.flip(0)]).repeat(-(-n // (2 * x.numel())))[:max(n, 2 * x.numel())].contiguous()
    rc, out = _cast16(x, U.DTYPES.index(dst), cuda)
    assert rc == 0
    assert bool((out[x.numel():] == SENTINEL).all())
    got = out[:x.numel()].view(dst).cpu()
    want = x.to(dst)
    nan = want.isnan()
    assert torch.equal(got.isnan(), nan)
    bad = (_bits(got) != _bits(want)) & ~nan
    assert not bad.any(), (f"{int(bad.sum())} conversions differ, first {float(x[bad][0])!r} -> "
                           f"{float(got[bad][0])!r}, want {float(want[bad][0])!r}")
    rc, out = _cast16(x[:64], 2, cuda)
    assert rc == INVALID and bool((out == SENTINEL).all())


@dtypes
@pytest.mark.parametrize("nhwc", [False, True])
def test_to_rgb8_bit_equal(cuda, dt, nhwc):
    """Every finite pattern and +-inf; then an image past the grid cap."""
    from cake_amd.ops import hip as K
    p = U.all_patterns(dt, finite=False)
    p = p[~p.isnan()]
    H = W = 148                                          # 3 * 148^2 >= 65536
    flat = torch.zeros(3 * H * W, dtype=dt)
    flat[:p.numel()] = p
    for img in (flat.view(1, H, W, 3) if nhwc else flat.view(1, 3, H, W),
                torch.randn(3 * 600 * 600, generator=torch.Generator().manual_seed(6)).to(dt).view(
                    (1, 600, 600, 3) if nhwc else (1, 3, 600, 600))):
        got = K.to_rgb8(img.to(cuda), nhwc=nhwc).cpu()
        want = U.to_rgb8_ref(img, nhwc)
        bad = got != want
        assert not bad.any(), (f"{int(bad.sum())} bytes differ, first got {int(got[bad][0])} want "
                               f"{int(want[bad][0])}")
