"""gemv_rows.hip: the MFMA GEMV for 1..16 activation rows and the per-row RoPE / KV write of
the lock-step batched decode step.

Exact arithmetic first (tests/_exact.py: integer operands, every partial sum below 2^24, so
the f32 result is known to the bit whatever the summation order), then random normal operands
against float64 under the f32 summation bound, then what batched decoding rests on: a row's
result does not depend, to the bit, on how many rows ride with it or on the slot it sits in.

Shapes the launcher treats differently (gemv_rows.hip / gemv_rows_kernel.h):
  * a workgroup works on R row tiles of 16 weight rows; the tuning's R is halved while the
    grid would have fewer than 512 workgroups.  N_R2 = 16353 is the first N at which R = 2
    holds (ceil(N / 32) = 512; 16352 runs R = 1), N_R4 = 32705 the first for R = 4.
  * the grid is capped (max_blocks): with a cap of 3, N_CAP1 = 49 is the first N whose 4 row
    tiles need a second trip of a workgroup at R = 1; N_R2 / N_R4 on 3 workgroups loop with
    R = 2 / 4.
"""
import functools

import pytest
import torch

import _exact as X
import _ulp as U

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
MS = [1, 2, 7, 8, 9, 16]
KS = [32, 64, 96, 2080]
NS = [1, 15, 16, 17, 48]
N_CAP1, N_R2, N_R4 = 49, 16353, 32705
N_SMALL = max(NS + [N_CAP1])
CANARY = -77.0
EPIS = ("store32", "resid32", "swiglu")


def linear_case(M, N, K, dt, device="cpu"):
    return X.gemm_case(M, N, K, dt, device=device)


def gated_case(M, I, K, dt, device="cpu"):
    """act_case with an intermediate width of at least I (a multiple of 16): w2 is the packed
    gate | up [2 F, K]."""
    F = -(-I // 16) * 16
    c = X.act_case(M, 2 * F, K, dt, device=device)
    assert c["F"] == F
    return c


@functools.lru_cache(maxsize=None)
def _linear(M, N, K, dt):
    return linear_case(M, N, K, dt, "cuda")


@functools.lru_cache(maxsize=None)
def _gated(M, I, K, dt):
    return gated_case(M, I, K, dt, "cuda")


@pytest.fixture
def rows_tuning():
    from cake_amd.ops import hip as K_
    prev = {e: K_.get_gemv_rows_tuning(e) for e in EPIS}
    yield K_
    for e, (t, u, mb) in prev.items():
        K_.set_gemv_rows_tuning(e, tiles=t, unroll=u, max_blocks=mb)


def _same(got, want, what):
    if not torch.equal(got, want):
        bad = got != want
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} differ, first at {i}: "
                             f"got {float(got[i])}, want {float(want[i])}")


def _canary_out(M, N, dtype, fill=CANARY):
    """A [18, N + 5] buffer of canaries and the [18, N] view a launch writes rows [0, M) of."""
    big = torch.full((18, N + 5), fill, device="cuda", dtype=dtype)
    return big, big[:, :N]


def _untouched(big, M, N, fill, what):
    keep = torch.ones_like(big, dtype=torch.bool)
    keep[:M, :N] = False
    assert bool((big[keep] == fill).all()), f"{what}: written outside [{M}, {N}]"


def _check_linear(K_, c, M, N, dt, what):
    x, w = c["x"], c["w"][:N]
    big, out = _canary_out(M, N, torch.float32)
    K_.gemv_rows(x, w, out, "store32", M=M)
    _same(big[:M, :N], c["y"][:, :N], f"{what} store32")
    _untouched(big, M, N, CANARY, f"{what} store32")
    big, out = _canary_out(M, N, torch.float32)
    big[:M, :N] = c["r32"][:, :N]
    K_.gemv_rows(x, w, out, "resid32", M=M)
    _same(big[:M, :N], c["yr32"][:, :N], f"{what} resid32")
    _untouched(big, M, N, CANARY, f"{what} resid32")


def _check_swiglu(K_, c, M, I, dt, what):
    F = c["F"]
    w = torch.cat([c["w2"][:I], c["w2"][F:F + I]]).contiguous()      # packed gate | up [2 I, K]
    big, out = _canary_out(M, I, dt)
    K_.gemv_rows(c["x"], w, out, "swiglu", M=M)
    d = X.ulp_distance(big[:M, :I], c["swiglu"].to(dt)[:, :I])
    lim = X.act_allowance(c, "swiglu", dt)[:, :I]
    bad = d > lim
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what} swiglu: {int(bad.sum())} outputs beyond their bound, first "
                             f"at {i}: got {float(big[i])}, want {float(c['swiglu'][i])} "
                             f"({int(d[i])} ulp, allowed {int(lim[i])})")
    _untouched(big, M, I, CANARY, f"{what} swiglu")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M", MS)
def test_exact_epilogues(cuda, rows_tuning, dt, K, M):
    """store32 and resid32 bit-equal to exact_linear, swiglu within act_allowance; a canary
    output unchanged outside [M, N].  Default geometry for the N list; N_CAP1 on a grid capped
    at 3 workgroups; both k-step unrolls."""
    K_ = rows_tuning
    c, g = _linear(M, N_SMALL, K, dt), _gated(M, N_SMALL, K, dt)
    for N in NS:
        _check_linear(K_, c, M, N, dt, f"N {N}")
        _check_swiglu(K_, g, M, N, dt, f"N {N}")
    for unroll in (2, 4):
        for e in EPIS:
            K_.set_gemv_rows_tuning(e, tiles=1, unroll=unroll, max_blocks=3)
        _check_linear(K_, c, M, N_CAP1, dt, f"cap 3, unroll {unroll}, N {N_CAP1}")
        _check_swiglu(K_, g, M, N_CAP1, dt, f"cap 3, unroll {unroll}, N {N_CAP1}")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M,K", [(7, 32), (16, 96)])
def test_exact_tile_boundaries(cuda, rows_tuning, dt, M, K):
    """Two and four row tiles per workgroup at the first N that keeps them (N_R2, N_R4), on
    the whole grid and on 3 workgroups, and the N just below N_R2 (back to one tile)."""
    K_ = rows_tuning
    c = _linear(M, N_R4, K, dt)
    g = _gated(M, N_R2, K, dt)
    for tiles, N in ((2, N_R2), (2, N_R2 - 1), (4, N_R4)):
        for cap in (4096, 3):
            for e in ("store32", "resid32"):
                K_.set_gemv_rows_tuning(e, tiles=tiles, unroll=4, max_blocks=cap)
            _check_linear(K_, c, M, N, dt, f"tiles {tiles}, cap {cap}, N {N}")
    for cap in (4096, 3):
        K_.set_gemv_rows_tuning("swiglu", tiles=2, unroll=4, max_blocks=cap)
        _check_swiglu(K_, g, M, N_R2, dt, f"tiles 2, cap {cap}, N {N_R2}")


@functools.lru_cache(maxsize=None)
def _normal(dt):
    g = torch.Generator().manual_seed(5)
    M, N, K = 16, 256, 4096
    x = torch.randn(M, K, generator=g).to(dt)
    w = (torch.randn(2 * N, K, generator=g) / 64).to(dt)
    r = torch.randn(M, N, generator=g)
    x64, w64 = x.double(), w.double()
    y = x64 @ w64.t()                                    # [M, 2N]
    mag = x64.abs() @ w64.abs().t()                      # sum_k |x w|
    return dict(M=M, N=N, K=K, x=x.cuda(), w=w.cuda(), r=r.cuda(), r64=r.double(), y=y, mag=mag)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M", [8, 16])
def test_normal_operands(cuda, dt, M):
    """K 4096, N 256, random normal operands against float64: |got - ref| <= K 2^-24 sum|x w|,
    the bound of an f32 sum of K exact products in any order; resid32 adds the one f32
    rounding of the final add.  swiglu: the two sums' bounds carried through silu (|silu'| <=
    1.1) and the product, plus the rule of tests/_ulp.py for the activation and its 16-bit
    rounding."""
    from cake_amd.ops import hip as K_
    c = _normal(dt)
    N, K = c["N"], c["K"]
    x, y, mag = c["x"][:M], c["y"][:M], c["mag"][:M]
    bound = K * 2.0 ** -24 * mag
    out = torch.empty(M, N, device=cuda)
    K_.gemv_rows(x, c["w"][:N], out, "store32")
    err = (out.double().cpu() - y[:, :N]).abs()
    print(f"store32 {dt} M {M}: worst error / bound {float((err / bound[:, :N]).max()):.3e}")
    assert bool((err <= bound[:, :N]).all())
    res = c["r"][:M].clone()
    K_.gemv_rows(x, c["w"][:N], res, "resid32")
    ref = c["r64"][:M] + y[:, :N]
    err = (res.double().cpu() - ref).abs()
    lim = bound[:, :N] + 2.0 ** -24 * ref.abs()
    print(f"resid32 {dt} M {M}: worst error / bound {float((err / lim).max()):.3e}")
    assert bool((err <= lim).all())
    act = torch.empty(M, N, device=cuda, dtype=dt)
    K_.gemv_rows(x, c["w"], act, "swiglu")
    gate, up = y[:, :N], y[:, N:]
    ref = U.silu_t(gate) * up
    carried = 1.1 * bound[:, :N] * (up.abs() + bound[:, N:]) + U.silu_t(gate).abs() * bound[:, N:]
    lim = U.allowance(ref, ref.abs() + U.F32_FLUSH * (gate * up).abs(), dt) + carried
    err = (act.double().cpu() - ref).abs()
    print(f"swiglu {dt} M {M}: worst error / bound {float((err / lim).max()):.3e}")
    assert bool((err <= lim).all())


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("epi", EPIS)
def test_row_independence(cuda, dt, epi):
    """Bit for bit: row b of an M = 8 call equals that row run alone as M = 1 in slot 0, and
    the same row in a permuted batch."""
    from cake_amd.ops import hip as K_
    c = _normal(dt)
    M, N = 8, c["N"]
    x = c["x"][:M].contiguous()
    w = c["w"] if epi == "swiglu" else c["w"][:N]
    odt = dt if epi == "swiglu" else torch.float32

    def run(rows):
        out = c["r"][rows].clone().to(odt) if epi == "resid32" else \
            torch.zeros(len(rows), N, device=cuda, dtype=odt)
        K_.gemv_rows(x[rows].contiguous(), w, out, epi)
        return out

    full = run(list(range(M)))
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    permuted = run(perm)
    for slot, b in enumerate(perm):
        _same(permuted[slot], full[b], f"row {b} in slot {slot} of the permuted batch")
    for b in range(M):
        _same(run([b])[0], full[b], f"row {b} alone")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("hd", [64, 128])
def test_rope_kv_rows(cuda, dt, hd):
    """q, k and v of five rows at positions 0, S - 1, 17, S and -1 against float64 (the RoPE
    rule of tests/_ulp.py; v is one rounding: bit-equal): the first three write their own
    cache row of layer 1, the last two nothing; every other byte of every cache and of q_out
    stays as it was."""
    from cake_amd.ops import hip as K_
    nh, nkv, S, L, layer = 4, 2, 64, 2, 1
    pos = [0, S - 1, 17, S, -1]
    M = len(pos)
    g = torch.Generator().manual_seed(hd)
    qkv = torch.randn(M, (nh + 2 * nkv) * hd, generator=g)
    inv = U.inv_freq(hd)
    fill = lambda: torch.randn(L, nkv, S, hd, generator=g).to(dt)       # noqa: E731
    k0, v0 = [fill() for _ in range(M)], [fill() for _ in range(M)]
    kc, vc = [t.cuda() for t in k0], [t.cuda() for t in v0]
    q0 = torch.full((M, nh * hd), CANARY)
    q = q0.cuda()
    K_.rope_kv_rows(qkv.cuda(), torch.tensor(pos, dtype=torch.int32, device=cuda), inv.cuda(), q,
                    kc, vc, layer=layer)
    torch.cuda.synchronize()
    q = q.cpu()
    nq, nk = nh * hd, nkv * hd
    for m, p in enumerate(pos):
        kg, vg = kc[m].cpu(), vc[m].cpu()
        if not 0 <= p < S:
            assert torch.equal(q[m], q0[m]), f"row {m} (pos {p}) wrote q"
            assert torch.equal(kg.view(torch.int16), k0[m].view(torch.int16)), f"row {m} wrote k"
            assert torch.equal(vg.view(torch.int16), v0[m].view(torch.int16)), f"row {m} wrote v"
            continue
        ref, A = U.rope_ref(qkv[m:m + 1, :nq], nh, hd, p, inv)
        err = (q[m:m + 1].double() - ref).abs()
        lim = 2.0 ** -24 * ref.abs() + U.K * U.EPS24 * A
        assert bool((err <= lim).all()), f"row {m} (pos {p}): q off by {float((err / lim).max())} bounds"
        ref, A = U.rope_ref(qkv[m:m + 1, nq:nq + nk], nkv, hd, p, inv)
        U.assert_rule(kg[layer, :, p, :].reshape(1, nk), ref, A, f"row {m} (pos {p}) k")
        _same(vg[layer, :, p, :].reshape(nk), qkv[m, nq + nk:].to(dt), f"row {m} (pos {p}) v")
        for got, was, name in ((kg, k0[m], "k"), (vg, v0[m], "v")):
            keep = torch.ones(L, nkv, S, hd, dtype=torch.bool)
            keep[layer, :, p, :] = False
            assert torch.equal(got.view(torch.int16)[keep], was.view(torch.int16)[keep]), \
                f"row {m}: {name} cache changed outside row {p} of layer {layer}"


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M,H", [(1, 512), (8, 4096), (3, 1100)])
def test_rmsnorm_split_rows(cuda, dt, M, H):
    """The two-term RMSNorm of the batched lm_head: the first term is cake_rmsnorm's row bit
    for bit, and the two terms together hold the float64 value to f32 accuracy -- the RMSNorm
    rule of tests/_ulp.py without its 16-bit half ulp, plus the second term's own rounding:
    2^-8 of the first term's half ulp, or half the subnormal spacing of the dtype where the
    second term is that small (f16: 2^-25)."""
    from cake_amd.ops import hip as K_
    g = torch.Generator().manual_seed(M + H)
    x = torch.randn(M, H, generator=g) * 3
    w = (1 + torch.randn(H, generator=g) / 8).to(dt)
    out = torch.full((2 * M + 1, H), CANARY, device=cuda, dtype=dt)
    K_.rmsnorm_split_rows(x.cuda(), w.cuda(), 1e-5, out[:2 * M])
    one = torch.empty(M, H, device=cuda, dtype=dt)
    K_.rmsnorm(x.cuda(), w.cuda(), 1e-5, one)
    _same(out[:M], one, "first term vs rmsnorm")
    assert bool((out[2 * M] == CANARY).all())
    ref, A = U.rmsnorm_ref(x, w, 1e-5)
    got = out[:M].double().cpu() + out[M:2 * M].double().cpu()
    lim = U.K * U.EPS24 * A + 2.0 ** -8 * 0.5 * U.ulp16(ref, dt) + \
        0.5 * 2.0 ** (U.EMIN[dt] - U.MANT[dt])
    err = (got - ref).abs()
    print(f"{dt} [{M}, {H}]: worst error / bound {float((err / lim).max()):.3e}")
    assert bool((err <= lim).all())


def test_refusals(cuda):
    """M = 0, M = 17 and K = 48 are refused by the entry point, before any launch."""
    from cake_amd.ops import hip as K_
    from cake_amd.ops._lib import KernelError
    dt = torch.bfloat16
    x = torch.zeros(17, 64, device=cuda, dtype=dt)
    w = torch.zeros(16, 64, device=cuda, dtype=dt)
    out = torch.full((17, 16), CANARY, device=cuda)
    for M in (0, 17):
        with pytest.raises(KernelError):
            K_.gemv_rows(x, w, out, "store32", M=M)
    with pytest.raises(KernelError):
        K_.gemv_rows(x[:4, :48].contiguous(), w[:, :48].contiguous(), out, "store32")
    assert bool((out == CANARY).all())
