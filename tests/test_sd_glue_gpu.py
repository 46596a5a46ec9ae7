"""Value-level checks of the glue and noise kernels both native engines rest on: the
scheduler's Philox normal and the full scheduler step, the seeded weight fill, the
tensor-parallel slice sum, the CLIP embedding sum, the 16-bit widening, the scaled copy and
the timestep embedding.  References: tests/_glue.py (float64, or the exact operation);
outputs sit in front of sentinel guard elements."""
import functools
import math

import numpy as np
import pytest
import torch

import _glue as G
import _ulp as U

pytestmark = pytest.mark.gpu
DT_IDS = ["bf16", "f16"]
dtypes = pytest.mark.parametrize("dt", U.DTYPES, ids=DT_IDS)
SENTINEL = 0x5A5A                      # a finite value in both 16-bit dtypes
SENT32 = 12345.678                     # guard value of f32 buffers
INVALID = 1                            # hipErrorInvalidValue
CAP = 4096 * 256                       # items one trip of a capped elementwise grid covers
Z_TOL = 1e-3     # a quarter of a bf16 ulp at |z| = 1 (below what the 16-bit UNet input resolves;
                 # G_TOL of the sampling tests); a wrong word, counter or index is O(1)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int16)


def _guarded16(n, dt, dev, guard=64):
    buf = torch.full((n + guard,), SENTINEL, dtype=torch.int16, device=dev).view(dt)
    return buf, buf[:n]


def _guarded32(n, dev, guard=64):
    buf = torch.full((n + guard,), SENT32, dtype=torch.float32, device=dev)
    return buf, buf[:n]


def _guard_ok(buf, n):
    tail = buf[n:]
    if buf.dtype == torch.float32:
        return bool((tail == torch.tensor(SENT32, dtype=torch.float32)).all())
    return bool((tail.view(torch.int16) == SENTINEL).all())


def _assert_rule32(got, ref, A, what):
    """The rule of _ulp.py for an f32 output: the f32 spacing as its first term."""
    got = got.detach().cpu()
    assert got.dtype == torch.float32 and got.shape == ref.shape, what
    bad = U.violations(got, ref, A)
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        err = (got.double() - ref).abs()
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the rule, first at "
            f"{list(i)}: got {float(got[i])!r}, float64 {float(ref[i])!r}, error "
            f"{float(err[i]):.3e}, allowed {float(U.allowance(ref, A, torch.float32)[i]):.3e}; "
            f"the smallest k that passes: {U.min_k(got, ref, A):g}")


# ---------------------------------------------------------------------------
# the scheduler's noise, value by value
# ---------------------------------------------------------------------------

NOISE_N = 1 << 16
NOISE_RUNS = [(12345, 0), (12345, 51), (12345, 174), (12345, 178), (12345, 209), ((7 << 32) | 5, 3)]
NOISE_ROWS = 210                       # the coef table: a row for every step above


@functools.lru_cache(maxsize=16)
def _z_ref(n, step, seed):
    return G.sd_normal_ref(np.arange(n), step, seed)


def _noise(cuda, dt, step_t, seed):
    """x after one noise-only step (coef (0, 0, 1, 1), zero pred, x = 0): the normals."""
    from cake_amd.ops import hip as K
    coef = torch.tensor([[0.0, 0.0, 1.0, 1.0]] * NOISE_ROWS, device=cuda)
    pred = torch.zeros(NOISE_N, device=cuda, dtype=dt)
    buf, x = _guarded32(NOISE_N, cuda)
    x.zero_()
    K.sched_step(x, pred, False, 1.0, coef, step_t, torch.tensor([seed], device=cuda, dtype=torch.int64))
    assert _guard_ok(buf, NOISE_N)
    return x.cpu()


@dtypes
def test_sched_noise_values(cuda, dt):
    """Every one of 2^16 normals of six (seed, step) pairs within 1e-3 of sd_normal_ref: Philox
    words 0 and 1 of counter (element, step), key (seed low, seed high).  The pinned extreme
    draws (n1 = 0: the largest radius; n1 = 2^24 - 1: u1 = 1.0, z = 0) are among them.
    Measured on the MI355X (printed): the largest |z - ref| over all runs is 4.71e-07, in both
    dtypes; with the fast __logf / __cosf the kernel used before it was 1.67e-06."""
    from cake_amd.ops import hip as K
    covered = set()
    worst = 0.0
    for seed, step in NOISE_RUNS:
        z = _noise(cuda, dt, torch.tensor([step], device=cuda, dtype=torch.int32), seed)
        ref = _z_ref(NOISE_N, step, seed)
        err = np.abs(z.double().numpy() - ref)
        print(f"sched noise {DT_IDS[U.DTYPES.index(dt)]} seed {seed} step {step}: max |z - ref| = "
              f"{err.max():.3e} at {int(err.argmax())}")
        worst = max(worst, float(err.max()))
        assert err.max() <= Z_TOL, (seed, step, int(err.argmax()), float(err.max()))
        for j, (s, st, i, n1) in enumerate(G.SD_EXTREMES):
            if (s, st) == (seed, step):
                assert i < NOISE_N and int(G.sd_words(i, st, s)[0]) == n1
                assert abs(float(z[i]) - G.SD_EXTREME_Z[j]) <= Z_TOL
                if n1 == G.N_MAX:
                    assert float(z[i]) == 0.0            # u1 = 1.0: log 0, exactly no noise
                covered.add(j)
    assert covered == set(range(len(G.SD_EXTREMES)))
    print(f"sched noise {DT_IDS[U.DTYPES.index(dt)]}: max error over all runs {worst:.3e}")
    # the step advanced on the device: the values of the new step
    step_t = torch.tensor([50], device=cuda, dtype=torch.int32)
    K.step_advance(step_t)
    z = _noise(cuda, dt, step_t, 12345)
    assert int(step_t.item()) == 51
    assert np.abs(z.double().numpy() - _z_ref(NOISE_N, 51, 12345)).max() <= Z_TOL
    direct = _noise(cuda, dt, torch.tensor([51], device=cuda, dtype=torch.int32), 12345)
    assert torch.equal(z.view(torch.int32), direct.view(torch.int32))


# ---------------------------------------------------------------------------
# the full scheduler step
# ---------------------------------------------------------------------------

SCHED_SEED = 12345
SCHED_G = 7.5


@dtypes
@pytest.mark.parametrize("cfg", [False, True], ids=["nocfg", "cfg"])
@pytest.mark.parametrize("n,steps", [(1000, (0, 1, 2)), (CAP + 77, (1,))], ids=["n1000", "past-cap"])
def test_sched_step_full(cuda, dt, cfg, n, steps):
    """x' = A x + B e + N z with nonzero A, B, N, S against float64 under the rule (A term:
    |A x| + |B| (|u| + g |c - u|) + |N z|), with and without cfg and next_in; a ragged last
    block (n = 1000) and past one trip of the capped grid.  next_in is the 16-bit rounding of
    the device's own x' * S bit for bit, its cfg halves equal; pred is not written.
    Measured on the MI355X (printed): the kernel needs k = 4 at most (K = 128), largest error
    2.5e-06.  Before this test the noise used __logf / __cosf and needed k = 512 at three of
    the 2^20 elements without cfg, and the f16 next_in was one rounding of the exact product
    (v_fma_mixlo_f16), which differs from the f32 product's rounding in the past-cap case."""
    from cake_amd.ops import hip as K
    x0, pred, coef = G.sched_inputs(n, cfg, dt, U.seed_of("sched", cfg, n))
    m = (2 if cfg else 1) * n
    seed = torch.tensor([SCHED_SEED], device=cuda, dtype=torch.int64)
    pred_d, coef_d = pred.to(cuda), coef.to(cuda)
    for step in steps:
        z = torch.from_numpy(_z_ref(n, step, SCHED_SEED)) if float(coef[step, 2]) else None
        ref, A = G.sched_step_ref(x0, pred, cfg, SCHED_G, coef, step, SCHED_SEED, z=z)
        step_t = torch.tensor([step], device=cuda, dtype=torch.int32)
        outs = []
        for with_next in (False, True):
            what = f"sched_step n {n} cfg {cfg} step {step} next_in {with_next}"
            xbuf, x = _guarded32(n, cuda)
            x.copy_(x0)
            nbuf, nxt = _guarded16(m, dt, cuda)
            K.sched_step(x, pred_d, cfg, SCHED_G, coef_d, step_t, seed, nxt if with_next else None)
            got = x.cpu()
            assert _guard_ok(xbuf, n) and _guard_ok(nbuf, m if with_next else 0), what
            assert torch.equal(_bits(pred_d).cpu(), _bits(pred)), what + ": pred written"
            print(f"{what}: k needed {U.min_k(got, ref, A):g}, max error "
                  f"{float((got.double() - ref).abs().max()):.3e}")
            _assert_rule32(got, ref, A, what)
            if with_next:
                want = (got * coef[step, 3]).to(dt)          # one f32 product, one rounding
                assert torch.equal(_bits(nxt[:n]).cpu(), _bits(want)), what + ": next_in"
                if cfg:
                    assert torch.equal(_bits(nxt[n:]), _bits(nxt[:n])), what + ": cfg halves"
            outs.append(got)
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


# ---------------------------------------------------------------------------
# fill_normal
# ---------------------------------------------------------------------------

FILL_BIG = 16384 * 256 * 8 + 8 * 300 + 5       # past the capped grid's first trip, with a tail
FILL_N = [1, 7, 8, 9, 15, 4099, FILL_BIG]
FILL_MS = [(0.0, 1.0), (0.25, 0.02)]
FILL_KEYS = [1, G.GOLDEN]


def _fill_indices(n):
    if n <= 1 << 17:
        return np.arange(n)
    edge = 16384 * 256 * 8
    rnd = np.random.default_rng(n).integers(0, n, 1 << 16)
    ext = [2 * p + e for _, p, _ in G.FILL_EXTREMES for e in (0, 1)]
    assert max(ext) < n
    idx = np.unique(np.concatenate([np.arange(4096), np.arange(n - 4096, n),
                                    np.arange(edge - 4096, min(edge + 4096, n)), rnd, ext]))
    assert idx[0] >= 0 and idx[-1] < n          # (a gather past the buffer traps on the device)
    return idx


@functools.lru_cache(maxsize=32)
def _fill_ref(n, key):
    idx = _fill_indices(n)
    return idx, G.fill_normal_ref(key, idx)


@functools.lru_cache(maxsize=8)
def _rounded_moments(mean, std, dt):
    """Mean and std of round_dt(f32(mean + std z)), z ~ N(0, 1), on 2^20 midpoint quantiles:
    what the moments of a correct fill estimate (the rounding adds about ulp^2 / 12 of
    variance, visible at std = 0.02 in bf16; the quantile grid itself is off by ~ 2e-6)."""
    q = (torch.arange(1 << 20, dtype=torch.float64) + 0.5) / (1 << 20)
    v = (mean + std * torch.special.ndtri(q)).float().to(dt).double()
    return float(v.mean()), float(v.std(unbiased=False))


@dtypes
@pytest.mark.parametrize("n", FILL_N)
def test_fill_normal(cuda, dt, n):
    """Element i is mean + std * fill_normal_ref(key, i) within half an output ulp + 1e-3 std
    (every element, or the sampled ones of the large fill: both ends, the elements around the
    first trip of the capped grid, 2^16 random ones, the two extreme pairs); the moments of the
    whole buffer; same key, same bits; the guard behind n."""
    from cake_amd.ops import hip as K
    fills = {}
    for mean, std in FILL_MS:
        m32, s32 = float(np.float32(mean)), float(np.float32(std))
        for key in FILL_KEYS:
            what = f"fill_normal n {n} N({mean}, {std}^2) key {key:#x}"
            buf, out = _guarded16(n, dt, cuda)
            K.fill_normal(out, mean, std, key)
            assert _guard_ok(buf, n), what + ": guard"
            idx, z = _fill_ref(n, key)
            got = out[torch.from_numpy(idx).to(cuda)].cpu().double()
            ref = torch.from_numpy(m32 + s32 * z)
            err = (got - ref).abs()
            allow = 0.5 * U.ulp16(ref, dt) + 1e-3 * s32
            bad = err > allow
            assert not bad.any(), (what, int(bad.sum()), int(idx[bad.numpy()][0]),
                                   float(got[bad][0]), float(ref[bad][0]))
            if key == 1 and n == FILL_BIG:
                for (_, p, hi), zz in zip(G.FILL_EXTREMES, G.FILL_EXTREME_Z):
                    for e in (0, 1):
                        j = int(np.searchsorted(idx, 2 * p + e))
                        assert idx[j] == 2 * p + e and abs(float(ref[j]) - (m32 + s32 * zz[e])) < 1e-5
            if n >= 4099:
                v = out.double()
                em, es = _rounded_moments(m32, s32, dt)
                dm, ds = float(v.mean()), float(v.std(unbiased=False))
                print(f"{what}: mean {dm:.6g} (expect {em:.6g}), std {ds:.6g} (expect {es:.6g})")
                assert abs(dm - em) <= 5 * s32 / math.sqrt(n), what
                assert abs(ds - es) <= 5 * s32 / math.sqrt(2 * n), what
            again = torch.empty_like(out)
            K.fill_normal(again, mean, std, key)
            assert torch.equal(_bits(again), _bits(out)), what + ": not reproducible"
            fills[(mean, std, key)] = out
        if n >= 8:
            a, b = (fills[(mean, std, k)] for k in FILL_KEYS)
            assert not torch.equal(_bits(a), _bits(b))


@dtypes
def test_fill_normal_refuses_misaligned(cuda, dt):
    from cake_amd.ops._lib import kernels
    buf, out = _guarded16(64, dt, cuda, guard=0)
    for off in (1, 4, 7):
        rc = kernels().cake_fill_normal(U.DTYPES.index(dt), out[off:].data_ptr(), 32, 0.0, 1.0, 1, _st())
        torch.cuda.synchronize()
        assert rc == INVALID and _guard_ok(buf, 0)
    assert kernels().cake_fill_normal(2, out.data_ptr(), 32, 0.0, 1.0, 1, _st()) == INVALID
    assert kernels().cake_fill_normal(U.DTYPES.index(dt), out.data_ptr(), 0, 0.0, 1.0, 1, _st()) == 0
    torch.cuda.synchronize()
    assert _guard_ok(buf, 0)


# ---------------------------------------------------------------------------
# sum_slices
# ---------------------------------------------------------------------------

SUM_BIG = CAP * 4 + 6
SUM_N = [1, 2, 3, 4, 5, 1023, 1027, SUM_BIG]


def _ceil4(n):
    return (n + 3) // 4 * 4


@pytest.mark.parametrize("n", SUM_N)
def test_sum_slices(cuda, n):
    """Bit for bit the sequential f32 sum in kernel order (out or 0, then w = 0 .. W - 1; plain
    IEEE adds, so f32 torch on the CPU is exact), slices `stride` apart with NaN between them.
    Strides: n rounded up to 4, and that plus 64 (a stride must be a multiple of 4)."""
    from cake_amd.ops import hip as K
    g = torch.Generator().manual_seed(n)
    for W in ((2,) if n == SUM_BIG else (1, 2, 3, 8)):
        for stride in (_ceil4(n), _ceil4(n) + 64):
            src = torch.full(((W - 1) * stride + n + 64,), float("nan"))
            for w in range(W):
                src[w * stride:w * stride + n] = torch.randn(n, generator=g) * (10.0 ** (w % 3 - 1))
            out0 = torch.randn(n, generator=g)
            src_d = src.to(cuda)
            for acc in (0, 1):
                what = f"sum_slices n {n} W {W} stride {stride} accumulate {acc}"
                want = out0.clone() if acc else torch.zeros(n)
                for w in range(W):
                    want = want + src[w * stride:w * stride + n]
                buf, out = _guarded32(n, cuda)
                out.copy_(out0)
                K.sum_slices(out, src_d, W, stride, n, bool(acc))
                assert _guard_ok(buf, n), what + ": guard"
                assert not want.isnan().any()
                assert torch.equal(out.cpu().view(torch.int32), want.view(torch.int32)), what


def test_sum_slices_refusals(cuda):
    from cake_amd.ops._lib import kernels
    fn = kernels().cake_sum_slices
    buf, out = _guarded32(64, cuda, guard=0)
    src = torch.ones(256, device=cuda)
    o, s = out.data_ptr(), src.data_ptr()
    for args in [(o, s, 2, 4, 8, 0),          # stride < n
                 (o, s, 2, 10, 8, 0),         # stride % 4
                 (o + 4, s, 2, 8, 8, 0),      # misaligned out
                 (o, s + 4, 2, 8, 8, 0),      # misaligned src
                 (o, s, 0, 8, 8, 0),          # W = 0
                 (o, s, 2, 8, -1, 0)]:
        assert fn(*args, _st()) == INVALID, args
    assert fn(o, s, 2, 8, 0, 0, _st()) == 0   # n = 0: nothing to do
    torch.cuda.synchronize()
    assert _guard_ok(buf, 0)
    from cake_amd.ops import hip as K
    with pytest.raises(ValueError):
        K.sum_slices(out, src, 2, 4, 8, False)
    with pytest.raises(ValueError):
        K.sum_slices(out, src[:12], 2, 8, 8, False)       # src shorter than the last slice


# ---------------------------------------------------------------------------
# clip_embed, widen16, scale_copy
# ---------------------------------------------------------------------------

@dtypes
@pytest.mark.parametrize("rows,T,D,V", [(77, 77, 768, 1000), (154, 77, 40, 50), (154, 77, 7000, 300)])
def test_clip_embed_bit_equal(cuda, dt, rows, T, D, V):
    """out[r] = tok[clamp(ids[r])] + pos[r % T], one rounding of the f32 sum; ids outside
    [0, V) are clamped; rows = 2 T wraps the position; 154 x 7000 is past the capped grid."""
    from cake_amd.ops import hip as K
    g = torch.Generator().manual_seed(rows + D)
    tok = torch.randn(V, D, generator=g).to(dt)
    pos = (0.5 * torch.randn(T, D, generator=g)).to(dt)
    ids = torch.randint(0, V, (rows,), generator=g).int()
    ids[:4] = torch.tensor([0, V - 1, -5, V + 3], dtype=torch.int32)
    ids[-2:] = torch.tensor([V + 3, -5], dtype=torch.int32)
    buf, out = _guarded16(rows * D, dt, cuda)
    K.clip_embed(tok.to(cuda), pos.to(cuda), ids.to(cuda), T, out.view(rows, D))
    want = (tok[ids.long().clamp(0, V - 1)].float() + pos[torch.arange(rows) % T].float()).to(dt)
    assert _guard_ok(buf, rows * D)
    assert torch.equal(_bits(out.view(rows, D)).cpu(), _bits(want))


def test_clip_embed_refusals(cuda):
    from cake_amd.ops._lib import kernels
    fn = kernels().cake_clip_embed
    buf, out = _guarded16(64, torch.bfloat16, cuda, guard=0)
    tok = torch.ones(4, 8, device=cuda, dtype=torch.bfloat16)
    ids = torch.zeros(4, device=cuda, dtype=torch.int32)
    p = (tok.data_ptr(), tok.data_ptr(), ids.data_ptr())
    for rows, T, D, V in [(0, 2, 8, 4), (-1, 2, 8, 4), (4, 0, 8, 4), (4, 2, 0, 4), (4, 2, 8, 0),
                          (4, -2, 8, 4), (4, 2, -8, 4), (4, 2, 8, -4)]:
        assert fn(0, *p, rows, T, D, V, out.data_ptr(), _st()) == INVALID, (rows, T, D, V)
    assert fn(2, *p, 4, 2, 8, 4, out.data_ptr(), _st()) == INVALID       # no f32 tables
    torch.cuda.synchronize()
    assert _guard_ok(buf, 0)


@dtypes
def test_widen16_bit_equal(cuda, dt):
    """Every 16-bit code (the infinities; NaN for NaN) widens to torch's .float()."""
    from cake_amd.ops import hip as K
    from cake_amd.ops._lib import kernels
    x = U.all_patterns(dt, finite=False)
    assert x.numel() == 65536
    for xs in (x, x[15360:15361]):                        # all of them; n = 1
        n = xs.numel()
        buf, out = _guarded32(n, cuda)
        K.widen16(xs.to(cuda), out)
        assert _guard_ok(buf, n)
        got, want = out.cpu(), xs.float()
        nan = want.isnan()
        assert torch.equal(got.isnan(), nan)
        assert torch.equal(got[~nan].view(torch.int32), want[~nan].view(torch.int32))
    buf, out = _guarded32(8, cuda, guard=0)
    xd = x[:8].to(cuda)
    for n in (0, -3):
        assert kernels().cake_widen16(U.DTYPES.index(dt), xd.data_ptr(), n, out.data_ptr(), _st()) == INVALID
    torch.cuda.synchronize()
    assert _guard_ok(buf, 0)
    with pytest.raises(ValueError):
        K.widen16(xd[:0], out)


@dtypes
@pytest.mark.parametrize("n", [1, 1000, CAP + 3])
def test_scale_copy_bit_equal(cuda, dt, n):
    """out = round16(x * scale), one f32 product; written twice under dup, else the second
    half stays."""
    from cake_amd.ops import hip as K
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g) * 3
    special = torch.tensor([0.0, -0.0, 65504.0, 7e4, -3.3e5, 1e-8, -6e-8, 3.4e38, 1e-40, 359375.0])
    k = min(n, special.numel())
    x[n - k:] = special[:k]
    xd = x.to(cuda)
    for scale in (1.0, 0.18215, 1 / 0.18215):
        want = (x * torch.tensor(scale, dtype=torch.float32)).to(dt)
        for dup in (False, True):
            buf, out = _guarded16(2 * n, dt, cuda)
            K.scale_copy(xd, scale, dup, out if dup else out[:n])
            what = f"scale_copy n {n} scale {scale} dup {dup}"
            assert torch.equal(_bits(out[:n]).cpu(), _bits(want)), what
            if dup:
                assert torch.equal(_bits(out[n:]).cpu(), _bits(want)) and _guard_ok(buf, 2 * n), what
            else:
                assert _guard_ok(buf, n), what + ": second half written"


# ---------------------------------------------------------------------------
# timestep_embed
# ---------------------------------------------------------------------------

TE_STEPS = [0, 2, 5, None]            # device step index; None: a null step pointer (row 0)


@pytest.mark.parametrize("dt", U.DTYPES + [torch.float32], ids=DT_IDS + ["f32"])
@pytest.mark.parametrize("dim", G.TE_DIMS)
def test_timestep_embed_rule(cuda, dt, dim):
    """sin | cos of t exp(-ln(1e4) k / (half - shift)) against float64 under the rule with
    A = |angle| (an f32 output: the f32 spacing as the first term); the table read at device
    steps 0, 2, 5 and through a null step; t = 0 gives exactly 0 and 1."""
    from cake_amd.ops import hip as K
    table = torch.tensor(G.TE_TABLE, device=cuda)
    half = dim // 2
    worst = 0.0
    for flip, shift in U.TE_FLIP_SHIFT:
        for B in (1, 3):
            for s in TE_STEPS:
                t = G.TE_TABLE[s or 0]
                what = f"timestep_embed dim {dim} flip {flip} shift {shift} B {B} step {s} t {t}"
                n = B * dim
                buf, out = _guarded32(n, cuda) if dt == torch.float32 else _guarded16(n, dt, cuda)
                step = None if s is None else torch.tensor([s], device=cuda, dtype=torch.int32)
                K.timestep_embed(table, step, B, dim, flip, shift, out.view(B, dim))
                assert _guard_ok(buf, n), what
                ref, A = G.timestep_embed_ref(t, B, dim, flip, shift)
                got = out.view(B, dim).cpu()
                worst = max(worst, U.min_k(got, ref, A))
                if dt == torch.float32:
                    _assert_rule32(got, ref, A, what)
                else:
                    U.assert_rule(got, ref, A, what)
                if t == 0.0:
                    sin, cos = (got[:, half:], got[:, :half]) if flip else (got[:, :half], got[:, half:])
                    assert bool((sin == 0).all()) and bool((cos == 1).all()), what
    print(f"timestep_embed dim {dim} {dt}: the kernel needs k = {worst:g} (K = {U.K})")
