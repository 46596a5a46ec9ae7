"""Inputs whose correct result is exact, for bit-level tests of the MFMA kernels.

Integer operands (GEMM / conv): every product and every partial sum is an integer below
2^24 (in units of the operands' power-of-two scales), so f32 accumulation in ANY order is
exact and the only rounding left is the final one to the 16-bit output.

Block-code attention: keys come in blocks of 16 that share one random +-1 vector; a query
row is a multiple of its target block's vector, so its score on the target block beats every
other block by more than 110 (natural-log units) and f32 exp() of the gap is exactly 0.  V
is one-hot inside a block, so the output is 1/n at the columns of the n visible keys of the
target block and exactly 0 elsewhere.  One key dropped, duplicated or wrongly masked
changes n.

Plain torch; every builder works on the device it is given (CPU by default).
"""
from __future__ import annotations

import math

import torch

EXACT_INT = {torch.bfloat16: 256, torch.float16: 2048}  # integers up to here are exact
MIN_GAP = 110.0       # exp(-110) = 1.7e-48 < 2^-150: rounds to 0 in f32 (denormals included)
BLOCK = 16


# ---------------------------------------------------------------------------
# integer operands
# ---------------------------------------------------------------------------

def int_operands(shape, lo: int, hi: int, dtype, seed: int, *, scale: float = 1.0,
                 sparsity: float = 0.0, device="cpu") -> torch.Tensor:
    """Uniform integers in [lo, hi] times `scale` (a power of two), each zeroed with
    probability `sparsity`, as `dtype`; raises unless every value is exact in `dtype`."""
    if math.frexp(scale)[0] != 0.5:
        raise ValueError(f"scale {scale} is not a power of two")
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(lo, hi + 1, tuple(shape), generator=g, dtype=torch.int64).double()
    if sparsity > 0.0:
        t = t * (torch.rand(tuple(shape), generator=g, dtype=torch.float64) >= sparsity)
    t = t * scale
    out = t.to(dtype)
    if not torch.equal(out.double(), t):
        raise AssertionError(f"[{lo}, {hi}] * {scale} is not exact in {dtype}")
    if dtype in EXACT_INT and max(abs(lo), abs(hi)) > EXACT_INT[dtype]:
        raise AssertionError(f"integers up to {max(abs(lo), abs(hi))} are not all exact in {dtype}")
    return out.to(device)


def _units(t: torch.Tensor, unit: float, name: str) -> torch.Tensor:
    u = t.double() / unit
    if not torch.equal(u, u.round()):
        raise AssertionError(f"{name} is not a multiple of its unit {unit}")
    return u


def check_exact_sum(K: int, x, w, extra=(), *, x_unit: float = 1.0, w_unit: float = 1.0) -> None:
    """Every partial sum of sum_k x_k w_k (+ the `extra` addends) stays an integer below
    2^24 in units of x_unit * w_unit: K * max|x| * max|w| + sum max|extra| < 2^24."""
    unit = x_unit * w_unit
    bound = K * float(_units(x, x_unit, "x").abs().max()) * float(_units(w, w_unit, "w").abs().max())
    for i, t in enumerate(extra):
        if t is not None:
            bound += float(_units(t, unit, f"addend {i}").abs().max())
    if not bound < 2 ** 24:
        raise AssertionError(f"partial sums may reach {bound} >= 2^24 units: not exact in f32")


def exact_linear(x, w, bias=None, resid=None, *, x_unit: float = 1.0,
                 w_unit: float = 1.0) -> torch.Tensor:
    """x [M, K] @ w [N, K]^T (+ bias [N]) (+ resid [M, N]) in float64, returned as f32.

    Raises unless the result is exact: the operands are multiples of their units, every
    possible partial sum is below 2^24 units (so f32 accumulation in any order is exact),
    and the plain f32 computation gives the same values.  The expectation of a 16-bit
    output is `.to(dtype)` of the result (one round-to-nearest-even)."""
    K = x.shape[-1]
    check_exact_sum(K, x, w, (bias, resid), x_unit=x_unit, w_unit=w_unit)
    y = x.double() @ w.double().t()
    y32 = x.float() @ w.float().t()
    if bias is not None:
        y = y + bias.double()
        y32 = y32 + bias.float()
    if resid is not None:
        y = y + resid.double()
        y32 = y32 + resid.float()
    ref = y.float()
    if not (torch.equal(ref.double(), y) and torch.equal(ref, y32)):
        raise AssertionError("the f32 computation is not exact on these operands")
    return ref


def rounding_coverage(ref: torch.Tensor, dtype) -> tuple[float, int]:
    """(fraction of the exact f32 outputs that `dtype` cannot hold, number of exact ties:
    values halfway between two neighbours of `dtype`)."""
    r = ref.to(dtype).float()
    inexact = r != ref
    mant = 7 if dtype == torch.bfloat16 else 10
    _, e = torch.frexp(ref)                       # |ref| in [2^(e-1), 2^e)
    ulp = torch.ldexp(torch.ones_like(ref), e - 1 - mant)
    ties = inexact & ((ref - r).abs() * 2 == ulp)
    return float(inexact.float().mean()), int(ties.sum())


def ulp_distance(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Distance between two tensors of one 16-bit float dtype in units in the last place
    (steps along the ordered line of representable values; +0 and -0 coincide)."""
    if a.dtype != b.dtype or a.dtype not in EXACT_INT:
        raise TypeError("ulp_distance: two tensors of one 16-bit float dtype expected")

    def line(t):
        bits = t.contiguous().view(torch.int16).to(torch.int32)
        mag = bits & 0x7FFF
        return torch.where(bits < 0, -mag, mag)
    return (line(a) - line(b)).abs()


# ---------------------------------------------------------------------------
# block-code attention
# ---------------------------------------------------------------------------

class BlockCode:
    """K / V of `hkv` kv heads over `keys` rows, of which the first `live` are live.

    Block b of kv head g holds the keys j with (j + (16 - phase) % 16) // 16 == b, all equal
    to codes[g, b] (+-1 entries); phase 8 starts with a half block of 8 keys, so blocks
    straddle every 16-key boundary.  V[g, j] is one-hot at column
    col0(g) + (j - phase) % 16, col0(g) = 16 * (g % (D // 16)); V rows >= live are NaN (K
    rows keep the pattern: a dead key that leaks through a mask scores like the target)."""

    def __init__(self, D: int, keys: int, live: int, phase: int, hkv: int, dtype, seed: int,
                 device="cpu"):
        if phase not in (0, 8) or D < BLOCK or not 1 <= live <= keys:
            raise ValueError("block code: phase 0 or 8, D >= 16, 1 <= live <= keys")
        self.D, self.keys, self.live, self.phase, self.hkv = D, keys, live, phase, hkv
        self.dtype, self.device = dtype, device
        j = torch.arange(keys)
        self.block_of = ((j + (BLOCK - phase) % BLOCK) // BLOCK).to(device)      # [keys]
        self.nblocks = int(self.block_of[-1]) + 1
        self.live_blocks = int(self.block_of[live - 1]) + 1
        g = torch.Generator().manual_seed(seed)
        self.codes = (torch.randint(0, 2, (hkv, self.nblocks, D), generator=g) * 2 - 1) \
            .double().to(device)
        self.k = self.codes[:, self.block_of].to(dtype)                            # [hkv, keys, D]
        col = (j - phase) % BLOCK
        col = col[None, :] + BLOCK * (torch.arange(hkv) % (D // BLOCK))[:, None]   # [hkv, keys]
        self.col = col.to(device)
        v = torch.zeros(hkv, keys, D, dtype=torch.float64, device=device)
        v.scatter_(2, self.col[:, :, None], 1.0)
        self.v64 = v.clone()
        v[:, live:] = float("nan")
        self.v = v.to(dtype)


def block_code_queries(bc: BlockCode, targets: torch.Tensor, c: float, *, scale: float | None = None,
                       last_key: torch.Tensor | None = None):
    """Queries aimed at blocks, with their exact expected output.

    targets [H, R] (block ids; H = hkv * group, head h reads kv head h // group); row r of
    head h is c * codes[h // group, targets[h, r]].  A key j is visible to row r when
    j < live and (last_key given) j <= last_key[r].

    Returns (q [H, R, D] in bc.dtype, expect [H, R, D] f32, n [H, R] visible keys of the
    target block).  Raises unless every non-target visible score is at least MIN_GAP below
    the target score, every row has n >= 1, and the f32 softmax reference computed here
    equals the closed form exactly."""
    if math.frexp(c)[0] != 0.5:
        raise ValueError("c must be a power of two")
    dev = bc.device
    targets = targets.to(dev)
    H, R = targets.shape
    if H % bc.hkv:
        raise ValueError("heads not a multiple of kv heads")
    group = H // bc.hkv
    kvh = torch.arange(H, device=dev) // group
    scale = 1.0 / math.sqrt(bc.D) if scale is None else scale
    q64 = c * bc.codes[kvh[:, None], targets]                                      # [H, R, D]
    q = q64.to(bc.dtype)
    if not torch.equal(q.double(), q64):
        raise AssertionError(f"c = {c} is not exact in {bc.dtype}")
    kk = bc.codes[:, bc.block_of]                                                  # [hkv, keys, D]
    j = torch.arange(bc.keys, device=dev)
    vis = (j < bc.live)[None, None, :].expand(H, R, -1)
    if last_key is not None:
        vis = vis & (j[None, None, :] <= last_key.to(dev)[None, :, None])
    in_target = bc.block_of[None, None, :] == targets[:, :, None]
    dots = (q64.view(bc.hkv, group * R, bc.D) @ kk.transpose(1, 2)).view(H, R, bc.keys)  # exact
    s = dots * scale
    n = (vis & in_target).sum(-1)
    if int(n.min()) < 1:
        raise AssertionError("a query's target block has no visible key")
    top = c * bc.D * scale
    other = s.masked_fill(~vis | in_target, float("-inf"))
    gap = top - float(other.max())
    if not gap >= MIN_GAP:
        raise AssertionError(f"worst score gap {gap:.1f} < {MIN_GAP}: another seed / c needed")
    # closed form: 1/n at the columns of the visible keys of the target block
    w = (vis & in_target).double() / n[:, :, None]
    def pv(p):  # [H, R, keys] f64 probabilities x V of the head's kv head
        return (p.view(bc.hkv, group * R, bc.keys) @ bc.v64).view(H, R, bc.D).float()
    expect = pv(w)
    # f32 softmax reference over the visible keys
    s32 = (dots.float() * scale).masked_fill(~vis, float("-inf"))
    p = torch.softmax(s32, -1)
    ref = pv(p.double())
    if not torch.equal(ref, expect):
        raise AssertionError("f32 softmax reference differs from the closed form")
    return q, expect, n, gap


def block_code_attention(*, D: int, keys: int, live: int | None = None, phase: int = 0,
                         targets, c: float, dtype, hkv: int = 1, seed: int = 0,
                         scale: float | None = None, last_key=None, device="cpu"):
    """One-call form: (q, k, v, expect, n, gap, bc); see BlockCode / block_code_queries."""
    bc = BlockCode(D, keys, keys if live is None else live, phase, hkv, dtype, seed, device)
    q, expect, n, gap = block_code_queries(bc, targets, c, scale=scale, last_key=last_key)
    return q, bc.k, bc.v, expect, n, gap, bc


def assert_block_code_output(out: torch.Tensor, expect: torch.Tensor, n: torch.Tensor,
                             what: str = "") -> None:
    """out (16-bit, [..., D]) against the f32 closed form: finite, exactly 0 in the zero
    columns, bit-equal where n is a power of two (1/n is exact), within 1 ulp elsewhere
    (1/n goes through an approximate reciprocal)."""
    assert torch.isfinite(out.float()).all(), f"{what}: non-finite output"
    want = expect.to(out.dtype)
    zero = expect == 0
    bad0 = zero & (out != 0)
    assert not bad0.any(), (f"{what}: {int(bad0.sum())} non-zeros in zero columns, first at "
                            f"{bad0.nonzero()[0].tolist()} = {float(out[bad0][0])}")
    d = ulp_distance(out, want)
    pow2 = ((n & (n - 1)) == 0)[..., None].expand_as(d)
    lim = torch.where(pow2, 0, 1)
    bad = d > lim
    if bad.any():
        i = bad.nonzero()[0].tolist()
        t = tuple(i)
        raise AssertionError(f"{what}: {int(bad.sum())} elements off, first at {i}: got "
                             f"{float(out[t])}, want {float(want[t])} (n = {int(n[t[:-1]])}, "
                             f"{int(d[t])} ulp)")


# ---------------------------------------------------------------------------
# the cases of the GPU tests (test_exact_cpu.py runs every builder below on the CPU)
# ---------------------------------------------------------------------------

GEMM_SHAPES = [(1, 64, 64, 1), (77, 200, 320, 1), (300, 520, 1024, 3), (513, 136, 648, 2),
               (130, 264, 72, 1), (64, 64, 8, 1)]                      # M, N, K, splits
# the smallest shapes at which the four-wave tiles' split_plan takes the in-kernel pair
PAIR_SHAPES = [(256, 256, 128), (200, 512, 128), (200, 512, 256)]      # M, N, K (splits 2)
GEMV_KS = [8, 256, 1792, 2048, 3584, 4096, 14336]
GEMV_NS = [1, 6, 257]
ACT_LIMIT = 16.0


def gemm_case(M: int, N: int, K: int, dtype, device="cpu") -> dict:
    """Integer operands in [-8, 8] with every exact expectation of the plain epilogues."""
    seed = M + N + K
    x = int_operands((M, K), -8, 8, dtype, seed, device=device)
    w = int_operands((N, K), -8, 8, dtype, seed + 1, device=device)
    b = int_operands((N,), -32, 32, dtype, seed + 2, device=device)
    r16 = int_operands((M, N), -128, 128, dtype, seed + 3, device=device)
    r32 = int_operands((M, N), -1000, 1000, torch.float32, seed + 4, device=device)
    return dict(x=x, w=w, b=b, r16=r16, r32=r32, y=exact_linear(x, w), yb=exact_linear(x, w, b),
                yr32=exact_linear(x, w, None, r32), ybr32=exact_linear(x, w, b, r32),
                ybr16=exact_linear(x, w, b, r16))


def act_f64(name: str, y: torch.Tensor) -> torch.Tensor:
    y = y.double()
    if name == "silu":
        return y * torch.sigmoid(y)
    if name == "quick_gelu":
        return y * torch.sigmoid(1.702 * y)
    if name == "gelu":
        return 0.5 * y * (1 + torch.erf(y / math.sqrt(2.0)))
    if name == "gelu_tanh":
        return 0.5 * y * (1 + torch.tanh(math.sqrt(2.0 / math.pi) * (y + 0.044715 * y ** 3)))
    raise ValueError(name)


def act_f32(name: str, y: torch.Tensor) -> torch.Tensor:
    """The same activations in plain f32 torch (the reference-to-reference yardstick)."""
    import torch.nn.functional as F
    y = y.float()
    if name == "silu":
        return F.silu(y)
    if name == "quick_gelu":
        return y * torch.sigmoid(1.702 * y)
    if name == "gelu":
        return F.gelu(y)
    if name == "gelu_tanh":
        return F.gelu(y, approximate="tanh")
    raise ValueError(name)


def gated_f(N: int) -> int:
    return N // 32 * 16


def act_case(M: int, N: int, K: int, dtype, device="cpu") -> dict:
    """Sparse quarter-integer operands: the pre-activation is exact, |y| <= 16, at least
    half of it non-zero.  w2 / b2: the [2F, K] weight of the gated epilogues."""
    seed = 7 * (M + N + K)
    sp = 1.0 - min(1.0, math.sqrt(6.0 / K))   # about six non-zero products per output
    kw = dict(scale=0.25, sparsity=sp, device=device)
    x = int_operands((M, K), -4, 4, dtype, seed, **kw)
    w = int_operands((N, K), -4, 4, dtype, seed + 1, **kw)
    b = int_operands((N,), -16, 16, dtype, seed + 2, scale=1 / 16, device=device)
    Fh = gated_f(N)
    w2 = int_operands((2 * Fh, K), -4, 4, dtype, seed + 3, **kw)
    b2 = int_operands((2 * Fh,), -16, 16, dtype, seed + 4, scale=1 / 16, device=device)
    u = dict(x_unit=0.25, w_unit=0.25)
    yb = exact_linear(x, w, b, **u)
    g = exact_linear(x, w2, **u)
    gb = exact_linear(x, w2, b2, **u)
    for name, t in (("y + b", yb), ("gated y", g), ("gated y + b", gb)):
        if float(t.abs().max()) > ACT_LIMIT or float((t != 0).float().mean()) < 0.5:
            raise AssertionError(f"{name}: max {float(t.abs().max())}, non-zero "
                                 f"{float((t != 0).float().mean()):.2f}")
    return dict(x=x, w=w, b=b, w2=w2, b2=b2, F=Fh, yb=yb,
                pre=dict(silu=yb, quick_gelu=yb, gelu=yb, swiglu=g[:, :Fh], geglu=gb[:, Fh:]),
                silu=act_f64("silu", yb), quick_gelu=act_f64("quick_gelu", yb),
                gelu=act_f64("gelu", yb),
                swiglu=act_f64("silu", g[:, :Fh]) * g[:, Fh:].double(),
                geglu=gb[:, :Fh].double() * act_f64("gelu_tanh", gb[:, Fh:]),
                f32=dict(silu=act_f32("silu", yb), quick_gelu=act_f32("quick_gelu", yb),
                         gelu=act_f32("gelu", yb),
                         swiglu=act_f32("silu", g[:, :Fh]) * g[:, Fh:],
                         geglu=gb[:, :Fh] * act_f32("gelu_tanh", gb[:, Fh:])))


def act_allowance(case: dict, name: str, dtype) -> torch.Tensor:
    """Allowed ulp distance per output of an activation epilogue: 1 ulp (a rounding-boundary
    flip: the pre-activation is exact and f32 evaluation errs far below half a 16-bit ulp)
    plus the distance the f32-torch yardstick itself has from the float64 value, taken as
    the worst over the outputs whose activated operand lies in the same unit interval
    [floor(y), floor(y) + 1).  The yardstick is off only where f32 cancels: the erf and tanh GELUs
    below about -3 (y (1 + erf(y / sqrt 2)) / 2: the sum loses its leading bits)."""
    d = ulp_distance(case["f32"][name].to(dtype), case[name].to(dtype))
    bucket = (case["pre"][name].floor().clamp(-16, 16) + 16).long()
    worst = torch.zeros(33, dtype=d.dtype, device=d.device).scatter_reduce(
        0, bucket.reshape(-1), d.reshape(-1), "amax")
    return 1 + worst[bucket]


def gemv_case(K: int, N: int, dtype, device="cpu") -> dict:
    x = int_operands((K,), -8, 8, dtype, K + N, device=device)
    w = int_operands((N, K), -8, 8, dtype, K + N + 1, device=device)
    out0 = int_operands((N,), -1000, 1000, torch.float32, K + N + 2, device=device)
    return dict(x=x, w=w, out0=out0, y=exact_linear(x[None], w)[0],
                yacc=exact_linear(x[None], w, None, out0[None])[0])


# --- decode GEMV over quantised weights ----------------------------------------

GEMV_FMT_KS = [32, 2048, 4096, 14336]
E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)  # the value of an e2m1 code's low 3 bits


def gemv_fmt_case(fmt: str, K: int, N: int, dtype, device="cpu") -> dict:
    """Exact operands of the fp8 (`w8`) / MXFP4 (`w4`) decode GEMV: x integers, `quant` the
    kernel's weight operands, y / yacc from exact_linear on their dequantised values.

    w8: codes are the integers [-8, 8] as e4m3fn bytes, row scales 2^-2 .. 2^2: in units of
    2^-2 a weight is at most 8 * 16, so K 14336 reaches 14336 * 8 * 128 + 4000 < 2^24.
    w4: every e2m1 code (both zeros included), e8m0 bytes 125 .. 129 per 32-block: in units
    of 2^-3 a weight is at most 6 * 4 * 8 = 192; |x| <= 8 keeps K <= 4096 below 2^24, and at
    K 14336 x is drawn from [-6, 6] (14336 * 6 * 192 + 8000 < 2^24 <= 14336 * 7 * 192)."""
    seed = 3 * (K + N) + (1 if fmt == "w8" else 2)
    g = torch.Generator().manual_seed(seed)
    if fmt == "w8":
        x = int_operands((K,), -8, 8, dtype, seed)
        codes = int_operands((N, K), -8, 8, torch.float32, seed + 1).to(torch.float8_e4m3fn)
        scale = torch.ldexp(torch.ones(N), torch.randint(-2, 3, (N,), generator=g))
        w = codes.float() * scale[:, None]
        quant, w_unit = (codes.view(torch.uint8), scale), 2.0 ** -2
    elif fmt == "w4":
        w_unit = 2.0 ** -3
        xmax = min(8, (2 ** 24 - 1 - int(1000 / w_unit)) // (K * 192))
        x = int_operands((K,), -xmax, xmax, dtype, seed)
        nib = torch.randint(0, 16, (N, K), generator=g)
        e8 = torch.randint(125, 130, (N, K // 32), generator=g)
        lut = torch.tensor(E2M1 + tuple(-v for v in E2M1))
        w = torch.ldexp(lut[nib].reshape(N, -1, 32), (e8 - 127)[:, :, None]).reshape(N, K)
        quant = ((nib[:, 0::2] | (nib[:, 1::2] << 4)).to(torch.uint8), e8.to(torch.uint8))
    else:
        raise ValueError(fmt)
    out0 = int_operands((N,), -1000, 1000, torch.float32, seed + 2)
    y = exact_linear(x[None], w, w_unit=w_unit)[0]
    yacc = exact_linear(x[None], w, None, out0[None], w_unit=w_unit)[0]
    return dict(x=x.to(device), quant=tuple(t.to(device) for t in quant), w=w,
                out0=out0.to(device), y=y.to(device), yacc=yacc.to(device))


# --- convolution -------------------------------------------------------------

CONV_SHAPES = [(2, 9, 7, 128, 320, 3, 1, False), (1, 15, 17, 64, 64, 3, 2, False),
               (2, 8, 8, 64, 128, 3, 1, True), (2, 12, 12, 192, 64, 1, 1, False),
               (1, 8, 8, 320, 4, 3, 1, False)]                 # N, H, W, IC, OC, k, stride, up
CONV_HALO_SHAPE = (2, 21, 19, 128, 192, 3, 1, False)
CONV_SMALL_IC = [(2, 12, 10, 4, 320, 3, 1, False), (1, 17, 13, 4, 64, 3, 2, False),
                 (1, 16, 16, 3, 128, 3, 1, False), (1, 15, 16, 3, 64, 3, 2, False)]
CONV_OUT_NCHW = (2, 12, 10, 320, 4, 3, 1, False)
CONV1X1_SMALL = [(1, 20, 20, 4, 4), (2, 17, 9, 8, 8), (1, 5, 7, 3, 16), (3, 8, 8, 16, 1)]


def conv_case(N, H, W, IC, OC, k, stride, up, dtype) -> dict:
    """Integer conv operands (CPU tensors) with exact float64 F.conv2d expectations.  The
    border pixels of x are large (+-24..32), so a padded tap that reads a wrapped or
    neighbouring pixel instead of zero moves the output by hundreds.
    x [N,H,W,IC]; w [OC,IC,k,k] (wp: packed [OC,k,k,IC]); y* are NHWC f32."""
    import torch.nn.functional as F
    seed = N + H + W + IC + OC + k + stride
    x = int_operands((N, H, W, IC), -4, 4, dtype, seed).double()
    big = int_operands((N, H, W, IC), 24, 32, dtype, seed + 1).double() * \
        (int_operands((N, H, W, IC), 0, 1, dtype, seed + 2).double() * 2 - 1)
    edge = torch.zeros(H, W, dtype=torch.bool)
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
    x = torch.where(edge[None, :, :, None], big, x).to(dtype)
    w = int_operands((OC, IC, k, k), -4, 4, dtype, seed + 3)
    b = int_operands((OC,), -32, 32, dtype, seed + 4)
    pad = k // 2
    VH, VW = H << int(up), W << int(up)
    OH, OW = (VH + 2 * pad - k) // stride + 1, (VW + 2 * pad - k) // stride + 1
    b2 = int_operands((N, OC), -500, 500, torch.float32, seed + 5)
    r = int_operands((N, OH, OW, OC), -128, 128, dtype, seed + 6)
    check_exact_sum(k * k * IC, x, w, (b, b2, r))

    def conv(t):
        xc = x.to(t).permute(0, 3, 1, 2)
        if up:
            xc = F.interpolate(xc, scale_factor=2.0, mode="nearest")
        return F.conv2d(xc, w.to(t), None, stride=stride, padding=pad).permute(0, 2, 3, 1)
    y64, y32 = conv(torch.float64), conv(torch.float32)
    if not torch.equal(y64, y32.double()):
        raise AssertionError("the f32 convolution is not exact on these operands")
    yb = y64 + b.double()
    full = yb + b2.double()[:, None, None, :] + r.double()
    for t in (yb, full):
        if not torch.equal(t.float().double(), t):
            raise AssertionError("conv expectation not exact in f32")
    return dict(x=x, w=w, wp=w.permute(0, 2, 3, 1).contiguous(), b=b, b2=b2, r=r,
                y=y64.float().contiguous(), yb=yb.float().contiguous(),
                full=full.float().contiguous(), stride=stride, pad=pad, up=up)


def conv1x1_case(N, H, W, IC, OC, dtype) -> dict:
    seed = N + H + W + IC + OC
    x = int_operands((N, H, W, IC), -16, 16, dtype, seed)
    w = int_operands((OC, IC), -8, 8, dtype, seed + 1)
    b = int_operands((OC,), -32, 32, dtype, seed + 2)
    yb = exact_linear(x.reshape(-1, IC), w, b).view(N, H, W, OC)
    return dict(x=x, w=w, b=b, yb=yb)


# --- attention ---------------------------------------------------------------

ATTN_C = {40: 64.0, 64: 64.0, 80: 32.0, 128: 32.0, 160: 16.0, 512: 16.0}   # q = c * code
DECODE_SHAPES = [(32, 8, 128), (4, 1, 64), (8, 8, 64)]                  # nh, nkv, hd
DECODE_TKS = [(1, 2048), (16, 2048), (17, 2048), (64, 2048), (65, 2048), (320, 2048),
              (321, 2048), (1000, 2048), (2047, 2048), (8190, 8192)]     # Tk, S
HEADS_TKS = [1, 16, 17, 128, 601]
HEADS_S = 1000
FLASH_SHAPES = [(1, 8, 2, 300, 300, 128, True, 0), (1, 8, 2, 150, 250, 128, True, 100),
                (2, 4, 4, 200, 77, 40, False, 0), (1, 5, 5, 130, 300, 80, False, 0),
                (1, 2, 2, 100, 100, 160, False, 0),
                (1, 12, 12, 77, 77, 64, True, 0)]          # B, H, Hkv, N, M, D, causal, pos0
FLASH_KSPLIT_SHAPES = [(1, 3, 3, 200, 1000, 64, False, 0), (1, 2, 2, 64, 513, 40, False, 0)]
FLASH_FORCED_SPLIT_SHAPES = [(1, 8, 2, 300, 300, 128, True, 0), (1, 8, 2, 150, 250, 128, True, 100)]
ATTN512_SHAPES = [(1, 70, 33), (2, 200, 777)]
FLASH_DEAD_ROWS = 24    # NaN V rows behind the M keys a flash launch is given


def decode_targets(bc: BlockCode, nh: int):
    """Target blocks [nh, 1] of successive decode launches on one cache: head h of launch l
    aims at block (h + l * nh) % live_blocks, so the heads of one kv head differ (where
    there are enough blocks), consecutive launches differ, and every live block is some
    head's target; at least two launches."""
    LB = bc.live_blocks
    h = torch.arange(nh)
    for l in range(max(2, -(-LB // nh))):
        yield ((h + l * nh + (l if LB <= nh else 0)) % LB)[:, None]


def decode_case(nkv: int, hd: int, Tk: int, S: int, phase: int, dtype, device="cpu"):
    """The [nkv, S, hd] cache of one (Tk, phase): Tk live rows, the rest dead."""
    return BlockCode(hd, S, Tk, phase, nkv, dtype, seed=0, device=device)


def flash_case(B, H, Hkv, N, M, D, causal, pos0, phase, dtype, device="cpu"):
    """q [B,H,N,D], k / v [B,Hkv,M,D] (views of M + FLASH_DEAD_ROWS rows; the V rows behind
    M are NaN), expect [B,H,N,D] f32, n [B,H,N].  Non-causal: row r of head h aims at block
    (7 r + h) % nblocks.  Causal: even rows aim at the block of their own diagonal key (only
    part of it is visible: an off-by-one mask changes n), odd rows at an earlier block."""
    qs, ks, vs, es, ns = [], [], [], [], []
    r = torch.arange(N)
    h = torch.arange(H)
    for b in range(B):
        bc = BlockCode(D, M + FLASH_DEAD_ROWS, M, phase, Hkv, dtype, seed=b, device=device)
        if causal:
            own = bc.block_of.cpu()[pos0 + r]                                  # [N]
            early = (7 * r[None, :] + h[:, None]) % own.clamp(min=1)[None, :]
            t = torch.where((r % 2 == 0)[None, :], own[None, :].expand(H, -1), early)
            last = pos0 + r
        else:
            t = (7 * r[None, :] + h[:, None]) % bc.live_blocks
            last = None
        q, e, n, _ = block_code_queries(bc, t, ATTN_C[D], last_key=last)
        qs.append(q), ks.append(bc.k), vs.append(bc.v), es.append(e), ns.append(n)
    q, k, v = torch.stack(qs), torch.stack(ks), torch.stack(vs)
    # projection-style layouts: [B, rows, heads, D] viewed as [B, heads, rows, D]
    lay = lambda t: t.transpose(1, 2).contiguous().transpose(1, 2)
    return lay(q), lay(k)[:, :, :M], lay(v)[:, :, :M], torch.stack(es), torch.stack(ns)


def attn512_case(B, N, M, dtype, device="cpu"):
    """q [B,N,512], k / v [B,M,512], expect [B,N,512] f32, n [B,N]."""
    out = []
    r = torch.arange(N)
    for b in range(B):
        bc = BlockCode(512, M, M, 8 * (b % 2), 1, dtype, seed=b, device=device)
        q, e, n, _ = block_code_queries(bc, ((7 * r + b) % bc.live_blocks)[None, :], ATTN_C[512])
        out.append((q[0], bc.k[0], bc.v[0], e[0], n[0]))
    return tuple(torch.stack(t) for t in zip(*out))
