"""float64 references and one acceptance rule for the norm, RoPE and elementwise kernels.

Every reference is computed in float64 from exactly the values the kernel reads (its 16-bit
or f32 inputs widened).  A kernel output `got` (16-bit) passes at an element when

    |got - ref64| <= 0.5 * ulp16(ref64) + K * 2^-24 * A

ulp16 is the spacing of the output dtype at the reference value (one correct rounding costs
half of it) and A is the magnitude of the terms that cancel in an f32 evaluation:

  norms     (|x| + |mean|) * rstd * |gamma| + |beta|   (RMSNorm: |x| * r * |w|)
  + SiLU    1.1 * A_norm + |silu(y)|   (|silu'| <= 1.1 carries the pre-activation's error,
                                        the product x * sigmoid(x) adds its own)
  RoPE      |a| + |b|
  products  |result|  (+ 2^-102 |g u| where a sigmoid is a factor: f32 holds no sigmoid
                      below 2^-126, and K 2^-24 2^-102 |g u| is K times that flush)

K is not chosen: it is twice the smallest power of two at which the f32 yardstick (the same
formula in plain f32 torch, in the kernel's algorithmic form, never an emulation of the
kernel) passes the rule at every case below.  test_ulp_cpu.py measures it and pins the
constants here.

Builders raise on a badly chosen case (`check_cap`): where K * 2^-24 * A is above one output
ulp for more than 1 % of the elements the rule checks little.  Exempt by construction are the
cases whose point is the A term: the conditioning sweep, LayerNorm's mean offsets, the
exact-statistics inputs (distinct large means; judged in ulp, not by the rule alone) and the
constant groups of the eps-visible inputs and one-element groups (rstd = eps^-1/2 there).

Plain torch on the CPU; the GPU tests move the inputs over.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from _exact import rounding_coverage, ulp_distance  # noqa: F401  (the tests use both from here)

MANT = {torch.bfloat16: 7, torch.float16: 10}
EMIN = {torch.bfloat16: -126, torch.float16: -14}
DTYPES = [torch.bfloat16, torch.float16]
EPS24 = 2.0 ** -24
F32_FLUSH = 2.0 ** -102     # EPS24 * F32_FLUSH = 2^-126, the smallest normal f32

# Measured by test_ulp_cpu.py::test_yardstick_k over every case of this file (509 per dtype;
# it prints the k each family needs).  The f32 yardstick needs k = 64 at one case, f32
# torch.nn.functional.group_norm on the 32800-element groups of GroupNorm NHWC
# (1, 4100, 64, 8), f16, eps-visible (f32 summation error grows with the group; plain
# two-pass f32 needs 16 there).  Everything else needs at most 4: RMSNorm 4 (H = 12288),
# the norms, GEGLU and SiLU * up 2, RoPE 1; the conditioning sweep 4 (bf16) and 2 (f16).
# With the Stable Diffusion families at the end of this file (611 cases per dtype): the
# timestep embedding 16 (f16, dim 2560, t = 999), the scheduler step 2.
YARDSTICK_K = 64
K = 2 * YARDSTICK_K


def ulp16(ref: torch.Tensor, dtype) -> torch.Tensor:
    """Spacing of `dtype` at the float64 value `ref` (the subnormal spacing below the
    smallest normal)."""
    _, e = torch.frexp(ref.abs())                        # |ref| in [2^(e-1), 2^e)
    e = (e - 1).clamp(min=EMIN[dtype])
    return torch.ldexp(torch.ones_like(ref), e - MANT[dtype])


def allowance(ref, A, dtype, k: float = K) -> torch.Tensor:
    return 0.5 * ulp16(ref, dtype) + k * EPS24 * A


def violations(got: torch.Tensor, ref: torch.Tensor, A: torch.Tensor, k: float = K) -> torch.Tensor:
    """Elements of the 16-bit `got` outside the rule.  An element equal to the correctly
    rounded reference always passes (overflow to inf, NaN for NaN)."""
    got = got.detach().cpu()
    want = ref.to(got.dtype)
    same = (got == want) | (got.isnan() & want.isnan())
    ok = (got.double() - ref).abs() <= allowance(ref, A, got.dtype, k)
    return ~(ok | same)


def assert_rule(got, ref, A, what: str = "", k: float = K) -> None:
    got = got.detach().cpu()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    bad = violations(got, ref, A, k)
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        want = ref.to(got.dtype)
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the rule, first at "
            f"{list(i)}: got {float(got[i])!r}, float64 {float(ref[i])!r} (rounds to "
            f"{float(want[i])!r}), {int(ulp_distance(got, want)[i])} ulp, allowed "
            f"{float(allowance(ref, A, got.dtype, k)[i]):.3e}")


def min_k(got, ref, A) -> float:
    """Smallest power of two k (0 if none is needed) at which `got` passes the rule."""
    if not violations(got, ref, A, 0.0).any():
        return 0.0
    k = 2.0 ** -6
    while violations(got, ref, A, k).any():
        k *= 2
        if k > 2 ** 40:
            raise AssertionError("no k below 2^40 passes")
    return k


def check_cap(ref, A, dtype, what: str = "", k: float = K) -> None:
    frac = float((k * EPS24 * A > ulp16(ref, dtype)).double().mean())
    if frac > 0.01:
        raise AssertionError(f"{what}: the A term exceeds one ulp at {frac:.1%} of the elements: "
                             f"badly chosen case")


def max_ulp(got, ref, floor: float = 0.25) -> int:
    """Largest ulp distance from the correctly rounded reference over |ref| > floor."""
    got = got.detach().cpu()
    d = ulp_distance(got, ref.to(got.dtype))
    m = ref.abs() > floor
    return int(d[m].max()) if m.any() else 0


# ---------------------------------------------------------------------------
# references (float64) and yardsticks (the same code run in float32)
# ---------------------------------------------------------------------------

def silu_t(y):
    return y * torch.sigmoid(y)


def _norm(x, dims, g, b, eps, silu):
    """Two-pass mean / variance normalisation in x's dtype: (y, A)."""
    mean = x.mean(dims, keepdim=True)
    var = ((x - mean) ** 2).mean(dims, keepdim=True)
    rstd = torch.rsqrt(var + eps)
    y = (x - mean) * rstd * g + b
    A = (x.abs() + mean.abs()) * rstd * g.abs() + b.abs()
    if silu:
        y = silu_t(y)
        A = 1.1 * A + y.abs()
    return y, A


def layer_norm_ref(x, gamma, beta, eps, t=torch.float64):
    return _norm(x.to(t), (-1,), gamma.to(t), beta.to(t), eps, False)


def group_norm_nchw_ref(x, gamma, beta, G, eps, silu, t=torch.float64):
    B, C = x.shape[:2]
    xx = x.to(t).reshape(B, G, C // G, -1)
    y, A = _norm(xx, (2, 3), gamma.to(t).view(1, G, C // G, 1), beta.to(t).view(1, G, C // G, 1),
                 eps, silu)
    return y.reshape(x.shape), A.reshape(x.shape)


def group_norm_nhwc_ref(x, gamma, beta, G, eps, silu, skip=None, t=torch.float64):
    """x [N, ..., C] (++ skip along channels)."""
    if skip is not None:
        x = torch.cat([x, skip], -1)
    N, C = x.shape[0], x.shape[-1]
    xx = x.to(t).reshape(N, -1, G, C // G)
    y, A = _norm(xx, (1, 3), gamma.to(t).view(1, 1, G, C // G), beta.to(t).view(1, 1, G, C // G),
                 eps, silu)
    return y.reshape(x.shape), A.reshape(x.shape)


def group_norm_nhwc_yardstick(x, gamma, beta, G, eps, silu, skip=None):
    """f32 torch.nn.functional.group_norm on the channels-first view."""
    if skip is not None:
        x = torch.cat([x, skip], -1)
    xc = x.float().movedim(-1, 1).contiguous()   # (the channels-last CPU path forms E[x^2] - mean^2)
    y = F.group_norm(xc, G, gamma.float(), beta.float(), eps)
    if silu:
        y = F.silu(y)
    return y.movedim(1, -1).contiguous()


def rmsnorm_ref(x, w, eps, t=torch.float64):
    xx = x.to(t)
    r = torch.rsqrt((xx * xx).mean(-1, keepdim=True) + eps)
    y = xx * r * w.to(t)
    return y, y.abs()


def gelu_tanh_t(g):
    """0.5 g (1 + tanh u) written as g * sigmoid(2u), the form of common.h's gelu_tanh
    (no cancellation at negative g, so float64 stays a reference there)."""
    return g * torch.sigmoid(1.5957691216057308 * (g + 0.044715 * g * g * g))


def geglu_ref(h, t=torch.float64):
    Fh = h.shape[-1] // 2
    a, g = h[..., :Fh].to(t), h[..., Fh:].to(t)
    y = a * gelu_tanh_t(g)
    return y, y.abs() + F32_FLUSH * (a * g).abs()


def silu_mul_ref(g, u, t=torch.float64):
    y = silu_t(g.to(t)) * u.to(t)
    return y, y.abs() + F32_FLUSH * (g.to(t) * u.to(t)).abs()


def rope_ref(x, n: int, hd: int, pos0: int, inv_freq, t=torch.float64):
    """x [T, n * hd] (16-bit) rotated at positions pos0.. ; the angle is the f32 product
    float32(pos) * float32(inv_freq[i]), its sin / cos are taken in `t`."""
    T = x.shape[0]
    pos = torch.arange(pos0, pos0 + T, dtype=torch.float32)
    ang = (pos[:, None] * inv_freq.float().cpu()[None, :]).to(t)          # [T, hd/2]
    c, s = torch.cos(ang)[:, None, :], torch.sin(ang)[:, None, :]
    xx = x.to(t).reshape(T, n, hd)
    a, b = xx[..., :hd // 2], xx[..., hd // 2:]
    y = torch.cat([a * c - b * s, a * s + b * c], -1).reshape(T, n * hd)
    A = (a.abs() + b.abs()).repeat(1, 1, 2).reshape(T, n * hd)
    return y, A


def to_rgb8_ref(img, nhwc: bool) -> torch.Tensor:
    """trunc(clamp(x / 2 + 0.5, 0, 1) * 255) in float64 -> u8 [B, H, W, 3]."""
    v = torch.trunc((img.double() / 2 + 0.5).clamp(0, 1) * 255).to(torch.uint8)
    return (v if nhwc else v.permute(0, 2, 3, 1)).contiguous()


def all_patterns(dtype, finite: bool = True) -> torch.Tensor:
    """Every 16-bit pattern as `dtype` (the finite ones only by default)."""
    t = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)
    return t[torch.isfinite(t)] if finite else t


# ---------------------------------------------------------------------------
# group layouts: a [groups, elements] matrix placed into the tensor a kernel reads
# ---------------------------------------------------------------------------

def hw_shape(HW: int) -> tuple[int, int]:
    h = max(d for d in range(1, int(math.isqrt(HW)) + 1) if HW % d == 0)
    return h, HW // h


class Rows:
    """LayerNorm / RMSNorm: [rows, C], one group per row."""

    def __init__(self, rows, C):
        self.ng, self.e, self.C, self.G = rows, C, C, 1
        self.shape = (rows, C)

    def place(self, grp):
        return grp.reshape(self.shape).contiguous()

    def chan(self, v):                       # a per-channel vector broadcast to the tensor
        return v.expand(self.shape)


class NCHW(Rows):
    def __init__(self, B, C, H, W, G):
        self.ng, self.e, self.C, self.G = B * G, C // G * H * W, C, G
        self.shape = (B, C, H, W)

    def chan(self, v):
        return v.view(1, -1, 1, 1).expand(self.shape)


class NHWC(Rows):
    """[N, h, w, C] with h * w = HW."""

    def __init__(self, N, HW, C, G):
        self.ng, self.e, self.C, self.G = N * G, HW * (C // G), C, G
        self.N, self.HW = N, HW
        self.shape = (N, *hw_shape(HW), C)

    def place(self, grp):
        g = grp.reshape(self.N, self.G, self.HW, self.C // self.G).permute(0, 2, 1, 3)
        return g.reshape(self.shape).contiguous()


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def affine(C: int, dtype, seed: int, eighths: bool = False):
    """gamma = 1 + 0.25 N with every seventh entry negated, beta = 0.1 N; or (eighths) odd
    multiples of 1/8 in [-15/8, 15/8] and multiples of 1/4 in [-1, 1]: the outputs
    +-gamma + beta of the exact-statistics inputs are then never 0, where a distance in ulp
    says nothing about a kernel whose mean is not exact (Welford's running division)."""
    g = _gen(seed)
    if eighths:
        gamma = (2 * torch.randint(0, 8, (C,), generator=g) + 1).double() / 8
        gamma = gamma * (torch.randint(0, 2, (C,), generator=g) * 2 - 1)
        beta = torch.randint(-4, 5, (C,), generator=g).double() / 4
    else:
        gamma = 1 + 0.25 * torch.randn(C, generator=g, dtype=torch.float64)
        gamma[::7] = -gamma[::7]
        beta = 0.1 * torch.randn(C, generator=g, dtype=torch.float64)
    return gamma.to(dtype), beta.to(dtype)


def random_x(L, mean: float, std: float, dtype, seed: int) -> torch.Tensor:
    grp = mean + std * torch.randn(L.ng, L.e, generator=_gen(seed), dtype=torch.float64)
    return L.place(grp).to(dtype)


EXACT_LIMIT = {torch.bfloat16: 256, torch.float16: 511}   # |m| + a <= this


def exact_x(L, dtype, seed: int, centred: bool = False) -> torch.Tensor:
    """Every group holds m +- a in equal numbers at shuffled places: m an integer distinct
    per group (0 when `centred`: RMSNorm), a in {1, 2, 4}.  Mean m and variance a^2 are exact
    in any summation order; raises when a condition fails."""
    if L.e % 2:
        raise AssertionError(f"exact statistics need an even group size, got {L.e}")
    g = _gen(seed)
    a = torch.tensor([1.0, 2.0, 4.0], dtype=torch.float64)[torch.arange(L.ng) % 3]
    lim = EXACT_LIMIT[dtype] - 4
    if centred:
        m = torch.zeros(L.ng, dtype=torch.float64)
    else:
        if L.ng > 2 * lim + 1:
            raise AssertionError(f"{L.ng} groups need more distinct means than +-{lim} holds")
        m = (torch.randperm(2 * lim + 1, generator=g)[:L.ng] - lim).double()
    sign = torch.ones(L.ng, L.e, dtype=torch.float64)
    sign[:, L.e // 2:] = -1
    sign = sign.gather(1, torch.rand(L.ng, L.e, generator=g).argsort(1))
    grp = m[:, None] + a[:, None] * sign
    x = L.place(grp).to(dtype)
    if not torch.equal(L.place(grp), x.double()):
        raise AssertionError("a value is not representable")
    if float(grp.abs().max()) > EXACT_LIMIT[dtype] or 64 * float(grp.abs().max()) ** 2 >= 2 ** 24:
        raise AssertionError("a 64-term sum of squares may reach 2^24")
    if not (torch.equal(grp.mean(1), m) and torch.equal(((grp - m[:, None]) ** 2).mean(1), a * a)):
        raise AssertionError("group statistics are not m, a^2")
    return x


def check_exact_out(ref, dtype) -> None:
    if not torch.equal(ref.to(dtype).double(), ref):
        raise AssertionError("the exact-statistics output is not representable")


EPSVIS_CONST = 2.0 ** -6   # small, so that rstd = eps^-1/2 = 1000 keeps the A term of a
                           # constant group near one ulp of beta


def epsvis_x(L, dtype, seed: int, phase: int = 0) -> torch.Tensor:
    """Group i is of kind (i + phase) % 4: 0 N(0, 1e-3) (var ~ 1e-6 < eps), 1 constant
    (var = 0), 2 all zero, 3 N(0, 1)."""
    grp = torch.randn(L.ng, L.e, generator=_gen(seed), dtype=torch.float64)
    kind = (torch.arange(L.ng) + phase) % 4
    grp[kind == 0] *= 1e-3
    sgn = torch.where(torch.arange(L.ng) % 2 == 0, 1.0, -1.0).double()
    grp = torch.where((kind == 1)[:, None], (EPSVIS_CONST * sgn)[:, None].expand_as(grp), grp)
    grp[kind == 2] = 0.0
    return L.place(grp).to(dtype)


# ---------------------------------------------------------------------------
# the cases (test_ulp_cpu.py runs every builder; the GPU tests run the kernels on them)
# ---------------------------------------------------------------------------

RMS_T = 3
RMS_H = [4, 8, 1020, 1024, 1028, 2048, 2052, 4096, 4100, 8192, 8196, 12288]
LN_ROWS = [1, 5]
LN_C = [8, 504, 512, 520, 1024, 1032, 2048, 2056, 100, 4]      # wave kernel up to 2048
LN_MEANS = [0.0, 64.0, 256.0]
GEGLU_ROWS = 3
GEGLU_F = [8, 1280, 100]
GN_NCHW = [(1, 32, 1, 1, 32), (2, 64, 3, 5, 32), (1, 64, 8, 8, 32), (1, 8, 2, 4, 8),
           (1, 320, 16, 16, 32), (2, 96, 5, 7, 32)]                          # B, C, H, W, G
GN_NHWC = [(1, 16, 128, 32), (2, 17, 256, 32), (1, 15, 320, 32), (1, 33, 384, 32),
           (1, 33, 4096, 32), (1, 64, 64, 1), (1, 32, 1024, 256), (3, 1, 64, 8),
           (1, 4100, 64, 8)]                                                 # N, HW, C, G
GN_TWO = [(2, 35, 328, 312, 32), (2, 35, 8, 120, 4)]                         # N, HW, Cx, Cs, G
EPS_VISIBLE = [1e-5, 1e-6]
COND = [(0.0, 1.0), (16.0, 1.0), (64.0, 1.0), (256.0, 1.0), (-256.0, 1.0), (200.0, 0.5),
        (1000.0, 4.0)]                                                       # mean, std
COND_NHWC = [(1, 64, 64, 32), (1, 256, 320, 32)]                             # N, HW, C, G
ROPE_S = 131072
ROPE_POS0 = [0, 1, 4095, 8191, None]      # None: the last T rows of the cache
ROPE_T = [1, 7]
ROPE_HD = [64, 128]
ROPE_SCALAR_HD = [24, 40]
ROPE_THETA = 500000.0


def seed_of(*key) -> int:
    import zlib
    return zlib.crc32(repr(tuple(float(k) if isinstance(k, (int, float)) else str(k)
                                 for k in key)).encode()) % (2 ** 31)


def norm_case(L, kind: str, dtype, *, mean=0.0, std=1.0, eps=1e-5, phase=0, silu=False,
              ref_fn=None, cap=None) -> dict:
    """Inputs (CPU) of one norm case on layout L with its float64 (ref, A).

    kind: random | exact | epsvis.  ref_fn(x, gamma, beta, eps) -> (ref, A).  The cap is
    checked unless the case is exempt (module docstring)."""
    if cap is None:
        cap = kind == "random" and mean == 0.0 and L.e > 1
    s = seed_of(kind, L.shape, L.G, mean, std, phase)
    for attempt in range(4):     # a tiny tensor may need another seed to keep the cap
        gamma, beta = affine(L.C, dtype, s + 1, eighths=kind == "exact")
        if kind == "random":
            x = random_x(L, mean, std, dtype, s)
        elif kind == "exact":
            x, eps = exact_x(L, dtype, s), 0.0
        elif kind == "epsvis":
            x = epsvis_x(L, dtype, s, phase)
        else:
            raise ValueError(kind)
        ref, A = ref_fn(x, gamma, beta, eps)
        if not torch.isfinite(ref).all():
            raise AssertionError("non-finite reference")
        if kind == "exact" and not silu:
            check_exact_out(ref, dtype)
        if not cap:
            break
        try:
            check_cap(ref, A, dtype, f"{kind} {L.shape}")
            break
        except AssertionError:
            if attempt == 3:
                raise
            s += 10
    return dict(x=x, gamma=gamma, beta=beta, eps=eps, ref=ref, A=A)


def rms_case(H: int, kind: str, dtype, eps: float = 1e-5) -> dict:
    """x f32 [3, H]; w as `affine`'s gamma.  epsvis: row 0 scaled to 1e-3, row 1 zero."""
    L = Rows(RMS_T, H)
    s = seed_of("rms", kind, H)
    w, _ = affine(H, dtype, s + 1, eighths=kind == "exact")
    if kind == "exact":
        x, eps = exact_x(L, torch.float16, s, centred=True).float(), 0.0
    else:
        x = (3.0 * torch.randn(RMS_T, H, generator=_gen(s), dtype=torch.float64)).float()
        if kind == "epsvis":
            x[0] *= 1e-3
            x[1] = 0.0
    ref, A = rmsnorm_ref(x, w, eps)
    if kind == "exact":
        check_exact_out(ref, dtype)
    check_cap(ref, A, dtype, f"rms {kind} {H}")
    return dict(x=x, w=w, eps=eps, ref=ref, A=A)


def geglu_case(Fh: int, dtype) -> dict:
    h = torch.randn(GEGLU_ROWS, 2 * Fh, generator=_gen(seed_of("geglu", Fh)),
                    dtype=torch.float64).mul(2.0).to(dtype)
    ref, A = geglu_ref(h)
    check_cap(ref, A, dtype, f"geglu {Fh}")
    return dict(h=h, ref=ref, A=A)


def gate_sweep(dtype) -> tuple[torch.Tensor, torch.Tensor]:
    """(gate, other): every finite pattern as the gate, twice: the other operand 1 and 3;
    padded with zeros to a multiple of 8 columns."""
    p = all_patterns(dtype)
    n = (p.numel() + 7) // 8 * 8
    gate = torch.zeros(2, n, dtype=dtype)
    gate[:, :p.numel()] = p
    other = torch.ones(2, n, dtype=dtype)
    other[1] = 3.0
    return gate, other


def rope_inputs(T: int, nh: int, nkv: int, hd: int, dtype, seed: int):
    """One fused [T, (nh + 2 nkv) hd] projection output."""
    return torch.randn(T, (nh + 2 * nkv) * hd, generator=_gen(seed), dtype=torch.float64).to(dtype)


def inv_freq(hd: int) -> torch.Tensor:
    f = 1.0 / (ROPE_THETA ** (torch.arange(0, hd, 2, dtype=torch.float64) / hd))
    return f.float()


# --- per-shape case lists: (name, case) with case["kind"], shared by the CPU and GPU tests

EPSVIS_RUNS = [(0, 1e-5), (1, 1e-6), (2, 1e-5), (3, 1e-6)]   # (phase, eps): every kind of group
                                                             # comes first once, both eps


def _norm_cases(L, dtype, ref_fn, silu=False, means=(0.0,)):
    out = []
    for m in means:
        out.append((f"random mean {m:g}", norm_case(L, "random", dtype, mean=m, silu=silu,
                                                    ref_fn=ref_fn)))
    for phase, eps in EPSVIS_RUNS:
        out.append((f"epsvis phase {phase} eps {eps:g}",
                    norm_case(L, "epsvis", dtype, eps=eps, phase=phase, silu=silu, ref_fn=ref_fn)))
    if L.e % 2 == 0:
        out.append(("exact", norm_case(L, "exact", dtype, silu=silu, ref_fn=ref_fn)))
    for name, c in out:
        c["kind"] = name.split()[0]
    return out


def rms_cases(H: int, dtype):
    out = [("random", rms_case(H, "random", dtype)),
           ("epsvis eps 1e-05", rms_case(H, "epsvis", dtype, 1e-5)),
           ("epsvis eps 1e-06", rms_case(H, "epsvis", dtype, 1e-6)),
           ("exact", rms_case(H, "exact", dtype))]
    for name, c in out:
        c["kind"] = name.split()[0]
    return out


def ln_cases(rows: int, C: int, dtype):
    return _norm_cases(Rows(rows, C), dtype, layer_norm_ref, means=LN_MEANS)


def gn_nchw_cases(shape, dtype, silu: bool):
    B, C, H, W, G = shape
    fn = lambda x, g, b, eps: group_norm_nchw_ref(x, g, b, G, eps, silu)
    return _norm_cases(NCHW(B, C, H, W, G), dtype, fn, silu)


def gn_nhwc_cases(shape, dtype, silu: bool):
    N, HW, C, G = shape
    fn = lambda x, g, b, eps: group_norm_nhwc_ref(x, g, b, G, eps, silu)
    return _norm_cases(NHWC(N, HW, C, G), dtype, fn, silu)


def gn_two_cases(shape, dtype, silu: bool):
    """As gn_nhwc_cases on C = Cx + Cs; the test splits case["x"] at Cx."""
    N, HW, Cx, Cs, G = shape
    return gn_nhwc_cases((N, HW, Cx + Cs, G), dtype, silu)


COND_FAMILIES = ["layer_norm", "group_norm", "group_norm_nhwc", "two_source"]


def cond_layout(family: str, shape):
    """The conditioning sweep's layout of `family` for the NHWC shape (N, HW, C, G): the
    NCHW tensor of the same groups, or one LayerNorm row per group.  The channels-last
    kernels need at least 4 channels per group: below that (C = 64, G = 32) they run the
    shape with G = C / 8."""
    N, HW, C, G = shape
    if family == "layer_norm":
        return Rows(N * G, HW * (C // G))
    if family == "group_norm":
        return NCHW(N, C, *hw_shape(HW), G)
    if C // G < 4:
        G = C // 8
    return NHWC(N, HW, C, G)


def cond_case(family: str, shape, mean: float, std: float, dtype) -> dict:
    L = cond_layout(family, shape)
    G = L.G
    fn = {"layer_norm": layer_norm_ref,
          "group_norm": lambda x, g, b, eps: group_norm_nchw_ref(x, g, b, G, eps, False)}.get(
        family, lambda x, g, b, eps: group_norm_nhwc_ref(x, g, b, G, eps, False))
    c = norm_case(L, "random", dtype, mean=mean, std=std, ref_fn=fn, cap=False)
    c["G"] = G
    return c


def yardstick(family: str, c: dict, G: int = 1, silu: bool = False) -> torch.Tensor:
    """The f32 yardstick of a norm case, rounded to the case's dtype."""
    dt = c["gamma"].dtype
    if family == "layer_norm":
        y = layer_norm_ref(c["x"], c["gamma"], c["beta"], c["eps"], torch.float32)[0]
    elif family == "group_norm":
        y = group_norm_nchw_ref(c["x"], c["gamma"], c["beta"], G, c["eps"], silu, torch.float32)[0]
    else:
        y = group_norm_nhwc_yardstick(c["x"], c["gamma"], c["beta"], G, c["eps"], silu)
    return y.to(dt)


# ---------------------------------------------------------------------------
# Stable Diffusion step glue (references: _glue.py): the timestep embedding and the scheduler
# step as families of the rule.  The embedding's A = |angle| reaches 999, so its A term is
# above one output ulp at the slow frequencies by construction (the conditioning of sin / cos
# at a large f32 argument is the point of the term): no check_cap there.
# ---------------------------------------------------------------------------

MANT[torch.float32], EMIN[torch.float32] = 23, -126     # ulp16 / allowance of an f32 output

TE_FLIP_SHIFT = [(False, 0.0), (False, 1.0), (True, 0.0), (True, 1.0)]
SCHED_CPU_N = 1000


def timestep_embed_yardstick(t: float, B: int, dim: int, flip: bool, shift: float) -> torch.Tensor:
    """The embedding in plain f32 torch (f32 output; round it to the case's dtype)."""
    import _glue as G
    return G.timestep_embed_ref(t, B, dim, flip, shift, torch.float32)[0]


def sd_glue_cases(dt):
    """(family, name, case, f32 yardstick rounded to dt) of the two Stable Diffusion families,
    for test_ulp_cpu.py::test_yardstick_k."""
    import _glue as G
    for dim in G.TE_DIMS:
        for flip, shift in TE_FLIP_SHIFT:
            for t in G.TE_TABLE:
                ref, A = G.timestep_embed_ref(t, 1, dim, flip, shift)
                name = f"dim {dim} flip {flip} shift {shift} t {t}"
                y = timestep_embed_yardstick(t, 1, dim, flip, shift)
                yield "timestep_embed", name, dict(ref=ref, A=A), y.to(dt)
    for cfg in (False, True):
        x, pred, coef = G.sched_inputs(SCHED_CPU_N, cfg, dt, seed_of("sched", cfg))
        for step in range(coef.shape[0]):
            ref, A = G.sched_step_ref(x, pred, cfg, 7.5, coef, step, 12345)
            y = G.sched_step_ref(x, pred, cfg, 7.5, coef, step, 12345, torch.float32)[0]
            # x' is an f32 output: the yardstick is judged in f32
            yield "sched_step", f"cfg {cfg} step {step}", dict(ref=ref, A=A), y
