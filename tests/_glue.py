"""Host references of the glue and noise kernels: the Stable Diffusion scheduler's Philox
normal (sd_small.hip normal_from), the seeded weight fill (elementwise.hip normal_pair), the
timestep embedding and the scheduler step.  numpy / torch in float64, taking exactly the f32
intermediates the kernels form (the uniforms and the angle); everything after them is
evaluated in float64.  test_glue_ref_cpu.py checks this file; test_sd_glue_gpu.py compares
the kernels with it; _ulp.py registers the last two as families of its rule."""
from __future__ import annotations

import math

import numpy as np
import torch

from _philox import N_MAX, philox4x32_10

F32 = np.float32
TWO_M24 = F32(2.0 ** -24)
TWO_PI_F32 = F32(6.283185307179586)
MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15

# (seed, step, index, n1) with n1 = word 0 >> 8 at its smallest and largest, from a CPU scan
# of seed 12345 (indices below 2^16); and their reference normals
SD_EXTREMES = [(12345, 51, 40858, 0), (12345, 178, 1670, 0),
               (12345, 174, 15242, N_MAX), (12345, 209, 23178, N_MAX)]
SD_EXTREME_Z = [2.29024, -5.85882, 0.0, 0.0]
# (key, pair, r >> 40) of the fill at its smallest and largest u1, from a scan of key 1; and
# their reference (even, odd) normals
FILL_EXTREMES = [(1, 10860855, 0), (1, 15353537, N_MAX)]
FILL_EXTREME_Z = [(5.37242, -2.09957), (0.0, 0.0)]


# ---------------------------------------------------------------------------
# the scheduler's noise
# ---------------------------------------------------------------------------

def sd_words(index, step, seed):
    """(n1, n2) = words 0 and 1 of Philox(counter (index, step, 0, 0), key (seed low word,
    seed high word)), each shifted right by 8."""
    seed = int(seed) & MASK64
    w = philox4x32_10(index, step, 0, 0, seed & 0xFFFFFFFF, seed >> 32)
    return (w[0] >> np.uint64(8)).astype(np.int64), (w[1] >> np.uint64(8)).astype(np.int64)


def sd_uniforms(n1, n2):
    """(u1, u2) in float32 as the kernel forms them: u1 = (f32(n1) + 0.5f) * 2^-24 in (0, 1]
    (the add rounds to even above 2^23, so n1 = 2^24 - 1 gives 1.0), u2 = f32(n2) * 2^-24."""
    u1 = (np.asarray(n1).astype(F32) + F32(0.5)) * TWO_M24
    u2 = np.asarray(n2).astype(F32) * TWO_M24
    return u1.astype(F32), u2.astype(F32)


def _box_muller(u1, u2):
    """(radius, angle) in float64 from the f32 uniforms; the angle is the f32 product."""
    rad = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    ang = (TWO_PI_F32 * u2).astype(F32).astype(np.float64)
    return rad, ang


def sd_normal_ref(index, step, seed):
    """z = sqrt(-2 ln u1) cos(f32(2 pi u2)) in float64 for element `index` of step `step`."""
    rad, ang = _box_muller(*sd_uniforms(*sd_words(index, step, seed)))
    return rad * np.cos(ang)


def sd_normal_f32(index, step, seed):
    """The same in plain float32 (the yardstick of the rule, never the reference)."""
    u1, u2 = sd_uniforms(*sd_words(index, step, seed))
    return (np.sqrt(F32(-2.0) * np.log(u1)) * np.cos(TWO_PI_F32 * u2)).astype(F32)


# ---------------------------------------------------------------------------
# the seeded fill
# ---------------------------------------------------------------------------

def mix64(z):
    """The splitmix64 finaliser of elementwise.hip, on uint64 arrays (wrapping)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def fill_hash(key, pair):
    """r = mix64(key ^ mix64(pair + 0x9e3779b97f4a7c15)) of pair index `pair`."""
    pair = np.asarray(pair).astype(np.uint64)
    with np.errstate(over="ignore"):
        inner = mix64(pair + np.uint64(GOLDEN))
    return mix64(np.uint64(int(key) & MASK64) ^ inner)


def fill_uniforms(r):
    """u1 = f32((r >> 40) + 1) * 2^-24 in (0, 1], u2 = f32(r & 0xffffff) * 2^-24 in [0, 1)."""
    hi = (r >> np.uint64(40)).astype(np.int64) + 1
    lo = (r & np.uint64(0xFFFFFF)).astype(np.int64)
    return (hi.astype(F32) * TWO_M24).astype(F32), (lo.astype(F32) * TWO_M24).astype(F32)


def fill_normal_ref(key, i):
    """The standard normal of element i: pair i // 2; even i its radius * cos, odd i its
    radius * sin (float64)."""
    i = np.asarray(i).astype(np.int64)
    rad, ang = _box_muller(*fill_uniforms(fill_hash(key, i // 2)))
    return np.where(i % 2 == 0, rad * np.cos(ang), rad * np.sin(ang))


def fill_normal_f32(key, i):
    i = np.asarray(i).astype(np.int64)
    u1, u2 = fill_uniforms(fill_hash(key, i // 2))
    rad, ang = np.sqrt(F32(-2.0) * np.log(u1)), TWO_PI_F32 * u2
    return np.where(i % 2 == 0, rad * np.cos(ang), rad * np.sin(ang)).astype(F32)


# ---------------------------------------------------------------------------
# timestep embedding and scheduler step: float64 (ref, A) for the rule of _ulp.py
# ---------------------------------------------------------------------------

TE_DIMS = [6, 256, 320, 2560]
TE_TABLE = [999.0, 761.0, 500.5, 21.0, 1.0, 0.0]
LN_1E4 = math.log(10000.0)


def timestep_embed_ref(t: float, B: int, dim: int, flip: bool, shift: float, dt=torch.float64):
    """out [B, dim]: sin | cos (cos | sin when flip) of angle_k = t exp(-ln(1e4) k / (half -
    shift)), k < half = dim / 2.  The error-magnitude term is |angle|: an f32 evaluation
    carries the relative error of the exponential into the argument of sin / cos."""
    half = dim // 2
    k = torch.arange(half, dtype=dt)
    t = torch.tensor(float(np.float32(t)), dtype=dt)
    ang = torch.exp(-LN_1E4 * k / (half - float(np.float32(shift)))) * t
    s, c = torch.sin(ang), torch.cos(ang)
    row = torch.cat([c, s] if flip else [s, c])
    A = torch.cat([ang, ang]).abs()
    return row.expand(B, dim).contiguous(), A.expand(B, dim).contiguous().double()


def sched_step_ref(x, pred, cfg: bool, guidance: float, coef, step: int, seed: int,
                   dt=torch.float64, z=None):
    """x' = A x + B e + N z with (A, B, N, S) = coef[step] (f32), e = u + g (c - u) from pred =
    [u; c] under cfg (else pred), z the Philox normal of (element, step, seed): (x', A_term)
    with A_term = |A x| + |B| (|u| + g |c - u|) + |N z|.  z: that normal, if the caller has it."""
    n = x.numel()
    a, b, nz, _ = (float(v) for v in coef[step].double())
    g = float(np.float32(guidance))
    xx = x.to(dt)
    u = pred[:n].to(dt)
    if cfg:
        c = pred[n:2 * n].to(dt)
        e, emag = u + g * (c - u), u.abs() + abs(g) * (c - u).abs()
    else:
        e, emag = u, u.abs()
    idx = np.arange(n)
    if nz == 0.0:
        z = torch.zeros(n, dtype=dt)
    elif z is None:      # (a caller that keeps sd_normal_ref of this step passes it in)
        z = sd_normal_ref(idx, step, seed) if dt == torch.float64 else sd_normal_f32(idx, step, seed)
        z = torch.from_numpy(np.ascontiguousarray(z)).to(dt)
    y = a * xx + b * e + nz * z
    A = (a * xx).abs() + abs(b) * emag + (nz * z).abs()
    return y, A.double()


SCHED_COEF = [[0.9, -0.3, 0.0, 0.5], [1.0, -0.41, 0.73, 1.7], [1.1, 0.2, 0.25, 0.18215]]


def sched_inputs(n: int, cfg: bool, dtype, seed: int):
    """(x f32 [n], pred 16-bit [(2) n], coef f32 [3, 4]) of one scheduler-step case (CPU)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g, dtype=torch.float64).mul(3.0).float()
    pred = torch.randn((2 if cfg else 1) * n, generator=g, dtype=torch.float64).to(dtype)
    return x, pred, torch.tensor(SCHED_COEF, dtype=torch.float32)
