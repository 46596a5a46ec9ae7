"""Shared helpers of the FP8 (e4m3) KV-cache tests.

The oracle of the format is ``cake_amd.ops.reference.quant_kv_fp8`` / ``dequant_kv_fp8``;
``nearest_code_f64`` is the independent check of that oracle (a nearest-code search in
float64 over the 254 finite codes, ties to the even code)."""
from __future__ import annotations

import torch

import _exact as X
from cake_amd.ops import reference as R

NAN_CODES = (0x7F, 0xFF)
FINITE_CODES = torch.tensor([c for c in range(256) if c not in NAN_CODES], dtype=torch.uint8)
DTYPES = [torch.bfloat16, torch.float16]


def code_values_f64() -> torch.Tensor:
    """The value of each of the 256 e4m3fn codes from the bit fields (NaN at 0x7F / 0xFF)."""
    c = torch.arange(256)
    sign = torch.where(c >= 128, -1.0, 1.0).double()
    e, m = (c >> 3) & 15, (c & 7).double()
    v = torch.where(e == 0, m / 8 * 2.0 ** -6, (1 + m / 8) * torch.exp2(e.double() - 7))
    v = sign * v
    v[list(NAN_CODES)] = float("nan")
    return v


def nearest_code_f64(x: torch.Tensor) -> torch.Tensor:
    """uint8 codes of x (any shape, finite) by exhaustive search: the finite code nearest to
    clamp(x, -448, 448) in float64, ties to the code with an even low bit, the sign bit that
    of x (so -0.0 and small negatives give 0x80)."""
    vals = code_values_f64()
    mag = vals[:127]                                   # codes 0x00..0x7E: 0 .. 448, ascending
    a = x.double().abs().clamp(max=448.0).reshape(-1)
    d = (a[:, None] - mag[None, :]).abs()              # exact in f64 (f32 inputs, 4-bit codes)
    best = d.min(dim=1).values
    cand = d == best[:, None]                          # one code, or two on a tie
    idx = torch.arange(127)
    even = cand & (idx % 2 == 0)[None, :]
    pick = torch.where(cand.sum(1) > 1, even.float().argmax(1), cand.float().argmax(1))
    code = pick | (torch.signbit(x.reshape(-1)).long() << 7)
    return code.to(torch.uint8).reshape(x.shape)


def block_code_codes(bc: X.BlockCode):
    """(k8, v8) uint8 caches of a block-code cache: +-1 K, one-hot V, and the NaN dead V rows
    as the NaN code 0x7F.  Asserts that the conversion loses nothing."""
    dev = bc.k.device
    k, v = bc.k.cpu(), bc.v.cpu().float()      # the oracle runs on the CPU
    live = torch.arange(bc.keys) < bc.live
    assert bool(torch.isnan(v[:, ~live]).all()) and bool(torch.isfinite(v[:, live]).all())
    k8 = R.quant_kv_fp8(k)
    v8 = R.quant_kv_fp8(torch.nan_to_num(v, nan=0.0))
    v8[:, ~live] = 0x7F
    assert torch.equal(R.dequant_kv_fp8(k8).to(bc.dtype), k)
    back = R.dequant_kv_fp8(v8)
    assert torch.equal(back[:, live].to(bc.dtype), v[:, live].to(bc.dtype))
    assert bool(torch.isnan(back[:, ~live]).all())
    k8, v8 = k8.to(dev), v8.to(dev)
    return k8, v8


def gaussian_codes(nkv: int, S: int, hd: int, seed: int):
    """(k8, v8) uint8 [nkv, S, hd] on the CPU: K ~ N(0, 1), V ~ 4 N(0, 1) quantised with the
    oracle — no saturation, subnormal codes present."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randn(nkv, S, hd, generator=g)
    v = torch.randn(nkv, S, hd, generator=g) * 4
    assert float(v.abs().max()) < 448 and float(k.abs().max()) < 448
    k8, v8 = R.quant_kv_fp8(k), R.quant_kv_fp8(v)
    assert int(((v8 & 0x78) == 0).sum()) > 0  # zero exponent field: subnormal codes occur
    return k8, v8


def widen_codes(codes: torch.Tensor, dt) -> torch.Tensor:
    """dequant(codes).to(dt) through a 256-entry table (NaN for the NaN codes), on the codes'
    device."""
    lut = R.dequant_kv_fp8(torch.arange(256, dtype=torch.uint8)).to(dt).to(codes.device)
    return lut[codes.long()]


def with_dead_rows(codes: torch.Tensor, Tk: int) -> torch.Tensor:
    """A copy of a [nkv, S, hd] code cache with rows >= Tk set to the NaN code 0x7F."""
    out = codes.clone()
    out[:, Tk:] = 0x7F
    return out


def rope_reference_f32(q, k, inv_freq, pos0: int):
    """The prefill writer's f32 rotation of 16-bit q [T, nh, hd] / k [T, nkv, hd] with the
    kernel's formula: angle = f32(pos) * inv_freq, out = (a c - b s, a s + b c) in f32."""
    T = k.shape[0]
    pos = torch.arange(pos0, pos0 + T, dtype=torch.float32, device=k.device)
    ang = pos[:, None] * inv_freq[None, :].float()
    c, s = torch.cos(ang)[:, None, :], torch.sin(ang)[:, None, :]

    def rot(x):
        xf = x.float()
        h = xf.shape[-1] // 2
        a, b = xf[..., :h], xf[..., h:]
        return torch.cat([a * c - b * s, a * s + b * c], dim=-1)
    return rot(q), rot(k)


def near_boundary(x: torch.Tensor, ulps: int = 1) -> torch.Tensor:
    """Elements of f32 x within `ulps` f32 ulps of an e4m3 rounding boundary (the midpoint of
    two neighbouring codes): moving x by that much changes its code."""
    x = x.float()
    up = x
    dn = x
    for _ in range(ulps):
        up = torch.nextafter(up, torch.full_like(x, float("inf")))
        dn = torch.nextafter(dn, torch.full_like(x, float("-inf")))
    return (R.quant_kv_fp8(up) != R.quant_kv_fp8(dn))


def code_steps(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Distance of two code tensors in code steps along the ordered value line."""
    def line(c):
        c = c.to(torch.int32)
        mag = c & 0x7F
        return torch.where(c >= 128, -mag, mag)
    return (line(a) - line(b)).abs()


__all__ = ["FINITE_CODES", "NAN_CODES", "DTYPES", "code_values_f64", "nearest_code_f64",
           "block_code_codes", "gaussian_codes", "widen_codes", "with_dead_rows",
           "rope_reference_f32", "near_boundary", "code_steps"]
