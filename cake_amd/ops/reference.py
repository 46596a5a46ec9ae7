"""Plain-PyTorch implementation of the Llama-3 math.

Used (a) as the CPU / f32 execution backend — the reference's ``--cpu`` mode —
and (b) as the numerical oracle for every HIP kernel test.  It mirrors:

* RMSNorm           cake-core/src/models/llama3/transformer.rs:60,68 (candle RmsNorm)
* RoPE (half-split) cake-core/src/models/llama3/attention.rs:25-35, cache.rs:23-61
* GQA attention     cake-core/src/models/llama3/attention.rs:38-123 (f32 softmax)
* SwiGLU            cake-core/src/models/llama3/mlp.rs:15-18
* repeat penalty    cake-core/src/models/llama3/llama.rs:311-320

All math is f32 internally; inputs/outputs keep the caller's dtype except the
residual stream, which is f32.
"""
from __future__ import annotations

import math

import torch


def rms_norm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    xf = x.float()
    r = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return xf * r * w.float()


def inv_freq(head_dim: int, theta: float, rope_scaling: dict | None = None) -> torch.Tensor:
    """θ_i = 1/θ^(2i/d) (cache.rs:29-32), with optional Llama-3.1 'llama3' scaling."""
    f = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float64) / head_dim))
    if rope_scaling and rope_scaling.get("rope_type", rope_scaling.get("type")) == "llama3":
        factor = rope_scaling["factor"]
        lo = rope_scaling.get("low_freq_factor", 1.0)
        hi = rope_scaling.get("high_freq_factor", 4.0)
        old = rope_scaling.get("original_max_position_embeddings", 8192)
        lo_wl, hi_wl = old / lo, old / hi
        wl = 2 * math.pi / f
        out = torch.where(wl > lo_wl, f / factor, f)
        smooth = (old / wl - lo) / (hi - lo)
        mid = (1 - smooth) * out / factor + smooth * out
        is_mid = (wl >= hi_wl) & (wl <= lo_wl)
        f = torch.where(is_mid, mid, out)
    return f.float()


def rope(x: torch.Tensor, positions: torch.Tensor, inv_f: torch.Tensor) -> torch.Tensor:
    """x [T, nheads, hd] -> rotated (f32). Non-interleaved: pairs (i, i + hd/2)."""
    ang = positions.float()[:, None] * inv_f.to(x.device)[None, :]  # [T, hd/2]
    c, s = torch.cos(ang)[:, None, :], torch.sin(ang)[:, None, :]
    xf = x.float()
    h = xf.shape[-1] // 2
    a, b = xf[..., :h], xf[..., h:]
    return torch.cat([a * c - b * s, a * s + b * c], dim=-1)


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, pos0: int) -> torch.Tensor:
    """q [T, nh, hd]; k, v [Tk, nkv, hd] (Tk = pos0 + T).  Causal with offset. f32 out."""
    T, nh, hd = q.shape
    Tk, nkv, _ = k.shape
    rep = nh // nkv
    qf = q.float().transpose(0, 1)                                      # [nh, T, hd]
    kf = k.float().transpose(0, 1).repeat_interleave(rep, dim=0)        # [nh, Tk, hd]
    vf = v.float().transpose(0, 1).repeat_interleave(rep, dim=0)
    att = (qf @ kf.transpose(1, 2)) / math.sqrt(hd)                     # [nh, T, Tk]
    if T > 1 or pos0 + T < Tk:
        qi = torch.arange(T, device=q.device)[:, None] + pos0
        kj = torch.arange(Tk, device=q.device)[None, :]
        att = att.masked_fill(kj > qi, float("-inf"))
    att = torch.softmax(att, dim=-1)
    return (att @ vf).transpose(0, 1)                                   # [T, nh, hd]


def silu_mul(g: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    gf = g.float()
    return gf * torch.sigmoid(gf) * u.float()


FP8_E4M3_MAX = 448.0


def quant_rows_fp8(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """FP8 weight-only storage of a [N, K] matrix (the oracle of quant_fp8.hip).

    scale[n] = amax_n / 448 in f32 (1 for an all-zero row); codes are OCP e4m3fn,
    ``rne(clamp(float(w) / scale[n], -448, 448))`` — clamped before the conversion, so the
    NaN code never appears.  Returns (codes uint8 [N, K], scale f32 [N])."""
    wf = w.float()
    amax = wf.abs().amax(dim=1)
    scale = torch.where(amax == 0, torch.ones_like(amax), amax / FP8_E4M3_MAX)
    v = (wf / scale[:, None]).clamp(-FP8_E4M3_MAX, FP8_E4M3_MAX)
    return v.to(torch.float8_e4m3fn).view(torch.uint8), scale


def dequant_rows_fp8(codes: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """f32 [N, K] = scale[n] * fp8(codes[n, k])."""
    return codes.view(torch.float8_e4m3fn).float() * scale.float()[:, None]


def gemm_w8a8_ref(a8: torch.Tensor, sa: torch.Tensor, w8: torch.Tensor, sw: torch.Tensor,
                  epi: str = "store") -> torch.Tensor:
    """float64 oracle of the FP8 x FP8 prefill GEMM (gemm_w8a8.hip), before the output's own
    rounding: ``(sa[m] * sw[n]) * sum_k fp8(a8[m, k]) * fp8(w8[n, k])`` with the codes' exact
    values.  ``store`` / ``resid32``: the [M, N] product (resid32 adds it to the caller's
    residual).  ``swiglu``: w8 / sw hold 2 N rows, gate rows first; silu(gate) * up."""
    a = a8.view(torch.float8_e4m3fn).double()
    w = w8.view(torch.float8_e4m3fn).double()
    y = (a @ w.T) * (sa.double()[:, None] * sw.double()[None, :])
    if epi == "swiglu":
        n = y.shape[1] // 2
        g, u = y[:, :n], y[:, n:]
        return g * torch.sigmoid(g) * u
    if epi not in ("store", "resid32"):
        raise ValueError(f"gemm_w8a8_ref: unknown epilogue {epi!r}")
    return y


MXFP4_BLOCK = 32
# e2m1 magnitudes by code (s e e m: the sign is bit 3) and the midpoints between them
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
E2M1_MIDPOINTS = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)


def quant_rows_mxfp4(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """OCP MXFP4 weight-only storage of a [N, K] matrix, K % 32 == 0 (the oracle of
    quant_mxfp4.hip): e2m1 elements with one e8m0 power-of-two scale per 32 consecutive k.

    Scale: ``e = clamp(floor(log2(amax_block)) - 2, -126, 127)`` stored as the byte
    ``e + 127`` (127 for an all-zero block; never 0xFF).  Element: ``v = w / 2^e`` (exact),
    ``|v|`` saturated to 6 and rounded to the nearest of {0, .5, 1, 1.5, 2, 3, 4, 6}, ties
    to the even code; bit 3 is the sign bit of ``w`` (a small negative may become -0).
    Element 2i sits in the low nibble of byte i, 2i+1 in the high nibble.
    Returns (codes uint8 [N, K/2], e8 uint8 [N, K/32])."""
    N, K = w.shape
    if K < MXFP4_BLOCK or K % MXFP4_BLOCK:
        raise ValueError(f"mxfp4 rows need K % {MXFP4_BLOCK} == 0, got {K}")
    wf = w.float().reshape(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
    amax = wf.abs().amax(dim=2)
    fl = torch.frexp(amax)[1] - 1  # floor(log2(amax)), exact (any value where amax == 0)
    e = torch.where(amax == 0, torch.zeros_like(fl), (fl - 2).clamp(-126, 127))
    a = torch.ldexp(wf.abs(), -e[:, :, None])
    mid = torch.tensor(E2M1_MIDPOINTS, dtype=torch.float32, device=w.device)
    mag = torch.bucketize(a, mid)  # midpoints strictly below |v|: a tie stays on the lower code
    # ... and moves up where the upper code is the even one
    mag = mag + ((a == 0.75) | (a == 1.75) | (a == 3.5)).to(mag.dtype)
    code = (mag | (torch.signbit(wf).to(mag.dtype) << 3)).reshape(N, K // 2, 2)
    packed = (code[:, :, 0] | (code[:, :, 1] << 4)).to(torch.uint8)
    return packed, (e + 127).to(torch.uint8)


def dequant_rows_mxfp4(codes: torch.Tensor, e8: torch.Tensor) -> torch.Tensor:
    """f32 [N, K] = 2^(e8[n, k / 32] - 127) * e2m1(code[n, k])."""
    N, K2 = codes.shape
    c = codes.to(torch.int64)
    nib = torch.stack((c & 15, c >> 4), dim=2).reshape(N, 2 * K2)
    lut = torch.tensor(E2M1_VALUES + tuple(-v for v in E2M1_VALUES), dtype=torch.float32,
                       device=codes.device)
    e = e8.to(torch.int32) - 127
    return torch.ldexp(lut[nib].reshape(N, -1, MXFP4_BLOCK), e[:, :, None]).reshape(N, 2 * K2)


def apply_repeat_penalty(logits: torch.Tensor, penalty: float, context: list[int]) -> torch.Tensor:
    """candle_transformers::utils::apply_repeat_penalty semantics (unique tokens)."""
    out = logits.clone()
    for t in sorted(set(int(x) for x in context)):
        if 0 <= t < out.shape[-1]:
            s = out[..., t]
            out[..., t] = torch.where(s >= 0, s / penalty, s * penalty)
    return out


def quant_kv_fp8(x: torch.Tensor) -> torch.Tensor:
    """FP8 KV-cache storage (the oracle of every kv_fmt = 1 writer): one OCP e4m3fn code per
    element and no scale, ``code = rne_e4m3(clamp(float(x), -448, 448))`` — clamped before the
    conversion, so a finite input never gives the NaN code.  Returns uint8, x's shape."""
    return x.float().clamp(-FP8_E4M3_MAX, FP8_E4M3_MAX).to(torch.float8_e4m3fn).view(torch.uint8)


def dequant_kv_fp8(codes: torch.Tensor) -> torch.Tensor:
    """f32 = fp8(code); every value is exact in bf16 and in f16."""
    return codes.view(torch.float8_e4m3fn).float()


LOGPROB_MAX_TOP = 20
LOGPROB_REC_WORDS = 48  # int32 words of one device record (192 bytes)


def logprob_topk_ref(x_f32: torch.Tensor, tok: int, k: int) -> dict:
    """Oracle of the generated-token log-prob record (logprob.hip) for one row.

    ``x_f32`` is the f32 row that token selection sees: the logits after the repeat penalty,
    before temperature, top-k / top-p and the draw.  Returns

    * ``logit`` = ``x[tok]`` (float32, bit for bit), ``lse`` = ``log sum_v exp(x[v])`` in
      float64 (``-inf`` if every logit is ``-inf``), ``logprob`` = ``float64(logit) - lse``
      (``-inf`` when the logit is ``-inf``);
    * ``top_ids`` (int32 [k]) / ``top_logits`` (float32 [k]): the ``k`` largest logits in
      descending order, the lower id first at ties (a stable sort by ``(-x, id)``); entries
      past ``min(k, V)`` are id ``-1``, logit ``-inf``; ``top_logprobs`` float64 likewise.

    NaN logits are outside the contract."""
    if not 0 <= k <= LOGPROB_MAX_TOP:
        raise ValueError(f"k must be in [0, {LOGPROB_MAX_TOP}], got {k}")
    x = x_f32.detach().reshape(-1).to(torch.float32).cpu()
    V = x.numel()
    x64 = x.double()
    m = x64.max()
    if torch.isinf(m) and m < 0:
        lse = float("-inf")
    else:
        lse = float(m + torch.log(torch.exp(x64 - m).sum()))
    # descending stable sort of x: equal values keep their id order
    order = torch.sort(x, descending=True, stable=True).indices[:min(k, V)]
    top_ids = torch.full((k,), -1, dtype=torch.int32)
    top_logits = torch.full((k,), float("-inf"), dtype=torch.float32)
    top_ids[:order.numel()] = order.to(torch.int32)
    top_logits[:order.numel()] = x[order]

    def lp(v: torch.Tensor) -> torch.Tensor:
        v64 = v.double()
        return torch.where(torch.isinf(v64) & (v64 < 0), v64, v64 - lse)

    logit = x[int(tok)].clone()
    return {"id": int(tok), "logit": logit, "lse": lse, "logprob": float(lp(logit)),
            "top_ids": top_ids, "top_logits": top_logits, "top_logprobs": lp(top_logits)}


LOGIT_BIAS_MAX = 300  # OpenAI's limit on logit_bias entries


def ordered_key(x) -> "np.ndarray":
    """The order-preserving u32 key of sampling.hip for float32 values (numpy uint32)."""
    import numpy as np
    u = np.asarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def min_p_offset(temperature: float, min_p: float) -> float:
    """``d = float32(T * ln(min_p))``: formed in float64 and rounded once."""
    import numpy as np
    return float(np.float32(float(temperature) * math.log(float(min_p))))


def logit_controls_ref(x, generated, presence: float = 0.0, frequency: float = 0.0, bias=None,
                       min_p: float | None = None, temperature: float = 0.0):
    """Oracle of logit_controls.hip for one row: ``(x_adj, cut_key | None)``.

    ``x`` is the f32 row after the repeat penalty; ``generated`` the tokens this generation has
    produced so far (the prompt is not counted); ``bias`` a mapping or a sequence of pairs
    ``id -> b`` with distinct ids.  In numpy float32, every operation rounded on its own:

    1. ``c[v]`` = occurrences of v in ``generated``; for ``c[v] > 0``:
       ``x[v] = x[v] - (presence + frequency * float32(c[v]))`` (skipped when both are zero);
    2. ``x[id] = x[id] + b`` for every bias entry, after the penalty;
    3. with ``temperature > 0`` and ``0 < min_p <= 1``: ``cut = max(x) + d``,
       ``d = float32(T ln min_p)``, and the sampling set is
       ``ordered(x[v]) >= cut_key = min(ordered(cut), ordered(max))`` (the second term only
       matters for a maximum of -0.0 with d = 0, whose sum is +0.0).  Otherwise ``None``.

    Returns ``x_adj`` as a float32 CPU tensor and the key as an int.  NaN logits are outside the
    contract."""
    import numpy as np
    if isinstance(x, torch.Tensor):
        x = x.detach().reshape(-1).to(torch.float32).cpu().numpy()
    x = np.array(x, dtype=np.float32).reshape(-1)
    V = x.size
    pres, freq = np.float32(presence), np.float32(frequency)
    if pres != 0 or freq != 0:
        c = np.bincount(np.asarray([t for t in generated if 0 <= int(t) < V], dtype=np.int64),
                        minlength=V)
        hit = c > 0
        pen = pres + freq * c[hit].astype(np.float32)  # float32 product, then float32 sum
        x[hit] = x[hit] - pen.astype(np.float32)
    items = list(bias.items()) if hasattr(bias, "items") else list(bias or [])
    if len(items) > LOGIT_BIAS_MAX or len({int(i) for i, _ in items}) != len(items):
        raise ValueError("bias: at most 300 entries with distinct ids")
    for i, b in items:
        x[int(i)] = x[int(i)] + np.float32(b)
    cut_key = None
    if temperature > 0 and min_p is not None and 0 < min_p <= 1:
        keys = ordered_key(x)
        kmax = keys.max()
        xmax = x[int(keys.argmax())]
        cut = np.float32(xmax + np.float32(min_p_offset(temperature, min_p)))
        cut_key = int(min(int(ordered_key(cut)), int(kmax)))
    return torch.from_numpy(x), cut_key
