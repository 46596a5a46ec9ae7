"""Shared helpers of the sequence-scoring tests (score.hip, cake_engine_score).

* ``lse_ref``: float64 log-sum-exp, gathered target logit and lowest-index argmax of a logit
  matrix: the yardstick of the kernel and of the engine.
* ``ref_all_logits``: the plain-torch forward of ``tests/_w8a8.py::ref_prefill_logits`` kept
  for every row, with the final norm output rounded to the model dtype as the scoring head's
  16-bit GEMM operand is.
* kernel cases: ``family_logits`` (the input families), ``chunks_of`` (the chunkings) and
  ``lse_bound`` (the error rule).
* ``windows``: the window rule of ``--score-file`` restated independently of the package.
"""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import torch

from _w8a8 import plain_projection
from cake_amd.ops import reference as R
from cake_amd.utils.safetensors_io import SafeTensors

EPS24 = 2.0 ** -24
LSE_K = 128.0   # |lse - ref64| <= 2^-24 (|ref64| + K)

TS = [1, 3, 65]
VS = [1, 255, 1000, 2052, 8705]
CHUNKINGS = ["one", "c256", "c513", "strided"]
FAMILIES = ["normal", "x30", "offset", "dominant"]


def lse_ref(x64: np.ndarray, target: np.ndarray):
    """(lse float64 [T], target logit float64 [T] (NaN where target < 0), argmax int64 [T] with
    the lowest index at ties, max float64 [T]) of float64 logits [T, V].  A row of -inf
    gives lse -inf and argmax 0."""
    x = np.asarray(x64, dtype=np.float64)
    T = x.shape[0]
    m = x.max(axis=1)
    safe = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        lse = safe + np.log(np.exp(x - safe[:, None]).sum(axis=1))
    top = x.argmax(axis=1)   # numpy returns the first maximum
    tgt = np.full(T, np.nan)
    has = np.asarray(target) >= 0
    tgt[has] = x[np.arange(T)[has], np.asarray(target)[has]]
    return lse, tgt, top, m


def lse_bound(ref: np.ndarray) -> np.ndarray:
    return EPS24 * (np.abs(ref) + LSE_K)


def family_logits(family: str, T: int, V: int, seed: int = 0) -> np.ndarray:
    """float32 [T, V].  normal: N(0, 1); x30: the same times 30; offset: N(0, 1) plus a per-row
    offset of +-1e4 (the max subtraction); dominant: one value per row 50 above the rest."""
    g = np.random.default_rng(1000 * seed + 7 * T + V + FAMILIES.index(family))
    x = g.standard_normal((T, V)).astype(np.float32)
    if family == "x30":
        x = (x * np.float32(30)).astype(np.float32)
    elif family == "offset":
        off = np.where(np.arange(T) % 2 == 0, 1e4, -1e4).astype(np.float32)
        x = (x + off[:, None]).astype(np.float32)
    elif family == "dominant":
        col = g.integers(0, V, T)
        x[np.arange(T), col] = (x.max(axis=1) + np.float32(50)).astype(np.float32)
    elif family != "normal":
        raise ValueError(family)
    return x


def random_targets(T: int, V: int, seed: int = 0) -> np.ndarray:
    g = np.random.default_rng(77 + seed + T + V)
    t = g.integers(0, V, T).astype(np.int32)
    t[T - 1] = -1 if T > 1 else t[T - 1]
    return t


def chunks_of(V: int, chunking: str):
    """[(v0, Vc)] of a chunking, or None where the chunk exceeds V."""
    if chunking in ("one", "strided"):
        return [(0, V)]
    w = {"c256": 256, "c513": 513}[chunking]
    if w > V:
        return None
    return [(v0, min(w, V - v0)) for v0 in range(0, V, w)]


def windows(n_tokens: int, S: int) -> list[tuple[int, int]]:
    """[start, end) of the consecutive windows of S tokens; a last window of one token is
    dropped (it has no scored token)."""
    out = []
    for a in range(0, n_tokens, S):
        b = min(a + S, n_tokens)
        if b - a >= 2:
            out.append((a, b))
    return out


def ref_all_logits(model_dir, tokens: list[int], dtype=torch.bfloat16,
                   projection=plain_projection) -> torch.Tensor:
    """f32 logits [T, V] of every position: the forward of ``_w8a8.ref_prefill_logits`` (the
    engine's 16-bit rounding points, f32 residual stream), with the final norm output rounded
    to ``dtype`` before the float64 head product, as the scoring head's GEMM takes it."""
    d = Path(model_dir)
    cfg = json.loads((d / "config.json").read_text())
    st = SafeTensors(d / "model.safetensors")
    names = set(st.keys())

    def W(name):
        return st.get(name).to(dtype)

    H, L = cfg["hidden_size"], cfg["num_hidden_layers"]
    nh = cfg["num_attention_heads"]
    nkv = cfg.get("num_key_value_heads") or nh
    hd, eps = H // nh, float(cfg.get("rms_norm_eps", 1e-5))
    inv_f = R.inv_freq(hd, float(cfg.get("rope_theta", 10000.0)), cfg.get("rope_scaling"))
    T = len(tokens)
    pos = torch.arange(T)
    h = W("model.embed_tokens.weight")[torch.tensor(tokens)].float()
    for l in range(L):
        p = f"model.layers.{l}."
        x = R.rms_norm(h, W(p + "input_layernorm.weight"), eps).to(dtype)
        wqkv = torch.cat([W(p + f"self_attn.{n}_proj.weight") for n in "qkv"])
        qkv = projection(x, wqkv, "store").to(dtype)
        q = qkv[:, :nh * hd].view(T, nh, hd)
        k = qkv[:, nh * hd:(nh + nkv) * hd].view(T, nkv, hd)
        v = qkv[:, (nh + nkv) * hd:].view(T, nkv, hd)
        q, k = R.rope(q, pos, inv_f).to(dtype), R.rope(k, pos, inv_f).to(dtype)
        att = R.attention(q, k, v, 0).to(dtype).reshape(T, nh * hd)
        h = h + projection(att, W(p + "self_attn.o_proj.weight"), "resid32").float()
        x = R.rms_norm(h, W(p + "post_attention_layernorm.weight"), eps).to(dtype)
        wgu = torch.cat([W(p + "mlp.gate_proj.weight"), W(p + "mlp.up_proj.weight")])
        act = projection(x, wgu, "swiglu").to(dtype)
        h = h + projection(act, W(p + "mlp.down_proj.weight"), "resid32").float()
    x = R.rms_norm(h, W("model.norm.weight"), eps).to(dtype)
    tied = bool(cfg.get("tie_word_embeddings")) or "lm_head.weight" not in names
    head = W("model.embed_tokens.weight") if tied else W("lm_head.weight")
    return (x.double() @ head.double().T).float()
