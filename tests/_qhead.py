"""Shared helpers of the quantised lm_head tests (``head="fp8" | "mxfp4"``).

The head's two formats are the projections' (tests/_fp8.py, tests/_mxfp4.py): their grid
matrices are lossless under the engine's quantisation, so on a checkpoint whose head is
one the quantised-head engine and the 16-bit engine hold the same mathematical head and
the 16-bit engine is the oracle.
"""
from __future__ import annotations

import dataclasses
from pathlib import Path

import torch

import _fp8
import _mxfp4
from _fp8 import tiny_cfg
from cake_amd.ops import reference as R
from cake_amd.utils.safetensors_io import SafeTensors, save_file
from cake_amd.utils.synth import write_checkpoint

FORMATS = ("fp8", "mxfp4")
HEAD = "lm_head.weight"
EMBED = "model.embed_tokens.weight"
# grid exponents for rows of unit scale (an embedding table, N(0, 1) in the synthetic
# checkpoints): uniform e4m3 codes have an rms near 120, uniform e2m1 codes near 3
UNIT_EXPONENTS = {"fp8": (-8, -7, -6), "mxfp4": (-2, -1, 0)}


def tied_cfg():
    """The tiny architecture with tied embeddings."""
    return dataclasses.replace(tiny_cfg(), tie_word_embeddings=True)


def grid_matrix(fmt: str, N: int, K: int, gen: torch.Generator, exponents=None):
    """(w bf16, codes, scales) of the format's grid matrix (see _fp8 / _mxfp4)."""
    mod = _fp8 if fmt == "fp8" else _mxfp4
    if exponents is None:
        return mod.grid_matrix(N, K, gen)
    return mod.grid_matrix(N, K, gen, exponents)


def quant(fmt: str, w: torch.Tensor):
    """Oracle (codes, scales) of a matrix."""
    return R.quant_rows_fp8(w) if fmt == "fp8" else R.quant_rows_mxfp4(w)


def dequant(fmt: str, codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """Oracle f32 matrix of (codes, scales)."""
    return R.dequant_rows_fp8(codes, scales) if fmt == "fp8" else R.dequant_rows_mxfp4(codes, scales)


def round_trip(fmt: str, w: torch.Tensor) -> torch.Tensor:
    """dequant(quant(w)) in w's dtype (exact: a product of an 8- or 4-bit value and a scale
    is rounded to the 16-bit dtype only where the scale is no power of two, as the engine's
    dequantise kernels do)."""
    return dequant(fmt, *quant(fmt, w)).to(w.dtype)


def rewrite_head(src, dst, head=None, embed=None, drop_head: bool = False) -> Path:
    """Copy the single-file checkpoint ``src`` to ``dst`` with ``lm_head.weight`` replaced by
    ``head`` and ``model.embed_tokens.weight`` by ``embed`` (None: kept); ``drop_head``
    leaves ``lm_head.weight`` out (a tied checkpoint)."""
    src, dst = Path(src), Path(dst)
    dst.mkdir(parents=True, exist_ok=True)
    for f in src.iterdir():
        if f.name != "model.safetensors":
            (dst / f.name).write_bytes(f.read_bytes())
    st = SafeTensors(src / "model.safetensors")
    out = {k: st.get(k).clone() for k in st.keys()}
    if head is not None:
        assert HEAD in out and out[HEAD].shape == head.shape
        out[HEAD] = head.to(out[HEAD].dtype).contiguous()
    if embed is not None:
        assert out[EMBED].shape == embed.shape
        out[EMBED] = embed.to(out[EMBED].dtype).contiguous()
    if drop_head:
        out.pop(HEAD, None)
    save_file(out, dst / "model.safetensors", {"format": "pt"})
    return dst


def head_tensor(model_dir) -> torch.Tensor:
    return SafeTensors(Path(model_dir) / "model.safetensors").get(HEAD)


def write_base_checkpoint(out_dir, seed: int = 3, tied: bool = False) -> Path:
    return write_checkpoint(Path(out_dir), tied_cfg() if tied else tiny_cfg(), torch.bfloat16,
                            seed=seed, single_file=True)


def write_grid_head_checkpoint(out_dir, fmt: str, seed: int = 3, base=None) -> Path:
    """The tiny bf16 checkpoint (or ``base``) with the head replaced by a grid matrix of
    ``fmt``."""
    out_dir = Path(out_dir)
    if base is None:
        base = write_base_checkpoint(out_dir / "base", seed)
    cfg = tiny_cfg()
    gen = torch.Generator().manual_seed(3000 + seed)
    w = grid_matrix(fmt, cfg.vocab_size, cfg.hidden_size, gen)[0]
    return rewrite_head(base, out_dir / f"grid_head_{fmt}", head=w)


def write_tied_grid_checkpoint(out_dir, fmt: str, seed: int = 3) -> Path:
    """The tied tiny checkpoint with the embedding (= the head) a grid matrix of ``fmt`` at
    unit scale."""
    out_dir = Path(out_dir)
    base = write_base_checkpoint(out_dir / "tied_base", seed, tied=True)
    cfg = tied_cfg()
    gen = torch.Generator().manual_seed(4000 + seed)
    w = grid_matrix(fmt, cfg.vocab_size, cfg.hidden_size, gen, UNIT_EXPONENTS[fmt])[0]
    return rewrite_head(base, out_dir / f"tied_grid_{fmt}", embed=w, drop_head=True)


def head_bytes(cfg, head: str) -> int:
    """Bytes of a quantised head: V H + 4 V (fp8) or V H / 2 + V H / 32 (mxfp4)."""
    V, H = cfg.vocab_size, cfg.hidden_size
    return {"fp8": V * H + 4 * V, "mxfp4": V * H // 2 + V * H // 32}[head]


def expected_weight_bytes(cfg, weights: str, head: str) -> int:
    """_mxfp4.expected_weight_bytes with the head's format: a quantised head replaces the
    16-bit one when untied and is an extra allocation when tied (the gather keeps the
    16-bit table)."""
    base = _mxfp4.expected_weight_bytes(cfg, weights)
    if head == "model":
        return base
    tied = bool(getattr(cfg, "tie_word_embeddings", False))
    return base - (0 if tied else 2 * cfg.vocab_size * cfg.hidden_size) + head_bytes(cfg, head)


__all__ = ["FORMATS", "tiny_cfg", "tied_cfg", "grid_matrix", "quant", "dequant", "round_trip",
           "rewrite_head", "head_tensor", "write_base_checkpoint", "write_grid_head_checkpoint",
           "write_tied_grid_checkpoint", "head_bytes", "expected_weight_bytes"]
