"""Shared helpers of the MXFP4 weight-only tests (modelled on tests/_fp8.py).

``write_grid_checkpoint`` builds a checkpoint that is lossless under the engine's
quantisation: every 32-element block of every projection row is ``2^e * e2m1(code)`` with a
magnitude-4 or magnitude-6 code in it, so the block exponent comes out as exactly ``e`` and
quantise -> dequantise reproduces the bf16 weights bit for bit.  On it the mxfp4 engine and
the 16-bit engine hold the same mathematical weights: the 16-bit engine is the oracle.
"""
from __future__ import annotations

from pathlib import Path

import torch

from _fp8 import is_projection, projection_tensors, rewrite_projections, tiny_cfg
from cake_amd.ops import reference as R
from cake_amd.utils.synth import write_checkpoint

BLOCK = 32
GRID_EXPONENTS = (-8, -7, -6)  # weight rms ~0.02, as the synthetic checkpoints


def grid_spacing_half(a: torch.Tensor) -> torch.Tensor:
    """Half the e2m1 grid spacing around |v| = a (a <= 6): 0.25 below 2, 0.5 in [2, 4),
    1 in [4, 6]."""
    return torch.where(a < 2, 0.25, torch.where(a < 4, 0.5, 1.0))


def grid_matrix(N: int, K: int, gen: torch.Generator, exponents=GRID_EXPONENTS):
    """(w bf16 [N, K], codes uint8 [N, K/2], e8 uint8 [N, K/32]) with
    w = 2^e_block * e2m1(code): random 4-bit codes (-0 included), a magnitude-4 or -6 code
    in every block, e_block drawn per block."""
    nb = K // BLOCK
    code = torch.randint(0, 16, (N, nb, BLOCK), generator=gen, dtype=torch.int64)
    col = torch.randint(0, BLOCK, (N, nb, 1), generator=gen)
    top = torch.randint(6, 8, (N, nb, 1), generator=gen) | (
        torch.randint(0, 2, (N, nb, 1), generator=gen) << 3)
    code.scatter_(2, col, top)
    e = torch.tensor(exponents)[torch.randint(0, len(exponents), (N, nb), generator=gen)]
    pairs = code.reshape(N, K // 2, 2)
    packed = (pairs[:, :, 0] | (pairs[:, :, 1] << 4)).to(torch.uint8)
    e8 = (e + 127).to(torch.uint8)
    w = R.dequant_rows_mxfp4(packed, e8)
    wb = w.to(torch.bfloat16)
    assert torch.equal(wb.float(), w)  # exact in bf16
    return wb, packed, e8


def write_grid_checkpoint(out_dir, seed: int = 3) -> Path:
    """The tiny bf16 checkpoint with every projection replaced by a grid matrix."""
    out_dir = Path(out_dir)
    base = write_checkpoint(out_dir / "base", tiny_cfg(), torch.bfloat16, seed=seed,
                            single_file=True)
    gen = torch.Generator().manual_seed(2000 + seed)

    def grid(_name, t):
        return grid_matrix(t.shape[0], t.shape[1], gen)[0]

    return rewrite_projections(base, out_dir / "grid", grid)


def expected_weight_bytes(cfg, fmt: str) -> int:
    """Device weight bytes of the whole model: a projection [N, K] is N K / 2 + N K / 32
    bytes (mxfp4), N K + 4 N (fp8) or 2 N K (model); embedding, head (if untied) and norms
    2 per element."""
    H, V, I, L = cfg.hidden_size, cfg.vocab_size, cfg.intermediate_size, cfg.num_hidden_layers
    hd = cfg.head_dim if getattr(cfg, "head_dim", None) else H // cfg.num_attention_heads
    nq, nk = cfg.num_attention_heads * hd, cfg.num_key_value_heads * hd
    tied = bool(getattr(cfg, "tie_word_embeddings", False))
    rest = 2 * (V * H * (1 if tied else 2) + H + L * 2 * H)
    per = {"mxfp4": lambda n, k: n * k // 2 + n * k // 32, "fp8": lambda n, k: n * k + 4 * n,
           "model": lambda n, k: 2 * n * k}[fmt]
    projs = [((nq + 2 * nk), H), (H, nq), (2 * I, H), (H, I)]
    return rest + L * sum(per(n, k) for n, k in projs)


__all__ = ["tiny_cfg", "grid_matrix", "write_grid_checkpoint", "rewrite_projections",
           "projection_tensors", "grid_spacing_half", "expected_weight_bytes", "is_projection"]
