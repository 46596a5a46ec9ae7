"""Shared helpers of the FP8 (e4m3) weight-only tests.

``write_grid_checkpoint`` builds a checkpoint that is lossless under the engine's
quantisation: every projection row is ``2^e_row * fp8_value`` with a +-448 code in it, so
the row scale comes out as exactly ``2^e_row`` and quantise -> dequantise reproduces the
bf16 weights bit for bit.  On it the fp8 engine and the 16-bit engine hold the same
mathematical weights: the 16-bit engine is the oracle.
"""
from __future__ import annotations

from pathlib import Path

import torch

from cake_amd.models.llama3.config import preset
from cake_amd.utils.safetensors_io import SafeTensors, save_file
from cake_amd.utils.synth import write_checkpoint

PROJECTIONS = ("self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight",
               "self_attn.o_proj.weight", "mlp.gate_proj.weight", "mlp.up_proj.weight",
               "mlp.down_proj.weight")
GRID_EXPONENTS = (-14, -13, -12)  # weight std ~0.02, as the synthetic checkpoints


def tiny_cfg():
    """The tiny architecture of tests/test_engine_gpu.py."""
    return preset("llama3-8b", num_hidden_layers=3, vocab_size=2048, intermediate_size=1024,
                  hidden_size=512, num_attention_heads=8, num_key_value_heads=2,
                  bos_token_id=1, eos_token_id=2)


def is_projection(name: str) -> bool:
    return name.endswith(PROJECTIONS)


def half_spacing(v: torch.Tensor) -> torch.Tensor:
    """Half an e4m3 code spacing at |v| (v = w / scale, |v| <= 448): the rounding bound
    ``0.5 * 2^(max(floor(log2|v|), -6) - 3)`` (3 mantissa bits, subnormals below 2^-6)."""
    e = (torch.frexp(v.abs().float())[1] - 1).clamp_min(-6)  # floor(log2|v|), exact
    return 0.5 * torch.exp2(e.float() - 3.0)


def grid_matrix(N: int, K: int, gen: torch.Generator, exponents=GRID_EXPONENTS):
    """(w bf16 [N, K], codes uint8 [N, K], scale f32 [N]) with w = 2^e_row * fp8(codes):
    random codes without the NaN code, a +-448 code in every row, e_row drawn per row."""
    codes = torch.randint(0, 256, (N, K), generator=gen, dtype=torch.int32)
    codes[(codes & 0x7F) == 0x7F] = 0x3C  # NaN codes -> 1.5
    col = torch.randint(0, K, (N,), generator=gen)
    sign = torch.randint(0, 2, (N,), generator=gen, dtype=torch.int32) * 0x80
    codes[torch.arange(N), col] = 0x7E | sign  # +-448
    codes = codes.to(torch.uint8)
    e = torch.tensor(exponents)[torch.randint(0, len(exponents), (N,), generator=gen)]
    scale = torch.exp2(e.float())
    w = codes.view(torch.float8_e4m3fn).float() * scale[:, None]
    wb = w.to(torch.bfloat16)
    assert torch.equal(wb.float(), w)  # exact in bf16
    return wb, codes, scale


def rewrite_projections(src: Path, dst: Path, fn) -> Path:
    """Copy the single-file checkpoint ``src`` to ``dst`` with every projection weight
    replaced by ``fn(name, tensor)``."""
    dst = Path(dst)
    dst.mkdir(parents=True, exist_ok=True)
    for f in Path(src).iterdir():
        if f.name != "model.safetensors":
            (dst / f.name).write_bytes(f.read_bytes())
    st = SafeTensors(Path(src) / "model.safetensors")
    out = {}
    for k in st.keys():
        t = st.get(k)
        out[k] = fn(k, t).contiguous() if is_projection(k) else t.clone()
    save_file(out, dst / "model.safetensors", {"format": "pt"})
    return dst


def write_grid_checkpoint(out_dir, seed: int = 3) -> Path:
    """The tiny bf16 checkpoint with every projection replaced by a grid matrix."""
    out_dir = Path(out_dir)
    base = write_checkpoint(out_dir / "base", tiny_cfg(), torch.bfloat16, seed=seed,
                            single_file=True)
    gen = torch.Generator().manual_seed(1000 + seed)

    def grid(_name, t):
        return grid_matrix(t.shape[0], t.shape[1], gen)[0]

    return rewrite_projections(base, out_dir / "grid", grid)


def projection_tensors(model_dir) -> dict[str, torch.Tensor]:
    st = SafeTensors(Path(model_dir) / "model.safetensors")
    return {k: st.get(k) for k in st.keys() if is_projection(k)}


def expected_weight_bytes(cfg, fp8: bool) -> int:
    """Device weight bytes of the whole model: projections 1 byte per element + 4 per row
    (fp8) or 2 per element; embedding, head (if untied) and norms 2 per element."""
    H, V, I, L = cfg.hidden_size, cfg.vocab_size, cfg.intermediate_size, cfg.num_hidden_layers
    hd = cfg.head_dim if getattr(cfg, "head_dim", None) else H // cfg.num_attention_heads
    nq, nk = cfg.num_attention_heads * hd, cfg.num_key_value_heads * hd
    tied = bool(getattr(cfg, "tie_word_embeddings", False))
    rest = 2 * (V * H * (1 if tied else 2) + H + L * 2 * H)
    projs = [((nq + 2 * nk), H), (H, nq), (2 * I, H), (H, I)]
    per_layer = sum(n * k + 4 * n if fp8 else 2 * n * k for n, k in projs)
    return rest + L * per_layer


__all__ = ["tiny_cfg", "grid_matrix", "write_grid_checkpoint", "rewrite_projections",
           "projection_tensors", "half_spacing", "expected_weight_bytes", "is_projection"]
