"""Native Llama engine with the FP8 MFMA prefill (weights="fp8", prefill="fp8").

The oracle is the plain-torch forward of tests/_w8a8.py: hook off it must reproduce the
16-bit engine on the grid checkpoint (a test of its own); with the w8a8 hook every
projection is quant_rows_fp8 of the activation rows, then the float64 code GEMM.  No bound is
placed on the format's own error: the distances are recorded in
profiles/w8a8_engine_error.json."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import _w8a8 as W
from _fp8 import tiny_cfg, write_grid_checkpoint
from cake_amd.models.llama3.config import preset
from cake_amd.utils.synth import write_checkpoint

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = dict(atol=2e-2, rtol=2e-2)  # engine-vs-oracle logits, as tests/test_engine_gpu.py
PROMPT = [1, 17, 300, 5, 99, 1024, 7, 8]                      # as tests/test_fp8_engine_gpu.py
LONG = [1] + torch.randint(3, 2048, (44,), generator=torch.Generator().manual_seed(4)).tolist()
DT = {"bf16": torch.bfloat16, "f16": torch.float16}


@pytest.fixture(scope="module")
def grid(tmp_path_factory):
    return write_grid_checkpoint(tmp_path_factory.mktemp("w8a8_grid"))


def _engine(path, **kw):
    from cake_amd.engine import NativeLlama
    return NativeLlama(path, max_seq=kw.pop("max_seq", 256), **kw)


def _prefill(path, prompt, **kw):
    eng = _engine(path, **kw)
    out = torch.from_numpy(eng.prefill_logits(prompt).copy())
    eng.close()
    return out


@functools.lru_cache(maxsize=None)
def _oracle(path, dtype, hook):
    fn = W.w8a8_projection if hook else W.plain_projection
    return W.ref_prefill_logits(path, LONG, DT[dtype], fn)


def _dist(a, b) -> float:
    return float((a.double() - b.double()).abs().max())


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_reference_forward_reproduces_the_16bit_engine(cuda, grid, dtype):
    got = _prefill(grid, LONG, dtype=dtype)
    want = _oracle(grid, dtype, False)
    print(f"{dtype}: 16-bit engine vs plain reference forward: max |diff| {_dist(got, want):.4g}, "
          f"logit abs max {float(want.abs().max()):.4g}")
    assert torch.isfinite(got).all()
    assert torch.allclose(got, want, **TOL)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_prefill_fp8_matches_the_quantised_oracle(cuda, grid, dtype):
    """Within TOL of the oracle, and strictly closer to it than to the weights="fp8" engine
    (an engine that ignored the option sits at distance 0 from the latter)."""
    got = _prefill(grid, LONG, dtype=dtype, weights="fp8", prefill="fp8")
    parent = _prefill(grid, LONG, dtype=dtype, weights="fp8")
    e16 = _prefill(grid, LONG, dtype=dtype)
    want = _oracle(grid, dtype, True)
    d_oracle, d_parent, d_16 = _dist(got, want), _dist(got, parent), _dist(got, e16)
    rec = {"checkpoint": "synthetic tiny grid (3 layers, H 512, I 1024, V 2048), seed 3",
           "dtype": dtype, "prompt_tokens": len(LONG),
           "max_abs_logit_diff_prefill_fp8_vs_oracle": d_oracle,
           "max_abs_logit_diff_prefill_fp8_vs_weights_fp8_engine": d_parent,
           "max_abs_logit_diff_prefill_fp8_vs_16bit_engine": d_16,
           "max_abs_logit_diff_oracle_vs_plain_reference": _dist(want, _oracle(grid, dtype, False)),
           "logit_abs_max": float(want.abs().max())}
    print(rec)
    if dtype == "bf16":
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "w8a8_engine_error.json"), "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    assert torch.isfinite(got).all()
    assert torch.allclose(got, want, **TOL), f"fp8 prefill vs oracle: max |diff| {d_oracle}"
    assert d_parent > 0, "the option changed nothing: the fp8 prefill is not run"
    assert d_oracle < d_parent, (d_oracle, d_parent)


def test_chunked_prefill_agrees_with_one_shot(cuda, grid):
    """A worker engine (open_layers) fed 40 rows at once and as chunks of 33 + 7 (pos0 > 0), then
    a decode step: the activation scales are per token, so only the attention's chunking
    differs."""
    cfg = tiny_cfg()
    H, layers = cfg.hidden_size, list(range(cfg.num_hidden_layers))
    x = torch.randn(41, H, generator=torch.Generator().manual_seed(11)).numpy().astype(np.float32)
    eng = _engine(grid, dtype="bf16", weights="fp8", prefill="fp8", layers=layers)
    whole = eng.forward(layers, 0, x[:40].copy())
    a = eng.forward(layers, 0, x[:33].copy(), session=2)
    b = eng.forward(layers, 33, x[33:40].copy(), session=2)
    c1 = eng.forward(layers, 40, x[40:41].copy())
    c2 = eng.forward(layers, 40, x[40:41].copy(), session=2)
    plain = _engine(grid, dtype="bf16", weights="fp8", layers=layers)
    ref = plain.forward(layers, 0, x[:40].copy())
    plain.close()
    eng.close()
    chunked = np.concatenate([a, b])
    assert np.isfinite(whole).all() and np.isfinite(chunked).all()
    print(f"chunked vs one-shot: max |diff| {float(np.abs(chunked - whole).max()):.4g}; "
          f"one-shot vs weights=fp8 engine: {float(np.abs(whole - ref).max()):.4g}")
    assert np.allclose(chunked, whole, **TOL)
    assert np.allclose(c1, c2, **TOL)
    assert not np.array_equal(whole, ref), "the worker engine ignored prefill_fmt"


def _check_generate(eng, prompt, n, more=0):
    """As tests/test_kv8_engine_gpu.py: every greedy token is the argmax of the engine's own
    teacher-forced row (captured replay == eager), and a second generate repeats the first."""
    got = eng.generate(prompt, n, repeat_penalty=1.0)
    assert len(got.tokens) == n
    logits = torch.from_numpy(eng.forced_logits(prompt, got.tokens[:-1]))
    assert logits.argmax(dim=1).tolist() == got.tokens
    assert eng.generate(prompt, n, repeat_penalty=1.0).tokens == got.tokens
    if more:
        first = eng.generate(prompt, n - more, repeat_penalty=1.0).tokens
        assert first + eng.continue_(more).tokens == got.tokens


@pytest.mark.parametrize("extra", [{}, {"head": "fp8", "kv": "fp8"}])
def test_generate_captured_matches_eager(cuda, grid, extra):
    eng = _engine(grid, dtype="bf16", weights="fp8", prefill="fp8", **extra)
    _check_generate(eng, PROMPT, 24, more=7)
    _check_generate(eng, LONG, 12)
    eng.close()


def test_weight_bytes_unchanged(cuda, grid):
    got = {}
    for prefill in ("model", "fp8"):
        eng = _engine(grid, dtype="bf16", weights="fp8", prefill=prefill)
        got[prefill] = (eng.weight_bytes(), eng.kv_bytes())
        eng.close()
    assert got["model"] == got["fp8"]


def test_refusals(cuda, grid, tmp_path):
    import ctypes as C

    from cake_amd.engine import EngineOpts, NativeLlama, lib
    for weights in ("model", "mxfp4"):
        with pytest.raises(RuntimeError, match="prefill_fmt 1.*weight_fmt 1"):
            NativeLlama(grid, max_seq=256, weights=weights, prefill="fp8")
    with pytest.raises(RuntimeError, match="tensor parallel"):
        NativeLlama(grid, max_seq=256, tp=True, world=2, rank=0, weights="fp8", prefill="fp8",
                    connect_timeout_s=1.0)
    with pytest.raises(RuntimeError, match="prefill_fmt 1.*tensor parallel"):
        NativeLlama(grid, max_seq=256, tp=True, world=2, rank=0, prefill="fp8",
                    connect_timeout_s=1.0)
    err = C.create_string_buffer(1024)
    opts = EngineOpts(256, 0, 0, 1, 0, 1 | 2 << 8, 0, 0, 0)   # weight_fmt 1, prefill_fmt 2
    assert not lib().cake_engine_open(str(grid).encode(), C.byref(opts), err, len(err))
    assert "prefill_fmt must be" in err.value.decode()
    # H = 320: fine for fp8 weights (divisible by 16), not a multiple of the MFMA step's k
    cfg = preset("llama3-8b", num_hidden_layers=1, vocab_size=512, intermediate_size=640,
                 hidden_size=320, num_attention_heads=5, num_key_value_heads=1,
                 bos_token_id=1, eos_token_id=2)
    narrow = write_checkpoint(tmp_path / "h320", cfg, torch.bfloat16, seed=1, single_file=True)
    with pytest.raises(RuntimeError, match="divisible by 128"):
        NativeLlama(narrow, max_seq=64, weights="fp8", prefill="fp8")


def test_cake_cli_prefill_dtype_fp8(cuda, grid, tmp_path):
    """cake-cli --weight-dtype fp8 --prefill-dtype fp8 generates on the native engine and logs
    the prefill's format."""
    cli = os.path.join(ROOT, "cake_amd", "lib", "cake-cli")
    r = subprocess.run([cli, "--model", str(grid), "--topology", str(tmp_path / "none.yml"),
                        "--temperature", "0", "-n", "8", "--dtype", "bf16", "--prompt",
                        "hello there", "--max-seq-len", "256", "--weight-dtype", "fp8",
                        "--prefill-dtype", "fp8"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT,
                       env=dict(os.environ, CAKE_LOG="warning"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "prefill fp8 e4m3 activations" in r.stderr and "native engine" in r.stderr
    assert "tokens generated" in r.stderr and r.stdout.strip()
