"""Native Llama engine with an FP8 (e4m3) KV cache (kv="fp8").

The oracle is the engine itself in its emulated mode (kv="fp8-emulated": the 16-bit cache and
every 16-bit reader, each writer storing the value of the code the fp8 writer stores).  With
the arithmetic order identical, the fp8 engine must equal it bit for bit on every path:
one-shot and chunked prefill, eager and captured decode, every weight format."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from _fp8 import tiny_cfg, write_grid_checkpoint
from cake_amd.utils.synth import write_checkpoint

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROMPT = [1, 17, 300, 5, 99, 1024, 7, 8]                      # as tests/test_fp8_engine_gpu.py
FORCED = [11, 250, 3, 1999, 640, 77, 5, 1203, 42, 900, 31, 8]


@pytest.fixture(scope="module")
def grid(tmp_path_factory):
    return write_grid_checkpoint(tmp_path_factory.mktemp("kv8_grid"))


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return write_checkpoint(tmp_path_factory.mktemp("kv8_plain") / "base", tiny_cfg(),
                            torch.bfloat16, seed=5, single_file=True)


def _engine(path, **kw):
    from cake_amd.engine import NativeLlama
    return NativeLlama(path, max_seq=kw.pop("max_seq", 256), **kw)


def _outputs(path, n_gen=24, **kw):
    eng = _engine(path, **kw)
    out = {"prefill": eng.prefill_logits(PROMPT).copy(),
           "forced": eng.forced_logits(PROMPT, FORCED).copy(),
           "tokens": eng.generate(PROMPT, n_gen, repeat_penalty=1.0).tokens if n_gen else None}
    eng.close()
    return out


def _assert_bit_equal(a, b, what):
    for key in ("prefill", "forced"):
        assert np.isfinite(a[key]).all(), f"{what}: {key} not finite"
        same = np.array_equal(a[key].view(np.int32), b[key].view(np.int32))
        print(f"{what}: {key} bit-equal {same}, max |diff| {float(np.abs(a[key] - b[key]).max())}")
        assert same, f"{what}: {key} logits differ from the emulated engine's"
    assert a["tokens"] == b["tokens"], f"{what}: greedy tokens differ"


@pytest.mark.parametrize("weights", ["model", "fp8", "mxfp4"])
def test_kv8_is_bit_equal_to_the_emulated_engine(cuda, grid, weights):
    got = _outputs(grid, dtype="bf16", weights=weights, kv="fp8")
    want = _outputs(grid, dtype="bf16", weights=weights, kv="fp8-emulated")
    assert got["forced"].shape == (len(FORCED) + 1, 2048) and len(got["tokens"]) == 24
    _assert_bit_equal(got, want, f"weights {weights}")


def test_kv8_f16_engine_is_bit_equal_to_the_emulated_engine(cuda, grid):
    got = _outputs(grid, dtype="f16", kv="fp8")
    want = _outputs(grid, dtype="f16", kv="fp8-emulated")
    _assert_bit_equal(got, want, "f16")


def test_kv8_engine_runs_the_quantised_cache(cuda, plain):
    """An ordinary checkpoint: the fp8-cache logits differ from the 16-bit-cache engine's
    (the quantised values are what attention reads).  The distance is a property of the
    format, recorded in profiles/kv8_engine_error.json and only required to be finite."""
    e16 = _outputs(plain, n_gen=0, dtype="bf16")
    e8 = _outputs(plain, n_gen=0, dtype="bf16", kv="fp8")
    emu = _outputs(plain, n_gen=0, dtype="bf16", kv="fp8-emulated")
    _assert_bit_equal(dict(e8, tokens=None), dict(emu, tokens=None), "plain checkpoint")
    err_forced = float(np.abs(e8["forced"] - e16["forced"]).max())
    err_prefill = float(np.abs(e8["prefill"] - e16["prefill"]).max())
    rec = {"checkpoint": "synthetic tiny (3 layers, H 512, I 1024, V 2048), seed 5, bf16",
           "forced_tokens": len(FORCED),
           "max_abs_logit_diff_kv_fp8_vs_kv_16bit_forced": err_forced,
           "max_abs_logit_diff_kv_fp8_vs_kv_16bit_prefill": err_prefill,
           "max_abs_logit_diff_kv_fp8_vs_emulated": float(np.abs(e8["forced"] - emu["forced"]).max()),
           "logit_abs_max": float(np.abs(e16["forced"]).max())}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "kv8_engine_error.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(rec)
    assert err_forced > 0 and err_prefill > 0, "the fp8 cache changed nothing: it is not read"
    assert np.isfinite(err_forced) and np.isfinite(err_prefill)


def _check_generate(eng, prompt, n, more=0):
    """Greedy, penalty 1: every generated token is the argmax of the same engine's
    teacher-forced logits row for it (captured replay == eager launch), a second generate
    returns the same tokens, and so does a generate followed by continue_."""
    got = eng.generate(prompt, n, repeat_penalty=1.0)
    assert len(got.tokens) == n
    logits = torch.from_numpy(eng.forced_logits(prompt, got.tokens[:-1]))
    assert logits.argmax(dim=1).tolist() == got.tokens
    assert eng.generate(prompt, n, repeat_penalty=1.0).tokens == got.tokens
    if more:  # (1 + a multiple of steps_per_graph decode steps, then the rest)
        first = eng.generate(prompt, n - more, repeat_penalty=1.0).tokens
        assert first + eng.continue_(more).tokens == got.tokens


@pytest.mark.parametrize("spg", [1, 4])
def test_kv8_captured_graph_matches_eager(cuda, grid, spg):
    eng = _engine(grid, dtype="bf16", kv="fp8", steps_per_graph=spg)
    _check_generate(eng, PROMPT, 24, more=7)
    eng.close()


def test_kv8_captured_graph_crosses_one_split_bound(cuda, grid):
    """A 330-token prompt: the live length is past the one-split attention bound."""
    g = torch.Generator().manual_seed(2)
    prompt = torch.randint(3, 2048, (330,), generator=g).tolist()
    eng = _engine(grid, dtype="bf16", kv="fp8", weights="mxfp4", max_seq=512)
    _check_generate(eng, prompt, 24, more=7)
    want = _engine(grid, dtype="bf16", kv="fp8-emulated", weights="mxfp4", max_seq=512)
    assert want.generate(prompt, 24, repeat_penalty=1.0).tokens == \
        eng.generate(prompt, 24, repeat_penalty=1.0).tokens
    want.close()
    eng.close()


def test_kv8_chunked_prefill_reads_the_cache(cuda, grid):
    """A worker engine (open_layers) fed a prompt as two chunks, then a decode step: the second
    chunk (pos0 > 0) attends to the first through the cache.  fp8 equals emulated bit for
    bit, and what the second chunk computes depends on the first."""
    cfg = tiny_cfg()
    H, layers = cfg.hidden_size, list(range(cfg.num_hidden_layers))
    g = torch.Generator().manual_seed(11)
    x = torch.randn(41, H, generator=g).numpy().astype(np.float32)
    other = torch.randn(33, H, generator=g).numpy().astype(np.float32)
    outs = {}
    for kv in ("fp8", "fp8-emulated"):
        eng = _engine(grid, dtype="bf16", kv=kv, layers=layers)
        a = eng.forward(layers, 0, x[:33].copy())
        b = eng.forward(layers, 33, x[33:40].copy())
        c = eng.forward(layers, 40, x[40:41].copy())
        # the same second chunk behind a different first chunk, in another session
        eng.forward(layers, 0, other.copy(), session=2)
        b2 = eng.forward(layers, 33, x[33:40].copy(), session=2)
        eng.close()
        outs[kv] = (a, b, c, b2)
    for name, got, want in zip(("chunk 1", "chunk 2", "decode step", "session 2"), outs["fp8"],
                               outs["fp8-emulated"]):
        assert np.isfinite(got).all(), name
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), f"{name} differs"
    assert not np.array_equal(outs["fp8"][1], outs["fp8"][3]), "chunk 2 ignores the cache"


def test_kv8_kv_bytes(cuda, grid):
    cfg = tiny_cfg()
    hd = cfg.hidden_size // cfg.num_attention_heads
    elems = 2 * cfg.num_hidden_layers * cfg.num_key_value_heads * 256 * hd
    got = {}
    for kv in ("model", "fp8", "fp8-emulated"):
        eng = _engine(grid, dtype="bf16", kv=kv)
        got[kv] = (eng.kv_bytes(), eng.weight_bytes())
        eng.close()
    assert got["model"][0] == elems * 2 and got["fp8"][0] == elems
    assert got["fp8"][0] * 2 == got["model"][0]
    assert got["fp8-emulated"][0] == got["model"][0]  # the oracle saves no memory
    assert got["fp8"][1] == got["model"][1] == got["fp8-emulated"][1]


def test_kv8_refusals(cuda, grid, monkeypatch):
    from cake_amd.engine import EngineOpts, NativeLlama, lib
    with pytest.raises(RuntimeError, match="tensor parallel"):
        NativeLlama(grid, max_seq=256, tp=True, world=2, rank=0, kv="fp8", connect_timeout_s=1.0)
    err = C.create_string_buffer(1024)
    opts = EngineOpts(256, 0, 0, 1, 0, 0, 0, 0, 3)
    assert not lib().cake_engine_open(str(grid).encode(), C.byref(opts), err, len(err))
    assert "kv_fmt" in err.value.decode()
    # an experimental decode path enabled at open: refused with a message, not ignored
    monkeypatch.setenv("CAKE_ATTN_HEADS", "64")
    with pytest.raises(RuntimeError, match="CAKE_ATTN_HEADS"):
        NativeLlama(grid, max_seq=256, kv="fp8")


def test_cake_cli_kv_dtype_fp8(cuda, grid, tmp_path):
    """cake-cli --kv-dtype fp8 generates on the native engine and logs the cache's format."""
    cli = os.path.join(ROOT, "cake_amd", "lib", "cake-cli")
    r = subprocess.run([cli, "--model", str(grid), "--topology", str(tmp_path / "none.yml"),
                        "--temperature", "0", "-n", "8", "--dtype", "bf16", "--prompt",
                        "hello there", "--max-seq-len", "256", "--kv-dtype", "fp8"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT,
                       env=dict(os.environ, CAKE_LOG="warning"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "kv cache fp8 e4m3" in r.stderr and "native engine" in r.stderr
    assert "tokens generated" in r.stderr and r.stdout.strip()
