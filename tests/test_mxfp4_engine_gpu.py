"""Native Llama engine with MXFP4 weight-only projections (weights="mxfp4").

On the lossless grid checkpoint of tests/_mxfp4.py the mxfp4 engine and the 16-bit engine
hold the same mathematical weights, so the 16-bit engine is the oracle; a second, ordinary
checkpoint proves that the quantised weights (not the originals) are what runs."""
import json
import os

import pytest
import torch

from _mxfp4 import (expected_weight_bytes, rewrite_projections, tiny_cfg,
                    write_grid_checkpoint)
from cake_amd.ops import reference as R
from cake_amd.utils.synth import write_checkpoint

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROMPT = [1, 17, 300, 5, 99, 1024, 7, 8]
FORCED = [11, 250, 3, 1999, 640, 77, 5, 1203, 42, 900, 31, 8]
TOL = dict(atol=2e-2, rtol=2e-2)  # engine-vs-oracle logits, as tests/test_engine_gpu.py


@pytest.fixture(scope="module")
def grid(tmp_path_factory):
    return write_grid_checkpoint(tmp_path_factory.mktemp("mxfp4_grid"))


def _engine(path, **kw):
    from cake_amd.engine import NativeLlama
    return NativeLlama(path, max_seq=kw.pop("max_seq", 256), **kw)


@pytest.fixture(scope="module")
def oracle(cuda, grid):
    """The bf16 16-bit engine's logits on the grid checkpoint, computed once."""
    eng = _engine(grid, dtype="bf16")
    out = {"prefill": torch.from_numpy(eng.prefill_logits(PROMPT)).clone(),
           "forced": torch.from_numpy(eng.forced_logits(PROMPT, FORCED)).clone(),
           "bytes": eng.weight_bytes()}
    eng.close()
    return out


def test_mxfp4_logits_match_16bit_engine(cuda, grid, oracle):
    eng = _engine(grid, dtype="bf16", weights="mxfp4")
    pre = torch.from_numpy(eng.prefill_logits(PROMPT))
    forced = torch.from_numpy(eng.forced_logits(PROMPT, FORCED))
    eng.close()
    print(f"prefill bit-equal: {torch.equal(pre, oracle['prefill'])}, max |diff| "
          f"{float((pre - oracle['prefill']).abs().max())}; forced max |diff| "
          f"{float((forced - oracle['forced']).abs().max())}")
    assert forced.shape == (len(FORCED) + 1, 2048)
    torch.testing.assert_close(pre, oracle["prefill"], **TOL)
    torch.testing.assert_close(forced, oracle["forced"], **TOL)


def test_mxfp4_engine_runs_the_quantised_weights(cuda, tmp_path):
    """An ordinary checkpoint: the mxfp4 engine agrees with the 16-bit engine on
    dequant(quant(w)), and its distance to the original weights' logits (the quantisation
    error, recorded in profiles/mxfp4_engine_error.json) is only required to be finite."""
    base = write_checkpoint(tmp_path / "base", tiny_cfg(), torch.bfloat16, seed=5,
                            single_file=True)
    changed = []

    def requant(name, w):
        codes, scale = R.quant_rows_mxfp4(w)
        dq = R.dequant_rows_mxfp4(codes, scale).to(torch.bfloat16)
        changed.append(int((dq != w).sum()))
        return dq

    rq = rewrite_projections(base, tmp_path / "requant", requant)
    assert sum(changed) > 0  # quantisation does change this checkpoint
    e16 = _engine(rq, dtype="bf16")
    want = torch.from_numpy(e16.forced_logits(PROMPT, FORCED)).clone()
    e16.close()
    e0 = _engine(base, dtype="bf16")
    orig = torch.from_numpy(e0.forced_logits(PROMPT, FORCED)).clone()
    e0.close()
    e4 = _engine(base, dtype="bf16", weights="mxfp4")
    got = torch.from_numpy(e4.forced_logits(PROMPT, FORCED)).clone()
    e4.close()
    torch.testing.assert_close(got, want, **TOL)
    err = float((got - orig).abs().max())
    # an engine that ran the original weights would sit at distance 0 from `orig`
    assert float((got - want).abs().max()) < err
    rec = {"checkpoint": "synthetic tiny (3 layers, H 512, I 1024, V 2048), seed 5, bf16",
           "forced_tokens": len(FORCED),
           "max_abs_logit_diff_mxfp4_vs_original": err,
           "max_abs_logit_diff_mxfp4_vs_requantised_16bit": float((got - want).abs().max()),
           "max_abs_logit_diff_requantised_vs_original": float((want - orig).abs().max()),
           "logit_abs_max": float(orig.abs().max())}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mxfp4_engine_error.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(rec)
    assert err == err and err != float("inf")


def _check_generate(eng, prompt, n):
    """Greedy, penalty 1: every generated token is the argmax of the same engine's
    teacher-forced logits row for it (captured replay == eager launch), and a second
    generate returns the same tokens."""
    got = eng.generate(prompt, n, repeat_penalty=1.0)
    assert len(got.tokens) == n
    logits = torch.from_numpy(eng.forced_logits(prompt, got.tokens[:-1]))
    assert logits.argmax(dim=1).tolist() == got.tokens
    assert eng.generate(prompt, n, repeat_penalty=1.0).tokens == got.tokens


def test_mxfp4_captured_graph_matches_eager(cuda, grid):
    eng = _engine(grid, dtype="bf16", weights="mxfp4")
    _check_generate(eng, PROMPT, 24)
    eng.close()


def test_mxfp4_captured_graph_multistep(cuda, grid):
    eng = _engine(grid, dtype="bf16", weights="mxfp4", steps_per_graph=4)
    _check_generate(eng, PROMPT, 24)
    eng.close()


def test_mxfp4_captured_graph_crosses_one_split_bound(cuda, grid):
    """A 330-token prompt: the live length is past the one-split attention bound."""
    g = torch.Generator().manual_seed(2)
    prompt = torch.randint(3, 2048, (330,), generator=g).tolist()
    eng = _engine(grid, dtype="bf16", weights="mxfp4", max_seq=512)
    _check_generate(eng, prompt, 24)
    eng.close()


def test_mxfp4_weight_bytes(cuda, grid, oracle):
    from cake_amd.models.llama3.config import LlamaConfig
    cfg = LlamaConfig.from_path(grid)
    eng = _engine(grid, dtype="bf16", weights="mxfp4")
    got = eng.weight_bytes()
    eng.close()
    e8 = _engine(grid, dtype="bf16", weights="fp8")
    fp8 = e8.weight_bytes()
    e8.close()
    assert got == expected_weight_bytes(cfg, "mxfp4")
    assert fp8 == expected_weight_bytes(cfg, "fp8")
    assert oracle["bytes"] == expected_weight_bytes(cfg, "model")
    assert got < fp8 < oracle["bytes"]


def test_mxfp4_refusals(cuda, grid):
    from cake_amd.engine import NativeLlama
    with pytest.raises(RuntimeError, match="tensor parallel"):
        NativeLlama(grid, max_seq=256, tp=True, world=2, rank=0, weights="mxfp4",
                    connect_timeout_s=1.0)
    with pytest.raises(ValueError):
        NativeLlama(grid, max_seq=256, weights="int4")


def test_mxfp4_width_not_divisible_by_32_is_refused(cuda, tmp_path):
    """intermediate_size 1040 = 32 * 32 + 16: fine for fp8 (16), refused for mxfp4."""
    from cake_amd.engine import NativeLlama, write_config
    from cake_amd.models.llama3.config import preset
    cfg = preset("llama3-8b", num_hidden_layers=1, vocab_size=256, intermediate_size=1040,
                 hidden_size=512, num_attention_heads=8, num_key_value_heads=2,
                 bos_token_id=1, eos_token_id=2)
    d = write_config(str(tmp_path / "w1040"), cfg)
    with pytest.raises(RuntimeError, match="divisible by 32"):
        NativeLlama(d, max_seq=64, random_init=True, seed=1, weights="mxfp4")
    NativeLlama(d, max_seq=64, random_init=True, seed=1, weights="fp8").close()


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_cake_cli_weight_dtype_mxfp4(cuda, grid, tmp_path, dtype):
    """cake-cli --weight-dtype mxfp4 generates on the native engine and logs the weight
    line, in either model dtype."""
    import subprocess
    cli = os.path.join(ROOT, "cake_amd", "lib", "cake-cli")
    r = subprocess.run([cli, "--model", str(grid), "--topology", str(tmp_path / "none.yml"),
                        "--temperature", "0", "-n", "8", "--dtype", dtype, "--prompt",
                        "hello there", "--max-seq-len", "256", "--weight-dtype", "mxfp4"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT,
                       env=dict(os.environ, CAKE_LOG="warning"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert f"weights mxfp4 projections ({dtype} rest)" in r.stderr and "native engine" in r.stderr
    assert "tokens generated" in r.stderr and r.stdout.strip()


def test_mxfp4_f16_engine(cuda, grid):
    """The bf16 grid checkpoint converted to f16 on load (exact: 2 significant bits), then
    quantised: forced logits stay within tolerance of the f16 16-bit engine."""
    e16 = _engine(grid, dtype="f16")
    want = torch.from_numpy(e16.forced_logits(PROMPT, FORCED)).clone()
    e16.close()
    e4 = _engine(grid, dtype="f16", weights="mxfp4")
    got = torch.from_numpy(e4.forced_logits(PROMPT, FORCED)).clone()
    e4.close()
    torch.testing.assert_close(got, want, **TOL)
