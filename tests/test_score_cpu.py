"""Sequence scoring: the CPU side (reference helpers, window rule, option surfaces)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _score as S
import _w8a8 as W
from _fp8 import write_grid_checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cake_amd", "lib", "cake-cli")
LONG = [1] + torch.randint(3, 2048, (44,), generator=torch.Generator().manual_seed(4)).tolist()


@pytest.fixture(scope="module")
def grid(tmp_path_factory):
    return write_grid_checkpoint(tmp_path_factory.mktemp("score_grid"))


def test_lse_ref_against_a_brute_force_loop():
    import math
    g = np.random.default_rng(0)
    x = (g.standard_normal((5, 37)) * 20).astype(np.float32).astype(np.float64)
    x[1, 3] = x[1, 30] = x[1].max() + 1      # a tie: the lower id
    x[2, ::2] = -np.inf
    x[3, :] = -np.inf
    target = np.array([0, 36, 1, 5, -1])
    lse, tgt, top, mx = S.lse_ref(x, target)
    for t in range(5):
        m = max(x[t])
        best = min(j for j in range(37) if x[t, j] == m)
        assert top[t] == best and mx[t] == m
        if m == -math.inf:
            assert lse[t] == -math.inf
        else:
            want = m + math.log(math.fsum(math.exp(v - m) for v in x[t]))
            assert abs(lse[t] - want) <= 1e-12 * max(1.0, abs(want))
        if target[t] < 0:
            assert math.isnan(tgt[t])
        else:
            assert tgt[t] == x[t, target[t]]
    assert top[1] == 3 and top[3] == 0


def test_kernel_case_builders():
    for fam in S.FAMILIES:
        x = S.family_logits(fam, 3, 1000)
        assert x.dtype == np.float32 and x.shape == (3, 1000) and np.isfinite(x).all()
    d = S.family_logits("dominant", 3, 1000)
    top2 = np.sort(d, axis=1)[:, -2:]
    assert (top2[:, 1] - top2[:, 0] >= 49.9).all()
    assert abs(S.family_logits("offset", 3, 1000)[0].mean()) > 9e3
    assert S.chunks_of(255, "c256") is None and S.chunks_of(1, "one") == [(0, 1)]
    assert S.chunks_of(1000, "c513") == [(0, 513), (513, 487)]
    assert sum(w for _, w in S.chunks_of(8705, "c256")) == 8705
    assert S.lse_bound(np.array([0.0]))[0] == 128 * 2.0 ** -24


def test_ref_all_logits_last_row_is_the_prefill_reference(grid):
    """The two differ only by the 16-bit rounding of one normed row."""
    rows = S.ref_all_logits(grid, LONG, torch.bfloat16)
    last = W.ref_prefill_logits(grid, LONG, torch.bfloat16)
    assert rows.shape == (len(LONG), 2048) and torch.isfinite(rows).all()
    d = float((rows[-1].double() - last.double()).abs().max())
    print(f"last row vs ref_prefill_logits: max |diff| {d:.4g}")
    assert d <= 1e-2
    # causal: a prefix's rows are the same rows
    head = S.ref_all_logits(grid, LONG[:9], torch.bfloat16)
    assert torch.allclose(head, rows[:9], atol=1e-5, rtol=0)


@pytest.mark.parametrize("S_", [2, 7, 64])
def test_window_rule(S_):
    from cake_amd.native_bridge import score_windows
    for n in (1, 2, S_, S_ + 1, 2 * S_, 2 * S_ + 1):
        got = score_windows(n, S_)
        assert [tuple(w) for w in got] == S.windows(n, S_), (n, S_)
        assert all(2 <= b - a <= S_ for a, b in got)
        scored = sum(b - a - 1 for a, b in got)
        full, rest = divmod(n, S_)
        assert scored == full * (S_ - 1) + max(rest - 1, 0)
        assert len(got) == full + (1 if rest >= 2 else 0)
    assert score_windows(1, S_) == []
    assert score_windows(2 * S_ + 1, S_) == [(0, S_), (S_, 2 * S_)]   # one-token tail dropped


def test_score_summary_is_the_mean_over_all_scored_tokens():
    from cake_amd.engine import score_result
    from cake_amd.native_bridge import score_summary
    g = np.random.default_rng(1)
    parts = []
    for n in (5, 3):
        toks = g.integers(0, 50, n).tolist()
        lse = g.standard_normal(n).astype(np.float32) + 5
        tgt = g.standard_normal(n).astype(np.float32)
        top = np.array(toks[1:] + [0], dtype=np.int32)
        top[0] = (top[0] + 1) % 50
        parts.append((toks, score_result(toks, lse, tgt, top, tgt.copy())))
    s = score_summary(8, parts)
    lp = np.concatenate([r.logprobs for _, r in parts])
    assert s["tokens"] == 8 and s["scored"] == 6 and s["windows"] == 2
    assert abs(s["nll"] + lp.mean()) < 1e-12 and abs(s["ppl"] - np.exp(s["nll"])) < 1e-9
    assert s["top1"] == 4 / 6
    r = parts[0][1]
    assert r.logprobs.dtype == np.float64 and len(r.logprobs) == 4
    assert r.nll == float(-r.logprobs.mean()) and r.ppl == float(np.exp(r.nll))


def test_native_llama_score_rejects_short_input_before_opening():
    from cake_amd.engine import NativeLlama
    eng = NativeLlama.__new__(NativeLlama)   # no engine, no library: nothing may be touched
    for toks in ([], [1]):
        with pytest.raises(ValueError, match="at least 2 tokens"):
            eng.score(toks)


def test_engine_surface_is_unchanged():
    import ctypes as C

    from cake_amd.engine import PREFILL_FORMATS, WEIGHT_FORMATS, EngineOpts
    assert C.sizeof(EngineOpts) == 40
    assert PREFILL_FORMATS == {"model": 0, "fp8": 1}
    assert WEIGHT_FORMATS == {"model": 0, "fp8": 1, "mxfp4": 2}
    src = open(os.path.join(ROOT, "cake_amd", "csrc", "engine", "llama_engine.h")).read()
    assert "int32_t cake_engine_score(void* engine, const int32_t* tokens, int32_t n" in src


def _run(cmd, **env):
    e = dict(os.environ, CAKE_LOG="warning", **env)
    return subprocess.run(cmd, capture_output=True, text=True, timeout=180, env=e, cwd=ROOT)


def _entry(entry):
    return [CLI] if entry == "cake-cli" else [sys.executable, "-m", "cake_amd.cli"]


@pytest.fixture(scope="module")
def text_file(tmp_path_factory):
    p = tmp_path_factory.mktemp("score_text") / "sample.txt"
    p.write_text("the quick brown fox jumps over the lazy dog\n", encoding="utf-8")
    return p


@pytest.mark.parametrize("entry", ["cake-cli", "python"])
def test_cli_lists_score_file(entry):
    r = _run([*_entry(entry), "--help"])
    assert r.returncode == 0 and "--score-file" in r.stdout
    assert "nll" in r.stdout[r.stdout.rindex("--score-file"):][:700]


@pytest.mark.parametrize("entry", ["cake-cli", "python"])
@pytest.mark.parametrize("how", ["CAKE_NATIVE=0", "--cpu", "--no-graph", "f32"])
def test_score_file_refused_on_the_python_engines(grid, tmp_path, text_file, entry, how):
    extra, env = [], {}
    if how == "CAKE_NATIVE=0":
        env["CAKE_NATIVE"] = "0"
    elif how == "f32":
        extra = ["--dtype", "f32"]
    else:
        extra = [how]
    r = _run([*_entry(entry), "--model", str(grid), "--topology", str(tmp_path / "none.yml"),
              "--score-file", str(text_file), *extra], **env)
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert "--score-file" in r.stderr and "native Llama engine" in r.stderr
    assert r.stdout.strip() == ""


@pytest.mark.parametrize("entry", ["cake-cli", "python"])
def test_score_file_refused_for_image_models(grid, tmp_path, text_file, entry):
    r = _run([*_entry(entry), "--model", str(grid), "--topology", str(tmp_path / "none.yml"),
              "--model-type", "image-model", "--score-file", str(text_file)])
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert "--score-file" in r.stderr and "native Llama engine" in r.stderr
    assert "text model only" in r.stderr and r.stdout.strip() == ""


@pytest.mark.parametrize("entry", ["cake-cli", "python"])
def test_score_file_refused_with_tensor_parallel(grid, tmp_path, text_file, entry):
    r = _run([*_entry(entry), "--model", str(grid), "--topology", str(tmp_path / "none.yml"),
              "--transport", "rccl", "--parallel", "tp", "--score-file", str(text_file)],
             WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert "--score-file" in r.stderr and "--parallel tp" in r.stderr
    assert r.stdout.strip() == ""
