"""Native Llama engine with a quantised lm_head (head="fp8" | "mxfp4"), chosen independently
of the projections' format.

On a checkpoint whose head is a lossless grid matrix (tests/_qhead.py) the quantised-head
engine and the 16-bit engine hold the same mathematical head, so the 16-bit engine is the
oracle; an ordinary checkpoint proves that the quantised head (not the original) is what
runs."""
import json
import os

import pytest
import torch

import _fp8
import _mxfp4
from _qhead import (FORMATS, expected_weight_bytes, head_tensor, rewrite_head, round_trip,
                    write_base_checkpoint, write_grid_head_checkpoint,
                    write_tied_grid_checkpoint)
from cake_amd.ops import reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROMPT = [1, 17, 300, 5, 99, 1024, 7, 8]
FORCED = [11, 250, 3, 1999, 640, 77, 5, 1203]
TOL = dict(atol=2e-2, rtol=2e-2)  # engine-vs-oracle logits, as tests/test_engine_gpu.py


def _engine(path, **kw):
    from cake_amd.engine import NativeLlama
    return NativeLlama(path, max_seq=kw.pop("max_seq", 256), dtype=kw.pop("dtype", "bf16"), **kw)


def _logits(path, **kw):
    eng = _engine(path, **kw)
    out = (torch.from_numpy(eng.prefill_logits(PROMPT)).clone(),
           torch.from_numpy(eng.forced_logits(PROMPT, FORCED)).clone(), eng.weight_bytes())
    eng.close()
    return out


@pytest.fixture(scope="module")
def grids(tmp_path_factory):
    """Per format: the tiny checkpoint whose projections AND head are grid matrices of that
    format, so weights=fmt and head=fmt are both lossless on it."""
    d = tmp_path_factory.mktemp("qhead_grids")
    out = {}
    for fmt, mod in (("fp8", _fp8), ("mxfp4", _mxfp4)):
        proj = mod.write_grid_checkpoint(d / f"proj_{fmt}")
        out[fmt] = write_grid_head_checkpoint(d / fmt, fmt, base=proj)
    return out


@pytest.fixture(scope="module")
def oracle(cuda, grids):
    """The 16-bit engine's logits on each grid checkpoint, computed once."""
    return {fmt: _logits(grids[fmt]) for fmt in FORMATS}


@pytest.mark.parametrize("same_weights", [False, True], ids=["weights-model", "weights-same"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_grid_head_logits_match_16bit_engine(cuda, grids, oracle, fmt, same_weights):
    pre, forced, _ = _logits(grids[fmt], head=fmt, weights=fmt if same_weights else "model")
    want_pre, want_forced, _ = oracle[fmt]
    print(f"head={fmt}: prefill max |diff| {float((pre - want_pre).abs().max()):.3e}, forced "
          f"max |diff| {float((forced - want_forced).abs().max()):.3e}")
    assert forced.shape == (len(FORCED) + 1, 2048)
    torch.testing.assert_close(pre, want_pre, **TOL)
    torch.testing.assert_close(forced, want_forced, **TOL)


@pytest.mark.parametrize("fmt", FORMATS)
def test_engine_runs_the_quantised_head(cuda, tmp_path, fmt):
    """An ordinary checkpoint: the head=fmt engine agrees with the 16-bit engine holding
    dequant(quant(lm_head)) and is farther from the 16-bit engine on the original head."""
    base = write_base_checkpoint(tmp_path / "base", seed=5)
    head = head_tensor(base)
    rq_head = round_trip(fmt, head)
    assert int((rq_head != head).sum()) > 0  # quantisation does change this head
    rq = rewrite_head(base, tmp_path / "requant", head=rq_head)
    _, want, _ = _logits(rq)
    _, orig, _ = _logits(base)
    _, got, _ = _logits(base, head=fmt)
    to_requant = float((got - want).abs().max())
    to_orig = float((got - orig).abs().max())
    rec = {"checkpoint": "synthetic tiny (3 layers, H 512, I 1024, V 2048), seed 5, bf16",
           "forced_tokens": len(FORCED),
           "max_abs_logit_diff_qhead_vs_requantised_16bit": to_requant,
           "max_abs_logit_diff_qhead_vs_original": to_orig,
           "logit_min": float(orig.min()), "logit_max": float(orig.max())}
    print(fmt, rec)
    path = os.path.join(ROOT, "profiles", "qhead_engine_error.json")
    try:
        with open(path) as f:
            allrec = json.load(f)
    except (OSError, ValueError):
        allrec = {}
    allrec[fmt] = rec
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(allrec, f, indent=1, sort_keys=True)
        f.write("\n")
    torch.testing.assert_close(got, want, **TOL)
    assert to_orig > to_requant


def _check_generate(eng, prompt, n):
    """Greedy, penalty 1: every generated token is the argmax of the same engine's
    teacher-forced logits row for it (captured replay == eager launch), and a second
    generate returns the same tokens."""
    got = eng.generate(prompt, n, repeat_penalty=1.0)
    assert len(got.tokens) == n
    logits = torch.from_numpy(eng.forced_logits(prompt, got.tokens[:-1]))
    assert logits.argmax(dim=1).tolist() == got.tokens
    assert eng.generate(prompt, n, repeat_penalty=1.0).tokens == got.tokens
    return got.tokens


@pytest.mark.parametrize("fmt", FORMATS)
def test_greedy_generation(cuda, grids, fmt):
    """The fused tail in the captured graph, one and four steps per replay, against the
    eager unfused head of the same engine; then the repeat penalty against the host rule on
    the forced logits; then a sampled run (the unfused head inside the graph)."""
    eng = _engine(grids[fmt], head=fmt)
    toks = _check_generate(eng, PROMPT, 24)
    pen = eng.generate(PROMPT, 24, repeat_penalty=1.1, repeat_last_n=64).tokens
    logits = torch.from_numpy(eng.forced_logits(PROMPT, pen[:-1]))
    ctx = list(PROMPT)
    for i, t in enumerate(pen):
        assert int(torch.argmax(R.apply_repeat_penalty(logits[i], 1.1, ctx[-64:]))) == t, i
        ctx.append(t)
    a = eng.generate(PROMPT, 24, temperature=0.8, seed=1234).tokens
    b = eng.generate(PROMPT, 24, temperature=0.8, seed=1234).tokens
    assert a == b and len(a) == 24
    eng.close()
    eng4 = _engine(grids[fmt], head=fmt, steps_per_graph=4)
    assert _check_generate(eng4, PROMPT, 24) == toks
    assert eng4.generate(PROMPT, 24, repeat_penalty=1.1, repeat_last_n=64).tokens == pen
    eng4.close()


@pytest.mark.parametrize("fmt", FORMATS)
def test_tied_embeddings(cuda, tmp_path, fmt):
    """tie_word_embeddings: the quantised head is made from the resident embedding, which
    stays 16-bit for the gather; on a grid embedding the logits match the 16-bit engine."""
    from cake_amd.models.llama3.config import LlamaConfig
    d = write_tied_grid_checkpoint(tmp_path, fmt)
    cfg = LlamaConfig.from_path(d)
    assert cfg.tie_word_embeddings
    want_pre, want_forced, bytes16 = _logits(d)
    pre, forced, bytesq = _logits(d, head=fmt)
    print(f"tied head={fmt}: forced max |diff| {float((forced - want_forced).abs().max()):.3e} "
          f"of |logit| <= {float(want_forced.abs().max()):.1f}")
    torch.testing.assert_close(pre, want_pre, **TOL)
    torch.testing.assert_close(forced, want_forced, **TOL)
    assert bytes16 == expected_weight_bytes(cfg, "model", "model")
    assert bytesq == expected_weight_bytes(cfg, "model", fmt) > bytes16
    eng = _engine(d, head=fmt)
    _check_generate(eng, PROMPT, 12)  # the fused tail gathers from the 16-bit table
    eng.close()


def test_weight_bytes(cuda, grids, oracle):
    from cake_amd.models.llama3.config import LlamaConfig
    cfg = LlamaConfig.from_path(grids["fp8"])
    assert oracle["fp8"][2] == expected_weight_bytes(cfg, "model", "model") \
        == _mxfp4.expected_weight_bytes(cfg, "model")
    for weights in ("model", "mxfp4"):
        got = {}
        for head in ("model", "fp8", "mxfp4"):
            eng = _engine(grids["fp8"], weights=weights, head=head)
            got[head] = eng.weight_bytes()
            eng.close()
            assert got[head] == expected_weight_bytes(cfg, weights, head), (weights, head)
        assert got["model"] == _mxfp4.expected_weight_bytes(cfg, weights)
        assert got["mxfp4"] < got["fp8"] < got["model"]


def test_refusals(cuda, grids, tmp_path):
    import ctypes as C
    from cake_amd import engine as E
    grid = grids["fp8"]
    # head_fmt = 3 through the C ABI
    opts = E.EngineOpts(256, 0, 0, 1, 0, 0, 0, 3)
    err = C.create_string_buffer(1024)
    assert not E.lib().cake_engine_open(str(grid).encode(), C.byref(opts), err, len(err))
    assert "head_fmt" in err.value.decode()
    with pytest.raises(ValueError):
        E.NativeLlama(grid, max_seq=256, head="int4")
    # tensor parallel: refused before any connection attempt (nothing listens on the address;
    # a connect would wait out connect_timeout_s), with a message of its own
    import time
    t0 = time.monotonic()
    with pytest.raises(RuntimeError, match="lm_head.*tensor parallel"):
        E.NativeLlama(grid, max_seq=256, tp=True, world=2, rank=1, head="fp8",
                      master_addr="127.0.0.1:9", connect_timeout_s=30.0)
    assert time.monotonic() - t0 < 5.0
    # the fp8 / TP message is still the projections' own
    with pytest.raises(RuntimeError, match="fp8 weights"):
        E.NativeLlama(grid, max_seq=256, tp=True, world=2, rank=1, weights="fp8", head="fp8",
                      master_addr="127.0.0.1:9", connect_timeout_s=30.0)
    # hidden 528 = 16 * 33: refused for an mxfp4 head at open, before any weight is made
    from cake_amd.models.llama3.config import preset
    cfg = preset("llama3-8b", num_hidden_layers=1, vocab_size=256, intermediate_size=1024,
                 hidden_size=528, num_attention_heads=4, num_key_value_heads=2,
                 bos_token_id=1, eos_token_id=2)
    d = E.write_config(str(tmp_path / "h528"), cfg)
    with pytest.raises(RuntimeError, match="mxfp4 lm_head.*divisible by 32"):
        E.NativeLlama(d, max_seq=64, random_init=True, seed=1, head="mxfp4")


def test_cake_cli_head_dtype(cuda, grids, tmp_path):
    """cake-cli --head-dtype fp8 --weight-dtype mxfp4 prints the text of the tokens the
    engine API generates with the same options, and logs the head's format."""
    import subprocess
    from cake_amd import native_bridge as B
    grid = write_grid_head_checkpoint(tmp_path, "fp8", base=_mxfp4.write_grid_checkpoint(
        tmp_path / "proj"))
    cli = os.path.join(ROOT, "cake_amd", "lib", "cake-cli")
    r = subprocess.run([cli, "--model", str(grid), "--topology", str(tmp_path / "none.yml"),
                        "--temperature", "0", "-n", "8", "--dtype", "bf16", "--prompt",
                        "hello there", "--system-prompt", "be brief", "--max-seq-len", "256",
                        "--weight-dtype", "mxfp4", "--head-dtype", "fp8"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT,
                       env=dict(os.environ, CAKE_LOG="warning"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "weights mxfp4 projections (bf16 rest), lm_head fp8 e4m3" in r.stderr
    assert "tokens generated" in r.stderr
    enc = json.loads(B.encode_chat(json.dumps({"model": str(grid), "system": "be brief",
                                               "prompt": "hello there"})))
    eng = _engine(grid, weights="mxfp4", head="fp8")
    toks = eng.generate(enc["ids"], 8, temperature=0.0, repeat_penalty=1.1, repeat_last_n=128,
                        eos_ids=enc["eos"]).tokens
    eng.close()
    text = "".join(B.decode_token(json.dumps({"model": str(grid), "id": t}))
                   for t in toks if t not in enc["eos"])
    assert len(toks) >= 1 and r.stdout == text + "\n"
