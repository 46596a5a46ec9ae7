"""NativeLlama.score / cake_engine_score / cake-cli --score-file on the GPU.

Oracle: the plain-torch forward of tests/_score.py (every row, the final norm rounded to the
model dtype) through the float64 log-sum-exp.  Bounds: TOL on logits (the project's
engine-vs-oracle tolerance); lse is 1-Lipschitz in the sup norm of the logits, so
|lse - oracle| <= B = 2e-2 + 2e-2 max|oracle logit|, log-probs within 2B, and the engine's
argmax must be within 2B of the oracle's maximum.  No row is excluded."""
import functools
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import _score as S
from _fp8 import write_grid_checkpoint

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = dict(atol=2e-2, rtol=2e-2)
PROMPT = [1, 17, 300, 5, 99, 1024, 7, 8]
LONG = [1] + torch.randint(3, 2048, (44,), generator=torch.Generator().manual_seed(4)).tolist()
DT = {"bf16": torch.bfloat16, "f16": torch.float16}


@pytest.fixture(scope="module")
def grid(tmp_path_factory):
    return write_grid_checkpoint(tmp_path_factory.mktemp("score_grid"))


def _engine(path, **kw):
    from cake_amd.engine import NativeLlama
    return NativeLlama(path, max_seq=kw.pop("max_seq", 256), **kw)


@functools.lru_cache(maxsize=None)
def _oracle(path, dtype):
    """(logits float64 [T, V], lse, target logit, argmax, max, B) of LONG; computed once."""
    x = S.ref_all_logits(path, LONG, DT[dtype]).double().numpy()
    target = np.array(LONG[1:] + [-1])
    lse, tgt, top, mx = S.lse_ref(x, target)
    for a in (x, lse, tgt, top, mx):
        a.setflags(write=False)
    return x, lse, tgt, top, mx, 2e-2 + 2e-2 * float(np.abs(x).max())


@functools.lru_cache(maxsize=None)
def _score16(path, dtype="bf16", vchunk=0):
    eng = _engine(path, dtype=dtype)
    r = eng.score(LONG, vchunk=vchunk)
    eng.close()
    return r


def _check_against_oracle(r, orc, rows=None, what=""):
    x, lse, tgt, top, mx, B = orc
    n = len(r.lse) if rows is None else rows
    assert len(r.lse) == len(r.top) == len(r.top_logit) == len(r.target_logit) == n
    assert np.isfinite(r.lse).all() and np.isfinite(r.top_logit).all()
    assert np.isfinite(r.target_logit[:-1]).all() and np.isnan(r.target_logit[-1])
    d_t = float(np.abs(r.target_logit[:-1] - tgt[:n - 1]).max())
    d_v = float(np.abs(r.top_logit - mx[:n]).max())
    d_l = float(np.abs(r.lse - lse[:n]).max())
    d_p = float(np.abs(r.logprobs - (tgt[:n - 1] - lse[:n - 1])).max())
    picked = x[np.arange(n), r.top]
    d_a = float((mx[:n] - picked).max())
    print(f"{what}: max |diff| target {d_t:.4g} top logit {d_v:.4g} lse {d_l:.4g} logprob "
          f"{d_p:.4g}; oracle max - oracle[top] {d_a:.4g}; B {B:.4g}; argmax agrees on "
          f"{int((r.top == top[:n]).sum())}/{n} rows")
    assert np.allclose(r.target_logit[:-1], tgt[:n - 1], **TOL)
    assert np.allclose(r.top_logit, mx[:n], **TOL)
    assert d_l <= B and d_p <= 2 * B
    assert (picked >= mx[:n] - 2 * B).all()
    assert (0 <= r.top).all() and (r.top < x.shape[1]).all()


def _close(a, b, B, what=""):
    """Two engine results within the bounds of each other (same rows)."""
    n = min(len(a.lse), len(b.lse))
    d_l = float(np.abs(a.lse[:n] - b.lse[:n]).max())
    d_v = float(np.abs(a.top_logit[:n] - b.top_logit[:n]).max())
    d_t = float(np.abs(a.target_logit[:n - 1] - b.target_logit[:n - 1]).max())
    print(f"{what}: max |diff| lse {d_l:.4g} top logit {d_v:.4g} target {d_t:.4g}")
    assert np.allclose(a.target_logit[:n - 1], b.target_logit[:n - 1], **TOL)
    assert np.allclose(a.top_logit[:n], b.top_logit[:n], **TOL)
    assert d_l <= B


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_score_matches_the_oracle(cuda, grid, dtype):
    _check_against_oracle(_score16(grid, dtype), _oracle(grid, dtype), what=dtype)


def test_output_consistency(cuda, grid):
    r = _score16(grid)
    n = len(LONG)
    assert r.lse.dtype == np.float32 and r.top.dtype == np.int32
    assert r.logprobs.dtype == np.float64 and r.logprobs.shape == (n - 1,)
    want = r.target_logit[:-1].astype(np.float64) - r.lse[:-1].astype(np.float64)
    assert np.array_equal(r.logprobs, want)
    assert abs(r.nll + r.logprobs.mean()) <= 1e-12 * max(1.0, abs(r.nll))
    assert abs(r.ppl - np.exp(r.nll)) <= 1e-12 * r.ppl
    assert r.top1 == sum(int(r.top[i]) == LONG[i + 1] for i in range(n - 1)) / (n - 1)
    assert (r.top_logit[:-1] >= r.target_logit[:-1]).all() and (r.lse >= r.top_logit).all()


def test_chunk_widths_agree(cuda, grid):
    orc = _oracle(grid, "bf16")
    base = _score16(grid)
    eng = _engine(grid, dtype="bf16")
    for vc in (256, 768, 2048):     # 768: the last chunk is partial (V = 2048)
        r = eng.score(LONG, vchunk=vc)
        _check_against_oracle(r, orc, what=f"vchunk {vc}")
        _close(r, base, orc[5], f"vchunk {vc} vs default")
    eng.close()


def test_prefix_rows(cuda, grid):
    """score(tokens[:17]) is rows [0, 17) of score(tokens): a misaligned target or row shows."""
    orc = _oracle(grid, "bf16")
    eng = _engine(grid, dtype="bf16")
    r = eng.score(LONG[:17])
    eng.close()
    assert np.isnan(r.target_logit[16])
    _close(r, _score16(grid), orc[5], "prefix 17")
    # rows [0, 16) have the same targets; the oracle's row 16 target differs, so check by hand
    x, lse, tgt, top, mx, B = orc
    assert np.allclose(r.target_logit[:16], tgt[:16], **TOL)
    assert float(np.abs(r.lse - lse[:17]).max()) <= B


def test_last_row_against_prefill_logits(cuda, grid):
    """Row n - 1 differs from prefill_logits only by the 16-bit rounding of the normed row."""
    B = _oracle(grid, "bf16")[5]
    eng = _engine(grid, dtype="bf16")
    pl = eng.prefill_logits(LONG).astype(np.float64)
    eng.close()
    r = _score16(grid)
    lse = float(S.lse_ref(pl[None, :], np.array([-1]))[0][0])
    print(f"last row: lse {r.lse[-1]:.6g} vs prefill_logits {lse:.6g}; top logit "
          f"{r.top_logit[-1]:.6g} vs {pl.max():.6g}")
    assert abs(float(r.lse[-1]) - lse) <= B
    assert np.allclose(r.top_logit[-1], pl.max(), **TOL)
    assert pl[r.top[-1]] >= pl.max() - 2 * B


@pytest.fixture(scope="module")
def grid4(tmp_path_factory):
    """The tiny checkpoint whose projections and head are mxfp4 grid matrices: weights="mxfp4"
    with head="mxfp4" hold the 16-bit engine's weights bit for bit.  (The fp8 grid of `grid`
    has three mantissa bits, so mxfp4 is lossy there.)"""
    import _mxfp4
    import _qhead
    d = tmp_path_factory.mktemp("score_grid4")
    return _qhead.write_grid_head_checkpoint(d, "mxfp4", base=_mxfp4.write_grid_checkpoint(d))


def _score_once(path, **kw):
    eng = _engine(path, dtype="bf16", **kw)
    r = eng.score(LONG)
    eng.close()
    return r


def test_lossless_mxfp4_scores_as_the_16bit_engine(cuda, grid4):
    base = _score_once(grid4)
    B = _oracle(grid4, "bf16")[5]
    _check_against_oracle(base, _oracle(grid4, "bf16"), what="16-bit on the mxfp4 grid")
    q = _score_once(grid4, weights="mxfp4", head="mxfp4")
    _close(q, base, B, "weights=mxfp4 head=mxfp4 vs 16-bit (lossless)")
    assert abs(q.nll - base.nll) <= 2 * B
    _check_against_oracle(q, _oracle(grid4, "bf16"), what="mxfp4 on the mxfp4 grid")


def test_lossy_formats_give_finite_scores_near_the_16bit_engine(cuda, grid):
    """Every storage mode scores; nll within 2B of the 16-bit engine's.  The distances are
    printed and not bounded more tightly: the gap is the format's own error."""
    B = _oracle(grid, "bf16")[5]
    base = _score16(grid)
    for kw in (dict(weights="fp8", head="fp8", kv="fp8", prefill="fp8"),
               dict(weights="mxfp4", head="mxfp4"), dict(weights="fp8", head="mxfp4", kv="fp8")):
        q = _score_once(grid, **kw)
        print(f"{kw}: nll {q.nll:.6g} vs 16-bit {base.nll:.6g} (gap {abs(q.nll - base.nll):.4g}, "
              f"2B {2 * B:.4g}); max |lse diff| {float(np.abs(q.lse - base.lse).max()):.4g}; "
              f"top agreement {float((q.top == base.top).mean()):.3f}")
        assert np.isfinite(q.lse).all() and np.isfinite(q.logprobs).all()
        assert np.isfinite(q.top_logit).all() and np.isnan(q.target_logit[-1])
        assert abs(q.nll - base.nll) <= 2 * B


def test_tied_embeddings(cuda, tmp_path):
    """The head is the embedding table (16-bit), or its quantised copy (head="fp8")."""
    import _qhead
    tied = _qhead.write_tied_grid_checkpoint(tmp_path, "fp8")   # no lm_head tensor in the file
    orc = _oracle(tied, "bf16")
    _check_against_oracle(_score_once(tied), orc, what="tied 16-bit")
    q = _score_once(tied, head="fp8")
    assert np.isfinite(q.lse).all() and np.isfinite(q.nll)
    print(f"tied head=fp8: nll {q.nll:.6g}")


def test_engine_state_after_score(cuda, grid):
    fresh = _engine(grid, dtype="bf16")
    want = fresh.generate(PROMPT, 24, repeat_penalty=1.0).tokens
    fresh.close()
    eng = _engine(grid, dtype="bf16")
    before = (eng.weight_bytes(), eng.kv_bytes())
    a = eng.score(LONG)
    assert (eng.weight_bytes(), eng.kv_bytes()) == before
    assert eng.generate(PROMPT, 24, repeat_penalty=1.0).tokens == want
    b = eng.score(LONG)          # and scoring after a generation repeats itself
    assert np.array_equal(a.lse, b.lse) and np.array_equal(a.top, b.top)
    assert eng.generate(PROMPT, 24, repeat_penalty=1.0).tokens == want
    eng.close()


def test_refusals(cuda, grid):
    eng = _engine(grid, dtype="bf16", max_seq=64)
    with pytest.raises(ValueError, match="at least 2"):
        eng.score([1])
    import ctypes as C

    from cake_amd.engine import lib
    one = (C.c_int32 * 1)(1)
    f, i = (C.c_float * 1)(), (C.c_int32 * 1)()
    err = C.create_string_buffer(256)
    assert lib().cake_engine_score(eng._h, one, 1, 0, f, f, i, f, err, len(err)) != 0
    assert "at least 2" in err.value.decode()
    with pytest.raises(RuntimeError, match="max_seq"):
        eng.score([1] + [5] * 64)
    with pytest.raises(RuntimeError, match="outside"):
        eng.score([1, 2048, 3])
    with pytest.raises(RuntimeError, match="outside"):
        eng.score([1, -1, 3])
    for bad in (-1, 100):
        with pytest.raises(RuntimeError, match="vchunk"):
            eng.score(LONG, vchunk=bad)
    ok = eng.score(LONG)         # the engine still works after the refusals
    assert np.isfinite(ok.lse).all()
    eng.close()
    worker = _engine(grid, dtype="bf16", layers=[0, 1, 2])
    with pytest.raises(RuntimeError, match="head"):
        worker.score(LONG)
    worker.close()


def test_pipeline_rank0_scores(cuda, grid, tmp_path):
    """Two ranks sharing the GPU (the pattern of tests/test_engine_gpu.py): rank 0's score is
    within the bounds of the single-rank engine's."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    addr = f"127.0.0.1:{s.getsockname()[1]}"
    s.close()
    rank0 = ("import sys, json; sys.path.insert(0, %r)\n"
             "from cake_amd.engine import NativeLlama\n"
             "e = NativeLlama(%r, max_seq=256, dtype='bf16', rank=0, world=2, master_addr=%r)\n"
             "r = e.score(%r)\n"
             "g = e.generate(%r, 8, repeat_penalty=1.0).tokens\n"
             "e.close()\n"
             "print(json.dumps({'lse': r.lse.tolist(), 'tgt': r.target_logit[:-1].tolist(),\n"
             "                  'top': r.top.tolist(), 'topv': r.top_logit.tolist(),\n"
             "                  'layers': [e.first_layer, e.end_layer], 'gen': g}), flush=True)\n"
             ) % (ROOT, str(grid), addr, LONG, PROMPT)
    rank1 = ("import sys; sys.path.insert(0, %r)\n"
             "from cake_amd.engine import NativeLlama\n"
             "e = NativeLlama(%r, max_seq=256, dtype='bf16', rank=1, world=2, master_addr=%r)\n"
             "e.serve()\n"
             "e.close()\n") % (ROOT, str(grid), addr)
    logs = [tmp_path / "rank0.log", tmp_path / "rank1.log"]
    procs = [subprocess.Popen([sys.executable, "-c", c], stdout=subprocess.PIPE,
                              stderr=open(lg, "w"), text=True)
             for c, lg in ((rank0, logs[0]), (rank1, logs[1]))]
    try:
        out0, _ = procs[0].communicate(timeout=240)
        procs[1].wait(timeout=60)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    msg = "\n".join(f"---- {lg.name} ----\n" + lg.read_text()[-3000:] for lg in logs)
    assert procs[0].returncode == 0 and procs[1].returncode == 0, msg
    got = json.loads(out0.strip().splitlines()[-1])
    assert got["layers"][0] == 0 and got["layers"][1] < 3
    base, B = _score16(grid), _oracle(grid, "bf16")[5]
    assert np.allclose(got["tgt"], base.target_logit[:-1], **TOL)
    assert np.allclose(got["topv"], base.top_logit, **TOL)
    assert float(np.abs(np.array(got["lse"]) - base.lse).max()) <= B
    x, mx = _oracle(grid, "bf16")[0], _oracle(grid, "bf16")[4]
    assert (x[np.arange(len(LONG)), np.array(got["top"])] >= mx - 2 * B).all()
    single = _engine(grid, dtype="bf16")
    assert got["gen"] == single.generate(PROMPT, 8, repeat_penalty=1.0).tokens
    single.close()


def test_cake_cli_score_file(cuda, grid, tmp_path):
    """cake-cli --score-file prints one JSON line equal to NativeLlama.score on the same ids;
    a file longer than --max-seq-len is scored in several windows."""
    from cake_amd.native_bridge import score_file_tokens, score_summary, score_windows
    cli = os.path.join(ROOT, "cake_amd", "lib", "cake-cli")
    short = tmp_path / "short.txt"
    short.write_text("the quick brown fox jumps over the lazy dog", encoding="utf-8")
    long_ = tmp_path / "long.txt"
    long_.write_text("so it goes, on and on, over the hills and far away. " * 12,
                     encoding="utf-8")
    eng = _engine(grid, dtype="bf16", max_seq=64)
    for path in (short, long_):
        ids = score_file_tokens(str(grid), str(path))
        assert ids[0] == 1 and len(ids) >= 2
        wins = score_windows(len(ids), 64)
        want = score_summary(len(ids), [(ids[a:b], eng.score(ids[a:b])) for a, b in wins])
        r = subprocess.run([cli, "--model", str(grid), "--topology", str(tmp_path / "none.yml"),
                            "--dtype", "bf16", "--max-seq-len", "64", "--score-file", str(path)],
                           capture_output=True, text=True, timeout=300, cwd=ROOT,
                           env=dict(os.environ, CAKE_LOG="warning"))
        assert r.returncode == 0, r.stderr[-3000:]
        assert "native engine" in r.stderr
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, r.stdout
        got = json.loads(lines[0])
        print(path.name, got)
        assert set(got) == {"tokens", "scored", "windows", "nll", "ppl", "top1"}
        assert got["tokens"] == len(ids) and got["windows"] == len(wins)
        assert got["scored"] == want["scored"] == sum(b - a - 1 for a, b in wins)
        for k in ("nll", "ppl", "top1"):
            assert abs(got[k] - want[k]) <= 1e-9 * max(1.0, abs(want[k])), (k, got[k], want[k])
        if path is long_:
            assert len(ids) > 64 and got["windows"] > 1
    eng.close()
