"""Log-probs of generated tokens: NativeLlama.generate(..., logprobs=K), cake_engine_logprobs
and cake-cli --logprobs-file on the GPU.

Oracle: ``forced_logits(prompt, tokens[:-1])`` runs the same decode kernels eagerly; row i, after
a host repeat penalty where one is set (2.0: ``/ p`` and ``* p`` are exact in f32), goes through
``ops/reference.py::logprob_topk_ref``.  Required: ids equal, ``logit`` and ``top_logits``
bit-equal to the forced logits, ``|lse - ref64| <= 2^-24 (|ref64| + 128)``, record id ==
token.  max_seq 256 and short contexts keep decode attention a single split in the eager and
the captured path alike."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import _score as S
from _fp8 import write_grid_checkpoint
from cake_amd.ops import reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROMPT = [1, 17, 300, 5, 99, 1024, 7, 8]
N = 24
FIELDS = ("ids", "logit", "lse", "top_ids", "top_logits")


@pytest.fixture(scope="module")
def grid(tmp_path_factory):
    return write_grid_checkpoint(tmp_path_factory.mktemp("logprobs_grid"))


def _engine(path, **kw):
    from cake_amd.engine import NativeLlama
    return NativeLlama(path, max_seq=kw.pop("max_seq", 256), dtype="bf16", **kw)


def _bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check(eng, tokens, lp, K, penalty=1.0, last_n=0, prompt=PROMPT, what=""):
    """lp (TokenLogprobs of `tokens`) against the oracle; returns the number of tokens that
    are not their row's argmax."""
    n = len(tokens)
    assert n > 0 and lp.ids.tolist() == list(tokens), what
    assert lp.top_ids.shape == lp.top_logits.shape == lp.top_logprobs.shape == (n, K), what
    assert lp.logprob.dtype == np.float64 and lp.top_logprobs.dtype == np.float64
    fl = eng.forced_logits(prompt, list(tokens[:-1]))
    worst, off_argmax = 0.0, 0
    for i in range(n):
        x = torch.from_numpy(fl[i])
        if penalty != 1.0:
            x = R.apply_repeat_penalty(x, penalty, (prompt + list(tokens[:i]))[-last_n:])
        ref = R.logprob_topk_ref(x, tokens[i], K)
        w = f"{what} token {i}"
        assert _bits(lp.logit[i])[()] == _bits(ref["logit"].numpy())[()], w
        assert np.array_equal(lp.top_ids[i], ref["top_ids"].numpy()), w
        assert np.array_equal(_bits(lp.top_logits[i]), _bits(ref["top_logits"].numpy())), w
        ratio = abs(float(lp.lse[i]) - ref["lse"]) / float(S.lse_bound(np.float64(ref["lse"])))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (w, ratio)
        assert lp.logprob[i] == float(lp.logit[i]) - float(lp.lse[i]), w
        assert np.array_equal(lp.top_logprobs[i],
                              lp.top_logits[i].astype(np.float64) - float(lp.lse[i])), w
        off_argmax += int(tokens[i] != int(torch.argmax(x)))
    print(f"{what}: {n} tokens, lse error / bound worst {worst:.3f}, off-argmax {off_argmax}")
    return off_argmax


def test_greedy_no_penalty(cuda, grid):
    eng = _engine(grid)
    r = eng.generate(PROMPT, N, repeat_penalty=1.0, logprobs=20)
    assert _check(eng, r.tokens, r.logprobs, 20, what="greedy") == 0
    assert (r.logprobs.top_ids[:, 0] == r.logprobs.ids).all()
    eng.close()


@pytest.mark.parametrize("last_n", [64, 300])   # the fused tail; the unfused tail
def test_greedy_penalty(cuda, grid, last_n):
    eng = _engine(grid)
    r = eng.generate(PROMPT, N, repeat_penalty=2.0, repeat_last_n=last_n, logprobs=5)
    _check(eng, r.tokens, r.logprobs, 5, penalty=2.0, last_n=last_n, what=f"penalty last_n {last_n}")
    eng.close()


def test_sampling(cuda, grid):
    eng = _engine(grid)
    kw = dict(temperature=0.8, top_k=40, top_p=0.9, seed=1234, repeat_penalty=1.0)
    r = eng.generate(PROMPT, N, logprobs=20, **kw)
    off = _check(eng, r.tokens, r.logprobs, 20, what="sampling")
    assert off >= 1            # the record follows the drawn token, not the argmax
    eng.close()


def test_tokens_do_not_depend_on_logprobs(cuda, grid):
    eng = _engine(grid)
    for kw in (dict(repeat_penalty=1.0), dict(repeat_penalty=1.1, repeat_last_n=64),
               dict(temperature=0.8, top_k=40, top_p=0.9, seed=7, repeat_penalty=1.0)):
        off = eng.generate(PROMPT, N, **kw)
        assert off.logprobs is None
        k20 = eng.generate(PROMPT, N, logprobs=20, **kw)
        k0 = eng.generate(PROMPT, N, logprobs=0, **kw)
        assert off.tokens == k20.tokens == k0.tokens
        assert k0.logprobs.top_ids.shape == (N, 0)
        assert np.array_equal(_bits(k0.logprobs.logit), _bits(k20.logprobs.logit))
        assert np.array_equal(_bits(k0.logprobs.lse), _bits(k20.logprobs.lse))
    eng.close()


def test_steps_per_graph(cuda, grid):
    recs = []
    for k in (1, 4):
        eng = _engine(grid, steps_per_graph=k)
        recs.append(eng.generate(PROMPT, N, repeat_penalty=2.0, repeat_last_n=64, logprobs=20))
        eng.close()
    a, b = recs
    assert a.tokens == b.tokens
    for f in FIELDS:
        assert getattr(a.logprobs, f).tobytes() == getattr(b.logprobs, f).tobytes(), f


def test_continue(cuda, grid):
    eng = _engine(grid)
    whole = eng.generate(PROMPT, 12, repeat_penalty=1.0, logprobs=5)
    head = eng.generate(PROMPT, 5, repeat_penalty=1.0, logprobs=5)
    tail = eng.continue_(7)
    assert head.tokens + tail.tokens == whole.tokens
    assert len(tail.logprobs.ids) == 7
    for f in FIELDS:
        got = np.concatenate([getattr(head.logprobs, f), getattr(tail.logprobs, f)])
        assert got.tobytes() == getattr(whole.logprobs, f).tobytes(), f
    eng.close()


def test_token_logprob_inside_callback(cuda, grid):
    eng = _engine(grid)
    seen = []

    def on_token(t):
        i = len(seen)
        cur = eng.token_logprob(i)
        assert int(cur.ids[0]) == t
        if i:
            assert eng.token_logprob(i - 1).logit[0] == seen[i - 1].logit[0]
        with pytest.raises(RuntimeError):
            eng.token_logprob(i + 1)       # not reported yet
        seen.append(cur)
        return False

    r = eng.generate(PROMPT, N, repeat_penalty=1.0, logprobs=5, on_token=on_token)
    assert len(seen) == N
    for f in FIELDS + ("logprob", "top_logprobs"):
        got = np.concatenate([getattr(s, f) for s in seen])
        assert got.tobytes() == getattr(r.logprobs, f).tobytes(), f
    eng.close()


@pytest.mark.parametrize("kw", [dict(head="fp8"), dict(weights="mxfp4", kv="fp8")],
                         ids=["head-fp8", "w-mxfp4-kv-fp8"])
def test_formats(cuda, grid, kw):
    eng = _engine(grid, **kw)
    r = eng.generate(PROMPT, N, repeat_penalty=1.0, logprobs=20)
    _check(eng, r.tokens, r.logprobs, 20, what=str(kw))
    eng.close()


def test_switching_and_memory(cuda, grid):
    eng = _engine(grid)
    mem = (eng.weight_bytes(), eng.kv_bytes())
    on = eng.generate(PROMPT, N, repeat_penalty=1.0, logprobs=3)
    assert (eng.weight_bytes(), eng.kv_bytes()) == mem
    off = eng.generate(PROMPT, N, repeat_penalty=1.0)
    assert off.logprobs is None and off.tokens == on.tokens
    with pytest.raises(RuntimeError):
        eng.token_logprob(0)
    again = eng.generate(PROMPT, N, repeat_penalty=1.0, logprobs=3)
    assert again.tokens == on.tokens
    for f in FIELDS:
        assert getattr(again.logprobs, f).tobytes() == getattr(on.logprobs, f).tobytes(), f
    assert (eng.weight_bytes(), eng.kv_bytes()) == mem
    eng.close()


def test_refusals(cuda, grid):
    import ctypes as C

    from cake_amd.engine import lib
    eng = _engine(grid)
    with pytest.raises(ValueError, match="20"):
        eng.generate(PROMPT, 4, logprobs=21)
    err = C.create_string_buffer(256)
    assert lib().cake_engine_set_logprobs(eng._h, 21, err, len(err)) != 0
    assert "20" in err.value.decode()
    assert len(eng.generate(PROMPT, 4, repeat_penalty=1.0, logprobs=2).logprobs.ids) == 4
    eng.close()
    worker = _engine(grid, layers=[0, 1, 2])
    with pytest.raises(RuntimeError, match="head"):
        worker.set_logprobs(5)
    worker.close()


def test_remote_worker_master(cuda, grid, tmp_path):
    """The master of a TCP worker decodes eagerly; its records against forced_logits."""
    from test_engine_gpu import _port, _wait_listen
    cli = os.path.join(ROOT, "cake_amd", "lib", "cake-cli")
    port = _port()
    topo = tmp_path / "topology.yml"
    topo.write_text(f"w1:\n  host: '127.0.0.1:{port}'\n  layers:\n    - 'model.layers.1'\n")
    w = subprocess.Popen([cli, "--mode", "worker", "--name", "w1", "--model", str(grid),
                          "--topology", str(topo), "--address", f"127.0.0.1:{port}",
                          "--max-seq-len", "256"], cwd=ROOT,
                         env=dict(os.environ, CAKE_LOG="warning"),
                         stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    eng = None
    try:
        _wait_listen(w, port, "worker w1")
        eng = _engine(grid, workers=[f"127.0.0.1:{port}"], worker_of=[-1, 0, -1],
                      remote_timeout_s=30.0)
        r = eng.generate(PROMPT, 10, repeat_penalty=2.0, repeat_last_n=64, logprobs=20)
        t = eng.continue_(4)
        assert len(t.logprobs.ids) == len(t.tokens) == 4
        both = type(r.logprobs)(*[np.concatenate([getattr(r.logprobs, f), getattr(t.logprobs, f)])
                                  for f in ("ids", "logit", "lse", "logprob", "top_ids",
                                            "top_logits", "top_logprobs")])
        _check(eng, r.tokens + t.tokens, both, 20, penalty=2.0, last_n=64, what="remote master")
    finally:
        if eng is not None:
            eng.close()
        if w.poll() is None:
            w.kill()
        w.communicate()


def test_cake_cli_logprobs_file(cuda, grid, tmp_path):
    """cake-cli --logprobs-file writes one JSON line per generated token, equal to
    NativeLlama's records for the same prompt ids and sampling."""
    from cake_amd.native_bridge import encode_chat
    cli = os.path.join(ROOT, "cake_amd", "lib", "cake-cli")
    out = tmp_path / "lp.jsonl"
    system, prompt = "You are a helpful AI assistant.", "the quick brown fox"
    r = subprocess.run([cli, "--model", str(grid), "--topology", str(tmp_path / "none.yml"),
                        "--dtype", "bf16", "--max-seq-len", "256", "--system-prompt", system,
                        "--prompt", prompt, "-n", "12", "--temperature", "0",
                        "--repeat-penalty", "1.0", "--logprobs-file", str(out),
                        "--top-logprobs", "5"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT,
                       env=dict(os.environ, CAKE_LOG="warning"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "native engine" in r.stderr
    lines = [json.loads(ln) for ln in out.read_text().splitlines() if ln.strip()]
    enc = json.loads(encode_chat(json.dumps({"model": str(grid), "system": system,
                                             "prompt": prompt})))
    eng = _engine(grid)
    want = eng.generate(enc["ids"], 12, repeat_penalty=1.0, eos_ids=enc["eos"], logprobs=5)
    eng.close()
    assert len(lines) == len(want.tokens) >= 1
    for i, ln in enumerate(lines):
        assert set(ln) == {"index", "id", "logprob", "top_ids", "top_logprobs"}
        assert ln["index"] == i and ln["id"] == want.tokens[i]
        assert ln["logprob"] == float(want.logprobs.logprob[i])
        assert ln["top_ids"] == want.logprobs.top_ids[i].tolist()
        assert ln["top_logprobs"] == want.logprobs.top_logprobs[i].tolist()
