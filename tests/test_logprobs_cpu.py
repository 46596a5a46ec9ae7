"""Log-probs of generated tokens: the CPU side (the oracle, the loop / engine surfaces, the REST
field with a fake generator, the CLI refusals)."""
import ctypes as C
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from _fp8 import write_grid_checkpoint
from cake_amd.models.base import Token
from cake_amd.ops.reference import logprob_topk_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cake_amd", "lib", "cake-cli")


# ---------------------------------------------------------------- logprob_topk_ref
@pytest.mark.parametrize("V,k", [(1, 1), (37, 5), (1000, 20), (2048, 0)])
def test_ref_against_log_softmax_and_topk(V, k):
    g = torch.Generator().manual_seed(V + k)
    x = (torch.randn(V, generator=g) * 7).float()
    assert x.unique().numel() == V          # tie free
    ls = torch.log_softmax(x.double(), 0)
    for tok in (0, V - 1, V // 2):
        r = logprob_topk_ref(x, tok, k)
        assert r["id"] == tok and r["logit"].dtype == torch.float32
        assert r["logit"].view(torch.int32) == x[tok].view(torch.int32)
        assert abs(r["logprob"] - float(ls[tok])) <= 1e-12 * max(1.0, abs(float(ls[tok])))
        n = min(k, V)
        tv, ti = torch.topk(x, n)
        assert r["top_ids"][:n].tolist() == ti.tolist() and r["top_ids"].dtype == torch.int32
        assert torch.equal(r["top_logits"][:n].view(torch.int32), tv.view(torch.int32))
        assert torch.allclose(r["top_logprobs"][:n], ls[ti], rtol=0, atol=1e-12)
        assert r["top_logprobs"].dtype == torch.float64


def test_ref_ties_take_the_lower_id():
    r = logprob_topk_ref(torch.full((50,), 0.25), 49, 20)
    assert r["top_ids"].tolist() == list(range(20))
    x = torch.zeros(50)
    x[[40, 7, 23]] = 3.0
    assert logprob_topk_ref(x, 0, 5)["top_ids"].tolist() == [7, 23, 40, 0, 1]


def test_ref_k_larger_than_v():
    x = torch.tensor([0.5, 2.0, -1.0])
    r = logprob_topk_ref(x, 1, 20)
    assert r["top_ids"].tolist() == [1, 0, 2] + [-1] * 17
    assert torch.isneginf(r["top_logits"][3:]).all() and torch.isneginf(r["top_logprobs"][3:]).all()
    for bad in (-1, 21):
        with pytest.raises(ValueError):
            logprob_topk_ref(x, 0, bad)


def test_ref_minus_inf_rows():
    ninf = float("-inf")
    x = torch.full((10,), ninf)
    r = logprob_topk_ref(x, 3, 4)
    assert r["lse"] == ninf and r["logprob"] == ninf and r["top_ids"].tolist() == [0, 1, 2, 3]
    assert not torch.isnan(r["top_logprobs"]).any()
    x[6] = 1.5
    r = logprob_topk_ref(x, 6, 3)
    assert r["lse"] == 1.5 and r["logprob"] == 0.0 and r["top_ids"].tolist() == [6, 0, 1]
    assert r["top_logprobs"].tolist() == [0.0, ninf, ninf]
    assert logprob_topk_ref(x, 0, 0)["logprob"] == ninf


# ---------------------------------------------------------------- loop / engine surfaces
def test_loop_spec_gains_three_trailing_fields():
    from cake_amd.ops.graph_loop import LoopSpec
    names = [f[0] for f in LoopSpec._fields_]
    assert names[-3:] == ["rec", "rec_bytes", "out_rec"]
    old = {"execs": 0, "n_execs": 8, "bucket_of": 16, "n_len": 24, "k": 28, "hist": 32,
           "base": 40, "pos": 44, "n": 48, "chunk": 52, "eos": 56, "n_eos": 64, "on_token": 72,
           "token_ctx": 80, "announce": 88, "announce_ctx": 96, "stream": 104,
           "out_tokens": 112, "out_ms": 120, "out_cap": 128}
    assert names[:-3] == list(old)
    for n, off in old.items():
        assert getattr(LoopSpec, n).offset == off, n
    assert LoopSpec.rec.offset == 136 and LoopSpec.rec_bytes.offset == 144
    assert LoopSpec.out_rec.offset == 152 and C.sizeof(LoopSpec) == 160
    src = open(os.path.join(ROOT, "cake_amd", "csrc", "driver", "graph_loop.h")).read()
    tail = src[src.index("int32_t out_cap;"):src.index("struct CakeLoopResult")]
    assert tail.index("const void* rec;") < tail.index("int32_t rec_bytes;") < tail.index(
        "void* out_rec;")


def test_engine_surface():
    from cake_amd.engine import EngineOpts, EngineSampling, GenResult, lib
    assert C.sizeof(EngineOpts) == 40 and C.sizeof(EngineSampling) == 32
    L = lib()
    assert L.cake_engine_set_logprobs.argtypes is not None
    assert len(L.cake_engine_logprobs.argtypes) == 10
    r = GenResult([1, 2], 3, 0.1, 0.2, 10.0, 1.0, 2.0)     # positional construction as before
    assert r.logprobs is None and r.p99_ms == 2.0
    t = Token(5, "x", False)
    assert t.logprob is None and t.top_logprobs is None


def test_native_llama_rejects_bad_k_before_the_engine():
    from cake_amd.engine import NativeLlama
    eng = NativeLlama.__new__(NativeLlama)   # no engine: nothing may be touched
    eng._h = None
    for bad in (-1, 21, 100):
        with pytest.raises(ValueError, match="20"):
            eng.set_logprobs(bad)


# ---------------------------------------------------------------- REST
class FakeTokenizer:
    def decode(self, ids, skip_special_tokens=False):
        return {7: "é", 9: ""}.get(ids[0], f"<{ids[0]}>")


class PlainLLM:
    """Five tokens, the last an EOS; no set_logprobs (as the Python engines)."""
    MODEL_NAME = "llama3"
    IDS = [3, 7, 9, 4, 2]

    def __init__(self):
        self.tokenizer = FakeTokenizer()
        self.k = None
        self.calls = []

    def add_message(self, m):
        pass

    def reset(self):
        pass

    def generated_tokens(self):
        return len(self.IDS)

    def stream(self, n, on_token, stop_at_eos=True):
        for i, tid in enumerate(self.IDS[:n]):
            t = Token(tid, self.tokenizer.decode([tid]), tid == 2)
            if self.k is not None:
                t.logprob = float("-inf") if tid == 4 else -0.5 * (i + 1)
                t.top_logprobs = [(tid, t.logprob), (11, float("-inf")), (12, -3.0)][:self.k]
            on_token(t)


class FakeLLM(PlainLLM):
    """The same with log-probs on its tokens after set_logprobs(k)."""

    def set_logprobs(self, k):
        self.calls.append(k)
        self.k = k


def _client(llm):
    from fastapi.testclient import TestClient

    from cake_amd.api.server import create_app
    from cake_amd.master import Master
    ctx = types.SimpleNamespace(args=types.SimpleNamespace(sample_len=8, metrics=None, trace=None),
                                sampling=None)
    return TestClient(create_app(Master(ctx, llm=llm)))


MSGS = [{"role": "user", "content": "hi"}]


def _entries_ok(entries, k):
    assert [e["id"] for e in entries] == [3, 7, 9, 4]          # the EOS emits nothing
    for e in entries:
        assert set(e) == {"token", "id", "logprob", "bytes", "top_logprobs"}
        assert e["bytes"] == list(e["token"].encode("utf-8"))
        assert len(e["top_logprobs"]) == k
        for a in e["top_logprobs"]:
            assert set(a) == {"token", "id", "logprob", "bytes"}
    assert entries[1]["token"] == "é" and entries[1]["bytes"] == [0xC3, 0xA9]
    assert entries[0]["logprob"] == -0.5 and entries[2]["logprob"] == -1.5
    assert entries[3]["logprob"] == -9999.0                     # -inf has no JSON form
    if k >= 2:
        assert entries[0]["top_logprobs"][1] == {"token": "<11>", "id": 11, "logprob": -9999.0,
                                                 "bytes": list(b"<11>")}


@pytest.mark.parametrize("k", [0, 3])
def test_api_non_stream(k):
    llm = FakeLLM()
    c = _client(llm)
    r = c.post("/api/v1/chat/completions",
               json={"messages": MSGS, "logprobs": True, "top_logprobs": k})
    assert r.status_code == 200, r.text
    ch = r.json()["choices"][0]
    assert ch["message"]["content"] == "<3>é<4>"
    _entries_ok(ch["logprobs"]["content"], k)
    assert llm.calls == [k]
    # and a request without the field: no key, and the generator is switched back off
    r = c.post("/api/v1/chat/completions", json={"messages": MSGS})
    assert r.status_code == 200 and "logprobs" not in r.json()["choices"][0]
    assert set(r.json()["choices"][0]) == {"index", "message", "finish_reason"}
    assert llm.calls == [k, None]


def test_api_logprobs_without_top_logprobs_means_zero_alternatives():
    r = _client(FakeLLM()).post("/api/v1/chat/completions",
                                json={"messages": MSGS, "logprobs": True})
    _entries_ok(r.json()["choices"][0]["logprobs"]["content"], 0)


def test_api_stream():
    c = _client(FakeLLM())
    r = c.post("/api/v1/chat/completions",
               json={"messages": MSGS, "stream": True, "logprobs": True, "top_logprobs": 2})
    lines = [ln for ln in r.text.splitlines() if ln.startswith("data: ")]
    assert lines[-1] == "data: [DONE]"
    chunks = [json.loads(ln[6:]) for ln in lines[:-1]]
    assert len(chunks) == 4
    for ch in chunks:
        assert len(ch["choices"][0]["logprobs"]["content"]) == 1
        assert ch["choices"][0]["delta"]["content"] == ch["choices"][0]["logprobs"]["content"][0]["token"]
    _entries_ok([ch["choices"][0]["logprobs"]["content"][0] for ch in chunks], 2)
    r = c.post("/api/v1/chat/completions", json={"messages": MSGS, "stream": True})
    chunks = [json.loads(ln[6:]) for ln in r.text.splitlines()
              if ln.startswith("data: ") and ln != "data: [DONE]"]
    assert len(chunks) == 4 and all("logprobs" not in ch["choices"][0] for ch in chunks)
    assert all(set(ch["choices"][0]) == {"index", "delta", "finish_reason"} for ch in chunks)


def test_api_refusals():
    c = _client(FakeLLM())
    for bad in ({"top_logprobs": 3}, {"logprobs": False, "top_logprobs": 3},
                {"logprobs": True, "top_logprobs": 21}, {"logprobs": True, "top_logprobs": -1},
                {"logprobs": True, "top_logprobs": 2.5}, {"logprobs": True, "top_logprobs": "3"},
                {"logprobs": True, "top_logprobs": True}):
        r = c.post("/api/v1/chat/completions", json=dict(messages=MSGS, **bad))
        assert r.status_code == 400, bad
        assert "top_logprobs" in r.json()["error"]
    plain = _client(PlainLLM())
    r = plain.post("/api/v1/chat/completions", json={"messages": MSGS, "logprobs": True})
    assert r.status_code == 400 and "native engine" in r.json()["error"]
    r = plain.post("/api/v1/chat/completions", json={"messages": MSGS})
    assert r.status_code == 200 and "logprobs" not in r.json()["choices"][0]


# ---------------------------------------------------------------- CLI
@pytest.fixture(scope="module")
def grid(tmp_path_factory):
    return write_grid_checkpoint(tmp_path_factory.mktemp("logprobs_grid"))


def _run(cmd, **env):
    e = dict(os.environ, CAKE_LOG="warning", **env)
    return subprocess.run(cmd, capture_output=True, text=True, timeout=180, env=e, cwd=ROOT)


def _entry(entry):
    return [CLI] if entry == "cake-cli" else [sys.executable, "-m", "cake_amd.cli"]


@pytest.mark.parametrize("entry", ["cake-cli", "python"])
def test_cli_lists_the_flags(entry):
    r = _run([*_entry(entry), "--help"])
    assert r.returncode == 0 and "--logprobs-file" in r.stdout and "--top-logprobs" in r.stdout


@pytest.mark.parametrize("entry", ["cake-cli", "python"])
@pytest.mark.parametrize("extra,word", [(["--top-logprobs", "3"], "--logprobs-file"),
                                        (["--logprobs-file", "LP", "--top-logprobs", "21"], "[0, 20]"),
                                        (["--logprobs-file", "LP", "--top-logprobs", "-1"], "[0, 20]")])
def test_cli_flag_pair_refusals(grid, tmp_path, entry, extra, word):
    lp = tmp_path / "lp.jsonl"
    extra = [str(lp) if x == "LP" else x for x in extra]
    r = _run([*_entry(entry), "--model", str(grid), "--topology", str(tmp_path / "none.yml"),
              *extra])
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert "--top-logprobs" in r.stderr and word in r.stderr
    assert r.stdout.strip() == "" and not lp.exists()


@pytest.mark.parametrize("entry", ["cake-cli", "python"])
@pytest.mark.parametrize("how", ["CAKE_NATIVE=0", "--cpu", "--no-graph", "f32", "image"])
def test_cli_refused_on_the_python_engines(grid, tmp_path, entry, how):
    extra, env = [], {}
    if how == "CAKE_NATIVE=0":
        env["CAKE_NATIVE"] = "0"
    elif how == "f32":
        extra = ["--dtype", "f32"]
    elif how == "image":
        extra = ["--model-type", "image-model"]
    else:
        extra = [how]
    lp = tmp_path / "lp.jsonl"
    r = _run([*_entry(entry), "--model", str(grid), "--topology", str(tmp_path / "none.yml"),
              "--logprobs-file", str(lp), "--top-logprobs", "5", *extra], **env)
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert "--logprobs-file" in r.stderr and "native Llama engine" in r.stderr
    assert ("text model only" in r.stderr) == (how == "image")
    assert r.stdout.strip() == "" and not lp.exists()


@pytest.mark.parametrize("entry", ["cake-cli", "python"])
def test_cli_refused_with_tensor_parallel(grid, tmp_path, entry):
    lp = tmp_path / "lp.jsonl"
    r = _run([*_entry(entry), "--model", str(grid), "--topology", str(tmp_path / "none.yml"),
              "--transport", "rccl", "--parallel", "tp", "--logprobs-file", str(lp)],
             WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert "--logprobs-file" in r.stderr and "--parallel tp" in r.stderr
    assert "tensor-parallel" in r.stderr and r.stdout.strip() == "" and not lp.exists()


def test_logprob_json_lines():
    from cake_amd.engine import TokenLogprobs, _logprob, logprob_json_lines
    logit = np.array([1.5, -np.inf], dtype=np.float32)
    lse = np.array([2.0, 2.0], dtype=np.float32)
    tl = np.array([[3.0, -np.inf], [1.0, 0.5]], dtype=np.float32)
    lp = TokenLogprobs(np.array([4, 9], dtype=np.int32), logit, lse, _logprob(logit, lse),
                       np.array([[4, 1], [2, 3]], dtype=np.int32), tl, _logprob(tl, lse[:, None]))
    rows = [json.loads(s) for s in logprob_json_lines(lp)]
    assert rows[0] == {"index": 0, "id": 4, "logprob": -0.5, "top_ids": [4, 1],
                       "top_logprobs": [1.0, float("-inf")]}
    assert rows[1]["logprob"] == float("-inf") and rows[1]["top_logprobs"] == [-1.0, -1.5]
