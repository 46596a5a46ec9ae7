"""Batched decode without a GPU: the REST ``n`` field against a stub generator (validation,
refusals that are never silent, response shape), ``--prompts-file`` in both command-line
front ends, and the ctypes signature of cake_engine_generate_batch."""
import ctypes as C
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest

from cake_amd.models.sampling import SamplingConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cake_amd", "lib", "cake-cli")
MSGS = [{"role": "user", "content": "hello"}]
URL = "/api/v1/chat/completions"


class PythonLLM:
    """What the REST layer sees of a Python generator: one sequence at a time."""
    MODEL_NAME = "llama3"

    def __init__(self):
        self.sampling = None
        self.messages = []

    def set_sampling(self, s):
        self.sampling = s

    def add_message(self, m):
        self.messages.append(m)


class NativeLLM(PythonLLM):
    """... and of the native engine's generator."""

    def __init__(self, refusal=None):
        super().__init__()
        self.refusal = refusal
        self.batches = []

    def set_logprobs(self, k):
        self.logprobs = k

    def set_logit_controls(self, c):
        self.controls = c

    def batch_refusal(self):
        return self.refusal

    def generate_n(self, n, max_tokens):
        self.batches.append((n, max_tokens, self.sampling.seed, len(self.messages)))
        return [(f"text {i}", 3 + i) for i in range(n)]


class StubMaster:
    def __init__(self, llm):
        self.llm = llm
        self.ctx = SimpleNamespace(sampling=SamplingConfig(temperature=0.0, seed=1),
                                   args=SimpleNamespace(sample_len=16))
        self.single = 0

    def reset(self):
        self.llm.messages = []

    def generate_text(self, sink, max_tokens=None, on_token=None):
        self.single += 1
        sink("one")
        return {"generated": 1}


def _client(llm):
    from fastapi.testclient import TestClient
    from cake_amd.api.server import create_app
    m = StubMaster(llm)
    return TestClient(create_app(m)), m


def test_rest_n_choices_and_usage():
    c, m = _client(NativeLLM())
    r = c.post(URL, json={"messages": MSGS, "n": 3, "max_tokens": 5, "seed": 40,
                          "temperature": 0.7})
    assert r.status_code == 200, r.text
    j = r.json()
    assert j["object"] == "chat.completion" and len(j["id"]) == 36
    assert [ch["index"] for ch in j["choices"]] == [0, 1, 2]
    assert [ch["message"] for ch in j["choices"]] == \
        [{"role": "assistant", "content": f"text {i}"} for i in range(3)]
    assert all(ch["finish_reason"] == "stop" for ch in j["choices"])
    assert j["usage"] == {"completion_tokens": 3 + 4 + 5}
    # one batch of 3 with the request's budget and seed (choice i draws with seed + i in the
    # engine), after the request's one message; the single-sequence path did not run
    assert m.llm.batches == [(3, 5, 40, 1)] and m.single == 0
    # no max_tokens: the server's --sample-len
    assert c.post(URL, json={"messages": MSGS, "n": 8}).status_code == 200
    assert m.llm.batches[-1][:2] == (8, 16)


def test_rest_n_absent_or_one_takes_the_single_path():
    c, m = _client(NativeLLM())
    for body in ({"messages": MSGS}, {"messages": MSGS, "n": 1}, {"messages": MSGS, "n": None},
                 {"messages": MSGS, "n": 1, "stream": True}):
        r = c.post(URL, json=body)
        assert r.status_code == 200, r.text
    assert m.single == 4 and m.llm.batches == []
    j = c.post(URL, json={"messages": MSGS, "n": 1}).json()
    assert len(j["choices"]) == 1 and j["choices"][0]["message"]["content"] == "one"


@pytest.mark.parametrize("n", [0, 9, -1, 1.5, "2", True, [2]])
def test_rest_n_out_of_range_is_400(n):
    c, m = _client(NativeLLM())
    r = c.post(URL, json={"messages": MSGS, "n": n})
    assert r.status_code == 400 and "n must be an integer in [1, 8]" in r.json()["error"]
    assert m.single == 0 and m.llm.batches == []


@pytest.mark.parametrize("extra,word", [
    ({"stream": True}, "streamed"),
    ({"logprobs": True}, "logprobs"),
    ({"logprobs": True, "top_logprobs": 2}, "logprobs"),
    ({"presence_penalty": 0.5}, "presence_penalty"),
    ({"frequency_penalty": -0.5}, "frequency_penalty"),
    ({"logit_bias": {"5": 1.0}}, "logit_bias"),
    ({"min_p": 0.1, "temperature": 0.8}, "min_p"),
])
def test_rest_n_with_what_a_batch_cannot_do_is_400(extra, word):
    c, m = _client(NativeLLM())
    r = c.post(URL, json={"messages": MSGS, "n": 2, **extra})
    assert r.status_code == 400 and "n > 1" in r.json()["error"] and word in r.json()["error"]
    assert m.single == 0 and m.llm.batches == []
    assert c.post(URL, json={"messages": MSGS, **extra}).status_code == 200   # n = 1: as before


def test_rest_n_on_engines_that_do_not_batch_is_400():
    c, m = _client(PythonLLM())
    r = c.post(URL, json={"messages": MSGS, "n": 2})
    assert r.status_code == 400 and "native engine" in r.json()["error"]
    assert m.single == 0
    for why in ("a tensor-parallel engine does not batch sequences",
                "a pipeline engine does not batch sequences",
                "an engine with remote workers does not batch sequences"):
        c, m = _client(NativeLLM(refusal=why))
        r = c.post(URL, json={"messages": MSGS, "n": 2})
        assert r.status_code == 400 and why in r.json()["error"]
        assert m.llm.batches == [] and m.single == 0


def test_native_generator_names_the_engines_that_do_not_batch():
    from cake_amd.models.llama3.native_generator import NativeLLM as Real
    base = dict(tp=False, world=1, _remote=None, weights="model", head="model", kv="model")

    def why(**kw):
        return Real(SimpleNamespace(**{**base, **kw}), None, [], SamplingConfig()).batch_refusal()

    assert why() is None
    assert "tensor-parallel" in why(tp=True, world=2)
    assert "pipeline" in why(world=2)
    assert "remote workers" in why(_remote=(1, 2))
    assert "weights fp8" in why(weights="fp8")
    assert "lm_head mxfp4" in why(head="mxfp4")
    assert "KV cache fp8" in why(kv="fp8")


def test_prompts_file_lines(tmp_path):
    from cake_amd.native_bridge import read_prompts_file
    p = tmp_path / "p.txt"
    p.write_text("one\r\ntwo words\nthree\n", encoding="utf-8")
    assert read_prompts_file(str(p)) == ["one", "two words", "three"]
    p.write_text("\n".join(f"p{i}" for i in range(8)), encoding="utf-8")     # no final newline
    assert len(read_prompts_file(str(p))) == 8
    for text, word in (("", "1 to 8 lines"), ("\n".join("x" * 9) + "\n", "1 to 8 lines"),
                       ("a\n\nb\n", "line 2"), ("a\n   \n", "line 2")):
        p.write_text(text, encoding="utf-8")
        with pytest.raises(ValueError) as e:
            read_prompts_file(str(p))
        assert word in str(e.value)


def _ctx(tmp_path, *flags):
    import torch
    from cake_amd.cli import build_parser
    from cake_amd.context import Context
    from cake_amd.utils.synth import tiny_config, write_checkpoint
    d = tmp_path / "m"
    if not d.exists():
        write_checkpoint(d, tiny_config(), torch.float32)
    args = build_parser().parse_args(["--model", str(d), "--topology", str(tmp_path / "none.yml"),
                                      "--cpu", *flags])
    return Context.from_args(args)


def test_python_cli_prompts_file_flag(tmp_path):
    from cake_amd.cli import build_parser, main, prompts_file_refusal
    assert build_parser().parse_args([]).prompts_file is None
    assert build_parser().parse_args(["--prompts-file", "a.txt"]).prompts_file == "a.txt"
    assert prompts_file_refusal(_ctx(tmp_path)) is None                      # the flag is off
    # a CPU run would take the Python path: refused, never decoded one by one
    why = prompts_file_refusal(_ctx(tmp_path, "--prompts-file", "a.txt"))
    assert "native Llama engine only" in why and "one sequence at a time" in why
    for flags, word in ((["--transport", "rccl"], "--transport rccl"),
                        (["--score-file", "s.txt"], "--score-file"),
                        (["--logprobs-file", "l.jsonl"], "--logprobs-file"),
                        (["--presence-penalty", "0.5"], "--presence-penalty"),
                        (["--weight-dtype", "fp8"], "--weight-dtype fp8"),
                        (["--kv-dtype", "fp8"], "--kv-dtype fp8")):
        why = prompts_file_refusal(_ctx(tmp_path, "--prompts-file", "a.txt", *flags))
        assert why and word in why, (flags, why)
    p = tmp_path / "p.txt"
    p.write_text("hello\n")
    rc = main(["--model", str(tmp_path / "m"), "--topology", str(tmp_path / "none.yml"), "--cpu",
               "--prompts-file", str(p)])
    assert rc == 2


def test_native_cli_prompts_file_flag(tmp_path):
    """cake-cli knows the flag and, on a CPU run, refuses as the Python entry does."""
    assert os.path.exists(CLI), "cake-cli not built"
    run = lambda *a: subprocess.run([CLI, *a], capture_output=True, text=True, timeout=180,  # noqa: E731
                                    cwd=ROOT, env=dict(os.environ, CAKE_LOG="warning"))
    r = run("--help")
    assert r.returncode == 0 and "--prompts-file" in r.stdout
    r = run("--prompts-file")
    assert r.returncode == 2 and "needs a value" in r.stderr
    ctx = _ctx(tmp_path)
    p = tmp_path / "p.txt"
    p.write_text("hello\n")
    args = ["--model", str(ctx.model_path), "--topology", str(tmp_path / "none.yml"), "--cpu",
            "--prompts-file", str(p)]
    nat = run(*args)
    py = subprocess.run([sys.executable, "-m", "cake_amd.cli", *args], capture_output=True,
                        text=True, timeout=180, cwd=ROOT)
    assert nat.returncode == py.returncode == 2
    assert "--prompts-file is served by the native Llama engine only" in nat.stderr
    assert nat.stdout == py.stdout == ""


def test_prompts_result_lines(tmp_path):
    """The bridge the native CLI prints through: one JSON object per prompt, EOS left out of
    the text."""
    from cake_amd import native_bridge as nb
    ctx = _ctx(tmp_path)
    _, eos = nb._tokenizer(str(ctx.model_path))
    stop = sorted(eos)[0]
    req = {"model": str(ctx.model_path), "prompts": [[1, 5, 6], [1, 7]],
           "tokens": [[9, 10, stop], [11]], "eos": sorted(eos)}
    lines = [json.loads(ln) for ln in nb.prompts_result_lines(json.dumps(req)).split("\n")]
    assert [ln["index"] for ln in lines] == [0, 1]
    assert [ln["n_prompt"] for ln in lines] == [3, 2]
    assert [ln["tokens"] for ln in lines] == [[9, 10, stop], [11]]
    want = "".join(nb.decode_token(json.dumps({"model": req["model"], "id": t})) for t in (9, 10))
    assert lines[0]["text"] == want and isinstance(lines[1]["text"], str)


def test_generate_batch_ctypes_signature():
    """The binding mirrors llama_engine.h (tests/test_abi_cpu.py compares every prototype);
    here: the entry point is bound, with the documented argument order."""
    from cake_amd import engine as E

    class Rec:
        def __init__(self):
            self.fns = {}

        def __getattr__(self, name):
            return self.fns.setdefault(name, SimpleNamespace())

    rec = Rec()
    E._bind(rec)
    fn = rec.fns["cake_engine_generate_batch"]
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    sp = C.POINTER(E.EngineStats)
    assert fn.restype is C.c_int32
    assert fn.argtypes == [C.c_void_p, ip, ip, C.c_int32, C.c_int32, C.POINTER(E.EngineSampling),
                           ip, C.c_int32, ip, ip, sp, sp, fp, C.c_char_p, C.c_int32]
    assert E.MAX_BATCH == 8
    assert "generate_batch" in dir(E.NativeLlama)
    hdr = open(os.path.join(ROOT, "cake_amd", "csrc", "engine", "llama_engine.h")).read()
    assert "int32_t cake_engine_generate_batch(" in hdr
