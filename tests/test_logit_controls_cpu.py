"""Logit controls (presence / frequency penalties, logit_bias, min_p) without a GPU: the oracle
against an independent float64 formulation, the Python front's value checks, the REST fields and
their 400s, and the command-line flags of both entry points."""
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from _fp8 import write_grid_checkpoint
from cake_amd.models.base import Token
from cake_amd.ops.reference import logit_controls_ref, min_p_offset, ordered_key

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cake_amd", "lib", "cake-cli")


# ---------------------------------------------------------------- oracle
def _ref64(x, generated, presence, frequency, bias):
    """The same arithmetic written independently, in float64 with python loops: exact for
    dyadic inputs of small magnitude, where the float32 oracle is exact too."""
    out = [float(v) for v in x]
    counts = {}
    for t in generated:
        counts[t] = counts.get(t, 0) + 1
    for v, c in counts.items():
        out[v] = out[v] - (presence + frequency * c)
    for i, b in (bias or {}).items():
        out[i] = out[i] + b
    return out


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_oracle_against_float64_on_dyadic_values(seed):
    rng = np.random.default_rng(seed)
    V = 97
    x = (rng.integers(-512, 512, size=V) / 64.0).astype(np.float32)       # k / 64
    gen = rng.integers(0, V, size=40).tolist() + [0, V - 1, V - 1]
    presence, frequency = 0.25 * int(rng.integers(-8, 9)), 0.125 * int(rng.integers(-16, 17))
    ids = rng.choice(V, size=12, replace=False).tolist() + [gen[0]]
    bias = {int(i): float(rng.integers(-400, 400)) / 4.0 for i in dict.fromkeys(ids)}
    got, cut = logit_controls_ref(x, gen, presence, frequency, bias)
    assert cut is None
    want = _ref64(x, gen, presence, frequency, bias)
    assert got.dtype.is_floating_point and got.numpy().dtype == np.float32
    assert got.numpy().astype(np.float64).tolist() == want
    assert not np.shares_memory(got.numpy(), x)                              # x is left alone


def test_oracle_order_and_rounding():
    # penalty first, bias second; each operation rounded to float32 on its own
    x = np.array([1.0, 2.0, -0.5, 3.0], dtype=np.float32)
    got, _ = logit_controls_ref(x, [3, 3, 1], 0.25, 0.5, {0: 4.0, 3: 1.0})
    assert got.tolist() == [5.0, 1.25, -0.5, 2.75]
    f, p, c = np.float32(0.1), np.float32(0.3), np.float32(3)
    x = np.array([np.float32(1 / 3)], dtype=np.float32)
    got, _ = logit_controls_ref(x, [0, 0, 0], 0.3, 0.1, {0: 0.7})
    step = np.float32(x[0] - np.float32(p + np.float32(f * c)))
    assert got.numpy()[0] == np.float32(step + np.float32(0.7))
    # a fused multiply-add would differ on such inputs somewhere: it is not what the oracle does
    # prompt tokens are the caller's to leave out; out-of-range ids in generated are ignored
    got, _ = logit_controls_ref(np.zeros(3, np.float32), [5, -1, 2], 1.0, 0.0)
    assert got.tolist() == [0.0, 0.0, -1.0]
    with pytest.raises(ValueError):
        logit_controls_ref(np.zeros(3, np.float32), [], bias=[(1, 1.0), (1, 2.0)])


def test_oracle_min_p():
    x = np.array([2.0, 1.0, 0.0, -3.0], dtype=np.float32)
    T, mp = 0.5, 0.25
    _, cut = logit_controls_ref(x, [], min_p=mp, temperature=T)
    d = np.float32(T * math.log(mp))
    assert min_p_offset(T, mp) == float(d)
    assert cut == int(ordered_key(np.float32(np.float32(2.0) + d)))
    # p[v] >= min_p p_max  <=>  x[v] >= max + T ln(min_p): here 2 - 0.693 = 1.307
    assert (ordered_key(x) >= cut).tolist() == [True, False, False, False]
    _, cut = logit_controls_ref(x, [], min_p=1.0, temperature=T)
    assert (ordered_key(x) >= cut).tolist() == [True, False, False, False]
    # the cut follows the adjusted row
    _, cut = logit_controls_ref(x, [0], presence=1.5, min_p=mp, temperature=T)
    assert (ordered_key(np.array([0.5, 1.0, 0.0, -3.0], np.float32)) >= cut).tolist() == \
        [True, True, False, False]
    for kw in (dict(min_p=mp, temperature=0.0), dict(min_p=None, temperature=T),
               dict(min_p=0.0, temperature=T)):
        assert logit_controls_ref(x, [], **kw)[1] is None
    # a maximum of -0.0 with d = 0: the sum is +0.0, the key stays the maximum's
    z = np.array([-0.0, -1.0], dtype=np.float32)
    _, cut = logit_controls_ref(z, [], min_p=1.0, temperature=T)
    assert (ordered_key(z) >= cut).tolist() == [True, False]


# ---------------------------------------------------------------- Python front
def test_logit_controls_values():
    from cake_amd.engine import LogitControls
    c = LogitControls(0.5, -0.25, {42: -100, 7: 2.5}, 0.25)
    assert (c.presence_penalty, c.frequency_penalty, c.min_p) == (0.5, -0.25, 0.25)
    assert c.logit_bias == {42: -100.0, 7: 2.5} and c.n_bias == 2 and not c.neutral
    assert c == LogitControls(0.5, -0.25, {42: -100, 7: 2.5}, 0.25) != LogitControls(0.5)
    assert LogitControls().neutral and LogitControls(0.0, 0.0, {}, 0.0).neutral
    assert LogitControls(min_p=None).min_p == 0.0
    for bad in (dict(presence_penalty=2.5), dict(frequency_penalty=-2.01), dict(min_p=1.5),
                dict(min_p=-0.1), dict(presence_penalty=True), dict(presence_penalty="1"),
                dict(frequency_penalty=float("nan")), dict(logit_bias={1: 101}),
                dict(logit_bias={1: float("inf")}), dict(logit_bias={-1: 1.0}),
                dict(logit_bias={"1": 1.0}), dict(logit_bias={True: 1.0}), dict(logit_bias=[(1, 1.0)]),
                dict(logit_bias={i: 1.0 for i in range(301)})):
        with pytest.raises(ValueError):
            LogitControls(**bad)
    LogitControls(logit_bias={i: 1.0 for i in range(300)})
    with pytest.raises(ValueError, match="vocabulary"):
        LogitControls(logit_bias={10: 1.0}).check_vocab(10)


def test_native_llama_rejects_bad_values_before_the_engine():
    from cake_amd.engine import NativeLlama
    eng = NativeLlama.__new__(NativeLlama)   # no engine: nothing may be touched
    eng._h, eng.vocab_size = None, 100
    for bad in (dict(presence_penalty=2.5), dict(frequency_penalty=3), dict(min_p=1.5),
                dict(logit_bias={1: 101.0}), dict(logit_bias={100: 1.0})):
        with pytest.raises(ValueError):
            eng.generate([1, 2], 4, **bad)


def test_engine_surface():
    import ctypes as C

    from cake_amd.engine import EngineOpts, EngineSampling, LogitControls, lib
    assert C.sizeof(EngineOpts) == 40 and C.sizeof(EngineSampling) == 32    # layouts kept
    assert C.sizeof(LogitControls) == 32
    assert len(lib().cake_engine_set_logit_controls.argtypes) == 4


# ---------------------------------------------------------------- REST
def test_request_logit_controls():
    from cake_amd.api.server import request_logit_controls as rq
    from cake_amd.engine import LogitControls
    assert rq({}) is None
    assert rq({"presence_penalty": None, "logit_bias": None, "min_p": None}) is None
    assert rq({"presence_penalty": 0, "frequency_penalty": 0.0, "logit_bias": {}, "min_p": 0}) is None
    assert rq({"logit_bias": {"42": -100}}) == LogitControls(logit_bias={42: -100.0})
    assert rq({"presence_penalty": 1, "frequency_penalty": -0.5, "min_p": 0.05}) == \
        LogitControls(1.0, -0.5, None, 0.05)
    for bad in ({"presence_penalty": True}, {"logit_bias": {str(i): 1 for i in range(301)}},
                {"logit_bias": {"1": 101}}, {"logit_bias": {"x": 1}}, {"logit_bias": {"1.5": 1}},
                {"logit_bias": {"-1": 1}}, {"logit_bias": [[1, 2]]}, {"logit_bias": {"1": "2"}},
                {"logit_bias": {"1": True}}, {"logit_bias": {"1": 1, "01": 2}},
                {"presence_penalty": 2.5}, {"frequency_penalty": "0.5"}, {"min_p": 1.5},
                {"min_p": -0.5}):
        with pytest.raises(ValueError):
            rq(bad)
    with pytest.raises(ValueError, match="vocabulary"):
        rq({"logit_bias": {"50": 1}}, vocab_size=50)


class FakeTokenizer:
    def decode(self, ids, skip_special_tokens=False):
        return f"<{ids[0]}>"


class PlainLLM:
    """Three tokens, the last an EOS; no set_logit_controls (as the Python engines)."""
    MODEL_NAME = "llama3"
    IDS = [3, 4, 2]

    def __init__(self):
        self.tokenizer = FakeTokenizer()
        self.calls = []

    def add_message(self, m):
        pass

    def reset(self):
        pass

    def generated_tokens(self):
        return len(self.IDS)

    def stream(self, n, on_token, stop_at_eos=True):
        for tid in self.IDS[:n]:
            on_token(Token(tid, self.tokenizer.decode([tid]), tid == 2))


class ControlLLM(PlainLLM):
    def set_logit_controls(self, c):
        self.calls.append(c)


def _client(llm):
    from fastapi.testclient import TestClient

    from cake_amd.api.server import create_app
    from cake_amd.master import Master
    ctx = types.SimpleNamespace(args=types.SimpleNamespace(sample_len=8, metrics=None, trace=None),
                                sampling=None)
    return TestClient(create_app(Master(ctx, llm=llm)))


MSGS = [{"role": "user", "content": "hi"}]
URL = "/api/v1/chat/completions"


def test_api_applies_and_clears_the_controls():
    from cake_amd.engine import LogitControls
    llm = ControlLLM()
    c = _client(llm)
    r = c.post(URL, json={"messages": MSGS, "frequency_penalty": 0.5, "logit_bias": {"42": -100},
                          "min_p": 0.1})
    assert r.status_code == 200, r.text
    assert r.json()["choices"][0]["message"]["content"] == "<3><4>"
    r = c.post(URL, json={"messages": MSGS})
    assert r.status_code == 200
    r = c.post(URL, json={"messages": MSGS, "presence_penalty": 0, "frequency_penalty": 0})
    assert r.status_code == 200
    assert llm.calls == [LogitControls(0.0, 0.5, {42: -100.0}, 0.1), None, None]


def test_api_refusals():
    c = _client(ControlLLM())
    for bad in ({"presence_penalty": 2.5}, {"frequency_penalty": True}, {"min_p": 1.5},
                {"logit_bias": {"x": 1}}, {"logit_bias": {"1": 101}},
                {"logit_bias": {str(i): 1 for i in range(301)}}):
        r = c.post(URL, json=dict(messages=MSGS, **bad))
        assert r.status_code == 400 and r.json()["error"].startswith("bad request: "), bad
    plain = _client(PlainLLM())     # a generator without set_logit_controls: never ignored
    for body in ({"frequency_penalty": 0.5}, {"presence_penalty": -1}, {"logit_bias": {"5": 1}},
                 {"min_p": 0.1}):
        r = plain.post(URL, json=dict(messages=MSGS, **body))
        assert r.status_code == 400 and "native engine" in r.json()["error"], body
    for body in ({}, {"frequency_penalty": 0, "presence_penalty": 0.0, "logit_bias": {}, "min_p": 0}):
        r = plain.post(URL, json=dict(messages=MSGS, **body))   # neutral: exactly as before
        assert r.status_code == 200 and r.json()["choices"][0]["message"]["content"] == "<3><4>"
    r = plain.post(URL, json={"messages": MSGS, "min_p": 2})    # invalid beats unsupported
    assert r.status_code == 400 and "min_p" in r.json()["error"]


def test_native_generator_carries_the_controls():
    from cake_amd.engine import LogitControls
    from cake_amd.models.llama3.native_generator import NativeLLM
    from cake_amd.models.sampling import SamplingConfig
    seen = []
    llm = NativeLLM.__new__(NativeLLM)
    llm.eng = types.SimpleNamespace(set_logit_controls=seen.append)
    llm.sampling = SamplingConfig()
    llm.logit_controls = None
    assert not set(llm._kw()) & {"presence_penalty", "frequency_penalty", "logit_bias", "min_p"}
    c = LogitControls(0.5, 0.25, {3: 1.0}, 0.125)
    llm.set_logit_controls(c)
    kw = llm._kw()
    assert (kw["presence_penalty"], kw["frequency_penalty"], kw["logit_bias"], kw["min_p"]) == \
        (0.5, 0.25, {3: 1.0}, 0.125)
    llm.set_logit_controls(LogitControls())
    assert llm.logit_controls is None and "min_p" not in llm._kw()
    llm.set_logit_controls(None)
    assert seen == [c, LogitControls(), None]


# ---------------------------------------------------------------- CLI
FLAGS = {"--presence-penalty": "0.5", "--frequency-penalty": "0.5", "--min-p": "0.1",
         "--logit-bias": "42:-100,7:2.5"}


@pytest.fixture(scope="module")
def grid(tmp_path_factory):
    return write_grid_checkpoint(tmp_path_factory.mktemp("logit_controls_grid"))


def _run(cmd, **env):
    e = dict(os.environ, CAKE_LOG="warning", **env)
    return subprocess.run(cmd, capture_output=True, text=True, timeout=180, env=e, cwd=ROOT)


def _entry(entry):
    return [CLI] if entry == "cake-cli" else [sys.executable, "-m", "cake_amd.cli"]


def test_parse_logit_bias():
    from cake_amd.cli import parse_logit_bias
    assert parse_logit_bias("42:-100,7:2.5") == {42: -100.0, 7: 2.5}
    for bad in ("42", "42:", ":1", "a:1", "1:x", "1:1,", "1:1,1:2", "-1:1", "1.5:1"):
        with pytest.raises(ValueError):
            parse_logit_bias(bad)


@pytest.mark.parametrize("entry", ["cake-cli", "python"])
def test_cli_lists_the_flags(entry):
    r = _run([*_entry(entry), "--help"])
    assert r.returncode == 0 and all(f in r.stdout for f in FLAGS)


@pytest.mark.parametrize("entry", ["cake-cli", "python"])
@pytest.mark.parametrize("flag", sorted(FLAGS))
def test_cli_refused_with_cpu(grid, tmp_path, entry, flag):
    r = _run([*_entry(entry), "--model", str(grid), "--topology", str(tmp_path / "none.yml"),
              flag, FLAGS[flag], "--cpu"])
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert flag in r.stderr and "native Llama engine" in r.stderr
    assert r.stdout.strip() == ""


@pytest.mark.parametrize("entry", ["cake-cli", "python"])
@pytest.mark.parametrize("flag", sorted(FLAGS))
def test_cli_refused_with_tensor_parallel(grid, tmp_path, entry, flag):
    r = _run([*_entry(entry), "--model", str(grid), "--topology", str(tmp_path / "none.yml"),
              "--transport", "rccl", "--parallel", "tp", flag, FLAGS[flag]],
             WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert flag in r.stderr and "--parallel tp" in r.stderr and "tensor-parallel" in r.stderr
    assert r.stdout.strip() == ""


@pytest.mark.parametrize("entry", ["cake-cli", "python"])
@pytest.mark.parametrize("how", ["CAKE_NATIVE=0", "--no-graph", "f32", "image"])
def test_cli_refused_on_the_other_python_engines(grid, tmp_path, entry, how):
    extra, env = [], {}
    if how == "CAKE_NATIVE=0":
        env["CAKE_NATIVE"] = "0"
    elif how == "f32":
        extra = ["--dtype", "f32"]
    elif how == "image":
        extra = ["--model-type", "image-model"]
    else:
        extra = [how]
    r = _run([*_entry(entry), "--model", str(grid), "--topology", str(tmp_path / "none.yml"),
              "--frequency-penalty", "0.5", *extra], **env)
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert "--frequency-penalty" in r.stderr and "native Llama engine" in r.stderr
    assert ("text model only" in r.stderr) == (how == "image")
    assert r.stdout.strip() == ""


@pytest.mark.parametrize("entry", ["cake-cli", "python"])
@pytest.mark.parametrize("extra,word", [(["--logit-bias", "42"], "ID:BIAS"),
                                        (["--logit-bias", "a:1"], "ID:BIAS"),
                                        (["--logit-bias", "1:1,1:2"], "--logit-bias"),
                                        (["--logit-bias", "1:101"], "100"),
                                        (["--presence-penalty", "2.5"], "[-2, 2]"),
                                        (["--min-p", "1.5"], "[0, 1]")])
def test_cli_bad_values(grid, tmp_path, entry, extra, word):
    r = _run([*_entry(entry), "--model", str(grid), "--topology", str(tmp_path / "none.yml"),
              "--cpu", *extra])
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert word in r.stderr and r.stdout.strip() == ""
