"""Logit controls in the native engine: NativeLlama.generate(..., presence_penalty=,
frequency_penalty=, logit_bias=, min_p=) on the GPU.

Oracle: ``forced_logits(prompt, tokens[:-1])`` runs the same decode kernels eagerly; row i, after
a host repeat penalty where one is set (2.0: ``/ p`` and ``* p`` are exact in f32), goes through
``ops/reference.py::logit_controls_ref`` with ``generated = tokens[:i]``.  Required: every greedy
token is the adjusted row's argmax (the lowest id at ties), every drawn token lies in the min_p
set, log-prob records are bit-equal to the adjusted row (``lse`` within ``_score.lse_bound``).
max_seq 256 and short contexts keep decode attention a single split in the eager and the
captured path alike.  The layer-sharded pipeline and the remote-worker master run the same
``select_tail`` and are not covered here (they need several GPU processes)."""
import math

import numpy as np
import pytest
import torch

import _score as S
from _fp8 import write_grid_checkpoint
from _sampling_ref import expected_set
from cake_amd.ops import reference as R

pytestmark = pytest.mark.gpu

PROMPT = [1, 17, 300, 5, 99, 1024, 7, 8]
PROMPT_B = [3, 41, 41, 900, 12, 5]
N = 24
FIELDS = ("ids", "logit", "lse", "top_ids", "top_logits")


@pytest.fixture(scope="module")
def grid(tmp_path_factory):
    return write_grid_checkpoint(tmp_path_factory.mktemp("logit_controls_grid"))


def _engine(path, **kw):
    from cake_amd.engine import NativeLlama
    return NativeLlama(path, max_seq=kw.pop("max_seq", 256), dtype="bf16", **kw)


def _bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _f32(v) -> float:
    return float(np.float32(v))


def _rows(eng, prompt, tokens, *, penalty=1.0, last_n=0, presence=0.0, frequency=0.0, bias=None,
          min_p=None, temperature=0.0):
    """(adjusted row, cut key | None, row before the controls) of every step of `tokens`; the
    engine carries the scalars as f32."""
    fl = eng.forced_logits(prompt, list(tokens[:-1]))
    out = []
    for i in range(len(tokens)):
        x = torch.from_numpy(fl[i])
        if penalty != 1.0:
            x = R.apply_repeat_penalty(x, penalty, (prompt + list(tokens[:i]))[-last_n:])
        adj, cut = R.logit_controls_ref(x, list(tokens[:i]), _f32(presence), _f32(frequency), bias,
                                        None if min_p is None else _f32(min_p), _f32(temperature))
        out.append((adj, cut, x))
    return out


def _check_records(lp, tokens, rows, K, what):
    assert lp.ids.tolist() == list(tokens), what
    worst = 0.0
    for i, (adj, _, _) in enumerate(rows):
        ref = R.logprob_topk_ref(adj, tokens[i], K)
        w = f"{what} token {i}"
        assert _bits(lp.logit[i])[()] == _bits(ref["logit"].numpy())[()], w
        assert np.array_equal(lp.top_ids[i], ref["top_ids"].numpy()), w
        assert np.array_equal(_bits(lp.top_logits[i]), _bits(ref["top_logits"].numpy())), w
        ratio = abs(float(lp.lse[i]) - ref["lse"]) / float(S.lse_bound(np.float64(ref["lse"])))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (w, ratio)
    print(f"{what}: {len(tokens)} tokens, lse error / bound worst {worst:.3f}")


@pytest.mark.parametrize("rp", [dict(repeat_penalty=1.0), dict(repeat_penalty=2.0, repeat_last_n=64)],
                         ids=["no-repeat-penalty", "repeat-penalty"])
def test_greedy(cuda, grid, rp):
    eng = _engine(grid)
    plain = eng.generate(PROMPT, N, **rp)
    b = plain.tokens[0]                        # what the uncontrolled run produces first
    a = next((t for t in plain.tokens if t != b), (b + 1) % eng.vocab_size)
    kw = dict(frequency_penalty=0.5, presence_penalty=0.25, logit_bias={a: 4.0, b: -100.0})
    r = eng.generate(PROMPT, N, logprobs=20, **kw, **rp)
    assert r.tokens != plain.tokens and b not in r.tokens
    rows = _rows(eng, PROMPT, r.tokens, penalty=rp["repeat_penalty"],
                 last_n=rp.get("repeat_last_n", 0), presence=0.25, frequency=0.5,
                 bias=kw["logit_bias"])
    changed = 0
    for i, (adj, cut, x) in enumerate(rows):
        assert cut is None
        assert r.tokens[i] == int(torch.argmax(adj)), i   # torch.argmax: the first maximum
        changed += int(torch.argmax(adj)) != int(torch.argmax(x))
    print(f"greedy {rp}: {changed} of {N} tokens differ from their unadjusted row's argmax; "
          f"{len(set(r.tokens))} distinct tokens (plain: {len(set(plain.tokens))})")
    assert changed >= 1
    _check_records(r.logprobs, r.tokens, rows, 20, f"greedy {rp}")
    eng.close()


def test_sampled_min_p(cuda, grid):
    eng = _engine(grid)
    T, k, p, mp = 0.8, 40, 0.9, 0.2
    kw = dict(temperature=T, top_k=k, top_p=p, seed=1234, repeat_penalty=1.0)
    off = eng.generate(PROMPT, N, **kw)
    # a second min_p chosen on the oracle so that it bites: the tiny model's rows are nearly flat
    # (0.2 cuts nothing inside its top 40), so take the cut halfway between the prefill row's
    # maximum and its 40th largest logit: min_p = exp(-gap / (2 T))
    x0 = np.sort(eng.prefill_logits(PROMPT))[::-1]
    mp_bite = float(np.float32(math.exp(-float(x0[0] - x0[k - 1]) / (2 * T))))
    assert 0.0 < mp_bite < 1.0
    shrunk = {}
    for m in (mp, mp_bite):
        r = eng.generate(PROMPT, N, min_p=m, **kw)
        smaller = 0
        for i, (adj, cut, _) in enumerate(_rows(eng, PROMPT, r.tokens, min_p=m, temperature=T)):
            keys = R.ordered_key(adj.numpy())
            assert cut is not None and keys[r.tokens[i]] >= cut, (m, i, r.tokens[i])
            kp = expected_set(adj, _f32(T), k, p).numpy()
            smaller += int(np.count_nonzero(kp & (keys >= cut)) < np.count_nonzero(kp))
        shrunk[m] = smaller
        print(f"min_p {m:.4f}: the set shrinks at {smaller} of {N} steps; tokens "
              f"{'differ from' if r.tokens != off.tokens else 'equal'} the run without min_p")
    assert shrunk[mp_bite] >= 1
    one = eng.generate(PROMPT, N, min_p=1.0, **kw)
    for i, (adj, cut, _) in enumerate(_rows(eng, PROMPT, one.tokens, min_p=1.0, temperature=T)):
        assert float(adj[one.tokens[i]]) == float(adj.max()), i
    # greedy ignores min_p: alone it leaves the default path, with a penalty it cuts nothing
    assert eng.generate(PROMPT, N, min_p=0.5, repeat_penalty=1.0).tokens == \
        eng.generate(PROMPT, N, repeat_penalty=1.0).tokens
    g = eng.generate(PROMPT, N, min_p=0.5, presence_penalty=0.5, repeat_penalty=1.0)
    for i, (adj, cut, _) in enumerate(_rows(eng, PROMPT, g.tokens, presence=0.5, min_p=0.5)):
        assert cut is None and g.tokens[i] == int(torch.argmax(adj)), i
    eng.close()


def test_continue(cuda, grid):
    eng = _engine(grid)
    kw = dict(repeat_penalty=1.0, logprobs=5, frequency_penalty=0.5, presence_penalty=0.25,
              logit_bias={17: 2.0})
    whole = eng.generate(PROMPT, 12, **kw)
    head = eng.generate(PROMPT, 5, **kw)
    tail = eng.continue_(7)
    assert head.tokens + tail.tokens == whole.tokens
    for f in FIELDS:
        got = np.concatenate([getattr(head.logprobs, f), getattr(tail.logprobs, f)])
        assert got.tobytes() == getattr(whole.logprobs, f).tobytes(), f
    eng.close()


def test_steps_per_graph(cuda, grid):
    recs = []
    for k in (1, 4):
        eng = _engine(grid, steps_per_graph=k)
        recs.append(eng.generate(PROMPT, N, repeat_penalty=2.0, repeat_last_n=64, logprobs=20,
                                 frequency_penalty=0.5, presence_penalty=0.25,
                                 logit_bias={17: 2.0, 5: -3.0}))
        eng.close()
    a, b = recs
    assert a.tokens == b.tokens
    for f in FIELDS:
        assert getattr(a.logprobs, f).tobytes() == getattr(b.logprobs, f).tobytes(), f


def test_state_between_generations(cuda, grid):
    """The table is reset per generation and the warm step (run when the graphs are captured,
    here in generation A) counts nothing twice; with the controls off again, or all neutral, the
    engine is the one that never had them."""
    ctl = dict(frequency_penalty=0.5, presence_penalty=0.25, logit_bias={17: 2.0}, logprobs=5,
               repeat_penalty=1.0)
    eng = _engine(grid)
    a = eng.generate(PROMPT, N, **ctl)
    rows = _rows(eng, PROMPT, a.tokens, presence=0.25, frequency=0.5, bias={17: 2.0})
    assert all(a.tokens[i] == int(torch.argmax(adj)) for i, (adj, _, _) in enumerate(rows))
    b = eng.generate(PROMPT_B, N, **ctl)
    fresh = _engine(grid)
    want = fresh.generate(PROMPT_B, N, **ctl)
    fresh.close()
    assert b.tokens == want.tokens
    for f in FIELDS:
        assert getattr(b.logprobs, f).tobytes() == getattr(want.logprobs, f).tobytes(), f
    off = eng.generate(PROMPT, N, repeat_penalty=1.0, logprobs=5)
    neutral = eng.generate(PROMPT, N, repeat_penalty=1.0, logprobs=5, presence_penalty=0.0,
                           frequency_penalty=0.0, logit_bias={}, min_p=0.0)
    never = _engine(grid)
    base = never.generate(PROMPT, N, repeat_penalty=1.0, logprobs=5)
    never.close()
    assert off.tokens == neutral.tokens == base.tokens != a.tokens
    for f in FIELDS:
        assert getattr(off.logprobs, f).tobytes() == getattr(base.logprobs, f).tobytes(), f
        assert getattr(neutral.logprobs, f).tobytes() == getattr(base.logprobs, f).tobytes(), f
    eng.close()


def test_formats(cuda, grid):
    eng = _engine(grid, weights="fp8", head="fp8", kv="fp8")
    kw = dict(frequency_penalty=0.5, presence_penalty=0.25, logit_bias={17: 2.0, 5: -100.0})
    r = eng.generate(PROMPT, N, repeat_penalty=1.0, logprobs=20, **kw)
    rows = _rows(eng, PROMPT, r.tokens, presence=0.25, frequency=0.5, bias=kw["logit_bias"])
    assert all(r.tokens[i] == int(torch.argmax(adj)) for i, (adj, _, _) in enumerate(rows))
    assert 5 not in r.tokens
    _check_records(r.logprobs, r.tokens, rows, 20, "fp8 weights / head / kv")
    eng.close()


def test_refusals(cuda, grid):
    import ctypes as C

    from cake_amd.engine import LogitControls, NativeLlama, lib
    eng = _engine(grid)
    V = eng.vocab_size
    with pytest.raises(ValueError, match="vocabulary"):
        eng.generate(PROMPT, 4, logit_bias={V: 1.0})
    err = C.create_string_buffer(512)
    ids = (C.c_int32 * 2)(V, 3)
    vals = (C.c_float * 2)(1.0, 1.0)
    c = LogitControls(presence_penalty=0.5)
    c.n_bias, c.bias_ids, c.bias_values = 2, ids, vals
    assert lib().cake_engine_set_logit_controls(eng._h, C.byref(c), err, len(err)) != 0
    assert "vocabulary" in err.value.decode()
    ids[0] = 3
    assert lib().cake_engine_set_logit_controls(eng._h, C.byref(c), err, len(err)) != 0
    assert "twice" in err.value.decode()
    c.n_bias = 301
    assert lib().cake_engine_set_logit_controls(eng._h, C.byref(c), err, len(err)) != 0
    assert "300" in err.value.decode()
    # the refused calls left the setting alone
    assert eng.generate(PROMPT, 4, repeat_penalty=1.0).tokens == \
        _engine(grid).generate(PROMPT, 4, repeat_penalty=1.0).tokens
    eng.close()
    worker = _engine(grid, layers=[0, 1, 2])
    with pytest.raises(RuntimeError, match="head"):
        worker.set_logit_controls(LogitControls(presence_penalty=0.5))
    worker.close()
    # tensor parallel: refused by the front before any library call or connection (the engine's
    # own refusal carries the same message; opening a tensor-parallel group needs several ranks)
    tp = NativeLlama.__new__(NativeLlama)
    tp._h, tp.tp, tp.vocab_size = None, True, V
    with pytest.raises(RuntimeError, match="tensor-parallel"):
        tp.set_logit_controls(LogitControls(frequency_penalty=0.5))
    tp.set_logit_controls(None)    # off is not refused
