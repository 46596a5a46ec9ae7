"""NativeLlama.generate_batch: lock-step batched decode of up to 8 sequences.

What batching must not change: a sequence's tokens and the logits its selection saw are, bit
for bit, those of the same prompt decoded alone through the same call -- whatever rides with
it and whichever slot it sits in.  Against the existing paths the batched step is judged by
logits: it makes the prefill path's 16-bit activation rounding and the decode path's
attention, so its distance to the repository's f32 torch model is held to twice the larger of
the two existing paths' own distances, both measured here."""
import json
import os

import numpy as np
import pytest
import torch

from cake_amd.models.llama3.config import preset
from cake_amd.utils.synth import write_checkpoint

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 24
MAX_SEQ = 512
SAMPLED = dict(temperature=0.8, top_k=20, top_p=0.9)
PEN = dict(repeat_penalty=1.1, repeat_last_n=16)


def _prompt(n, seed):
    g = torch.Generator().manual_seed(seed)
    return [1] + torch.randint(3, 2048, (n - 1,), generator=g).tolist()


# lengths 8, 40 and 330: the last crosses the 320-key one-split boundary of the decode attention
PROMPTS = [_prompt(8, 1), _prompt(40, 2), _prompt(330, 3)]


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    d = tmp_path_factory.mktemp("batch_ckpt")
    cfg = preset("llama3-8b", num_hidden_layers=3, vocab_size=2048, intermediate_size=1024,
                 hidden_size=512, num_attention_heads=8, num_key_value_heads=2,
                 bos_token_id=1, eos_token_id=2)
    write_checkpoint(d, cfg, torch.bfloat16, seed=3, single_file=True)
    return d


@pytest.fixture(scope="module")
def eng(cuda, ckpt):
    from cake_amd.engine import NativeLlama
    e = NativeLlama(ckpt, max_seq=MAX_SEQ, dtype="bf16")
    yield e
    e.close()


@pytest.fixture(scope="module")
def greedy(eng):
    """The three prompts as one greedy batch, with the logits: computed once."""
    return eng.generate_batch(PROMPTS, N, return_logits=True, **PEN)


def _same_result(a, b, what):
    assert a.tokens == b.tokens, f"{what}: tokens {a.tokens} vs {b.tokens}"
    if a.logits is not None and b.logits is not None:
        assert np.array_equal(a.logits, b.logits), f"{what}: logits differ"


def test_batch_invariance_greedy(eng, greedy):
    assert [len(r.tokens) for r in greedy] == [N] * 3
    assert [r.n_prompt for r in greedy] == [8, 40, 330]
    assert all(r.logits.shape == (N, 2048) for r in greedy)
    for b, p in enumerate(PROMPTS):
        alone = eng.generate_batch([p], N, return_logits=True, **PEN)[0]
        _same_result(alone, greedy[b], f"prompt {b} alone")
    perm = [2, 0, 1]
    again = eng.generate_batch([PROMPTS[i] for i in perm], N, return_logits=True, **PEN)
    for slot, b in enumerate(perm):
        _same_result(again[slot], greedy[b], f"prompt {b} in slot {slot}")


def test_batch_invariance_sampled(eng):
    seed = 11
    got = eng.generate_batch(PROMPTS, N, seed=seed, return_logits=True, **SAMPLED, **PEN)
    assert len({tuple(r.tokens) for r in got}) == 3
    for b, p in enumerate(PROMPTS):
        alone = eng.generate_batch([p], N, seed=seed + b, return_logits=True, **SAMPLED, **PEN)[0]
        _same_result(alone, got[b], f"sampled prompt {b} alone with seed + {b}")
    perm = [1, 2, 0]
    for slot, b in enumerate(perm):   # slot s draws with seed + s: choose the seed that lands on b's
        one = eng.generate_batch([PROMPTS[i] for i in perm], N, seed=seed + b - slot,
                                 return_logits=True, **SAMPLED, **PEN)[slot]
        _same_result(one, got[b], f"sampled prompt {b} in slot {slot}")


def _f32_logits(ckpt, seq, first):
    """Rows first.. of the f32 torch model's logits over seq (row i: after seq[:i + 1])."""
    from cake_amd.models.llama3.factory import load_model
    model = load_model(ckpt, "cpu", torch.float32, max_seq=MAX_SEQ, backend="torch")
    h = model.forward_hidden(model.embed(seq), 0)
    return torch.stack([model.head_logits(h[i]) for i in range(first, len(seq))]).numpy()


def test_batch_logits_against_existing_paths(eng, ckpt):
    """Teacher-forced along the batch's own greedy tokens (no penalty, so the rows are the raw
    logits).  e_dec: batch-1 forced_logits (decode path) vs the f32 torch model; e_pre:
    prefill_logits of every prefix vs the same; the batch's rows must stay within
    2 max(e_dec, e_pre) of the f32 model (the 2: summation order), and their argmax must
    equal the batch-1 decode path's wherever its top-2 margin exceeds twice that bound."""
    got = eng.generate_batch(PROMPTS, N, repeat_penalty=1.0, return_logits=True)
    e_dec = e_pre = e_batch = 0.0
    rows = []
    for b, p in enumerate(PROMPTS):
        toks = got[b].tokens
        assert len(toks) == N
        seq = p + toks[:N - 1]
        ref = _f32_logits(ckpt, seq, len(p) - 1)                      # [N, V]
        dec = eng.forced_logits(p, toks[:N - 1])                      # [N, V]; row 0 is prefill
        pre = np.stack([eng.prefill_logits(seq[:len(p) + i]) for i in range(N)])
        e_dec = max(e_dec, float(np.abs(dec[1:] - ref[1:]).max()))
        e_pre = max(e_pre, float(np.abs(pre - ref).max()))
        e_batch = max(e_batch, float(np.abs(got[b].logits - ref).max()))
        rows.append((got[b].logits, dec))
    bound = 2 * max(e_dec, e_pre)
    rec = {"checkpoint": "synthetic (3 layers, H 512, I 1024, V 2048), seed 3, bf16",
           "prompt_lengths": [len(p) for p in PROMPTS], "tokens": N,
           "e_dec_forced_logits_vs_f32_model": e_dec, "e_pre_prefill_logits_vs_f32_model": e_pre,
           "batch_vs_f32_model": e_batch, "bound": bound}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "batch_engine_error.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(rec)
    assert e_batch <= bound, rec
    for b, (lg, dec) in enumerate(rows):
        top2 = np.sort(dec, axis=1)[:, -2:]
        sure = (top2[:, 1] - top2[:, 0]) > 2 * bound
        assert sure.any()
        assert (lg.argmax(1)[sure] == dec.argmax(1)[sure]).all(), f"prompt {b}: argmax differs"


def test_batch_eos_ends_one_sequence_only(eng, greedy):
    """EOS = a token sequence 0 emits at step 3 of the EOS-free run: sequence 0 ends at its
    first occurrence, inclusive; the others are the EOS-free run (cut the same way should
    they emit it too)."""
    stop = greedy[0].tokens[3]
    got = eng.generate_batch(PROMPTS, N, eos_ids=[stop], return_logits=True, **PEN)
    for b, (r, free) in enumerate(zip(got, greedy)):
        n = free.tokens.index(stop) + 1 if stop in free.tokens else N
        assert r.tokens == free.tokens[:n], f"sequence {b}"
        assert np.array_equal(r.logits, free.logits[:n]), f"sequence {b}: logits"
    assert len(got[0].tokens) <= 4
    assert max(len(r.tokens) for r in got[1:]) > 4, "the EOS token ended every sequence"


def test_batch_identical_prompts(eng, greedy):
    """Three identical prompts: prefilled once, the cache prefix copied."""
    for b in (1, 2):
        got = eng.generate_batch([PROMPTS[b]] * 3, N, return_logits=True, **PEN)
        for i in range(3):
            _same_result(got[i], greedy[b], f"copy {i} of prompt {b}")


def test_generate_after_batch_equals_fresh_engine(eng, ckpt):
    from cake_amd.engine import NativeLlama
    eng.generate_batch(PROMPTS, N, **PEN)
    after = eng.generate(PROMPTS[1], N, **PEN).tokens
    sampled = eng.generate(PROMPTS[2], N, seed=4, **SAMPLED, **PEN).tokens
    fresh = NativeLlama(ckpt, max_seq=MAX_SEQ, dtype="bf16")
    try:
        assert fresh.generate(PROMPTS[1], N, **PEN).tokens == after
        assert fresh.generate(PROMPTS[2], N, seed=4, **SAMPLED, **PEN).tokens == sampled
    finally:
        fresh.close()


def test_batch_f16(cuda, ckpt):
    """The f16 engine: a batch equals its sequences decoded alone."""
    from cake_amd.engine import NativeLlama
    e = NativeLlama(ckpt, max_seq=MAX_SEQ, dtype="f16")
    try:
        got = e.generate_batch(PROMPTS[:2], 8, return_logits=True, **PEN)
        for b in range(2):
            _same_result(e.generate_batch([PROMPTS[b]], 8, return_logits=True, **PEN)[0], got[b],
                         f"f16 prompt {b}")
    finally:
        e.close()


def _refused(call, *words):
    with pytest.raises(RuntimeError) as ei:
        call()
    msg = str(ei.value)
    for w in words:
        assert w in msg, msg


def test_batch_refusals_on_the_supported_engine(eng):
    p = PROMPTS[0]
    _refused(lambda: eng.generate_batch([], 4), "1 to 8 prompts", "got 0")
    _refused(lambda: eng.generate_batch([p] * 9, 4), "1 to 8 prompts", "got 9")
    _refused(lambda: eng.generate_batch([p, []], 4), "empty prompt", "sequence 1")
    _refused(lambda: eng.generate_batch([p, PROMPTS[2]], MAX_SEQ - 330 + 1),
             "prompt + max_new exceeds max_seq", "sequence 1")
    eng.set_logprobs(3)
    try:
        _refused(lambda: eng.generate_batch([p], 4), "logprobs")
    finally:
        eng.set_logprobs(None)
    from cake_amd.engine import LogitControls
    eng.set_logit_controls(LogitControls(presence_penalty=0.5))
    try:
        _refused(lambda: eng.generate_batch([p], 4), "logit controls")
    finally:
        eng.set_logit_controls(None)
    assert len(eng.generate_batch([p], 4)[0].tokens) == 4       # and nothing was left behind


@pytest.mark.parametrize("kw,words", [
    (dict(weights="fp8"), ("fp8 weights", "weight_fmt 1")),
    (dict(weights="mxfp4"), ("mxfp4 weights", "weight_fmt 2")),
    (dict(head="fp8"), ("fp8 lm_head", "head_fmt 1")),
    (dict(kv="fp8"), ("quantised KV cache", "kv_fmt 1")),
    (dict(layers=[0, 1]), ("layers-only engine",)),
])
def test_batch_refusals_by_engine_kind(cuda, ckpt, kw, words):
    from cake_amd.engine import NativeLlama
    e = NativeLlama(ckpt, max_seq=64, dtype="bf16", **kw)
    try:
        _refused(lambda: e.generate_batch([PROMPTS[0]], 4), "generate_batch()", *words)
    finally:
        e.close()


def test_batch_refusal_on_a_master_with_tcp_workers(cuda, ckpt, tmp_path):
    """Layer 0 on a native TCP worker: the master engine refuses."""
    import subprocess
    from cake_amd.engine import NativeLlama
    from test_engine_gpu import _port, _wait_listen
    cli = os.path.join(ROOT, "cake_amd", "lib", "cake-cli")
    port = _port()
    topo = tmp_path / "topology.yml"
    topo.write_text(f"w1:\n  host: '127.0.0.1:{port}'\n  layers:\n    - 'model.layers.0'\n")
    w1 = subprocess.Popen([cli, "--mode", "worker", "--name", "w1", "--model", str(ckpt),
                           "--topology", str(topo), "--address", f"127.0.0.1:{port}",
                           "--max-seq-len", "64", "--dtype", "bf16"], cwd=ROOT,
                          env=dict(os.environ, CAKE_LOG="warning"), stdout=subprocess.DEVNULL,
                          stderr=subprocess.PIPE, text=True)
    try:
        _wait_listen(w1, port, "worker w1")
        e = NativeLlama(ckpt, max_seq=64, dtype="bf16", workers=[f"127.0.0.1:{port}"],
                        worker_of=[0, -1, -1])
        try:
            _refused(lambda: e.generate_batch([PROMPTS[0]], 4), "generate_batch()",
                     "remote workers")
        finally:
            e.close()
    finally:
        w1.kill()
        w1.communicate()


@pytest.mark.parametrize("kw,word", [("", "pipeline engine"), (", tp=True", "tensor-parallel engine")])
def test_batch_refusals_on_rank_groups(cuda, ckpt, tmp_path, kw, word):
    """Two rank processes of a pipeline / a tensor-parallel group: rank 0 refuses."""
    from test_engine_gpu import _group
    body = ("try:\n    e.generate_batch([[1, 17, 300]], 4)\n    out['err'] = ''\n"
            "except RuntimeError as ex:\n    out['err'] = str(ex)\n")
    got, msg = _group(tmp_path, ckpt, 2, body, kw=kw)
    assert "generate_batch()" in got["err"] and word in got["err"], (got, msg)
