"""Decode cost of the logit controls (NativeLlama.generate(..., presence_penalty=,
frequency_penalty=, logit_bias=, min_p=)).

One process opens one random-init engine of a named architecture and alternates the arms on it:
greedy off (the fused tail) / penalties / penalties + a 300-entry bias, and sampled (top-k 40,
top-p 0.9) without / with min_p.  Per round and arm: one generation of ``--steps`` decode steps
after a short prompt, the device p50 per token as the engine reports it.  One JSON line per
measurement, then one summary line per arm: the median p50, its spread over the rounds and the
difference to the arm's baseline (off for the greedy arms, sampled for sampled+min_p).

``--launch`` instead times the new launch next to cake_argmax on one row of the model's
vocabulary: three captured graphs of ``--reps`` repetitions each (argmax + finalize; controls +
argmax + finalize; the same with a 300-entry bias), microseconds per repetition.

    python scripts/bench_logit_controls.py --out profiles/logit_controls_decode_ab.jsonl
    python scripts/bench_logit_controls.py --launch --out profiles/logit_controls_launch.jsonl
"""
import argparse
import json
import shutil
import statistics
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

SAMPLED = dict(temperature=0.8, top_k=40, top_p=0.9, seed=1234)
PEN = dict(presence_penalty=0.25, frequency_penalty=0.5)


def _arms(V):
    bias = {int(i): float((i % 7) - 3) for i in range(1, 300 * 401, 401) if i < V}
    return {"off": ({}, None),
            "penalties": (PEN, "off"),
            "penalties+bias300": (dict(PEN, logit_bias=bias), "off"),
            "sampled": (SAMPLED, None),
            "sampled+min_p": (dict(SAMPLED, min_p=0.05), "sampled")}


def _emitter(path):
    out = open(path, "w") if path else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    return emit, out


def launch(a, cfg, emit):
    import torch

    from cake_amd.ops import hip
    dev, V = torch.device("cuda:0"), cfg.vocab_size
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(V, generator=g) * 3).to(dev)
    cap = a.reps + 64
    hist = torch.randint(0, V, (cap,), generator=g).to(torch.int32).to(dev)
    hl, tok, pos = (torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(3))
    slot = torch.zeros(1, dtype=torch.int64, device=dev)
    cnt = torch.zeros(V, dtype=torch.int32, device=dev)
    state = torch.zeros(hip.LOGIT_CONTROLS_STATE_WORDS, dtype=torch.int32, device=dev)
    bias = _arms(V)["penalties+bias300"][0]["logit_bias"]
    blocks = {"penalties": hip.pack_logit_controls(0.25, 0.5, None, None, 0.0, 32).to(dev),
              "penalties+bias300": hip.pack_logit_controls(0.25, 0.5, bias, None, 0.0, 32).to(dev)}
    row = x.clone()

    def reset():
        hl.fill_(32)
        pos.fill_(31)
        cnt.zero_()
        state.zero_()
        state[1] = 32
        row.copy_(x)

    def body(params):
        if params is not None:
            hip.logit_controls(row, hist, hl, cnt, params, state)
        hip.argmax(row, slot)
        hip.finalize_token(slot, tok, hist, hl, pos)

    graphs = {}
    for name, params in [("argmax", None), *blocks.items()]:
        reset()
        body(params)   # first launches outside capture
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(a.reps):
                body(params)
        graphs[name] = gr
    us = {n: [] for n in graphs}
    for _rnd in range(a.rounds + 1):      # the first round warms
        for name, gr in graphs.items():
            reset()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gr.replay()
            e1.record()
            torch.cuda.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / a.reps)
    base = statistics.median(us["argmax"][1:])
    for name, v in us.items():
        m = statistics.median(v[1:])
        emit({"model": a.model, "launch": name, "V": V, "reps": a.reps,
              "us_per_step": round(m, 3), "spread_us": round(max(v[1:]) - min(v[1:]), 3),
              "over_argmax_us": round(m - base, 3),
              "steps": "argmax + finalize" if name == "argmax"
              else "logit_controls + argmax + finalize"})


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--arms", default=None, help="comma-separated subset of the arms")
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--prompt", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launch", action="store_true", help="time the launch itself (see above)")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch

    from cake_amd.engine import NativeLlama, write_config
    from cake_amd.models.llama3.config import preset
    if not torch.cuda.is_available():
        raise SystemExit("bench_logit_controls: needs a GPU (no timing without one)")
    cfg = preset(a.model)
    emit, out = _emitter(a.out)
    if a.launch:
        try:
            launch(a, cfg, emit)
        finally:
            if out:
                out.close()
        return
    all_arms = _arms(cfg.vocab_size)
    arms = [n for n in (a.arms.split(",") if a.arms else all_arms) if n]
    d = tempfile.mkdtemp(prefix="cake_logit_controls_cfg_")
    write_config(d, cfg)
    g = torch.Generator().manual_seed(1234)
    prompt = torch.randint(0, cfg.vocab_size, (a.prompt,), generator=g).tolist()
    try:
        eng = NativeLlama(d, max_seq=a.prompt + a.steps + 64, dtype="bf16", random_init=True,
                          seed=1)
        try:
            run = lambda n: eng.generate(prompt, a.steps + 1, eos_ids=[], repeat_penalty=1.0,
                                         **all_arms[n][0])
            first = {n: run(n).tokens for n in arms}   # warm: graphs, buffers
            p50 = {n: [] for n in arms}
            for rnd in range(a.rounds):
                for n in arms:
                    r = run(n)
                    p50[n].append(r.p50_ms)
                    emit({"model": a.model, "arm": n, "round": rnd, "p50_ms": round(r.p50_ms, 5),
                          "p99_ms": round(r.p99_ms, 5), "tokens_per_s": round(r.tokens_per_s, 3),
                          "tokens_equal_to_first_run": r.tokens == first[n],
                          "distinct_tokens": len(set(r.tokens))})
            for n in arms:
                m = statistics.median(p50[n])
                rec = {"model": a.model, "summary": n, "p50_ms": round(m, 5),
                       "spread_ms": round(max(p50[n]) - min(p50[n]), 5)}
                ref = all_arms[n][1]
                if ref in p50:
                    base = statistics.median(p50[ref])
                    rec["baseline"] = ref
                    rec["over_baseline_us"] = round((m - base) * 1e3, 2)
                    rec["over_baseline_pct"] = round(100.0 * (m - base) / base, 3)
                emit(rec)
        finally:
            eng.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)
        if out:
            out.close()


if __name__ == "__main__":
    main()
