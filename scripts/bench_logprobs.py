"""Decode cost of the generated-token log-probs (NativeLlama.generate(..., logprobs=K)).

One process opens one random-init engine of a named architecture per configuration and
alternates three arms on it: off, K = 0 (logit and lse only) and K = 20.  Per round and arm:
one generation of ``--steps`` decode steps after a short prompt, the device p50 per token as
the engine reports it (events around each graph replay).  One JSON line per measurement, then
one summary line per configuration and arm: the median p50, its spread over the rounds, and
the difference to the off arm in microseconds and per cent.  The tokens of the three arms
must be equal.

    python scripts/bench_logprobs.py --out profiles/logprobs_decode_ab.jsonl
    python scripts/bench_logprobs.py --configs 16-bit --arms k20 --rounds 1   # under a profiler
"""
import argparse
import json
import shutil
import statistics
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

CONFIGS = {"16-bit": {}, "mxfp4+head=mxfp4": dict(weights="mxfp4", head="mxfp4")}
ARMS = {"off": None, "k0": 0, "k20": 20}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--prompt", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from cake_amd.engine import NativeLlama, write_config
    from cake_amd.models.llama3.config import preset
    if not torch.cuda.is_available():
        raise SystemExit("bench_logprobs: needs a GPU (no timing without one)")
    cfg = preset(a.model)
    d = tempfile.mkdtemp(prefix="cake_logprobs_cfg_")
    write_config(d, cfg)
    arms = [n for n in a.arms.split(",") if n]
    out = open(a.out, "w") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    g = torch.Generator().manual_seed(1234)
    prompt = torch.randint(0, cfg.vocab_size, (a.prompt,), generator=g).tolist()
    try:
        for name in [n for n in a.configs.split(",") if n]:
            eng = NativeLlama(d, max_seq=a.prompt + a.steps + 64, dtype="bf16", random_init=True,
                              seed=1, **CONFIGS[name])
            try:
                run = lambda k: eng.generate(prompt, a.steps + 1, eos_ids=[], logprobs=k)
                first = {n: run(ARMS[n]).tokens for n in arms}   # warm: graphs, buffers
                p50 = {n: [] for n in arms}
                for rnd in range(a.rounds):
                    for n in arms:
                        r = run(ARMS[n])
                        p50[n].append(r.p50_ms)
                        emit({"model": a.model, "config": name, "arm": n, "round": rnd,
                              "p50_ms": round(r.p50_ms, 5), "p99_ms": round(r.p99_ms, 5),
                              "tokens_per_s": round(r.tokens_per_s, 3),
                              "tokens_equal": r.tokens == first[arms[0]]})
                base = statistics.median(p50["off"]) if "off" in p50 else None
                for n in arms:
                    m = statistics.median(p50[n])
                    rec = {"model": a.model, "summary": name, "arm": n, "p50_ms": round(m, 5),
                           "spread_ms": round(max(p50[n]) - min(p50[n]), 5)}
                    if base:
                        rec["over_off_us"] = round((m - base) * 1e3, 2)
                        rec["over_off_pct"] = round(100.0 * (m - base) / base, 3)
                    emit(rec)
            finally:
                eng.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)
        if out:
            out.close()


if __name__ == "__main__":
    main()
