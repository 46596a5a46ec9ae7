"""Cost of NativeLlama.score against the same engine's prefill and against teacher forcing.

One process opens the random-init engine of a named architecture once per arm and alternates
the arms.  Per length T, round and arm: the best of three warm calls of

* ``prefill_logits(T)``  (TTFT: the prefill and the last row's head), and
* ``score(T)``           (the prefill and the head over every row),

and at ``--forced`` tokens ``forced_logits`` (one eager decode step per token, [T, V] logits
to the host) against ``score`` of the same tokens.  One JSON line per measurement, then one
summary line per length and arm: the medians, score / TTFT, and the rate of the head GEMM
taken from the difference (2 T V H flop over score - TTFT: an under-estimate of the GEMM's
own rate, since the difference also holds the row norm, the reducer and a quantised head's
widening).

    python scripts/bench_score.py --out profiles/score_ab.jsonl
"""
import argparse
import json
import shutil
import statistics
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

ARMS = {"16-bit": {}, "fp8": dict(weights="fp8"), "mxfp4": dict(weights="mxfp4"),
        "kv=fp8": dict(kv="fp8"), "fp8+prefill=fp8": dict(weights="fp8", prefill="fp8"),
        "fp8+head=fp8": dict(weights="fp8", head="fp8")}


def _best(fn, n=3):
    best = float("inf")
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--lengths", default="512,2048")
    ap.add_argument("--forced", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from cake_amd.engine import NativeLlama, write_config
    from cake_amd.models.llama3.config import preset
    if not torch.cuda.is_available():
        raise SystemExit("bench_score: needs a GPU (no timing without one)")
    cfg = preset(a.model)
    d = tempfile.mkdtemp(prefix="cake_score_cfg_")
    write_config(d, cfg)
    lengths = [int(x) for x in a.lengths.split(",") if x]
    names = [n for n in a.arms.split(",") if n]
    out = open(a.out, "w") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    g = torch.Generator().manual_seed(1234)
    toks = torch.randint(0, cfg.vocab_size, (max(lengths + [a.forced]),), generator=g).tolist()
    engines = {}
    try:
        for n in names:
            engines[n] = NativeLlama(d, max_seq=max(lengths + [a.forced]) + 64, dtype="bf16",
                                     random_init=True, seed=1, **ARMS[n])
        for T in lengths:
            p = toks[:T]
            ms = {n: {"ttft": [], "score": []} for n in names}
            for eng in engines.values():   # warm: plans, buffers, first launches
                eng.prefill_logits(p)
                eng.score(p)
            for rnd in range(a.rounds):
                for n, eng in engines.items():
                    t = _best(lambda: eng.prefill_logits(p))
                    s = _best(lambda: eng.score(p))
                    ms[n]["ttft"].append(t)
                    ms[n]["score"].append(s)
                    emit({"model": a.model, "arm": n, "T": T, "round": rnd,
                          "ttft_ms": round(t, 3), "score_ms": round(s, 3)})
            for n in names:
                t, s = statistics.median(ms[n]["ttft"]), statistics.median(ms[n]["score"])
                flop = 2.0 * T * cfg.vocab_size * cfg.hidden_size
                emit({"model": a.model, "summary_T": T, "arm": n, "ttft_ms": round(t, 3),
                      "score_ms": round(s, 3), "score_over_ttft": round(s / t, 4),
                      "ttft_spread_ms": round(max(ms[n]["ttft"]) - min(ms[n]["ttft"]), 3),
                      "score_spread_ms": round(max(ms[n]["score"]) - min(ms[n]["score"]), 3),
                      "head_tflops_from_difference": round(flop / ((s - t) * 1e-3) / 1e12, 2)
                      if s > t else None})
        if a.forced >= 2:
            T = a.forced
            p = toks[:T]
            for n, eng in engines.items():
                eng.score(p)
                eng.forced_logits(p[:1], p[1:])
                s = statistics.median(_best(lambda: eng.score(p)) for _ in range(a.rounds))
                f = statistics.median(_best(lambda: eng.forced_logits(p[:1], p[1:]), 1)
                                      for _ in range(a.rounds))
                emit({"model": a.model, "summary_forced_T": T, "arm": n, "score_ms": round(s, 3),
                      "forced_logits_ms": round(f, 3), "forced_over_score": round(f / s, 2)})
    finally:
        for eng in engines.values():
            eng.close()
        shutil.rmtree(d, ignore_errors=True)
        if out:
            out.close()


if __name__ == "__main__":
    main()
