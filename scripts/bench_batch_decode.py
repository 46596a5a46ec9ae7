"""Lock-step batched decode (NativeLlama.generate_batch) against batch-1 decode.

One process opens one random-init engine of a named architecture and alternates, per round,
the batch-1 arm (a one-token generate, then ``continue_`` for ``--steps`` graph-replayed decode
steps) with the batched arms B in ``--batches`` (``generate_batch`` of B distinct prompts for
``--steps`` eager lock-step steps).  Every figure is the engine's device-timed p50 per step.
One JSON line per measurement, then one summary line per B: t_B, t_1, the aggregate rate
B / t_B against 1 / t_1, and whether the batched step beats break-even (t_B < B t_1).

    python scripts/bench_batch_decode.py --out profiles/batch_decode_ab.jsonl
"""
import argparse
import json
import shutil
import statistics
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--batches", default="1,2,4,8")
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--prompt", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch

    from cake_amd.engine import NativeLlama, write_config
    from cake_amd.models.llama3.config import preset
    if not torch.cuda.is_available():
        raise SystemExit("bench_batch_decode: needs a GPU (no timing without one)")
    cfg = preset(a.model)
    batches = [int(b) for b in a.batches.split(",") if b]
    out = open(a.out, "w") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    g = torch.Generator().manual_seed(1234)
    prompts = [torch.randint(0, cfg.vocab_size, (a.prompt,), generator=g).tolist()
               for _ in range(max(batches))]
    d = tempfile.mkdtemp(prefix="cake_batch_decode_cfg_")
    write_config(d, cfg)
    try:
        eng = NativeLlama(d, max_seq=a.prompt + a.steps + 64, dtype="bf16", random_init=True, seed=1)
        try:
            def one():
                eng.generate(prompts[0], 1, eos_ids=[], repeat_penalty=1.0)
                return eng.continue_(a.steps, eos_ids=[])

            def many(B):
                return eng.generate_batch(prompts[:B], a.steps + 1, eos_ids=[], repeat_penalty=1.0)

            one()                      # warm: graphs, buffers
            for B in batches:
                many(B)
            t1, tb = [], {B: [] for B in batches}
            for rnd in range(a.rounds):
                r = one()
                t1.append(r.p50_ms)
                emit({"model": a.model, "arm": "batch-1 continue_", "round": rnd,
                      "p50_ms": round(r.p50_ms, 5), "p99_ms": round(r.p99_ms, 5),
                      "tokens_per_s": round(1e3 / r.p50_ms, 2)})
                for B in batches:
                    res = many(B)
                    tb[B].append(res[0].p50_ms)
                    emit({"model": a.model, "arm": f"generate_batch B={B}", "round": rnd,
                          "p50_ms": round(res[0].p50_ms, 5), "p99_ms": round(res[0].p99_ms, 5),
                          "aggregate_tokens_per_s": round(B * 1e3 / res[0].p50_ms, 2),
                          "tokens": [len(x.tokens) for x in res]})
            m1 = statistics.median(t1)
            for B in batches:
                mb = statistics.median(tb[B])
                emit({"model": a.model, "summary": f"B={B}", "t_B_ms": round(mb, 5),
                      "t_1_ms": round(m1, 5), "spread_ms": round(max(tb[B]) - min(tb[B]), 5),
                      "t_B_over_B_t_1": round(mb / (B * m1), 4), "beats_break_even": mb < B * m1,
                      "aggregate_tokens_per_s": round(B * 1e3 / mb, 2),
                      "batch_1_tokens_per_s": round(1e3 / m1, 2)})
        finally:
            eng.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)
        if out:
            out.close()


if __name__ == "__main__":
    main()
