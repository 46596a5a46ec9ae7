"""A/B of the FP8 MFMA prefill (weights="fp8", prefill="fp8") against the 16-bit engine and the
fp8-weights engine whose prefill dequantises every projection (the parent's path).

TTFT table: one process opens the random-init engine of a named architecture once per arm
(bf16; weights=fp8; weights=fp8 + prefill=fp8) and alternates the arms: per prompt length,
round and arm the best of three warm prefills (generate(prompt, 1).prefill_s), `--rounds`
rounds.  One JSON line per measurement, then one summary line per length with each arm's
median and round-to-round spread and whether the bar holds (new arm below the fp8 arm by more
than twice that arm's spread).

    python scripts/bench_w8a8_prefill.py --out profiles/w8a8_prefill_ab.jsonl
    python scripts/bench_w8a8_prefill.py --model llama3-70b --arms fp8 --ttft 512,2048 \\
        --out profiles/w8a8_prefill_ab_70b.jsonl

Per-shape table (`--shapes`): cake_gemm_w8a8 (its planner's tile, and every tile) against the
bf16 cake_gemm on its shipped plan for the four projection shapes of the 8B and 70B models at
512 and 2048 tokens, TFLOP/s from graph-captured timing (INNER launches per hipGraph, median
replay / INNER, as scripts/tune_sd_gemm.py).  The w8a8 figure includes nothing but the GEMM;
`quant_us` is the activation quantiser's launch on the same rows.

    python scripts/bench_w8a8_prefill.py --shapes --out profiles/w8a8_gemm_shapes.jsonl

Kernel table: run `--window 2048 --arms new` (the engine's open, one warm-up and one prefill of
the new arm, nothing else) under `rocprofv3 --kernel-trace --stats --output-format csv` in a
run of its own (the weight initialisers and the on-load quantiser are in the trace too), then

    python scripts/bench_w8a8_prefill.py --table <..._kernel_stats.csv> > profiles/w8a8_prefill2048_kernels.txt
"""
import argparse
import csv
import json
import shutil
import statistics
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

ARMS = {"bf16": dict(weights="model"), "fp8": dict(weights="fp8"),
        "fp8+prefill": dict(weights="fp8", prefill="fp8")}
INNER, REPS = 10, 10


def _open(cfg_dir, max_seq, **kw):
    from cake_amd.engine import NativeLlama
    return NativeLlama(cfg_dir, max_seq=max_seq, dtype="bf16", device=0, random_init=True, seed=1,
                       **kw)


def _prompt(cfg, n):
    import torch
    g = torch.Generator().manual_seed(1234)
    return torch.randint(0, cfg.vocab_size, (n,), generator=g).tolist()


def _emitter(path):
    out = open(path, "w") if path else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    return emit, out


def run(a):
    import torch
    from cake_amd.engine import write_config
    from cake_amd.models.llama3.config import preset
    if not torch.cuda.is_available():
        raise SystemExit("bench_w8a8_prefill: needs a GPU (no timing without one)")
    cfg = preset(a.model)
    d = tempfile.mkdtemp(prefix="cake_w8a8_cfg_")
    write_config(d, cfg)
    lengths = [a.window] if a.window else [int(x) for x in a.ttft.split(",") if x]
    names = [n for n in ARMS if a.arms == "all" or (a.arms == "fp8" and n != "bf16")
             or (a.arms == "new" and n == "fp8+prefill")]
    emit, out = _emitter(a.out)
    engines = {}
    try:
        for n in names:
            engines[n] = _open(d, max(lengths) + 64, **ARMS[n])
        if a.window:  # the profiled window: one warm-up and one prefill per arm
            p = _prompt(cfg, a.window)
            for n, eng in engines.items():
                eng.generate(p, 1, temperature=0.0, eos_ids=[])
                r = eng.generate(p, 1, temperature=0.0, eos_ids=[])
                emit({"window": n, "prompt": a.window, "ttft_ms": round(r.prefill_s * 1e3, 3)})
            return
        tokens = {}
        for T in lengths:
            p = _prompt(cfg, T)
            ms = {n: [] for n in names}
            for n, eng in engines.items():  # warm: plans, buffers, first launches
                tokens[(T, n)] = eng.generate(p, 1, temperature=0.0, eos_ids=[]).tokens
            for rnd in range(a.rounds):
                for n, eng in engines.items():
                    best = min(eng.generate(p, 1, temperature=0.0, eos_ids=[]).prefill_s
                               for _ in range(3))
                    ms[n].append(best * 1e3)
                    emit({"model": a.model, "arm": n, "ttft_prompt": T, "round": rnd,
                          "ttft_ms": round(best * 1e3, 3)})
            s = {"model": a.model, "summary_prompt": T}
            for n in names:
                s[n] = {"median_ms": round(statistics.median(ms[n]), 3),
                        "spread_ms": round(max(ms[n]) - min(ms[n]), 3)}
            gain = s["fp8"]["median_ms"] - s["fp8+prefill"]["median_ms"]
            s["gain_over_fp8_ms"] = round(gain, 3)
            s["bar_met"] = bool(gain > 2 * s["fp8"]["spread_ms"])
            if "bf16" in s:
                s["below_bf16"] = bool(s["fp8+prefill"]["median_ms"] < s["bf16"]["median_ms"])
            s["first_token"] = {n: tokens[(T, n)] for n in names}
            emit(s)
    finally:
        for eng in engines.values():
            eng.close()
        shutil.rmtree(d, ignore_errors=True)
        if out:
            out.close()


def timeit(fn):
    """GPU time per call in us: INNER calls captured in one hipGraph, median replay / INNER."""
    import torch
    fn()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(INNER):
            fn()
    g.replay()
    ts = []
    for _ in range(REPS):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        g.replay()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e) / INNER)
    del g
    return statistics.median(ts) * 1e3


def projection_shapes(cfg):
    """(name, epilogue, output features N, K) of the four per-layer projections."""
    H, I = cfg.hidden_size, cfg.intermediate_size
    hd = H // cfg.num_attention_heads
    nq, nk = cfg.num_attention_heads * hd, cfg.num_key_value_heads * hd
    return [("qkv", "store", nq + 2 * nk, H), ("o", "resid32", H, nq),
            ("gate|up", "swiglu", I, H), ("down", "resid32", H, I)]


def shapes(a):
    import torch
    from cake_amd.models.llama3.config import preset
    from cake_amd.ops import gemm as G
    from cake_amd.ops import hip as K_
    if not torch.cuda.is_available():
        raise SystemExit("bench_w8a8_prefill: needs a GPU (no timing without one)")
    emit, out = _emitter(a.out)
    dt, dev = torch.bfloat16, "cuda"
    try:
        for model in ("llama3-8b", "llama3-70b"):
            for name, epi, N, K in projection_shapes(preset(model)):
                Nw = 2 * N if epi == "swiglu" else N
                w = (torch.randn(Nw, K, device=dev) * K ** -0.5).to(dt)
                w8 = torch.empty(Nw, K, device=dev, dtype=torch.uint8)
                sw = torch.empty(Nw, device=dev)
                K_.quant_rows_fp8(w, w8, sw)
                for T in (512, 2048):
                    x = (torch.randn(T, K, device=dev) * 0.5).to(dt)
                    a8 = torch.empty(T, K, device=dev, dtype=torch.uint8)
                    sa = torch.empty(T, device=dev)
                    K_.quant_rows_fp8(x, a8, sa)
                    r32 = torch.zeros(T, N, device=dev)
                    o16 = torch.empty(T, N, device=dev, dtype=dt)
                    o8 = r32 if epi == "resid32" else o16
                    flop = 2.0 * T * Nw * K
                    t16 = timeit(lambda: G.linear(x, w, epi=epi, out=None if epi == "resid32" else o16,
                                                  resid=r32 if epi == "resid32" else None))
                    rec = {"model": model, "proj": name, "epi": epi, "T": T, "N": Nw, "K": K,
                           "bf16_plan": list(G.plan(T, Nw, K, epi)), "bf16_us": round(t16, 2),
                           "bf16_tflops": round(flop / t16 / 1e6, 1),
                           "quant_us": round(timeit(lambda: K_.quant_rows_fp8(x, a8, sa)), 2),
                           "w8a8_plan": K_.gemm_w8a8_plan(T, Nw, K)}
                    for cfg in range(K_.gemm_w8a8_num_cfgs()):
                        t8 = timeit(lambda: K_.gemm_w8a8(a8, sa, w8, sw, o8, epi, cfg=cfg))
                        rec[f"w8a8_cfg{cfg}_us"] = round(t8, 2)
                        rec[f"w8a8_cfg{cfg}_tflops"] = round(flop / t8 / 1e6, 1)
                    p = rec["w8a8_plan"]
                    rec["w8a8_us"], rec["w8a8_tflops"] = rec[f"w8a8_cfg{p}_us"], rec[f"w8a8_cfg{p}_tflops"]
                    emit(rec)
                del w, w8
                torch.cuda.empty_cache()
    finally:
        if out:
            out.close()


def table(path):
    """Kernels of a rocprofv3 --stats kernel_stats.csv by total time."""
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((float(r["TotalDurationNs"]), int(r["Calls"]), r["Name"]))
    rows.sort(reverse=True)
    total = sum(r[0] for r in rows) or 1.0
    print(f"{'kernel':<72} {'calls':>6} {'total_ms':>9} {'avg_us':>9} {'share':>6}")
    for ns, calls, name in rows[:24]:
        short = name if len(name) <= 72 else name[:69] + "..."
        print(f"{short:<72} {calls:>6} {ns / 1e6:>9.3f} {ns / calls / 1e3:>9.2f} {ns / total:>6.1%}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--model", default="llama3-8b", choices=["llama3-8b", "llama3-70b"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ttft", default="128,512,2048,4096", help="prompt lengths of the TTFT rows")
    ap.add_argument("--arms", default="all", choices=["all", "fp8", "new"],
                    help="fp8: the two fp8-weight arms only (70B: the 16-bit arm's memory); "
                         "new: the fp8 MFMA prefill arm only (--window)")
    ap.add_argument("--out", default=None, help="JSON lines file")
    ap.add_argument("--shapes", action="store_true", help="the per-shape GEMM table")
    ap.add_argument("--window", type=int, default=0, metavar="T",
                    help="one warm T-token prefill per arm and nothing else (for rocprofv3)")
    ap.add_argument("--table", default=None, metavar="KERNEL_STATS_CSV",
                    help="print the kernel table of a rocprofv3 --stats run and exit")
    a = ap.parse_args()
    if a.table:
        table(a.table)
    elif a.shapes:
        shapes(a)
    else:
        run(a)


if __name__ == "__main__":
    main()
