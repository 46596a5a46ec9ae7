"""A/B of batch-1 decode over a 16-bit and an FP8 (e4m3) KV cache (kv="model" / kv="fp8").

The sibling of scripts/bench_mxfp4_decode.py for the third storage format.  One process opens
the random-init engine of a named architecture once per (weight setting, kv arm) at
`--max-seq` and alternates the arms: per round, prompt length and arm a prefill of that many
tokens, a warm-up, then `--steps` timed decode steps, reading the device-timed per-token p50
the engine reports.  One JSON line per measurement: ms/token, the bytes a step reads (the
weight stream plus the live K and V rows of every layer), kv_bytes(), and the time and byte
ratios of the fp8 arm against the 16-bit arm of the same round.  Then TTFT at the `--ttft`
prompt lengths (the fp8 arm's prefill widens the live prefix once per layer).

    python scripts/bench_kv8_decode.py --out profiles/kv8_decode_ab.jsonl

Kernel table: run `--window --kv-arms <arm> --prompts <T>` (one decode window of one kv arm
at one context, nothing else) under `rocprofv3 --kernel-trace --stats --output-format csv`,
one run per arm and context, then

    python scripts/bench_kv8_decode.py --table model@2048=<csv> fp8@2048=<csv> ... \
        > profiles/kv8_decode8b_kernel_table.txt
"""
import argparse
import csv
import json
import re
import shutil
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))

from bench_fp8_decode import _prompt, _window  # noqa: E402  (adds the repo to sys.path)

WEIGHTS = {"model": ("model", "model"), "mxfp4": ("mxfp4", "mxfp4")}  # name -> weights, head
KV_ARMS = ("model", "fp8")


def _open(cfg_dir, weights, head, kv, max_seq):
    from cake_amd.engine import NativeLlama
    return NativeLlama(cfg_dir, max_seq=max_seq, dtype="bf16", device=0, random_init=True, seed=1,
                       weights=weights, head=head, kv=kv)


def run(a):
    import torch
    from cake_amd.engine import write_config
    from cake_amd.models.llama3.config import preset
    if not torch.cuda.is_available():
        raise SystemExit("bench_kv8_decode: needs a GPU (no timing without one)")
    cfg = preset(a.model)
    d = tempfile.mkdtemp(prefix="cake_kv8_cfg_")
    write_config(d, cfg)
    lens = [int(x) for x in a.prompts.split(",") if x]
    ttft = [int(x) for x in a.ttft.split(",") if x]
    settings = [w for w in a.weights.split(",") if w]
    if max(lens + ttft) + 1 + a.warmup + a.steps > a.max_seq:
        raise SystemExit("bench_kv8_decode: a prompt plus the decode window exceeds --max-seq")
    V, H = cfg.vocab_size, cfg.hidden_size
    out = open(a.out, "w") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    engines = {}
    try:
        for w in settings:
            for kv in a.kv_arms.split(","):
                engines[w, kv] = _open(d, *WEIGHTS[w], kv, a.max_seq)
        for eng in engines.values():  # cold: first launches + graph capture
            eng.generate(_prompt(cfg, 32), 2, temperature=0.0, eos_ids=[])
        if a.window:  # the profiled window: nothing else runs
            for T in lens:
                for (w, kv), eng in engines.items():
                    r = _window(eng, _prompt(cfg, T), a.warmup, a.steps)
                    emit({"window": f"{w}/{kv}", "prompt": T, "p50_ms": round(r.p50_ms, 4)})
            return
        for rnd in range(a.rounds):
            for T in lens:
                prompt = _prompt(cfg, T)
                for w in settings:
                    recs = {}
                    for kv in KV_ARMS:
                        eng = engines[w, kv]
                        r = _window(eng, prompt, a.warmup, a.steps)
                        # a step streams every weight once (an untied embedding is only
                        # indexed) and the live K and V rows of every layer
                        wbytes = eng.weight_bytes() - (0 if cfg.tie_word_embeddings else 2 * V * H)
                        live = T + 1 + a.warmup + a.steps / 2  # mean live length of the window
                        kvread = eng.kv_bytes() / a.max_seq * live
                        recs[kv] = {"model": a.model, "weights": w, "kv": kv, "round": rnd,
                                    "prompt": T, "steps": a.steps,
                                    "p50_ms_per_token": round(r.p50_ms, 4),
                                    "p99_ms_per_token": round(r.p99_ms, 4),
                                    "tok_per_s_p50": round(1e3 / r.p50_ms, 2),
                                    "kv_bytes": eng.kv_bytes(),
                                    "kv_read_GB_per_token": round(kvread / 1e9, 4),
                                    "GB_per_token": round((wbytes + kvread) / 1e9, 4)}
                    f8, m = recs["fp8"], recs["model"]
                    f8["time_vs_16bit_kv"] = round(f8["p50_ms_per_token"] / m["p50_ms_per_token"], 4)
                    f8["bytes_vs_16bit_kv"] = round(f8["GB_per_token"] / m["GB_per_token"], 4)
                    f8["ms_saved"] = round(m["p50_ms_per_token"] - f8["p50_ms_per_token"], 4)
                    for rec in recs.values():
                        emit(rec)
        for T in ttft:
            p = _prompt(cfg, T)
            for (w, kv), eng in engines.items():
                eng.generate(p, 1, temperature=0.0, eos_ids=[])  # warm: plans, buffers
                best = min(eng.generate(p, 1, temperature=0.0, eos_ids=[]).prefill_s
                           for _ in range(3))
                emit({"model": a.model, "weights": w, "kv": kv, "ttft_prompt": T,
                      "ttft_ms": round(best * 1e3, 3)})
    finally:
        for eng in engines.values():
            eng.close()
        shutil.rmtree(d, ignore_errors=True)
        if out:
            out.close()


# ---- kernel table from a rocprofv3 --stats kernel_stats.csv ------------------------------

def _classify(name):
    """Row label of a decode attention / QKV launch, or None."""
    m = re.search(r"(attn2_decode_kv8|attn2_decode|qkv_rope|"
                  r"dequant_kv_fp8|rope_kv_vec_q8|rope_kv_vec)_kernel<([^>]*)>", name)
    if not m:
        return None
    targs = [t.strip() for t in m.group(2).split(",")]
    if m.group(1) == "qkv_rope":  # <F, ...>: the weight format cake::W16 / W8 / W4
        return "qkv_rope" + {"W16": "", "W8": "_w8", "W4": "_w4"}[targs[0].split("::")[-1]]
    if m.group(1).startswith("attn2"):  # <DT, HD, NREP, PFD>
        return f"{m.group(1)} (prefetch {re.sub(r'[^0-9]', '', targs[3])})"
    return m.group(1)


def table(specs):
    """Per-kernel calls and mean time of each `label=kernel_stats.csv` run (a run holds one
    kv arm at one context, both weight settings: qkv_rope is the 16-bit-weight engine's
    launch, qkv_rope_w4 the mxfp4 engine's)."""
    print(f"{'run':<12} {'kernel':<34} {'calls':>8} {'avg_us':>9} {'total_ms':>10}")
    for spec in specs:
        run_label, _, path = spec.partition("=")
        rows = {}
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                label = _classify(r["Name"])
                if label:
                    e = rows.setdefault(label, {"calls": 0, "ns": 0.0})
                    e["calls"] += int(r["Calls"])
                    e["ns"] += float(r["TotalDurationNs"])
        for label in sorted(rows):
            e = rows[label]
            print(f"{run_label:<12} {label:<34} {e['calls']:>8} {e['ns'] / e['calls'] / 1e3:>9.2f} "
                  f"{e['ns'] / 1e6:>10.2f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--model", default="llama3-8b", choices=["llama3-8b", "llama3-70b"])
    ap.add_argument("--weights", default="model,mxfp4",
                    help="comma-separated weight settings: model, mxfp4 (mxfp4 projections and head)")
    ap.add_argument("--prompts", default="128,2048,8000", help="prompt lengths of the decode rows")
    ap.add_argument("--max-seq", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--ttft", default="512,2048", help="prompt lengths of the TTFT rows ('' = none)")
    ap.add_argument("--out", default=None, help="JSON lines file")
    ap.add_argument("--window", action="store_true",
                    help="one decode window per arm and prompt length and nothing else (for a "
                         "rocprofv3 run)")
    ap.add_argument("--kv-arms", default=",".join(KV_ARMS),
                    help="kv arms to open (the A/B needs both; a profiled --window takes one)")
    ap.add_argument("--table", default=None, nargs="+", metavar="LABEL=KERNEL_STATS_CSV",
                    help="print the attention / QKV kernel table of rocprofv3 --stats runs and exit")
    a = ap.parse_args()
    bad = [w for w in a.weights.split(",") if w and w not in WEIGHTS]
    if bad:
        ap.error(f"--weights: unknown setting {bad[0]!r} (choose from {', '.join(WEIGHTS)})")
    bad = [k for k in a.kv_arms.split(",") if k not in KV_ARMS]
    if bad or (not a.window and not a.table and a.kv_arms != ",".join(KV_ARMS)):
        ap.error("--kv-arms: model and / or fp8; fewer than both only with --window")
    if a.table:
        table(a.table)
    else:
        run(a)


if __name__ == "__main__":
    main()
