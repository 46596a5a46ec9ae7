"""A/B/C of batch-1 decode: model dtype, FP8 (e4m3) and MXFP4 weight-only projections.

The sibling of scripts/bench_fp8_decode.py with a free choice of arms.  One process opens the
random-init engine of a named architecture once per arm of `--arms` (bf16, fp8, mxfp4) and
alternates them: per round and arm a 32-token prompt, a warm-up, then `--steps` timed decode
steps, reading the device-timed per-token p50 the engine reports.  One JSON line per arm and
round (ms/token, bytes per token from weight_bytes(), the implied TB/s, and the time and
byte ratios against the fp8 and bf16 arms of the same round), then TTFT at the `--ttft`
prompt lengths (the quantised arms' prefill dequantises every projection once per layer).

    python scripts/bench_mxfp4_decode.py --out profiles/mxfp4_decode_ab.jsonl
    python scripts/bench_mxfp4_decode.py --model llama3-70b --out profiles/mxfp4_decode_ab_70b.jsonl
    python scripts/bench_mxfp4_decode.py --sweep --out profiles/mxfp4_decode_tuning_sweep.jsonl

Kernel table: run `--window` (one decode window per arm, nothing else) under
`rocprofv3 --kernel-trace --stats --output-format csv`, in a run of its own, then

    python scripts/bench_mxfp4_decode.py --table <..._kernel_stats.csv> > profiles/mxfp4_decode8b_kernel_table.txt

which puts every `_w4` kernel next to its `_w8` and 16-bit twins with bytes and TB/s.
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

from bench_fp8_decode import _open, _prompt, _window  # noqa: E402  (adds the repo to sys.path)

ARMS = {"bf16": "model", "fp8": "fp8", "mxfp4": "mxfp4"}
BYTES_PER_ELEMENT = {"bf16": 2.0, "fp8": 1.0, "mxfp4": 0.53125}


def _setup(a):
    import torch
    from cake_amd.engine import write_config
    from cake_amd.models.llama3.config import preset
    if not torch.cuda.is_available():
        raise SystemExit("bench_mxfp4_decode: needs a GPU (no timing without one)")
    cfg = preset(a.model)
    d = tempfile.mkdtemp(prefix="cake_mxfp4_cfg_")
    write_config(d, cfg)
    return cfg, d


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
    cfg, d = _setup(a)
    names = [n for n in a.arms.split(",") if n]
    ttft = [int(x) for x in a.ttft.split(",") if x]
    max_seq = max(4096, max(ttft + [0]) + 64)
    # every arm stays open: its projections, plus embedding / head / scratch each
    H, I, L, V = cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.vocab_size
    hd = H // cfg.num_attention_heads
    proj = L * ((cfg.num_attention_heads + 2 * cfg.num_key_value_heads) * hd * H +
                H * cfg.num_attention_heads * hd + 3 * I * H)
    need = int(sum(BYTES_PER_ELEMENT[n] for n in names) * proj) + len(names) * (
        4 * V * H + 4 * I * H + (3 << 30))
    free, _total = torch.cuda.mem_get_info()
    if free < need:
        raise SystemExit(f"bench_mxfp4_decode: {a.model} needs ~{need >> 30} GiB of HBM for "
                         f"arms {names}, {free >> 30} GiB free")
    emit, out = _emitter(a.out)
    arms = {}
    try:
        for n in names:
            arms[n] = _open(d, ARMS[n], max_seq)
        prompt = _prompt(cfg, a.prompt_len)
        for eng in arms.values():  # cold: first launches + graph capture
            eng.generate(prompt, 2, temperature=0.0, eos_ids=[])
        if a.window:  # the profiled window: nothing else runs
            for n, eng in arms.items():
                emit({"window": n, "p50_ms": round(_window(eng, prompt, a.warmup, a.steps).p50_ms, 4)})
            return
        for rnd in range(a.rounds):
            recs = {}
            for n, eng in arms.items():
                r = _window(eng, prompt, a.warmup, a.steps)
                nbytes = eng.weight_bytes()
                # the decode step streams every weight once, except that an untied
                # embedding table is only indexed (one row)
                stream = nbytes - (0 if cfg.tie_word_embeddings else 2 * V * H)
                recs[n] = {"model": a.model, "arm": n, "round": rnd, "steps": a.steps,
                           "p50_ms_per_token": round(r.p50_ms, 4),
                           "p99_ms_per_token": round(r.p99_ms, 4),
                           "tok_per_s_p50": round(1e3 / r.p50_ms, 2),
                           "weight_bytes": nbytes, "bytes_per_token": stream,
                           "implied_TBps": round(stream / (r.p50_ms * 1e-3) / 1e12, 3)}
            for n, rec in recs.items():
                for ref in ("fp8", "bf16"):
                    if ref in recs and ref != n:
                        rec[f"time_vs_{ref}"] = round(
                            rec["p50_ms_per_token"] / recs[ref]["p50_ms_per_token"], 3)
                        rec[f"bytes_vs_{ref}"] = round(
                            rec["bytes_per_token"] / recs[ref]["bytes_per_token"], 3)
                emit(rec)
        for T in ttft:
            p = _prompt(cfg, T)
            for n, eng in arms.items():
                eng.generate(p, 1, temperature=0.0, eos_ids=[])  # warm: plans, buffers
                best = min(eng.generate(p, 1, temperature=0.0, eos_ids=[]).prefill_s
                           for _ in range(3))
                emit({"model": a.model, "arm": n, "ttft_prompt": T, "ttft_ms": round(best * 1e3, 3)})
    finally:
        for eng in arms.values():
            eng.close()
        shutil.rmtree(d, ignore_errors=True)
        if out:
            out.close()


# one-at-a-time variations of the three MXFP4 launch geometries (kind, U, prefetch, max_blocks)
SWEEP = [None, ("swiglu", 2, 4, 2048), ("swiglu", 2, 4, 512), ("swiglu", 2, 0, 1024),
         ("qkv", 2, 4, 512), ("qkv", 2, 0, 1024), ("x16", 1, 4, 1024), ("x16", 4, 4, 1024),
         ("x16", 2, 2, 1024), ("x16", 2, 4, 512), ("x16", 2, 0, 1024), None]


def sweep(a):
    """p50 ms/token of the mxfp4 arm per launch geometry: a fresh engine per setting (the
    captured graphs bake the geometry in), the default first and last (drift)."""
    from cake_amd.ops import hip as K_
    cfg, d = _setup(a)
    prompt = _prompt(cfg, a.prompt_len)
    base = {k: K_.get_gemv_w4_tuning(k) for k in K_.GEMV_W4_KINDS}
    emit, out = _emitter(a.out)

    def restore():
        for k, (U, pf, mb) in base.items():
            K_.set_gemv_w4_tuning(k, U=U, prefetch=pf, max_blocks=mb)

    try:
        for setting in SWEEP:
            restore()
            if setting:
                K_.set_gemv_w4_tuning(setting[0], U=setting[1], prefetch=setting[2],
                                      max_blocks=setting[3])
            eng = _open(d, "mxfp4", 4096)
            try:
                eng.generate(prompt, 2, temperature=0.0, eos_ids=[])
                p50 = [round(_window(eng, prompt, a.warmup, a.steps).p50_ms, 4) for _ in range(2)]
            finally:
                eng.close()
            emit({"model": a.model, "setting": setting or "default",
                  "tuning": {k: K_.get_gemv_w4_tuning(k) for k in base},
                  "p50_ms_per_token": p50})
    finally:
        restore()
        shutil.rmtree(d, ignore_errors=True)
        if out:
            out.close()


# ---- kernel table from a rocprofv3 --stats kernel_stats.csv ------------------------------

H, I, NH, NKV, HD = 4096, 14336, 32, 8, 128  # llama3-8b
NQKV = (NH + 2 * NKV) * HD
SUFFIXES = ("", "_w8", "_w4")


def _bytes(n, k, sfx):
    return {"": 2 * n * k, "_w8": n * k + 4 * n, "_w4": n * k // 2 + n * k // 32}[sfx]


def _classify(name):
    """(row label, twin key, bytes) of a decode GEMV kernel name, or None."""
    # the weight format is the kernels' first template argument (cake::W16 / W8 / W4)
    m = re.search(r"(qkv_rope|swiglu|gemv_x16)_kernel<(?:cake::)?W(16|8|4), ([^>]*)>", name)
    if not m:
        # the MXFP4 gemv_x16 is a kernel of its own (gemv_w4_x16.hip): <DT, U, PFC, NX, ACCUM>
        m = re.search(r"(gemv_x16)_w(4)_kernel<([^>]*)>", name)
    if not m:
        return None
    kind, targs = m.group(1), [t.strip() for t in m.group(3).split(",")]
    sfx = {"16": "", "8": "_w8", "4": "_w4"}[m.group(2)]
    if kind == "qkv_rope":
        return "qkv_rope" + sfx, "qkv_rope", _bytes(NQKV, H, sfx)
    if kind == "swiglu":
        return "swiglu" + sfx, "swiglu", _bytes(2 * I, H, sfx)
    # template <F, DT, U, PFC, NX, ACCUM>, F stripped: NX tells o_proj (K = 4096 -> 2) from down_proj (14336 -> 7)
    nx = int(re.sub(r"\D", "", targs[3]) or 0)
    if nx == 7:
        return "down_proj" + sfx, "down_proj", _bytes(H, I, sfx)
    return "o_proj" + sfx, "o_proj", _bytes(H, H, sfx)


def table(path):
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            c = _classify(r["Name"])
            if not c:
                continue
            label, twin, nbytes = c
            e = rows.setdefault(label, {"twin": twin, "bytes": nbytes, "calls": 0, "ns": 0.0})
            e["calls"] += int(r["Calls"])
            e["ns"] += float(r["TotalDurationNs"])

    def avg(e):
        return e["ns"] / e["calls"] / 1e3

    print(f"{'kernel':<14} {'calls':>7} {'avg_us':>8} {'MB':>8} {'TB/s':>6} {'vs 16-bit':>10} "
          f"{'vs _w8':>8}")
    for twin in ("qkv_rope", "o_proj", "swiglu", "down_proj"):
        for sfx in SUFFIXES:
            e = rows.get(twin + sfx)
            if not e:
                continue
            rel = [f"{avg(e) / avg(rows[twin + s]):.2f}x" if twin + s in rows else "-"
                   for s in ("", "_w8")]
            print(f"{twin + sfx:<14} {e['calls']:>7} {avg(e):>8.2f} {e['bytes'] / 1e6:>8.1f} "
                  f"{e['bytes'] / avg(e) / 1e6:>6.2f} {rel[0]:>10} {rel[1]:>8}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--model", default="llama3-8b", choices=["llama3-8b", "llama3-70b"])
    ap.add_argument("--arms", default="bf16,fp8,mxfp4",
                    help="comma-separated arms to open and alternate: bf16, fp8, mxfp4")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--prompt-len", type=int, default=32)
    ap.add_argument("--ttft", default="512,2048", help="prompt lengths of the TTFT rows ('' = none)")
    ap.add_argument("--out", default=None, help="JSON lines file")
    ap.add_argument("--window", action="store_true",
                    help="one decode window per arm and nothing else (for a rocprofv3 run)")
    ap.add_argument("--sweep", action="store_true",
                    help="mxfp4 arm only: p50 per launch geometry of the three MXFP4 GEMV kinds")
    ap.add_argument("--table", default=None, metavar="KERNEL_STATS_CSV",
                    help="print the 8B kernel table of a rocprofv3 --stats run and exit")
    a = ap.parse_args()
    bad = [n for n in a.arms.split(",") if n and n not in ARMS]
    if bad:
        ap.error(f"--arms: unknown arm {bad[0]!r} (choose from {', '.join(ARMS)})")
    if a.table:
        table(a.table)
    elif a.sweep:
        sweep(a)
    else:
        run(a)


if __name__ == "__main__":
    main()
