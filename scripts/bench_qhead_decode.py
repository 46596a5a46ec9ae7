"""A/B of batch-1 decode with a quantised lm_head: weights in {fp8, mxfp4} x head in {model, fp8,
mxfp4}.

The sibling of scripts/bench_mxfp4_decode.py.  One process opens the random-init engine of a
named architecture once per arm (`--arms`, "weights:head" pairs) and alternates them: per
round and arm a 32-token prompt, a warm-up, then `--steps` timed decode steps, reading the
device-timed per-token p50 the engine reports.  One JSON line per arm and round: ms/token,
bytes per token from weight_bytes(), the implied TB/s, and the time and byte ratios against
the head=model arm with the same weights in the same round.

    python scripts/bench_qhead_decode.py --out profiles/qhead_decode_ab.jsonl
    python scripts/bench_qhead_decode.py --model llama3-70b --rounds 3 \\
        --arms mxfp4:model,mxfp4:fp8,mxfp4:mxfp4 --out profiles/qhead_decode_ab_70b.jsonl
    python scripts/bench_qhead_decode.py --sweep --out profiles/qhead_decode_tuning_sweep.jsonl

Kernel table: run `--window` (one decode window per arm, nothing else) under
`rocprofv3 --kernel-trace --stats --output-format csv`, in a run of its own, then

    python scripts/bench_qhead_decode.py --table <..._kernel_stats.csv> > profiles/qhead_decode8b_kernel_table.txt

which lists the head launches (fused greedy tail and plain, per format) with the bytes they
stream and TB/s.
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

FORMATS = ("model", "fp8", "mxfp4")
DEFAULT_ARMS = ",".join(f"{w}:{h}" for w in ("fp8", "mxfp4") for h in FORMATS)
BYTES_PER_ELEMENT = {"model": 2.0, "fp8": 1.0, "mxfp4": 0.53125}


def _open(cfg_dir, weights, head, max_seq):
    from cake_amd.engine import NativeLlama
    return NativeLlama(cfg_dir, max_seq=max_seq, dtype="bf16", device=0, random_init=True, seed=1,
                       weights=weights, head=head)


def _setup(a):
    import torch
    from cake_amd.engine import write_config
    from cake_amd.models.llama3.config import preset
    if not torch.cuda.is_available():
        raise SystemExit("bench_qhead_decode: needs a GPU (no timing without one)")
    cfg = preset(a.model)
    d = tempfile.mkdtemp(prefix="cake_qhead_cfg_")
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


def _arms(spec):
    arms = []
    for s in spec.split(","):
        if not s:
            continue
        w, _, h = s.partition(":")
        if w not in FORMATS or h not in FORMATS:
            raise SystemExit(f"--arms: {s!r} is not weights:head with each of {', '.join(FORMATS)}")
        arms.append((w, h))
    return arms


def run(a):
    import torch
    cfg, d = _setup(a)
    names = _arms(a.arms)
    H, I, L, V = cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.vocab_size
    hd = H // cfg.num_attention_heads
    proj = L * ((cfg.num_attention_heads + 2 * cfg.num_key_value_heads) * hd * H +
                H * cfg.num_attention_heads * hd + 3 * I * H)
    # every arm stays open: projections, embedding, head (+ its 16-bit temporary at open),
    # scratch
    need = int(sum(BYTES_PER_ELEMENT[w] for w, _ in names) * proj) + len(names) * (
        4 * V * H + 4 * I * H + (3 << 30)) + 2 * V * H
    free, _total = torch.cuda.mem_get_info()
    if free < need:
        raise SystemExit(f"bench_qhead_decode: {a.model} needs ~{need >> 30} GiB of HBM for "
                         f"{len(names)} arms, {free >> 30} GiB free")
    emit, out = _emitter(a.out)
    arms = {}
    try:
        for w, h in names:
            arms[(w, h)] = _open(d, w, h, 4096)
        prompt = _prompt(cfg, a.prompt_len)
        for eng in arms.values():  # cold: first launches + graph capture
            eng.generate(prompt, 2, temperature=0.0, eos_ids=[])
        if a.window:  # the profiled window: nothing else runs
            for (w, h), eng in arms.items():
                emit({"window": f"{w}:{h}",
                      "p50_ms": round(_window(eng, prompt, a.warmup, a.steps).p50_ms, 4)})
            return
        for rnd in range(a.rounds):
            recs = {}
            for (w, h), eng in arms.items():
                r = _window(eng, prompt, a.warmup, a.steps)
                nbytes = eng.weight_bytes()
                # the decode step streams every weight once, except the 16-bit embedding
                # table, which is only indexed (one row); a tied table is streamed when it
                # is the head and only indexed when the head is a quantised copy
                indexed = 0 if (cfg.tie_word_embeddings and h == "model") else 2 * V * H
                stream = nbytes - indexed
                recs[(w, h)] = {"model": a.model, "weights": w, "head": h, "round": rnd,
                                "steps": a.steps, "p50_ms_per_token": round(r.p50_ms, 4),
                                "p99_ms_per_token": round(r.p99_ms, 4),
                                "tok_per_s_p50": round(1e3 / r.p50_ms, 2),
                                "weight_bytes": nbytes, "bytes_per_token": stream,
                                "implied_TBps": round(stream / (r.p50_ms * 1e-3) / 1e12, 3)}
            for (w, h), rec in recs.items():
                ref = recs.get((w, "model"))
                if ref and h != "model":
                    rec["time_vs_head_model"] = round(
                        rec["p50_ms_per_token"] / ref["p50_ms_per_token"], 4)
                    rec["bytes_vs_head_model"] = round(
                        rec["bytes_per_token"] / ref["bytes_per_token"], 4)
                emit(rec)
    finally:
        for eng in arms.values():
            eng.close()
        shutil.rmtree(d, ignore_errors=True)
        if out:
            out.close()


# the head launch geometry (U, prefetch, max_blocks), one variation at a time: the grid cap
# and U, the default first, in the middle and last (its spread is the sweep's yardstick)
SWEEP = [None, (2, 4, 512), (2, 4, 2048), (2, 4, 4096), None, (1, 4, 1024), (4, 4, 1024),
         (2, 0, 1024), None]


def sweep(a):
    """p50 ms/token per head launch geometry, for head=fp8 and head=mxfp4 under mxfp4
    projections: a fresh engine per setting (the captured graphs bake the geometry in)."""
    from cake_amd.ops import hip as K_
    cfg, d = _setup(a)
    prompt = _prompt(cfg, a.prompt_len)
    tune = {"fp8": (K_.get_gemv_w8_tuning, K_.set_gemv_w8_tuning),
            "mxfp4": (K_.get_gemv_w4_tuning, K_.set_gemv_w4_tuning)}
    base = {h: get("head") for h, (get, _set) in tune.items()}
    emit, out = _emitter(a.out)

    def restore():
        for h, (_get, set_) in tune.items():
            U, pf, mb = base[h]
            set_("head", U=U, prefetch=pf, max_blocks=mb)

    try:
        for head in ("fp8", "mxfp4"):
            get, set_ = tune[head]
            for setting in SWEEP:
                restore()
                if setting:
                    set_("head", U=setting[0], prefetch=setting[1], max_blocks=setting[2])
                eng = _open(d, "mxfp4", head, 4096)
                try:
                    eng.generate(prompt, 2, temperature=0.0, eos_ids=[])
                    p50 = [round(_window(eng, prompt, a.warmup, a.steps).p50_ms, 4)
                           for _ in range(2)]
                finally:
                    eng.close()
                emit({"model": a.model, "weights": "mxfp4", "head": head,
                      "setting": setting or "default", "head_tuning": get("head"),
                      "p50_ms_per_token": p50})
    finally:
        restore()
        shutil.rmtree(d, ignore_errors=True)
        if out:
            out.close()


# ---- kernel table from a rocprofv3 --stats kernel_stats.csv ------------------------------

V8B, H8B = 128256, 4096  # llama3-8b
HEAD_BYTES = {"": 2 * V8B * H8B, "_w8": V8B * H8B + 4 * V8B, "_w4": V8B * H8B // 2 + V8B * H8B // 32}


def table(path):
    """The head launches of the trace: the fused greedy tail (SEL, the decode steps) and the
    plain f32-logits launch (the prefill heads) of each format, listed apart."""
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            # the weight format is the kernel's first template argument (cake::W16 / W8 / W4)
            m = re.search(r"gemv_norm_f32_kernel<(?:cake::)?W(16|8|4), ([^>]*)>", r["Name"])
            if not m:
                continue
            sel = m.group(2).split(",")[-1].strip() in ("true", "1")
            sfx = {"16": "", "8": "_w8", "4": "_w4"}[m.group(1)]
            e = rows.setdefault((sfx, sel), {"calls": 0, "ns": 0.0})
            e["calls"] += int(r["Calls"])
            e["ns"] += float(r["TotalDurationNs"])

    def avg(e):
        return e["ns"] / e["calls"] / 1e3

    print(f"{'kernel':<26} {'calls':>7} {'avg_us':>8} {'MB':>8} {'TB/s':>6} {'vs 16-bit':>10}")
    for sel in (True, False):
        for sfx in ("", "_w8", "_w4"):
            e = rows.get((sfx, sel))
            if not e:
                continue
            rel = f"{avg(e) / avg(rows[('', sel)]):.2f}x" if ("", sel) in rows else "-"
            nbytes = HEAD_BYTES[sfx]
            name = "gemv_norm_f32" + sfx + (" +select" if sel else " plain")
            print(f"{name:<26} {e['calls']:>7} {avg(e):>8.2f} {nbytes / 1e6:>8.1f} "
                  f"{nbytes / avg(e) / 1e6:>6.2f} {rel:>10}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--model", default="llama3-8b", choices=["llama3-8b", "llama3-70b"])
    ap.add_argument("--arms", default=DEFAULT_ARMS,
                    help="comma-separated weights:head arms to open and alternate")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--prompt-len", type=int, default=32)
    ap.add_argument("--out", default=None, help="JSON lines file")
    ap.add_argument("--window", action="store_true",
                    help="one decode window per arm and nothing else (for a rocprofv3 run)")
    ap.add_argument("--sweep", action="store_true",
                    help="p50 per launch geometry of the quantised head launch")
    ap.add_argument("--table", default=None, metavar="KERNEL_STATS_CSV",
                    help="print the 8B head-launch table of a rocprofv3 --stats run and exit")
    a = ap.parse_args()
    if a.table:
        table(a.table)
    elif a.sweep:
        sweep(a)
    else:
        _arms(a.arms)
        run(a)


if __name__ == "__main__":
    main()
