"""A/B of batch-1 decode with FP8 (e4m3) weight-only projections against the model dtype.

One process opens the random-init engine of a named architecture twice (bf16, and bf16 +
weights="fp8") and alternates the two arms: per round and arm a 32-token prompt, a warm-up,
then `--steps` timed decode steps, reading the device-timed per-token p50 the engine
reports.  One JSON line per arm and round (tok/s, ms/token, weight bytes per token from
weight_bytes(), the implied TB/s), then TTFT at the `--ttft` prompt lengths for both arms
(the fp8 arm's prefill dequantises every projection once per layer: that pass's cost).

    python scripts/bench_fp8_decode.py --out profiles/fp8_decode_ab.jsonl
    python scripts/bench_fp8_decode.py --model llama3-70b --out profiles/fp8_decode_ab_70b.jsonl

Kernel table: run `--window` (one decode window per arm, nothing else) under
`rocprofv3 --kernel-trace --stats --output-format csv`, in a run of its own, then

    python scripts/bench_fp8_decode.py --table <..._kernel_stats.csv> > profiles/fp8_decode8b_kernel_table.txt

which puts every `_w8` kernel next to its 16-bit twin with the bytes each streams and TB/s.
"""
import argparse
import csv
import json
import re
import shutil
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def _open(cfg_dir, weights, max_seq):
    from cake_amd.engine import NativeLlama
    return NativeLlama(cfg_dir, max_seq=max_seq, dtype="bf16", device=0, random_init=True, seed=1,
                       weights=weights)


def _prompt(cfg, n):
    import torch
    g = torch.Generator().manual_seed(1234)
    return torch.randint(0, cfg.vocab_size, (n,), generator=g).tolist()


def _window(eng, prompt, warmup, steps):
    kw = dict(temperature=0.0, repeat_penalty=1.1, repeat_last_n=128, eos_ids=[])
    eng.generate(prompt, 1 + warmup, **kw)
    r = eng.continue_(steps, eos_ids=[])
    if len(r.tokens) != steps:
        raise RuntimeError(f"timed {len(r.tokens)} decode steps, expected {steps}")
    return r


def run(a):
    import torch
    from cake_amd.engine import write_config
    from cake_amd.models.llama3.config import preset
    if not torch.cuda.is_available():
        raise SystemExit("bench_fp8_decode: needs a GPU (no timing without one)")
    cfg = preset(a.model)
    d = tempfile.mkdtemp(prefix="cake_fp8_cfg_")
    write_config(d, cfg)
    ttft = [int(x) for x in a.ttft.split(",") if x]
    max_seq = max(4096, max(ttft + [0]) + 64)
    arms = {}
    # both arms stay open: projections 2 + 1 bytes per element, plus embedding / head twice
    H, I, L, V = cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.vocab_size
    hd = H // cfg.num_attention_heads
    proj = L * ((cfg.num_attention_heads + 2 * cfg.num_key_value_heads) * hd * H +
                H * cfg.num_attention_heads * hd + 3 * I * H)
    need = 3 * proj + 8 * V * H + (6 << 30)
    free, _total = torch.cuda.mem_get_info()
    if free < need:
        raise SystemExit(f"bench_fp8_decode: {a.model} needs ~{need >> 30} GiB of HBM for both "
                         f"arms, {free >> 30} GiB free")
    out = open(a.out, "w") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    try:
        for name, w in (("bf16", "model"), ("fp8", "fp8")):
            if a.window and a.arms != "both" and a.arms != name:
                continue
            arms[name] = _open(d, w, max_seq)
        prompt = _prompt(cfg, a.prompt_len)
        for eng in arms.values():  # cold: first launches + graph capture
            eng.generate(prompt, 2, temperature=0.0, eos_ids=[])
        if a.window:  # the profiled window: nothing else runs
            for name, eng in arms.items():
                r = _window(eng, prompt, a.warmup, a.steps)
                emit({"window": name, "p50_ms": round(r.p50_ms, 4)})
            return
        for rnd in range(a.rounds):
            for name, eng in arms.items():
                r = _window(eng, prompt, a.warmup, a.steps)
                nbytes = eng.weight_bytes()
                # the decode step streams every weight once, except that an untied
                # embedding table is only indexed (one row)
                stream = nbytes - (0 if cfg.tie_word_embeddings else 2 * cfg.vocab_size * cfg.hidden_size)
                emit({"model": a.model, "arm": name, "round": rnd, "steps": a.steps,
                      "p50_ms_per_token": round(r.p50_ms, 4), "p99_ms_per_token": round(r.p99_ms, 4),
                      "tok_per_s_p50": round(1e3 / r.p50_ms, 2),
                      "tok_per_s_wall": round(r.tokens_per_s, 2),
                      "weight_bytes": nbytes, "bytes_per_token": stream,
                      "implied_TBps": round(stream / (r.p50_ms * 1e-3) / 1e12, 3)})
        for T in ttft:
            p = _prompt(cfg, T)
            for name, eng in arms.items():
                eng.generate(p, 1, temperature=0.0, eos_ids=[])  # warm: plans, buffers
                best = min(eng.generate(p, 1, temperature=0.0, eos_ids=[]).prefill_s
                           for _ in range(3))
                emit({"model": a.model, "arm": name, "ttft_prompt": T,
                      "ttft_ms": round(best * 1e3, 3)})
    finally:
        for eng in arms.values():
            eng.close()
        shutil.rmtree(d, ignore_errors=True)
        if out:
            out.close()


# one-at-a-time variations of the three fp8 launch geometries (kind, U, prefetch, max_blocks)
SWEEP = [None, ("swiglu", 2, 4, 1024), ("swiglu", 2, 4, 2048), ("swiglu", 2, 2, 512),
         ("qkv", 2, 4, 512), ("qkv", 2, 2, 1024), ("qkv", 2, 0, 1024), ("x16", 4, 4, 512),
         ("x16", 2, 4, 1024), ("x16", 4, 2, 1024), ("x16", 1, 4, 1024), None]


def sweep(a):
    """p50 ms/token of the fp8 arm per launch geometry: a fresh engine per setting (the
    captured graphs bake the geometry in), the default first and last (drift)."""
    import torch
    from cake_amd.engine import write_config
    from cake_amd.models.llama3.config import preset
    from cake_amd.ops import hip as K_
    if not torch.cuda.is_available():
        raise SystemExit("bench_fp8_decode: needs a GPU (no timing without one)")
    cfg = preset(a.model)
    d = tempfile.mkdtemp(prefix="cake_fp8_cfg_")
    write_config(d, cfg)
    prompt = _prompt(cfg, a.prompt_len)
    base = {k: K_.get_gemv_w8_tuning(k) for k in K_.GEMV_W8_KINDS}
    out = open(a.out, "w") if a.out else None
    try:
        for setting in SWEEP:
            for k, (U, pf, mb) in base.items():
                K_.set_gemv_w8_tuning(k, U=U, prefetch=pf, max_blocks=mb)
            if setting:
                K_.set_gemv_w8_tuning(setting[0], U=setting[1], prefetch=setting[2],
                                      max_blocks=setting[3])
            eng = _open(d, "fp8", 4096)
            try:
                eng.generate(prompt, 2, temperature=0.0, eos_ids=[])
                p50 = [round(_window(eng, prompt, a.warmup, a.steps).p50_ms, 4) for _ in range(2)]
            finally:
                eng.close()
            line = json.dumps({"model": a.model, "setting": setting or "default",
                               "tuning": {k: K_.get_gemv_w8_tuning(k) for k in base},
                               "p50_ms_per_token": p50})
            print(line, flush=True)
            if out:
                out.write(line + "\n")
    finally:
        for k, (U, pf, mb) in base.items():
            K_.set_gemv_w8_tuning(k, U=U, prefetch=pf, max_blocks=mb)
        shutil.rmtree(d, ignore_errors=True)
        if out:
            out.close()


# ---- kernel table from a rocprofv3 --stats kernel_stats.csv ------------------------------

H, I, NH, NKV, HD = 4096, 14336, 32, 8, 128  # llama3-8b
NQKV = (NH + 2 * NKV) * HD


def _bytes(n, k, fp8):
    return n * k + 4 * n if fp8 else 2 * n * k


def _classify(name):
    """(row label, twin key, bytes) of a decode GEMV kernel name, or None."""
    # the weight format is the kernels' first template argument (cake::W16 / W8 / W4)
    m = re.search(r"(qkv_rope|swiglu|gemv_x16)_kernel<(?:cake::)?W(16|8), ([^>]*)>", name)
    if not m:
        return None
    kind, w8, targs = m.group(1), m.group(2) == "8", [t.strip() for t in m.group(3).split(",")]
    if kind == "qkv_rope":
        return f"qkv_rope{'_w8' if w8 else ''}", "qkv_rope", _bytes(NQKV, H, w8)
    if kind == "swiglu":
        return f"swiglu{'_w8' if w8 else ''}", "swiglu", _bytes(2 * I, H, w8)
    # template <F, DT, U, PFC, NX, ACCUM>, F stripped: NX tells o_proj (K = 4096 -> 2) from down_proj (K = 14336 -> 7)
    nx = int(re.sub(r"\D", "", targs[3]) or 0)
    if nx == 7:
        return f"down_proj{'_w8' if w8 else ''}", "down_proj", _bytes(H, I, w8)
    return f"o_proj{'_w8' if w8 else ''}", "o_proj", _bytes(H, H, w8)


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
    print(f"{'kernel':<14} {'calls':>7} {'avg_us':>8} {'MB':>8} {'TB/s':>6} {'vs twin time':>12}")
    for twin in ("qkv_rope", "o_proj", "swiglu", "down_proj"):
        base = rows.get(twin)
        for label in (twin, twin + "_w8"):
            e = rows.get(label)
            if not e:
                continue
            avg = e["ns"] / e["calls"] / 1e3
            rel = f"{avg / (base['ns'] / base['calls'] / 1e3):.2f}x" if base else "-"
            print(f"{label:<14} {e['calls']:>7} {avg:>8.2f} {e['bytes'] / 1e6:>8.1f} "
                  f"{e['bytes'] / avg / 1e6:>6.2f} {rel:>12}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--model", default="llama3-8b", choices=["llama3-8b", "llama3-70b"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--prompt-len", type=int, default=32)
    ap.add_argument("--ttft", default="512,2048", help="prompt lengths of the TTFT rows ('' = none)")
    ap.add_argument("--out", default=None, help="JSON lines file")
    ap.add_argument("--window", action="store_true",
                    help="one decode window per arm and nothing else (for a rocprofv3 run)")
    ap.add_argument("--sweep", action="store_true",
                    help="fp8 arm only: p50 per launch geometry of the three fp8 GEMV kinds")
    ap.add_argument("--arms", default="both", choices=["both", "bf16", "fp8"])
    ap.add_argument("--table", default=None, metavar="KERNEL_STATS_CSV",
                    help="print the 8B kernel table of a rocprofv3 --stats run and exit")
    a = ap.parse_args()
    if a.table:
        table(a.table)
        return
    if a.sweep:
        sweep(a)
        return
    run(a)


if __name__ == "__main__":
    main()
