"""Per-kernel table of the 8B lock-step batched decode step beside its batch-1 twins, from a
rocprofv3 kernel-trace db of scripts/bench_batch_decode.py (one batched arm and the batch-1
arm in one process).

Every gemv_rows launch of a step is named by its place: store32 launches are q|k|v (one per
layer) and the lm_head (the largest grid), resid32 launches alternate o_proj / down_proj,
swiglu is gate|up.  Bytes are the weight bytes a launch must stream (the same for any B); the
batch-1 twins are qkv_rope / gemv_x16 / swiglu / the head kernels of the graph-replayed step.
The last lines give the per-step shares of the per-sequence attention and selection launches.

    rocprofv3 --kernel-trace -d prof -o run -- python scripts/bench_batch_decode.py \\
        --batches 8 --rounds 1 --steps 32
    python scripts/batch_kernel_table.py prof/.../run_results.db --batch 8
"""
import argparse
import re
import sqlite3

H, I, NH, NKV, HD, V, L = 4096, 14336, 32, 8, 128, 128256, 32
BYTES = {"qkv": (NH + 2 * NKV) * HD * H * 2, "o_proj": H * H * 2, "gate|up": 2 * I * H * 2,
         "down_proj": H * I * 2, "lm_head": V * H * 2}
SELECT = ("repeat_penalty", "argmax", "sample_threshold", "gumbel", "finalize")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("db")
    ap.add_argument("--batch", type=int, required=True)
    a = ap.parse_args()
    c = sqlite3.connect(a.db)
    cols = [r[1] for r in c.execute("pragma table_info(kernels)")]
    name_col = "kernel_name" if "kernel_name" in cols else "name"
    rows = c.execute(f"select {name_col}, start, end from kernels order by start").fetchall()
    rows_us = [(n, (e - s) / 1e3) for n, s, e in rows]
    batched, one = {}, {}
    n_res = n_x16 = n_store = 0
    step_other = {"attention": 0.0, "selection": 0.0, "rope_kv_rows": 0.0, "norm + embed + sum": 0.0}
    in_batch = False
    for n, us in rows_us:
        if "gemv_rows_kernel" in n:
            in_batch = True
            m = re.search(r"gemv_rows_kernel(?:<\d+, (\d+)|ILi\d+ELi(\d+)E)", n)
            epi = int(m.group(1) or m.group(2)) if m else -1
            if epi == 1:
                k = "o_proj" if n_res % 2 == 0 else "down_proj"
                n_res += 1
            elif epi == 3:
                k = "gate|up"
            else:
                k = "lm_head" if n_store % (L + 1) == L else "qkv"
                n_store += 1
            batched.setdefault(k, []).append(us)
            continue
        if "flash" in n or "gemm" in n:  # a prefill: not part of any step
            in_batch = False
        elif "qkv_rope_kernel" in n:
            in_batch = False
            one.setdefault("qkv", []).append(us)
        elif "swiglu_kernel" in n:
            one.setdefault("gate|up", []).append(us)
        elif "gemv_x16" in n:
            one.setdefault("o_proj" if n_x16 % 2 == 0 else "down_proj", []).append(us)
            n_x16 += 1
        elif "head_select" in n or "gemv_norm_f32" in n:
            one.setdefault("lm_head", []).append(us)
        elif in_batch:  # between gemv_rows launches: the rest of the batched step
            if "attn" in n:
                step_other["attention"] += us
            elif any(s in n for s in SELECT):
                step_other["selection"] += us
            elif "rope_kv_rows" in n:
                step_other["rope_kv_rows"] += us
            elif any(s in n for s in ("rmsnorm", "embed", "sum_slices")):
                step_other["norm + embed + sum"] += us
    steps = max(1, len(batched.get("lm_head", [])))
    print(f"B = {a.batch}; {steps} batched steps, {len(one.get('lm_head', []))} batch-1 steps in the trace")
    print(f"{'launch':<10} {'MB':>8} | {'gemv_rows us':>12} {'TB/s':>6} | {'batch-1 us':>10} {'TB/s':>6} | "
          f"{'rows / batch-1':>14}")
    tot_b = tot_1 = 0.0
    for k in ("qkv", "o_proj", "gate|up", "down_proj", "lm_head"):
        if k not in batched or k not in one:
            continue
        tb = sum(batched[k]) / len(batched[k])
        t1 = sum(one[k]) / len(one[k])
        per = 1 if k == "lm_head" else L
        tot_b += tb * per
        tot_1 += t1 * per
        b = BYTES[k]
        print(f"{k:<10} {b / 1e6:>8.1f} | {tb:>12.2f} {b / tb / 1e6:>6.2f} | {t1:>10.2f} "
              f"{b / t1 / 1e6:>6.2f} | {tb / t1:>14.2f}")
    print("MB and TB/s count the 16-bit rows in both columns; a bf16 batch-1 step whose engine packed "
          "its weights streams 13/16 of them")
    print(f"projection kernel time per step: batched {tot_b / 1e3:.3f} ms for {a.batch} tokens, "
          f"batch-1 {tot_1 / 1e3:.3f} ms for one")
    rest = {k: v / steps for k, v in step_other.items()}
    total = tot_b + sum(rest.values())
    for k, v in rest.items():
        print(f"{k:<20} {v:>9.1f} us per step ({100 * v / total:.1f} % of the step's kernel time)")
    print(f"kernel time per batched step: {total / 1e3:.3f} ms")


if __name__ == "__main__":
    main()
