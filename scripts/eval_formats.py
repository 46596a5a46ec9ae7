"""What each storage mode of the native Llama engine costs on one checkpoint and one text:
teacher-forced nll / perplexity per arm (NativeLlama.score), the gap to the 16-bit arm and
the top-1 agreement with the 16-bit arm's argmax.

Arms: 16-bit; weights=fp8; weights=mxfp4 (each with head=model); kv=fp8; weights=fp8 +
prefill=fp8.  One engine per arm, opened one after the other on the same checkpoint; every
arm scores the same windows of the same tokens (consecutive windows of --max-seq tokens, each
from position 0, as cake-cli --score-file).

    python scripts/eval_formats.py --model DIR --text FILE --out result.json
    python scripts/eval_formats.py --model DIR --tokens ids.json
    python scripts/eval_formats.py --preset llama3-8b --synthetic 1024 --max-seq 512 \\
        --out profiles/score_formats_synth.json

--preset opens random-init weights and --synthetic draws uniform random token ids: such a run
exercises the plumbing (every arm loads, scores and is compared) and says nothing about the
quality of a format on a trained model.
"""
import argparse
import json
import shutil
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

ARMS = {"16-bit": {}, "fp8": dict(weights="fp8"), "mxfp4": dict(weights="mxfp4"),
        "kv=fp8": dict(kv="fp8"), "fp8+prefill=fp8": dict(weights="fp8", prefill="fp8")}


def _tokens(a, vocab):
    if a.text:
        from cake_amd.native_bridge import score_file_tokens
        return score_file_tokens(a.model, a.text)
    if a.tokens:
        txt = Path(a.tokens).read_text()
        return [int(t) for t in (json.loads(txt) if txt.lstrip().startswith("[") else txt.split())]
    import torch
    g = torch.Generator().manual_seed(a.seed)
    return torch.randint(0, vocab, (a.synthetic,), generator=g).tolist()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--model", help="checkpoint directory")
    ap.add_argument("--preset", help="architecture name: random-init weights, no checkpoint")
    ap.add_argument("--text", help="UTF-8 text file ([bos] + its tokens; needs --model)")
    ap.add_argument("--tokens", help="token ids: a JSON list or whitespace-separated integers")
    ap.add_argument("--synthetic", type=int, default=0, help="this many uniform random ids")
    ap.add_argument("--max-seq", type=int, default=2048, help="window length")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--out")
    a = ap.parse_args()
    if bool(a.model) == bool(a.preset):
        raise SystemExit("eval_formats: one of --model DIR and --preset NAME")
    if sum(map(bool, (a.text, a.tokens, a.synthetic))) != 1 or (a.text and not a.model):
        raise SystemExit("eval_formats: one of --text (with --model), --tokens, --synthetic N")
    import numpy as np
    import torch
    from cake_amd.engine import NativeLlama, write_config
    from cake_amd.native_bridge import score_summary, score_windows
    if not torch.cuda.is_available():
        raise SystemExit("eval_formats: needs a GPU")
    tmp = None
    path, kw = a.model, {}
    if a.preset:
        from cake_amd.models.llama3.config import preset
        tmp = tempfile.mkdtemp(prefix="cake_eval_cfg_")
        path, kw = write_config(tmp, preset(a.preset)), dict(random_init=True, seed=a.seed)
    rec = {"checkpoint": a.model or f"{a.preset} (random init, seed {a.seed})",
           "tokens_from": a.text or a.tokens or f"{a.synthetic} uniform random ids, seed {a.seed}",
           "dtype": a.dtype, "max_seq": a.max_seq, "arms": {}}
    if a.preset or a.synthetic:
        rec["note"] = ("random-init weights and / or random tokens: a check of the plumbing, not "
                       "a quality result")
    ids = wins = ref_top = ref_nll = None
    try:
        for name in [n for n in a.arms.split(",") if n]:
            eng = NativeLlama(path, max_seq=a.max_seq, dtype=a.dtype, **kw, **ARMS[name])
            if ids is None:
                ids = _tokens(a, eng.vocab_size)
                wins = score_windows(len(ids), a.max_seq)
            parts = [(ids[s:e], eng.score(ids[s:e])) for s, e in wins]
            eng.close()
            s = score_summary(len(ids), parts)
            top = np.concatenate([r.top[:-1] for _, r in parts])
            if ref_top is None:   # the first arm is the yardstick (16-bit by default)
                ref_top, ref_nll = top, s["nll"]
            s["delta_nll"] = s["nll"] - ref_nll
            s["top1_agreement_with_first_arm"] = float((top == ref_top).mean())
            rec["arms"][name] = s
            print(f"{name:18s} nll {s['nll']:.6f}  ppl {s['ppl']:.4f}  dnll {s['delta_nll']:+.6f}  "
                  f"top-1 {s['top1']:.4f}  agreement {s['top1_agreement_with_first_arm']:.4f}",
                  flush=True)
    finally:
        if tmp:
            shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
