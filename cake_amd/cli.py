"""cake-cli: one entry point, master or worker mode (cake-cli/src/main.rs:8-63).

Flag names and defaults follow cake-core/src/lib.rs:21-200;
the image-generation flags double as the JSON keys of the image API.
MI355X additions: ``--max-seq-len``, ``--no-graph``, ``--trace FILE``,
``--log-level``.

    cake_amd/lib/cake-cli --model DIR --topology topology.yml --prompt "..."
    cake_amd/lib/cake-cli --mode worker --name w1 --model DIR --topology t.yml --address 0.0.0.0:10128
    cake_amd/lib/cake-cli --model DIR --api 0.0.0.0:8080

``cake-cli`` is the native executable (csrc/tools/cake_cli.cpp): it parses and
validates these flags and resolves the topology natively, then runs the role
with the compute runtime embedded in-process (:func:`run_parsed`).  ``python -m
cake_amd.cli`` takes the same flags (development entry).
"""
from __future__ import annotations

import argparse
import logging
import os
import sys

SD_VERSIONS = ["v1-5", "v2-1", "xl", "turbo"]


def _bool(s: str) -> bool:
    return str(s).lower() in ("1", "true", "yes", "on")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="cake-cli", description="MI355X-native distributed inference")
    a = ap.add_argument
    a("--device", type=int, default=0, help="GPU ordinal")
    a("--mode", choices=["master", "worker"], default="master")
    a("--name", default=None, help="worker name (must be in the topology)")
    a("--address", default="127.0.0.1:10128", help="worker bind address")
    a("--api", default=None, help="serve the REST API on this address instead of one CLI generation")
    a("--model", default="./cake-data/Meta-Llama-3-8B/")
    a("--topology", default="./cake-data/topology.yml")
    a("--prompt", default="The sky is blue because ")
    a("--system-prompt", default="You are a helpful AI assistant.")
    a("--seed", type=int, default=299792458)
    a("-n", "--sample-len", type=int, default=100)
    a("--temperature", type=float, default=1.0)
    a("--top-p", type=float, default=None)
    a("--top-k", type=int, default=None)
    a("--repeat-penalty", type=float, default=1.1)
    a("--repeat-last-n", type=int, default=128)
    a("--dtype", default=None, help="f16 (default), bf16 or f32")
    a("--cpu", action="store_true")
    a("--model-type", choices=["text-model", "image-model"], default="text-model")
    # SD args (lib.rs:90-127)
    a("--sd-tokenizer", default=None)
    a("--sd-tokenizer-2", default=None)
    a("--sd-version", choices=SD_VERSIONS, default="v1-5")
    a("--sd-use-f16", type=_bool, default=True)
    a("--sd-width", type=int, default=None)
    a("--sd-height", type=int, default=None)
    a("--sd-sliced-attention-size", type=int, default=None)
    a("--sd-clip", default=None)
    a("--sd-clip2", default=None)
    a("--sd-vae", default=None)
    a("--sd-unet", default=None)
    a("--sd-use-flash-attention", action="store_true")
    # image generation args (lib.rs:129-200)
    a("--sd-image-prompt", default="A very realistic photo of a rusty robot walking on a sandy beach")
    a("--sd-uncond-prompt", default="")
    a("--sd-tracing", action="store_true")
    a("--sd-n-steps", type=int, default=None)
    a("--sd-num-samples", type=int, default=1)
    a("--sd-bsize", type=int, default=1)
    a("--sd-intermediary-images", type=int, default=0)
    a("--sd-guidance-scale", type=float, default=None)
    a("--sd-img2img", default=None)
    a("--sd-img2img-strength", type=float, default=0.8)
    a("--sd-seed", type=int, default=None)
    # MI355X-native extras
    a("--transport", choices=["tcp", "rccl", "loopback"], default="tcp",
      help="rccl: torchrun one rank per GPU, rank 0 master, rank i serves topology node i; "
           "loopback: every topology node served in-process (wire protocol over 127.0.0.1)")
    a("--parallel", choices=["pp", "tp"], default="pp",
      help="with --transport rccl: pp = the topology's layer sharding (reference), "
           "tp = tensor parallel (every rank 1/N of every layer; topology layers ignored)")
    a("--hop", choices=["ipc", "dist"], default="ipc",
      help="--transport rccl pp: ipc = device-side hops captured in each rank's decode graph, "
           "dist = host-issued RCCL p2p per hop")
    a("--hop-dtype", choices=["f32", "bf16"], default="f32",
      help="hidden-state payload of an ipc hop (bf16 = the reference's 16-bit transport)")
    a("--max-seq-len", type=int, default=4096)
    a("--weight-dtype", choices=["model", "fp8", "mxfp4"], default="model",
      help="native Llama engine: fp8 = the per-layer projections as e4m3 codes with one "
           "scale per row, mxfp4 = as e2m1 codes with one power-of-two scale per 32 "
           "elements, both quantised on load (not with --parallel tp); model = --dtype")
    a("--head-dtype", choices=["model", "fp8", "mxfp4"], default="model",
      help="native Llama engine: the lm_head as fp8 (e4m3 codes, one scale per vocabulary "
           "row) or mxfp4, quantised on load, chosen independently of --weight-dtype (not "
           "with --parallel tp; workers hold no head and ignore it); model = --dtype")
    a("--kv-dtype", choices=["model", "fp8"], default="model",
      help="native Llama engine: fp8 = the KV cache as one e4m3 code per element, no scale "
           "(half the cache; every attention read sees the quantised values), chosen "
           "independently of --weight-dtype / --head-dtype (not with --parallel tp; each "
           "worker's own flag governs its own caches); model = --dtype")
    a("--prefill-dtype", choices=["model", "fp8"], default="model",
      help="native Llama engine: fp8 = the prefill projections on the fp8 matrix instruction, "
           "the activations quantised per token to e4m3 and multiplied with the resident fp8 "
           "codes (needs --weight-dtype fp8; not with --parallel tp; each worker's own flag "
           "governs its own layers); model = the weights' own prefill")
    a("--score-file", default=None, metavar="PATH",
      help="native Llama engine: score this UTF-8 text file instead of generating: "
           "[bos] + its tokens in consecutive windows of --max-seq-len, teacher forced; one "
           "JSON line {tokens, scored, windows, nll, ppl, top1} on stdout (any --weight-dtype "
           "/ --head-dtype / --kv-dtype / --prefill-dtype; not with --parallel tp)")
    a("--prompts-file", default=None, metavar="PATH",
      help="native Llama engine: decode the 1..8 lines of this UTF-8 text file as one "
           "lock-step batch, each line treated as --prompt treats its text (sequence i draws "
           "with --seed + i); one JSON line per prompt {index, n_prompt, tokens, text} on "
           "stdout (16-bit weights, lm_head and KV cache on one GPU; not with --parallel tp, "
           "a pipeline, topology workers, --logprobs-file or the logit-control flags)")
    a("--logprobs-file", default=None, metavar="PATH",
      help="native Llama engine: write one JSON line per generated token to PATH: {index, id, "
           "logprob, top_ids, top_logprobs}, over the logits token selection saw (after the "
           "repeat penalty, before temperature / top-k / top-p); not with --parallel tp")
    a("--top-logprobs", type=int, default=None, metavar="K",
      help="with --logprobs-file: alternatives per token, 0..20 (0 when absent)")
    a("--presence-penalty", type=float, default=None, metavar="F",
      help="native Llama engine: F in [-2, 2] subtracted once from the logit of every token "
           "this generation has already produced (after the repeat penalty; not with "
           "--parallel tp)")
    a("--frequency-penalty", type=float, default=None, metavar="F",
      help="native Llama engine: F in [-2, 2] subtracted from such a token's logit once per "
           "occurrence so far (not with --parallel tp)")
    a("--min-p", type=float, default=None, metavar="F",
      help="native Llama engine: sampled decoding keeps only tokens with p >= F * p_max, F in "
           "(0, 1], together with --top-k / --top-p; greedy ignores it (not with --parallel tp)")
    a("--logit-bias", default=None, metavar="ID:BIAS[,ID:BIAS...]",
      help="native Llama engine: added to those tokens' logits, at most 300 distinct ids, BIAS "
           "in [-100, 100] (not with --parallel tp)")
    a("--no-graph", action="store_true", help="disable hipGraph capture of the decode step")
    a("--trace", default=None, help="write a chrome-trace JSON of each text generation")
    a("--metrics", default=None, help="append one JSON line of stats per generation")
    a("--log-level", default=os.environ.get("CAKE_LOG", "info"))
    return ap


def setup_logging(level: str) -> None:
    # RUST_LOG default "info,tokenizers=error,actix_server=warn" (cake-cli/src/main.rs:14-22)
    logging.basicConfig(level=getattr(logging, level.upper(), logging.INFO),
                        format="[%(asctime)s %(levelname)s] %(message)s", datefmt="%H:%M:%S")
    logging.getLogger("uvicorn.access").setLevel(logging.WARNING)


def run_parsed(opts: dict) -> int:
    """Entry point of the native cake-cli / cake_start_worker (csrc/tools/cake_cli.cpp,
    csrc/runtime/capi.cpp): the flags were parsed and validated natively; ``opts``
    maps argparse dests to typed values.  Unknown keys are rejected."""
    ap = build_parser()
    args = ap.parse_args([])
    for k, v in opts.items():
        if not hasattr(args, k):
            raise ValueError(f"unknown option {k!r}")
        setattr(args, k, v)
    return _run(args)


def needs_native(fmt: str, flag: str = "--weight-dtype") -> str:
    """The refusal of a quantised ``--weight-dtype`` / ``--head-dtype`` / ``--kv-dtype`` /
    ``--prefill-dtype`` (fp8, mxfp4) on a Python engine path."""
    what = {"--kv-dtype": "KV cache", "--prefill-dtype": "prefill"}.get(flag, "weights")
    return (f"{flag} {fmt} is served by the native Llama engine only (a GPU, "
            "--dtype f16 or bf16, hipGraph decode, CAKE_NATIVE not 0); this run would "
            f"take the Python path, which has no {fmt} {what}: refusing rather than "
            "running 16-bit")


def _quant_refusal(ctx, flag: str, fmt: str) -> str | None:
    if fmt == "model":
        return None
    a = ctx.args
    if ctx.model_type != "text-model":
        return f"{flag} {fmt} applies to the text model only"
    from .models.llama3.native_generator import native_eligible
    if not native_eligible(ctx):
        return needs_native(fmt, flag)
    if a.transport == "rccl":
        if getattr(a, "parallel", "pp") == "tp":
            return f"{flag} {fmt} is not supported with --parallel tp yet"
        if getattr(a, "hop", "ipc") != "ipc":
            return needs_native(fmt, flag)
    elif a.mode == "worker" or a.transport == "loopback":
        # python -m cake_amd.cli workers are the Python worker (cake-cli hosts the native one)
        return needs_native(fmt, flag)
    return None


def weight_dtype_refusal(ctx) -> str | None:
    """Why this context cannot run its quantised ``--weight-dtype`` (fp8 or mxfp4; None: it
    can, or the option is off).  Every Python engine path refuses; none silently runs
    16-bit."""
    return _quant_refusal(ctx, "--weight-dtype", getattr(ctx, "weight_dtype", "model"))


def head_dtype_refusal(ctx) -> str | None:
    """The same for ``--head-dtype``, in the same wording.  A worker holds no head, so
    ``--mode worker`` accepts the option and ignores it."""
    if getattr(ctx.args, "mode", "master") == "worker" and ctx.model_type == "text-model":
        return None
    return _quant_refusal(ctx, "--head-dtype", getattr(ctx, "head_dtype", "model"))


def kv_dtype_refusal(ctx) -> str | None:
    """The same for ``--kv-dtype``, in the same wording (a native worker keeps its own
    caches, so ``cake-cli --mode worker`` serves it; the Python worker refuses)."""
    return _quant_refusal(ctx, "--kv-dtype", getattr(ctx, "kv_dtype", "model"))


def prefill_dtype_refusal(ctx) -> str | None:
    """The same for ``--prefill-dtype``, in the same wording (a native worker runs its own
    layers' prefill chunks, so ``cake-cli --mode worker`` serves it; the Python worker
    refuses).  On the native engine it needs ``--weight-dtype fp8``: the engine's own open
    refuses any other combination."""
    return _quant_refusal(ctx, "--prefill-dtype", getattr(ctx, "prefill_dtype", "model"))


def score_file_refusal(ctx) -> str | None:
    """Why this context cannot run ``--score-file`` (None: it can, or the option is off), in
    the wording of :func:`needs_native`: scoring is the native Llama engine's call, so every
    Python engine path and every image model refuses."""
    if not getattr(ctx, "score_file", None):
        return None
    a = ctx.args
    native = ("--score-file is served by the native Llama engine only (a GPU, --dtype f16 or "
              "bf16, hipGraph decode, CAKE_NATIVE not 0)")
    if ctx.model_type != "text-model":
        return native + ": it applies to the text model only"
    if a.transport == "rccl" and getattr(a, "parallel", "pp") == "tp":
        return ("--score-file is not supported with --parallel tp: a tensor-parallel engine "
                "shards the vocabulary")
    from .models.llama3.native_generator import native_eligible
    if (not native_eligible(ctx) or a.transport != "tcp" or a.mode == "worker"
            or getattr(a, "api", None)):
        return native + ("; this run would take the Python path, which has no sequence "
                         "scoring: refusing rather than generating")
    return None


def prompts_file_refusal(ctx) -> str | None:
    """Why this context cannot run ``--prompts-file`` (None: it can, or the option is off), in
    the wording of :func:`score_file_refusal`: refused where the engine's generate_batch is."""
    a = ctx.args
    if not getattr(a, "prompts_file", None):
        return None
    native = ("--prompts-file is served by the native Llama engine only (a GPU, --dtype f16 or "
              "bf16, hipGraph decode, CAKE_NATIVE not 0)")
    if ctx.model_type != "text-model":
        return native + ": it applies to the text model only"
    if a.transport == "rccl":
        return ("--prompts-file is not supported with --transport rccl: a pipeline or "
                "tensor-parallel engine does not batch sequences")
    if getattr(ctx, "score_file", None):
        return "--prompts-file and --score-file exclude each other"
    if getattr(a, "logprobs_file", None):
        return "--prompts-file does not record logprobs: drop --logprobs-file"
    try:
        if cli_logit_controls(a) is not None:
            return f"--prompts-file does not apply {LOGIT_CONTROL_FLAGS}"
    except ValueError as e:
        return str(e)
    for flag, val in (("--weight-dtype", ctx.weight_dtype), ("--head-dtype", ctx.head_dtype),
                      ("--kv-dtype", ctx.kv_dtype), ("--prefill-dtype", ctx.prefill_dtype)):
        if val != "model":
            return (f"--prompts-file runs 16-bit weights, lm_head and KV cache: not with "
                    f"{flag} {val}")
    if getattr(ctx.topology, "nodes", None):
        return ("--prompts-file is not supported with topology workers: an engine with remote "
                "workers does not batch sequences")
    from .models.llama3.native_generator import native_eligible
    if (not native_eligible(ctx) or a.transport != "tcp" or a.mode == "worker"
            or getattr(a, "api", None)):
        return native + ("; this run would take the Python path, which decodes one sequence at "
                         "a time: refusing rather than generating")
    return None


def run_prompts_file(ctx) -> int:
    """``--prompts-file``: one JSON line per prompt on stdout."""
    import json

    from .models.chat import Message
    from .models.llama3.native_generator import NativeLLM
    from .native_bridge import read_prompts_file
    try:
        lines = read_prompts_file(ctx.args.prompts_file)
    except (OSError, ValueError) as e:
        print(f"cake-cli: {e}", file=sys.stderr)
        return 2
    llm = NativeLLM.load(ctx)
    try:
        prompts = []
        for line in lines:
            llm.reset()
            llm.add_message(Message.system(ctx.args.system_prompt))
            llm.add_message(Message.user(line))
            prompts.append(list(llm._prompt()))
        room = llm.eng.max_seq - max(len(p) for p in prompts)
        if room <= 0:
            raise RuntimeError("prompt does not fit the KV cache (--max-seq-len)")
        outs = llm.generate_prompts(prompts, min(int(ctx.args.sample_len), room))
        for i, (p, toks) in enumerate(zip(prompts, outs)):
            print(json.dumps({"index": i, "n_prompt": len(p), "tokens": toks,
                              "text": llm.text_of(toks)}), flush=True)
    finally:
        llm.eng.close()
    return 0


def logprobs_file_refusal(ctx) -> str | None:
    """Why this context cannot run ``--logprobs-file`` / ``--top-logprobs`` (None: it can, or
    the options are off), in the wording of :func:`needs_native`."""
    a = ctx.args
    path, k = getattr(a, "logprobs_file", None), getattr(a, "top_logprobs", None)
    if k is not None:
        if not path:
            return "--top-logprobs needs --logprobs-file"
        if not 0 <= int(k) <= 20:
            return f"--top-logprobs must be in [0, 20], got {k}"
    if not path:
        return None
    native = ("--logprobs-file is served by the native Llama engine only (a GPU, --dtype f16 or "
              "bf16, hipGraph decode, CAKE_NATIVE not 0)")
    if ctx.model_type != "text-model":
        return native + ": it applies to the text model only"
    if a.transport == "rccl" and getattr(a, "parallel", "pp") == "tp":
        return ("--logprobs-file is not supported with --parallel tp: a tensor-parallel engine "
                "shards the vocabulary")
    from .models.llama3.native_generator import native_eligible
    if (not native_eligible(ctx) or a.transport != "tcp" or a.mode == "worker"
            or getattr(a, "api", None)):
        return native + ("; this run would take the Python path, which has no log-probs of "
                         "generated tokens: refusing rather than generating without them")
    return None


LOGIT_CONTROL_FLAGS = "--presence-penalty / --frequency-penalty / --min-p / --logit-bias"


def parse_logit_bias(text: str) -> dict[int, float]:
    """``ID:BIAS[,ID:BIAS...]`` -> ``{id: bias}``; ValueError on a malformed item or a repeated
    id (ranges: ``engine.LogitControls``)."""
    out: dict[int, float] = {}
    for item in text.split(","):
        tid, sep, val = item.partition(":")
        if not sep or not tid.isascii() or not tid.isdigit():
            raise ValueError(f"--logit-bias takes ID:BIAS[,ID:BIAS...], got {text!r}")
        try:
            b = float(val)
        except ValueError:
            raise ValueError(f"--logit-bias takes ID:BIAS[,ID:BIAS...], got {text!r}") from None
        if int(tid) in out:
            raise ValueError(f"--logit-bias names token id {int(tid)} twice")
        out[int(tid)] = b
    return out


def cli_logit_controls(a):
    """``engine.LogitControls`` of the four command-line flags, or None when none was given.
    ValueError on a bad value."""
    vals = [getattr(a, k, None) for k in ("presence_penalty", "frequency_penalty", "min_p",
                                          "logit_bias")]
    if all(v is None for v in vals):
        return None
    from .engine import LogitControls
    pres, freq, min_p, bias = vals
    return LogitControls(pres or 0.0, freq or 0.0, parse_logit_bias(bias) if bias else None,
                         min_p)


def logit_controls_refusal(ctx) -> str | None:
    """Why this context cannot honour the logit-control flags (None: it can, or none was
    given), in the wording of :func:`logprobs_file_refusal`: they are never silently ignored."""
    a = ctx.args
    try:
        if cli_logit_controls(a) is None:
            return None
    except ValueError as e:
        return str(e)
    native = (f"{LOGIT_CONTROL_FLAGS} are served by the native Llama engine only (a GPU, --dtype "
              "f16 or bf16, hipGraph decode, CAKE_NATIVE not 0)")
    if ctx.model_type != "text-model":
        return native + ": they apply to the text model only"
    if a.transport == "rccl" and getattr(a, "parallel", "pp") == "tp":
        return (f"{LOGIT_CONTROL_FLAGS} are not supported with --parallel tp: a tensor-parallel "
                "engine shards the vocabulary")
    if getattr(ctx, "score_file", None):
        return f"{LOGIT_CONTROL_FLAGS} apply to generation, not to --score-file"
    from .models.llama3.native_generator import native_eligible
    if (not native_eligible(ctx) or a.transport != "tcp" or a.mode == "worker"
            or getattr(a, "api", None)):
        return native + ("; this run would take the Python path (or serve the API, whose requests "
                         "carry their own values), which has no logit controls: refusing rather "
                         "than generating without them")
    return None


def main(argv: list[str] | None = None) -> int:
    return _run(build_parser().parse_args(argv))


def _run(args) -> int:
    setup_logging(args.log_level)
    from .context import Context
    ctx = Context.from_args(args)
    why = (weight_dtype_refusal(ctx) or head_dtype_refusal(ctx) or kv_dtype_refusal(ctx)
           or prefill_dtype_refusal(ctx) or score_file_refusal(ctx)
           or prompts_file_refusal(ctx)
           or logprobs_file_refusal(ctx) or logit_controls_refusal(ctx))
    if why:
        print(f"cake-cli: {why}", file=sys.stderr)
        return 2
    if getattr(args, "prompts_file", None):
        return run_prompts_file(ctx)
    if ctx.score_file:
        import json

        from .models.llama3.native_generator import score_file
        print(json.dumps(score_file(ctx, ctx.score_file)), flush=True)
        return 0
    if args.transport == "rccl":
        from .parallel.rccl_roles import run_rccl
        run_rccl(ctx)
        return 0
    if args.mode == "worker":
        from .parallel.worker import Worker
        Worker(ctx).run()
        return 0
    workers = []
    if args.transport == "loopback":
        from .parallel.loopback import start_loopback_workers
        workers = start_loopback_workers(ctx)
    from .master import Master
    try:
        Master(ctx).run()
    finally:
        if workers:
            from .parallel.loopback import stop_loopback_workers
            stop_loopback_workers(workers)
    return 0


if __name__ == "__main__":
    sys.exit(main())
