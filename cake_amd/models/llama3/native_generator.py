"""LLama text generator on the native engine (libcake_engine.so).

The reference's generator (cake-core/src/models/llama3/llama.rs:50-347) behind the
TextGenerator contract, with the whole token loop in C++: the chat template and the
tokenizer stay here (Python ``tokenizers``, the HF Rust library the reference links),
prefill, the graph-replayed decode, the repeat penalty and the sampling run in the
engine.  One class covers every native mode — all-local on one GPU, a pipeline rank 0
(the topology's placement, device hops) and a tensor-parallel rank 0 — so the REST API
(api/server.py, ``--api``) and the CLI master serve from the same engine the bench
measures.

Sampling: greedy, or the seeded temperature / top-k / top-p draw of the engine (device
Gumbel-max keyed by (seed, step): reproducible per seed, "parity unpinned" against the
reference's StdRng stream, as in the Python device path).
"""
from __future__ import annotations

from typing import Callable

from ..base import TextGenerator, Token
from ..chat import History, Message
from ..sampling import SamplingConfig


class NativeLLM(TextGenerator):
    MODEL_NAME = "llama3"

    def __init__(self, engine, tokenizer, eos_ids, sampling: SamplingConfig):
        self.eng = engine
        self.tokenizer = tokenizer
        self.eos_ids = set(eos_ids)
        self.sampling = sampling
        self.history = History()
        self.tokens: list[int] = []
        self.generated = 0
        self.last_stats = None
        self.last_result = None
        self.logprobs: int | None = None   # set_logprobs
        self.logit_controls = None         # set_logit_controls (engine.LogitControls)

    # ------------------------------------------------------------------ factory
    @classmethod
    def load(cls, ctx, engine=None) -> "NativeLLM":
        """All-local engine on ctx.device (or rank 0's ``engine`` of a running group)."""
        from .generator import load_tokenizer
        from ...engine import NativeLlama
        if engine is None:
            kw = {}
            topo = getattr(ctx, "topology", None)
            if topo is not None and getattr(topo, "nodes", None):
                from ...engine import remote_placement
                from .config import LlamaConfig
                L = LlamaConfig.from_path(ctx.model_path).num_hidden_layers
                worker_of, workers = remote_placement(topo, L)
                if any(w >= 0 for w in worker_of):
                    kw = dict(worker_of=worker_of, workers=workers)
            engine = NativeLlama(ctx.model_path, max_seq=ctx.max_seq_len,
                                 dtype=_dtype_name(ctx.dtype), device=ctx.device.index or 0,
                                 weights=getattr(ctx, "weight_dtype", "model"),
                                 head=getattr(ctx, "head_dtype", "model"),
                                 kv=getattr(ctx, "kv_dtype", "model"),
                                 prefill=getattr(ctx, "prefill_dtype", "model"), **kw)
        tok, eos = load_tokenizer(ctx.model_path, engine.eos_ids)
        return cls(engine, tok, eos, ctx.sampling)

    # ------------------------------------------------------------------ TextGenerator
    def add_message(self, message: Message) -> None:
        self.history.append(message)

    def reset(self) -> None:
        self.history.clear()
        self.tokens.clear()
        self.generated = 0

    def generated_tokens(self) -> int:
        return self.generated

    def set_sampling(self, sampling: SamplingConfig) -> None:
        """Per-request sampling (API): every generate call carries it to the engine."""
        self.sampling = sampling

    def set_logprobs(self, k: int | None) -> None:
        """Log-probs of the generated tokens from the next generation on: None = off, K in
        [0, 20] = on with the K most likely alternatives (``Token.logprob`` /
        ``Token.top_logprobs``).  Refused by a tensor-parallel engine."""
        self.eng.set_logprobs(k)
        self.logprobs = None if k is None else int(k)

    def set_logit_controls(self, c) -> None:
        """presence_penalty / frequency_penalty / logit_bias / min_p (``engine.LogitControls``)
        from the next generation on; None or all neutral = off.  ``ValueError`` for a bad
        value; refused by a tensor-parallel engine."""
        self.eng.set_logit_controls(c)
        self.logit_controls = None if c is None or c.neutral else c

    def latency_ms(self) -> tuple[float, float] | None:
        """(p50, p99) device time per decode token of the last generation."""
        r = self.last_result
        if r is None or not r.p50_ms:
            return None
        return float(r.p50_ms), float(r.p99_ms)

    def metrics(self) -> dict:
        r = self.last_result
        if r is None:
            return {}
        return {"engine": "native", "prefill_ms": round(r.prefill_s * 1e3, 3),
                "engine_tokens_per_s": round(r.tokens_per_s, 3),
                **({"walk": self.eng.walk()} if self.eng.world > 1 else {})}

    def _token(self, tid: int, lp=None) -> Token:
        """lp: the token's one-row TokenLogprobs, when the generation records them."""
        try:
            text = self.tokenizer.decode([tid], skip_special_tokens=False)
        except Exception:  # noqa: BLE001  (reference logs and returns None)
            text = None
        t = Token(id=tid, text=text, is_end_of_stream=tid in self.eos_ids)
        if lp is not None:
            t.logprob = float(lp.logprob[0])
            t.top_logprobs = [(int(i), float(v)) for i, v in
                              zip(lp.top_ids[0], lp.top_logprobs[0]) if i >= 0]
        return t

    def _kw(self) -> dict:
        s = self.sampling
        kw = dict(temperature=0.0 if s.greedy else float(s.temperature),
                  top_k=s.top_k, top_p=s.top_p, seed=int(s.seed),
                  repeat_penalty=float(s.repeat_penalty), repeat_last_n=int(s.repeat_last_n))
        c = self.logit_controls
        if c is not None:
            kw.update(presence_penalty=c.presence_penalty, frequency_penalty=c.frequency_penalty,
                      logit_bias=c.logit_bias, min_p=c.min_p)
        return kw

    def _prompt(self) -> list[int]:
        return self.tokenizer.encode(self.history.encode_dialog_to_prompt(),
                                     add_special_tokens=False).ids

    def next_token(self, index: int) -> Token:
        """The reference's per-token call: the first prefills the chat prompt, every
        later one is one more decode step of the same generation."""
        if self.generated == 0:
            self.tokens = self._prompt()
            r = self.eng.generate(self.tokens, 1, eos_ids=[], logprobs=self.logprobs,
                                  **self._kw())
        else:
            r = self.eng.continue_(1, eos_ids=[])
        tid = r.tokens[0]
        self.tokens.append(tid)
        self.generated += 1
        return self._token(tid, r.logprobs)

    def stream(self, max_tokens: int, on_token: Callable[[Token], None],
               stop_at_eos: bool = True) -> list[Token]:
        """Up to max_tokens tokens (the first from the prefill), streamed as they are read
        back; stops after an EOS id (inclusive) unless stop_at_eos is False."""
        out: list[Token] = []
        if max_tokens <= 0:
            return out
        self.tokens = self._prompt()
        room = self.eng.max_seq - len(self.tokens) - 3
        if room <= 0:
            raise RuntimeError("prompt does not fit the KV cache (--max-seq-len)")

        def cb(tid: int) -> None:
            lp = self.eng.token_logprob(len(out)) if self.logprobs is not None else None
            t = self._token(tid, lp)
            out.append(t)
            self.tokens.append(tid)
            self.generated += 1
            on_token(t)
        self.last_result = self.eng.generate(
            self.tokens, min(max_tokens, room), eos_ids=sorted(self.eos_ids) if stop_at_eos else [],
            on_token=cb, logprobs=self.logprobs, **self._kw())
        return out


    # ------------------------------------------------------------------ batched decode
    def batch_refusal(self) -> str | None:
        """Why this engine cannot run :meth:`generate_n` / ``generate_batch``, or None: known
        before any work is queued (the engine call refuses the same things)."""
        e = self.eng
        if getattr(e, "tp", False):
            return "a tensor-parallel engine does not batch sequences"
        if getattr(e, "world", 1) > 1:
            return "a pipeline engine does not batch sequences"
        if getattr(e, "_remote", None) is not None:
            return "an engine with remote workers does not batch sequences"
        fmts = [f"{k} {getattr(e, a)}" for k, a in (("weights", "weights"), ("lm_head", "head"),
                                                     ("KV cache", "kv"))
                if getattr(e, a, "model") != "model"]
        if fmts:
            return "batched decode runs 16-bit weights, lm_head and KV cache, not " + ", ".join(fmts)
        return None

    def _batch_kw(self) -> dict:
        s = self.sampling
        return dict(temperature=0.0 if s.greedy else float(s.temperature), top_k=s.top_k,
                    top_p=s.top_p, seed=int(s.seed), repeat_penalty=float(s.repeat_penalty),
                    repeat_last_n=int(s.repeat_last_n))

    def text_of(self, tokens: list[int]) -> str:
        """The text a generation of these tokens streams: every token's own decoding, the
        EOS left out."""
        return "".join(str(self._token(t)) for t in tokens if t not in self.eos_ids)

    def generate_n(self, n: int, max_tokens: int) -> list[tuple[str, int]]:
        """``n`` completions of the chat prompt on one lock-step batch (REST ``n``): choice i
        draws with seed + i.  [(text, generated tokens)]."""
        prompt = self._prompt()
        room = self.eng.max_seq - len(prompt)
        if room <= 0:
            raise RuntimeError("prompt does not fit the KV cache (--max-seq-len)")
        self.eng.set_logprobs(None)
        self.eng.set_logit_controls(None)
        res = self.eng.generate_batch([prompt] * n, min(max_tokens, room),
                                      eos_ids=sorted(self.eos_ids), **self._batch_kw())
        self.last_result = res[0]
        self.generated = sum(len(r.tokens) for r in res)
        return [(self.text_of(r.tokens), len(r.tokens)) for r in res]

    def generate_prompts(self, prompts: list[list[int]], max_tokens: int) -> list[list[int]]:
        """``--prompts-file``: the tokens of 1..8 tokenised prompts decoded as one batch."""
        res = self.eng.generate_batch(prompts, max_tokens, eos_ids=sorted(self.eos_ids),
                                      **self._batch_kw())
        self.last_result = res[0]
        return [r.tokens for r in res]


def score_file(ctx, path: str) -> dict:
    """``--score-file``: teacher-forced log-likelihood of a text file on the native engine,
    in windows of ``--max-seq-len`` tokens (native_bridge.score_windows); the result line's
    dict."""
    from ...native_bridge import score_file_tokens, score_summary, score_windows
    ids = score_file_tokens(str(ctx.model_path), path)
    if len(ids) < 2:
        raise RuntimeError("--score-file: fewer than 2 tokens, nothing to score")
    llm = NativeLLM.load(ctx)
    try:
        parts = [(ids[a:b], llm.eng.score(ids[a:b]))
                 for a, b in score_windows(len(ids), llm.eng.max_seq)]
    finally:
        llm.eng.close()
    return score_summary(len(ids), parts)


def _dtype_name(dtype) -> str:
    import torch
    if dtype == torch.bfloat16:
        return "bf16"
    if dtype == torch.float16:
        return "f16"
    raise ValueError(f"native engine dtype: bf16 or f16, not {dtype}")


def native_eligible(ctx, remote: bool = False) -> bool:
    """The native engine serves this context: a GPU, a 16-bit dtype, graphs on, and
    CAKE_NATIVE != 0 (``remote`` = a placement it cannot serve)."""
    import os

    import torch
    if os.environ.get("CAKE_NATIVE", "1") == "0" or remote:
        return False
    if ctx.device.type != "cuda" or getattr(ctx, "no_graph", False):
        return False
    if ctx.dtype not in (torch.float16, torch.bfloat16):
        return False
    from ...engine import LIB_PATH
    return LIB_PATH.exists()
