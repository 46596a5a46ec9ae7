"""ctypes front of the native Llama engine (csrc/engine/llama_engine.cpp, libcake_engine.so).

The engine runs the whole text path of an all-local model in C++ — checkpoint load,
MFMA prefill, hipGraph-captured decode steps and the token loop — with no PyTorch in
the process's compute path.  This module only marshals arguments: the native CLI
(cake-cli, csrc/tools/cake_cli.cpp) calls the same C ABI directly, and the tests pin it
token-for-token to the Python DeviceDecoder (tests/test_engine_gpu.py).

Reference: cake-core/src/cake/master.rs:80-124 (generation loop) and
cake-core/src/models/llama3/llama.rs:72-138, 277-341 (the Llama generator).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from pathlib import Path
from typing import Callable

LIB_PATH = Path(__file__).resolve().parent / "lib" / "libcake_engine.so"

TOKEN_CB = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_int32)


class EngineOpts(C.Structure):
    _fields_ = [("max_seq", C.c_int32), ("dtype", C.c_int32), ("device", C.c_int32),
                ("steps_per_graph", C.c_int32), ("init", C.c_int32), ("weight_fmt", C.c_int32),
                ("seed", C.c_uint64), ("head_fmt", C.c_int32), ("kv_fmt", C.c_int32)]


class PipeOpts(C.Structure):
    _fields_ = [("rank", C.c_int32), ("world", C.c_int32), ("master_addr", C.c_char_p),
                ("hop_bf16", C.c_int32), ("hop_timeout_s", C.c_double),
                ("connect_timeout_s", C.c_double), ("owners", C.POINTER(C.c_int32)),
                ("n_owners", C.c_int32)]


class TPOpts(C.Structure):
    _fields_ = [("rank", C.c_int32), ("world", C.c_int32), ("master_addr", C.c_char_p),
                ("timeout_s", C.c_double), ("connect_timeout_s", C.c_double)]


class RemoteOpts(C.Structure):
    _fields_ = [("worker_of", C.POINTER(C.c_int32)), ("n_layers", C.c_int32),
                ("workers", C.POINTER(C.c_char_p)), ("n_workers", C.c_int32),
                ("timeout_s", C.c_double)]


class EngineSampling(C.Structure):
    _fields_ = [("temperature", C.c_float), ("top_k", C.c_int32), ("top_p", C.c_float),
                ("seed", C.c_uint64), ("repeat_penalty", C.c_float),
                ("repeat_last_n", C.c_int32)]


class EngineStats(C.Structure):
    _fields_ = [("n_prompt", C.c_int32), ("n_generated", C.c_int32), ("prefill_s", C.c_double),
                ("decode_s", C.c_double), ("tokens_per_s", C.c_double), ("p50_ms", C.c_float),
                ("p99_ms", C.c_float)]


# CakeEngineOpts.weight_fmt and .head_fmt
WEIGHT_FORMATS = {"model": 0, "fp8": 1, "mxfp4": 2}
# CakeEngineOpts.kv_fmt ("fp8-emulated": the test oracle of "fp8", no CLI value)
KV_FORMATS = {"model": 0, "fp8": 1, "fp8-emulated": 2}

# prefill_fmt: bits 8 and up of CakeEngineOpts.weight_fmt (the 40-byte struct is full)
PREFILL_FORMATS = {"model": 0, "fp8": 1}
PREFILL_FMT_SHIFT = 8

_lib = None


def _bind(L) -> None:
    """Prototypes of llama_engine.h on a loaded library (tests/test_abi_cpu.py compares them
    with the header)."""
    P, I = C.c_void_p, C.c_int32
    L.cake_engine_open.argtypes = [C.c_char_p, C.POINTER(EngineOpts), C.c_char_p, I]
    L.cake_engine_open.restype = P
    L.cake_engine_open_pp.argtypes = [C.c_char_p, C.POINTER(EngineOpts), C.POINTER(PipeOpts),
                                      C.c_char_p, I]
    L.cake_engine_open_pp.restype = P
    L.cake_engine_open_tp.argtypes = [C.c_char_p, C.POINTER(EngineOpts), C.POINTER(TPOpts),
                                      C.c_char_p, I]
    L.cake_engine_open_tp.restype = P
    L.cake_engine_open_remote.argtypes = [C.c_char_p, C.POINTER(EngineOpts),
                                          C.POINTER(RemoteOpts), C.c_char_p, I]
    L.cake_engine_open_remote.restype = P
    L.cake_engine_serve.argtypes = [P, C.c_char_p, I]
    L.cake_engine_serve.restype = I
    L.cake_engine_rank_info.argtypes = [P, C.POINTER(C.c_int32)]
    L.cake_engine_rank_info.restype = I
    L.cake_engine_info.argtypes = [P, C.POINTER(C.c_int32)]
    L.cake_engine_info.restype = I
    L.cake_engine_eos.argtypes = [P, C.POINTER(C.c_int32), I]
    L.cake_engine_eos.restype = I
    L.cake_engine_weight_bytes.argtypes = [P]
    L.cake_engine_weight_bytes.restype = C.c_int64
    L.cake_engine_packed_bytes.argtypes = [P]
    L.cake_engine_packed_bytes.restype = C.c_int64
    L.cake_engine_kv_bytes.argtypes = [P]
    L.cake_engine_kv_bytes.restype = C.c_int64
    L.cake_engine_open_layers.argtypes = [C.c_char_p, C.POINTER(EngineOpts),
                                          C.POINTER(C.c_int32), I, C.c_char_p, I]
    L.cake_engine_open_layers.restype = P
    L.cake_engine_forward.argtypes = [P, C.c_uint64, C.POINTER(C.c_int32), I, I,
                                      C.POINTER(C.c_float), I, C.c_char_p, I]
    L.cake_engine_forward.restype = I
    L.cake_engine_drop_session.argtypes = [P, C.c_uint64]
    L.cake_engine_drop_session.restype = None
    L.cake_engine_generate.argtypes = [P, C.POINTER(C.c_int32), I, I, C.POINTER(EngineSampling),
                                       C.POINTER(C.c_int32), I, TOKEN_CB, P,
                                       C.POINTER(C.c_int32), I, C.POINTER(EngineStats),
                                       C.c_char_p, I]
    L.cake_engine_generate.restype = I
    L.cake_engine_generate_batch.argtypes = [P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), I, I,
                                             C.POINTER(EngineSampling), C.POINTER(C.c_int32), I,
                                             C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                             C.POINTER(EngineStats), C.POINTER(EngineStats),
                                             C.POINTER(C.c_float), C.c_char_p, I]
    L.cake_engine_generate_batch.restype = I
    L.cake_engine_continue.argtypes = [P, I, C.POINTER(C.c_int32), I, TOKEN_CB, P,
                                       C.POINTER(C.c_int32), I, C.POINTER(EngineStats),
                                       C.c_char_p, I]
    L.cake_engine_continue.restype = I
    L.cake_engine_forced_logits.argtypes = [P, C.POINTER(C.c_int32), I, C.POINTER(C.c_int32),
                                            I, C.POINTER(C.c_float), C.c_char_p, I]
    L.cake_engine_forced_logits.restype = I
    L.cake_engine_walk.argtypes = [P, C.c_char_p, I]
    L.cake_engine_walk.restype = I
    L.cake_engine_prefill_logits.argtypes = [P, C.POINTER(C.c_int32), I,
                                             C.POINTER(C.c_float), C.c_char_p, I]
    L.cake_engine_prefill_logits.restype = I
    FP = C.POINTER(C.c_float)
    L.cake_engine_score.argtypes = [P, C.POINTER(C.c_int32), I, I, FP, FP,
                                    C.POINTER(C.c_int32), FP, C.c_char_p, I]
    L.cake_engine_score.restype = I
    IP = C.POINTER(C.c_int32)
    L.cake_engine_set_logprobs.argtypes = [P, I, C.c_char_p, I]
    L.cake_engine_set_logprobs.restype = I
    L.cake_engine_logprobs.argtypes = [P, I, I, IP, FP, FP, IP, FP, C.c_char_p, I]
    L.cake_engine_logprobs.restype = I
    L.cake_engine_set_logit_controls.argtypes = [P, C.POINTER(LogitControls), C.c_char_p, I]
    L.cake_engine_set_logit_controls.restype = I
    L.cake_engine_close.argtypes = [P]
    L.cake_engine_close.restype = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise RuntimeError(f"{LIB_PATH} missing: run `python -m cake_amd.build`")
        L = C.CDLL(str(LIB_PATH))
        _bind(L)
        _lib = L
    return _lib


@dataclass
class GenResult:
    tokens: list[int] = field(default_factory=list)
    n_prompt: int = 0
    prefill_s: float = 0.0
    decode_s: float = 0.0
    tokens_per_s: float = 0.0
    p50_ms: float = 0.0
    p99_ms: float = 0.0
    logprobs: "TokenLogprobs | None" = None   # generate(..., logprobs=K)
    logits: "object | None" = None   # generate_batch(..., return_logits=True): f32 [tokens, V]


MAX_BATCH = 8   # prompts of one generate_batch call (llama_engine.h)


LOGPROBS_MAX_TOP = 20
LOGIT_BIAS_MAX = 300   # OpenAI's limit on logit_bias entries
NO_LOGIT_CONTROLS_TP = ("logit controls (presence_penalty, frequency_penalty, logit_bias, min_p) "
                        "are not available on a tensor-parallel engine (the vocabulary is "
                        "sharded)")


class LogitControls(C.Structure):
    """Per-request controls on the f32 row token selection sees, after the repeat penalty and
    before argmax / top-k / top-p / the draw / the log-prob record (OpenAI's fields and min_p);
    also the ctypes mirror of ``struct CakeLogitControls``:

    * ``presence_penalty`` / ``frequency_penalty`` in [-2, 2]: with ``c[v]`` the occurrences of
      v among the tokens this generation has produced so far (the prompt is not counted),
      ``x[v] -= presence + frequency * c[v]`` where ``c[v] > 0``;
    * ``logit_bias``: ``{id: bias}``, at most 300 distinct ids, each bias finite in
      [-100, 100]: ``x[id] += bias``, after the penalty;
    * ``min_p`` in (0, 1] (None or 0: off): with ``temperature > 0`` the sampling set is cut to
      ``x[v] >= max x + T ln(min_p)`` (p[v] >= min_p p_max) and intersected with top-k / top-p;
      greedy decoding ignores it.

    The constructor checks the values (``ValueError``) and keeps them as f32, the engine's
    type; ``neutral`` is true when nothing would change a token."""
    _fields_ = [("presence_penalty", C.c_float), ("frequency_penalty", C.c_float),
                ("min_p", C.c_float), ("n_bias", C.c_int32),
                ("bias_ids", C.POINTER(C.c_int32)), ("bias_values", C.POINTER(C.c_float))]

    def __init__(self, presence_penalty: float = 0.0, frequency_penalty: float = 0.0,
                 logit_bias: "dict[int, float] | None" = None, min_p: "float | None" = None):
        import math

        def num(name, v, lo, hi):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) \
                    or not lo <= v <= hi:
                raise ValueError(f"{name}: a number in [{lo}, {hi}], got {v!r}")
            return float(v)

        bias: dict[int, float] = {}
        if logit_bias is not None:
            if not isinstance(logit_bias, dict):
                raise ValueError("logit_bias: a mapping of token id to bias, "
                                 f"got {type(logit_bias).__name__}")
            if len(logit_bias) > LOGIT_BIAS_MAX:
                raise ValueError(f"logit_bias: at most {LOGIT_BIAS_MAX} entries, "
                                 f"got {len(logit_bias)}")
            for k, v in logit_bias.items():
                if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k < 2 ** 31:
                    raise ValueError("logit_bias: token ids are non-negative integers, "
                                     f"got {k!r}")
                bias[k] = num(f"logit_bias[{k}]", v, -100, 100)
        self._ids = (C.c_int32 * max(1, len(bias)))(*bias.keys())      # kept alive with self
        self._vals = (C.c_float * max(1, len(bias)))(*bias.values())
        super().__init__(num("presence_penalty", presence_penalty, -2, 2),
                         num("frequency_penalty", frequency_penalty, -2, 2),
                         0.0 if min_p is None else num("min_p", min_p, 0, 1), len(bias),
                         C.cast(self._ids, C.POINTER(C.c_int32)),
                         C.cast(self._vals, C.POINTER(C.c_float)))

    @property
    def logit_bias(self) -> "dict[int, float]":
        return {int(self._ids[i]): float(self._vals[i]) for i in range(self.n_bias)}

    @property
    def neutral(self) -> bool:
        return (self.presence_penalty == 0 and self.frequency_penalty == 0 and self.min_p == 0
                and self.n_bias == 0)

    def _key(self):
        return (self.presence_penalty, self.frequency_penalty, self.min_p,
                tuple(self.logit_bias.items()))

    def __eq__(self, other):
        return isinstance(other, LogitControls) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return (f"LogitControls(presence_penalty={self.presence_penalty!r}, frequency_penalty="
                f"{self.frequency_penalty!r}, logit_bias={self.logit_bias!r}, "
                f"min_p={self.min_p or None!r})")

    def check_vocab(self, vocab_size: int) -> "LogitControls":
        """``ValueError`` if a bias id is not below ``vocab_size``; returns self."""
        for k in self.logit_bias:
            if k >= vocab_size:
                raise ValueError(f"logit_bias: token id {k} is outside the vocabulary "
                                 f"[0, {vocab_size})")
        return self


@dataclass
class TokenLogprobs:
    """Log-probs of ``n`` generated tokens (``NativeLlama.generate(..., logprobs=K)``), over
    the f32 row token selection saw: after the repeat penalty, before temperature, top-k /
    top-p and the draw (with ``repeat_penalty=1`` the model's own distribution)."""
    ids: "np.ndarray"            # int32 [n]: the generated tokens
    logit: "np.ndarray"          # float32 [n]: x[id], bit for bit
    lse: "np.ndarray"            # float32 [n]: log sum exp of the row
    logprob: "np.ndarray"        # float64 [n]: logit - lse (-inf for a -inf logit)
    top_ids: "np.ndarray"        # int32 [n, K]: the K largest logits' ids, descending, the
    top_logits: "np.ndarray"     # float32 [n, K]   lower id first at ties; past V: -1 / -inf
    top_logprobs: "np.ndarray"   # float64 [n, K]


def logprob_json_lines(lp: "TokenLogprobs") -> list[str]:
    """The ``--logprobs-file`` lines of a generation: one JSON object per generated token,
    ``{index, id, logprob, top_ids, top_logprobs}`` (a -inf log-prob as ``-Infinity``)."""
    import json
    return [json.dumps({"index": i, "id": int(lp.ids[i]), "logprob": float(lp.logprob[i]),
                        "top_ids": [int(t) for t in lp.top_ids[i]],
                        "top_logprobs": [float(v) for v in lp.top_logprobs[i]]}) + "\n"
            for i in range(len(lp.ids))]


def _logprob(logit, lse):
    """float64 logit - lse, -inf where the logit is -inf (an all -inf row has lse -inf)."""
    import numpy as np
    l64 = np.asarray(logit, dtype=np.float64)
    s64 = np.asarray(lse, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isneginf(l64), -np.inf, l64 - s64)


@dataclass
class ScoreResult:
    """Teacher-forced scores of ``n`` tokens (:meth:`NativeLlama.score`).  Row ``i`` is the
    model's distribution after ``tokens[0..i]``; its target is ``tokens[i + 1]``."""
    lse: "np.ndarray"            # float32 [n]: log sum exp of the row's logits
    target_logit: "np.ndarray"   # float32 [n]: logit of tokens[i + 1]; NaN on the last row
    top: "np.ndarray"            # int32 [n]: argmax id (the lowest at ties)
    top_logit: "np.ndarray"      # float32 [n]: the logit there
    logprobs: "np.ndarray"       # float64 [n - 1]: target_logit - lse
    nll: float                   # mean of -logprobs
    ppl: float                   # exp(nll)
    top1: float                  # share of rows i < n - 1 with top[i] == tokens[i + 1]


def score_result(tokens, lse, target_logit, top, top_logit) -> ScoreResult:
    """The derived figures of one scored sequence from the engine's four arrays."""
    import numpy as np
    n = len(tokens)
    logprobs = target_logit[:n - 1].astype(np.float64) - lse[:n - 1].astype(np.float64)
    nll = float(-logprobs.mean())
    hits = int(np.count_nonzero(top[:n - 1] == np.asarray(tokens[1:], dtype=np.int32)))
    return ScoreResult(lse, target_logit, top, top_logit, logprobs, nll, float(np.exp(nll)),
                       hits / (n - 1))


class NativeLlama:
    """One model loaded by the native engine on one GPU."""

    def __init__(self, model_dir: str | Path, *, max_seq: int = 4096, dtype: str = "bf16",
                 device: int = 0, steps_per_graph: int = 1, rank: int = 0, world: int = 1,
                 master_addr: str = "127.0.0.1:29517", hop_bf16: bool = False,
                 hop_timeout_s: float = 30.0, connect_timeout_s: float = 600.0,
                 tp: bool = False, owners: list[int] | None = None, random_init: bool = False,
                 seed: int = 0, worker_of: list[int] | None = None,
                 workers: list[str] | None = None, remote_timeout_s: float = 120.0,
                 weights: str = "model", head: str = "model", kv: str = "model",
                 layers: list[int] | None = None, prefill: str = "model"):
        """world > 1: one rank of a layer-sharded pipeline, or with tp=True of a tensor-
        parallel group (rank 0 generates; the others call :meth:`serve`).  Every rank of
        one group must be constructed concurrently.  ``owners`` (pipeline): the rank of
        every layer (:func:`owners_from_topology`); None = contiguous shards.
        ``random_init``: only ``config.json`` is read; the weights are seeded normal
        draws on the device (benchmarks of a named architecture, no checkpoint).
        ``workers`` / ``worker_of`` (single process): TCP workers ("host:port") and the
        worker index of every layer (-1 = local) — the master's Client
        (cake-core/src/cake/client.rs:23-133), contiguous runs batched per round trip.
        ``weights``: "model" keeps every weight in ``dtype``; "fp8" stores the four
        per-layer projections (q|k|v, o, gate|up, down) as OCP e4m3fn codes with one f32
        scale per output row, quantised on load (embedding, lm_head, norms and the KV cache
        stay in ``dtype``); "mxfp4" stores them as OCP MXFP4, two e2m1 codes per byte with one
        power-of-two scale byte per 32 elements of a row (widths divisible by 32), also
        quantised on load.  Neither is available with ``tp=True``.
        ``head``: the lm_head's format, chosen independently of ``weights``: "model", "fp8"
        (e4m3fn codes and one f32 scale per vocabulary row) or "mxfp4" (hidden width
        divisible by 32), quantised on load.  The embedding stays in ``dtype``; with tied
        embeddings the quantised head is an extra allocation.  Ranks without the head ignore
        it; not available with ``tp=True``.
        ``kv``: the KV cache's format, chosen independently of both: "model" keeps it in
        ``dtype``; "fp8" stores one OCP e4m3fn code per element with no scale
        (``code = rne_e4m3(clamp(x, -448, 448))`` of the f32 value the writer holds), half
        the bytes, and every attention read — prefill included — sees the quantised values.
        "fp8-emulated" is the test oracle of "fp8" and nothing else: the 16-bit cache and
        its readers with every writer storing the code's value; it saves no memory, and an
        "fp8" engine equals it bit for bit.  Each pipeline rank's or worker's own value
        governs its own caches.  Not available with ``tp=True`` nor with the experimental
        decode launches of docs/ENV.md.
        ``prefill``: "model" runs prefill on the weights' own path (quantised weights are
        widened into a 16-bit scratch before a 16-bit GEMM); "fp8" runs the four per-layer
        prefill projections on the fp8 matrix instruction: the activation rows quantised per
        token (e4m3fn codes, scale = amax / 448) against the resident fp8 codes, f32
        accumulation, both scales applied to the finished sum.  Needs ``weights="fp8"`` and
        hidden, attention and intermediate widths divisible by 128; decode, the head and the
        KV format are unchanged.  Each pipeline rank's or worker's own value governs its own
        layers.  Not available with ``tp=True``.
        ``layers`` (single process): open as a TCP worker's engine holding only these layers
        (no embedding, no head); drive it with :meth:`forward`."""
        if dtype not in ("bf16", "f16"):
            raise ValueError("native engine dtype: bf16 or f16")
        if weights not in WEIGHT_FORMATS:
            raise ValueError(f"native engine weights: one of {sorted(WEIGHT_FORMATS)}, "
                             f"got {weights!r}")
        if head not in WEIGHT_FORMATS:
            raise ValueError(f"native engine head: one of {sorted(WEIGHT_FORMATS)}, got {head!r}")
        if kv not in KV_FORMATS:
            raise ValueError(f"native engine kv: one of {sorted(KV_FORMATS)}, got {kv!r}")
        if prefill not in PREFILL_FORMATS:
            raise ValueError(f"native engine prefill: one of {sorted(PREFILL_FORMATS)}, "
                             f"got {prefill!r}")
        self.prefill = prefill
        self.tp = bool(tp and world > 1)
        self.weights = weights
        self.head = head
        self.kv = kv
        opts = EngineOpts(int(max_seq), 0 if dtype == "bf16" else 1, int(device),
                          max(1, int(steps_per_graph)), 1 if random_init else 0,
                          WEIGHT_FORMATS[weights] | PREFILL_FORMATS[prefill] << PREFILL_FMT_SHIFT,
                          int(seed) & 0xFFFFFFFFFFFFFFFF, WEIGHT_FORMATS[head], KV_FORMATS[kv])
        err = C.create_string_buffer(1024)
        self._h = None
        if world > 1 and tp:
            self._addr = master_addr.encode()
            o = TPOpts(int(rank), int(world), self._addr, float(hop_timeout_s),
                       float(connect_timeout_s))
            self._h = lib().cake_engine_open_tp(str(model_dir).encode(), C.byref(opts),
                                                C.byref(o), err, len(err))
        elif world > 1:
            self._addr = master_addr.encode()
            own = None
            if owners is not None:
                own = (C.c_int32 * len(owners))(*[int(x) for x in owners])
            self._owners = own  # kept alive for the call
            pipe = PipeOpts(int(rank), int(world), self._addr, int(bool(hop_bf16)),
                            float(hop_timeout_s), float(connect_timeout_s),
                            C.cast(own, C.POINTER(C.c_int32)) if own is not None else None,
                            len(owners) if owners is not None else 0)
            self._h = lib().cake_engine_open_pp(str(model_dir).encode(), C.byref(opts),
                                                C.byref(pipe), err, len(err))
        elif layers is not None:
            ls = (C.c_int32 * len(layers))(*[int(x) for x in layers])
            self._h = lib().cake_engine_open_layers(str(model_dir).encode(), C.byref(opts), ls,
                                                    len(layers), err, len(err))
        elif workers:
            wo = (C.c_int32 * len(worker_of))(*[int(x) for x in worker_of])
            hs = (C.c_char_p * len(workers))(*[w.encode() for w in workers])
            self._remote = (wo, hs)  # kept alive for the call
            ro = RemoteOpts(C.cast(wo, C.POINTER(C.c_int32)), len(worker_of),
                            C.cast(hs, C.POINTER(C.c_char_p)), len(workers),
                            float(remote_timeout_s))
            self._h = lib().cake_engine_open_remote(str(model_dir).encode(), C.byref(opts),
                                                    C.byref(ro), err, len(err))
        else:
            self._h = lib().cake_engine_open(str(model_dir).encode(), C.byref(opts), err, len(err))
        if not self._h:
            raise RuntimeError(f"native engine: {err.value.decode(errors='replace')}")
        ri = (C.c_int32 * 4)()
        lib().cake_engine_rank_info(self._h, ri)
        self.rank, self.world, self.first_layer, self.end_layer = list(ri)
        info = (C.c_int32 * 8)()
        lib().cake_engine_info(self._h, info)
        (self.vocab_size, self.hidden_size, self.num_layers, self.num_heads, self.num_kv_heads,
         self.head_dim, self.intermediate_size, self.max_seq) = list(info)
        eos = (C.c_int32 * 16)()
        n = lib().cake_engine_eos(self._h, eos, 16)
        self.eos_ids = [int(eos[i]) for i in range(min(n, 16))]

    def weight_bytes(self) -> int:
        """Bytes of this rank's device weight allocations: embedding, head if untied,
        norms, projections and their scales (``weights="fp8"``: one f32 per row;
        ``"mxfp4"``: one byte per 32 elements), and a quantised head with its scales
        (``head="fp8"`` / ``"mxfp4"``; counted also when the embeddings are tied)."""
        return int(lib().cake_engine_weight_bytes(self._h))

    def packed_bytes(self) -> int:
        """Bytes of the packed (lossless 13-bit) copies of bf16 projections and lm_head the
        decode GEMVs of this rank stream instead of the 16-bit rows (``CAKE_PACK16``,
        docs/ENV.md); they sit beside the weights and are not part of ``weight_bytes``."""
        return int(lib().cake_engine_packed_bytes(self._h))

    def kv_bytes(self) -> int:
        """Bytes of one session's K + V cache on this rank: 2 x local layers x kv heads x
        max_seq x head_dim x element size (1 with ``kv="fp8"``, else 2)."""
        return int(lib().cake_engine_kv_bytes(self._h))

    def forward(self, layers: list[int], pos0: int, hidden, session: int = 1):
        """Worker compute (an engine opened with ``layers``): run `layers` over `hidden`
        (float32 numpy [T, H], updated in place and returned) at positions pos0.. with the
        KV cache of `session`.  T > 1 is a prefill chunk, T == 1 a decode step."""
        import numpy as np
        if hidden.dtype != np.float32 or hidden.ndim != 2 or not hidden.flags.c_contiguous:
            raise ValueError("forward: hidden must be a C-contiguous float32 [T, H] array")
        ls = (C.c_int32 * len(layers))(*[int(x) for x in layers])
        err = C.create_string_buffer(1024)
        rc = lib().cake_engine_forward(self._h, int(session), ls, len(layers), int(pos0),
                                       hidden.ctypes.data_as(C.POINTER(C.c_float)),
                                       hidden.shape[0], err, len(err))
        if rc:
            raise RuntimeError(f"native engine: {err.value.decode(errors='replace')}")
        return hidden

    def walk(self) -> str:
        """The token's walk as "rank:first-last" layer runs (comma separated)."""
        buf = C.create_string_buffer(4096)
        lib().cake_engine_walk(self._h, buf, len(buf))
        return buf.value.decode()

    def serve(self) -> None:
        """Pipeline worker: run rank 0's prefill relays and replay announcements until it
        closes the pipeline."""
        err = C.create_string_buffer(1024)
        if lib().cake_engine_serve(self._h, err, len(err)):
            raise RuntimeError(f"native engine: {err.value.decode(errors='replace')}")

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().cake_engine_close(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def prefill_logits(self, prompt: list[int]):
        import numpy as np
        arr = (C.c_int32 * len(prompt))(*prompt)
        out = np.empty(self.vocab_size, dtype=np.float32)
        err = C.create_string_buffer(1024)
        rc = lib().cake_engine_prefill_logits(self._h, arr, len(prompt),
                                              out.ctypes.data_as(C.POINTER(C.c_float)), err,
                                              len(err))
        if rc:
            raise RuntimeError(f"native engine: {err.value.decode(errors='replace')}")
        return out

    def score(self, tokens: list[int], *, vchunk: int = 0) -> ScoreResult:
        """Teacher-forced log-likelihood of ``tokens`` (2 <= n <= max_seq) from one prefill:
        per-row log-sum-exp, target logit, argmax and its logit, reduced on the device one
        vocabulary chunk at a time (``vchunk`` ids wide: a positive multiple of 256, or 0 =
        as wide as a 64 MB f32 chunk allows), plus ``logprobs``, ``nll``, ``ppl`` and
        ``top1``.  Works in every ``weights`` / ``head`` / ``kv`` / ``prefill`` mode, on a
        single rank, rank 0 of a pipeline and a master with TCP workers; not with
        ``tp=True`` nor on a ``layers`` engine.  The head here is a 16-bit GEMM over the
        16-bit normalised rows (a quantised head is widened chunk by chunk), so the last
        row differs from :meth:`prefill_logits`, whose head normalises in f32, by that
        rounding."""
        import numpy as np
        n = len(tokens)
        if n < 2:
            raise ValueError("score: at least 2 tokens (the first token is never scored)")
        arr = (C.c_int32 * n)(*[int(t) for t in tokens])
        lse, tgt, topv = (np.empty(n, dtype=np.float32) for _ in range(3))
        top = np.empty(n, dtype=np.int32)
        err = C.create_string_buffer(1024)
        fp = C.POINTER(C.c_float)
        rc = lib().cake_engine_score(self._h, arr, n, int(vchunk), lse.ctypes.data_as(fp),
                                     tgt.ctypes.data_as(fp),
                                     top.ctypes.data_as(C.POINTER(C.c_int32)),
                                     topv.ctypes.data_as(fp), err, len(err))
        if rc:
            raise RuntimeError(f"native engine: {err.value.decode(errors='replace')}")
        return score_result(tokens, lse, tgt, top, topv)

    def forced_logits(self, prompt: list[int], forced: list[int]):
        """Teacher forcing: f32 logits [len(forced) + 1, V] after the prompt and after each
        forced token (one eager decode step each, through every rank of the group)."""
        import numpy as np
        arr = (C.c_int32 * len(prompt))(*prompt)
        fa = (C.c_int32 * max(1, len(forced)))(*forced)
        out = np.empty((len(forced) + 1, self.vocab_size), dtype=np.float32)
        err = C.create_string_buffer(1024)
        rc = lib().cake_engine_forced_logits(self._h, arr, len(prompt), fa, len(forced),
                                             out.ctypes.data_as(C.POINTER(C.c_float)), err,
                                             len(err))
        if rc:
            raise RuntimeError(f"native engine: {err.value.decode(errors='replace')}")
        return out

    def generate(self, prompt: list[int], max_new: int, *, temperature: float = 0.0,
                 top_k: int | None = None, top_p: float | None = None, seed: int = 299792458,
                 repeat_penalty: float = 1.1, repeat_last_n: int = 128,
                 eos_ids: list[int] | None = None,
                 on_token: Callable[[int], bool | None] | None = None,
                 logprobs: int | None = None, presence_penalty: float = 0.0,
                 frequency_penalty: float = 0.0, logit_bias: dict[int, float] | None = None,
                 min_p: float | None = None) -> GenResult:
        """``logprobs``: None = off; K in [0, 20] = a log-prob record per generated token with
        the K most likely alternatives (:class:`TokenLogprobs` in ``GenResult.logprobs``; inside
        ``on_token``, :meth:`token_logprob`).  The tokens are the same either way.  Not with
        ``tp=True`` nor on a ``layers`` engine.
        ``presence_penalty`` / ``frequency_penalty`` / ``logit_bias`` / ``min_p``: the
        :class:`LogitControls` of this generation (and of the calls of :meth:`continue_` after
        it); all neutral = the default decode path.  The log-prob records see the row after the
        penalties and the bias.  Not with ``tp=True`` nor on a ``layers`` engine."""
        self.set_logit_controls(LogitControls(presence_penalty, frequency_penalty, logit_bias,
                                              min_p))
        self.set_logprobs(logprobs)
        arr = (C.c_int32 * len(prompt))(*prompt)
        smp = EngineSampling(float(temperature or 0.0), int(top_k or 0), float(top_p or 0.0),
                             int(seed) & 0xFFFFFFFFFFFFFFFF, float(repeat_penalty),
                             int(repeat_last_n))
        return self._run(lambda eos_arr, n_eos, cb, out, stats, err: lib().cake_engine_generate(
            self._h, arr, len(prompt), int(max_new), C.byref(smp), eos_arr, n_eos, cb, None, out,
            max(1, max_new), stats, err, len(err)), max_new, eos_ids, on_token)

    def generate_batch(self, prompts: list[list[int]], max_new: int, *, temperature: float = 0.0,
                       top_k: int | None = None, top_p: float | None = None,
                       seed: int = 299792458, repeat_penalty: float = 1.1,
                       repeat_last_n: int = 128, eos_ids: list[int] | None = None,
                       return_logits: bool = False) -> list[GenResult]:
        """Lock-step batched decode of 1..8 prompts: one pass over the weights per step for all
        of them.  One sampling setting; sequence ``b`` draws with ``seed + b``, and its tokens
        are bit for bit those of ``generate_batch([prompts[b]], ..., seed=seed + b)``.  A
        sequence ends at its first EOS (inclusive).  ``return_logits``: each result carries the
        f32 rows token selection saw, ``[len(tokens), V]`` (tests).  The times and the step
        percentiles of every result are the call's; ``tokens_per_s`` is the sequence's own.
        The engine refuses (``RuntimeError``) what it does not batch: pipeline, tensor-parallel,
        remote and layers-only engines, quantised weights / lm_head / KV cache, log-probs or
        logit controls left on by a previous :meth:`generate`, more than 8 or no prompts, an
        empty prompt, ``len(prompt) + max_new > max_seq``."""
        import numpy as np
        B = len(prompts)
        flat = [int(t) for p in prompts for t in p]
        offs = [0]
        for p in prompts:
            offs.append(offs[-1] + len(p))
        tok_arr = (C.c_int32 * max(1, len(flat)))(*flat)
        off_arr = (C.c_int32 * (B + 1))(*offs)
        eos = list(eos_ids or [])
        eos_arr = (C.c_int32 * max(1, len(eos)))(*eos)
        n_out = max(1, B) * max(1, int(max_new))
        out = (C.c_int32 * n_out)()
        out_len = (C.c_int32 * max(1, B))()
        seq_stats = (EngineStats * max(1, B))()
        smp = EngineSampling(float(temperature or 0.0), int(top_k or 0), float(top_p or 0.0),
                             int(seed) & 0xFFFFFFFFFFFFFFFF, float(repeat_penalty),
                             int(repeat_last_n))
        logits = None
        if return_logits and 1 <= B <= MAX_BATCH and max_new > 0:
            logits = np.empty((B, int(max_new), self.vocab_size), dtype=np.float32)
        err = C.create_string_buffer(1024)
        rc = lib().cake_engine_generate_batch(
            self._h, tok_arr, off_arr, B, int(max_new), C.byref(smp), eos_arr, len(eos), out,
            out_len, seq_stats, None,
            None if logits is None else logits.ctypes.data_as(C.POINTER(C.c_float)), err, len(err))
        if rc:
            raise RuntimeError(f"native engine: {err.value.decode(errors='replace')}")
        res = []
        for b in range(B):
            s, n = seq_stats[b], int(out_len[b])
            r = GenResult([int(out[b * int(max_new) + i]) for i in range(n)], s.n_prompt,
                          s.prefill_s, s.decode_s, s.tokens_per_s, s.p50_ms, s.p99_ms)
            if logits is not None:
                r.logits = logits[b, :n]
            res.append(r)
        return res

    def set_logprobs(self, k: int | None) -> None:
        """The log-prob setting of the next :meth:`generate` (None: off, 0..20: on)."""
        want = -1 if k is None else int(k)
        if k is not None and not 0 <= want <= LOGPROBS_MAX_TOP:
            raise ValueError(f"logprobs: an integer in [0, {LOGPROBS_MAX_TOP}] or None, got {k!r}")
        if want == getattr(self, "_lp_next", -1):
            return
        err = C.create_string_buffer(1024)
        if lib().cake_engine_set_logprobs(self._h, want, err, len(err)):
            raise RuntimeError(f"native engine: {err.value.decode(errors='replace')}")
        self._lp_next = want

    def set_logit_controls(self, c: LogitControls | None) -> None:
        """The :class:`LogitControls` of the next :meth:`generate` (None or all neutral: off).
        The values were checked when ``c`` was built and its ids are checked against the
        vocabulary here, before the library is touched (``ValueError``); the engine refuses
        controls on a tensor-parallel engine and on one without the head (``RuntimeError``)."""
        c = c or LogitControls()
        if not c.neutral and getattr(self, "tp", False):  # the engine's own refusal, before
            raise RuntimeError("native engine: " + NO_LOGIT_CONTROLS_TP)  # any library call
        c.check_vocab(self.vocab_size)
        if c == getattr(self, "_lc_next", LogitControls()):
            return
        err = C.create_string_buffer(1024)
        rc = lib().cake_engine_set_logit_controls(self._h, None if c.neutral else C.byref(c), err,
                                                  len(err))
        if rc:
            raise RuntimeError(f"native engine: {err.value.decode(errors='replace')}")
        self._lc_next = c

    def _logprobs(self, first: int, count: int) -> TokenLogprobs:
        import numpy as np
        k = self._lp_run
        ids = np.empty(count, dtype=np.int32)
        logit, lse = (np.empty(count, dtype=np.float32) for _ in range(2))
        top_ids = np.empty((count, LOGPROBS_MAX_TOP), dtype=np.int32)
        top_logits = np.empty((count, LOGPROBS_MAX_TOP), dtype=np.float32)
        err = C.create_string_buffer(1024)
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        rc = lib().cake_engine_logprobs(self._h, int(first), int(count), ids.ctypes.data_as(ip),
                                        logit.ctypes.data_as(fp), lse.ctypes.data_as(fp),
                                        top_ids.ctypes.data_as(ip), top_logits.ctypes.data_as(fp),
                                        err, len(err))
        if rc:
            raise RuntimeError(f"native engine: {err.value.decode(errors='replace')}")
        top_ids = np.ascontiguousarray(top_ids[:, :k])
        top_logits = np.ascontiguousarray(top_logits[:, :k])
        return TokenLogprobs(ids, logit, lse, _logprob(logit, lse), top_ids, top_logits,
                             _logprob(top_logits, lse[:, None]))

    def token_logprob(self, i: int) -> TokenLogprobs:
        """Inside ``on_token``: the record of token ``i`` of the running generate / continue
        call (any token reported so far, the current one included), as one-row arrays."""
        if getattr(self, "_lp_run", -1) < 0:
            raise RuntimeError("token_logprob: the generation runs without logprobs")
        return self._logprobs(int(i), 1)

    def continue_(self, max_new: int, *, eos_ids: list[int] | None = None,
                  on_token: Callable[[int], bool | None] | None = None) -> GenResult:
        """Up to max_new more tokens after the last generate / continue (same sampling and
        log-prob setting; the rate counts every token: all are decode steps)."""
        return self._run(lambda eos_arr, n_eos, cb, out, stats, err: lib().cake_engine_continue(
            self._h, int(max_new), eos_arr, n_eos, cb, None, out, max(1, max_new), stats, err,
            len(err)), max_new, eos_ids, on_token, continued=True)

    def _run(self, call, max_new, eos_ids, on_token, continued: bool = False) -> GenResult:
        if not continued:  # a continuation keeps the setting of its generation
            self._lp_run = getattr(self, "_lp_next", -1)
        eos = list(eos_ids or [])
        eos_arr = (C.c_int32 * max(1, len(eos)))(*eos)
        out = (C.c_int32 * max(1, max_new))()
        stats = EngineStats()
        err = C.create_string_buffer(1024)
        errors: list[BaseException] = []

        def _tok(_ctx, t):
            try:
                return 1 if on_token(int(t)) else 0
            except BaseException as e:  # noqa: BLE001  (re-raised after the call)
                errors.append(e)
                return 1

        cb = TOKEN_CB(_tok) if on_token is not None else TOKEN_CB()
        rc = call(eos_arr, len(eos), cb, out, C.byref(stats), err)
        if errors:
            raise errors[0]
        if rc:
            raise RuntimeError(f"native engine: {err.value.decode(errors='replace')}")
        res = GenResult([int(out[i]) for i in range(stats.n_generated)], stats.n_prompt,
                        stats.prefill_s, stats.decode_s, stats.tokens_per_s, stats.p50_ms,
                        stats.p99_ms)
        if getattr(self, "_lp_run", -1) >= 0:
            res.logprobs = self._logprobs(0, stats.n_generated)
        return res


def owners_from_topology(topology, num_layers: int, world: int) -> list[int]:
    """Layer -> pipeline rank of a topology: node i (file order) is rank i + 1, layers
    no node names stay on rank 0 (the master), as the reference's placement loop
    (cake-core/src/models/llama3/llama.rs:205-220, topology.rs:81-92)."""
    from .parallel.rccl_roles import owners_from_topology as f
    return f(topology, num_layers, world)


def remote_placement(topology, num_layers: int) -> tuple[list[int], list[str]]:
    """(worker_of, workers) of a topology for the master's TCP client: node i serves the
    layers it names (exact name lookup, topology.rs:81-92), the rest stay local."""
    nodes = list(topology.nodes)
    index = {id(n): i for i, n in enumerate(nodes)}
    worker_of = []
    for li in range(num_layers):
        node = topology.get_node_for_layer(f"model.layers.{li}")
        worker_of.append(-1 if node is None else index[id(node)])
    return worker_of, [n.host for n in nodes]


def write_config(path: str | Path, cfg) -> Path:
    """A model directory holding only ``config.json`` of ``cfg`` (random-init engines)."""
    import json
    p = Path(path)
    p.mkdir(parents=True, exist_ok=True)
    (p / "config.json").write_text(json.dumps(cfg.to_hf_dict()))
    return p
