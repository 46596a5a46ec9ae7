"""Tokenizer side of the native text path.

cake-cli generates text with the native engine (libcake_engine.so: checkpoint load,
prefill, graph-replayed decode, device token selection — no PyTorch); the one piece it
leaves to the interpreter it embeds is the HF tokenizer (tokenizers' Rust core behind
its Python binding), reached through these JSON-in / JSON-out functions
(csrc/runtime/embed.cpp call_python).  Prompt rendering and token text follow the
Python generator exactly (models/llama3/generator.py: the Llama-3 dialog template of
models/chat.py, per-token decode with special tokens kept).
"""
from __future__ import annotations

import json
from pathlib import Path

_cache: dict = {}


def _tokenizer(model_dir: str):
    t = _cache.get(model_dir)
    if t is None:
        from .models.llama3.config import LlamaConfig
        from .models.llama3.generator import load_tokenizer
        cfg = LlamaConfig.from_path(Path(model_dir))
        t = _cache[model_dir] = load_tokenizer(model_dir, cfg.eos_token_id)
    return t


def encode_chat(req: str) -> str:
    """{"model", "system", "prompt"} -> {"ids": [...], "eos": [...]}"""
    from .models.chat import History, Message
    r = json.loads(req)
    tok, eos = _tokenizer(r["model"])
    h = History()
    h.append(Message.system(r.get("system", "")))
    h.append(Message.user(r["prompt"]))
    ids = tok.encode(h.encode_dialog_to_prompt(), add_special_tokens=False).ids
    return json.dumps({"ids": list(ids), "eos": sorted(eos)})


def decode_token(req: str) -> str:
    """{"model", "id"} -> the token's text ("" when undecodable)."""
    r = json.loads(req)
    tok, _ = _tokenizer(r["model"])
    try:
        return tok.decode([int(r["id"])], skip_special_tokens=False) or ""
    except Exception:  # noqa: BLE001  (the generator streams nothing for such ids)
        return ""


PROMPTS_FILE_MAX = 8   # lines of a --prompts-file: the engine's lock-step batch


def read_prompts_file(path: str) -> list[str]:
    """The prompts of a ``--prompts-file``: 1..8 lines of UTF-8 text, none empty (a final
    newline is not a line).  ValueError otherwise."""
    lines = Path(path).read_text(encoding="utf-8").split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    lines = [ln.rstrip("\r") for ln in lines]
    if not 1 <= len(lines) <= PROMPTS_FILE_MAX:
        raise ValueError(f"--prompts-file takes 1 to {PROMPTS_FILE_MAX} lines, {path} has "
                         f"{len(lines)}")
    for i, ln in enumerate(lines):
        if not ln.strip():
            raise ValueError(f"--prompts-file: line {i + 1} of {path} is empty")
    return lines


def encode_prompts_file(req: str) -> str:
    """{"model", "system", "path"} -> {"prompts": [[ids], ...], "eos": [...]}: every line
    rendered and tokenised as ``--prompt`` is (encode_chat)."""
    r = json.loads(req)
    out, eos = [], []
    for line in read_prompts_file(r["path"]):
        one = json.loads(encode_chat(json.dumps({"model": r["model"], "system": r.get("system", ""),
                                                 "prompt": line})))
        out.append(one["ids"])
        eos = one["eos"]
    return json.dumps({"prompts": out, "eos": eos})


def prompts_result_lines(req: str) -> str:
    """{"model", "prompts": [[ids], ...], "tokens": [[ids], ...], "eos": [...]} -> the result
    lines of ``--prompts-file``, one JSON object per prompt: index, n_prompt, tokens, text
    (every token's own decoding, an EOS left out)."""
    r = json.loads(req)
    eos = set(r.get("eos", []))
    lines = []
    for i, (p, toks) in enumerate(zip(r["prompts"], r["tokens"])):
        text = "".join(decode_token(json.dumps({"model": r["model"], "id": t}))
                       for t in toks if t not in eos)
        lines.append(json.dumps({"index": i, "n_prompt": len(p), "tokens": list(toks),
                                 "text": text}))
    return "\n".join(lines)


def score_windows(n_tokens: int, max_seq: int) -> list[tuple[int, int]]:
    """[start, end) of the windows ``--score-file`` scores: consecutive runs of ``max_seq``
    tokens, each scored from position 0 (its first token unscored); a last window of one
    token has nothing to score and is dropped."""
    if max_seq < 2:
        raise ValueError("--score-file needs --max-seq-len >= 2")
    return [(a, min(a + max_seq, n_tokens)) for a in range(0, n_tokens, max_seq)
            if min(a + max_seq, n_tokens) - a >= 2]


def score_file_tokens(model_dir: str, path: str) -> list[int]:
    """``[bos] + encode(text)`` of a UTF-8 text file, no other special tokens."""
    from .models.llama3.config import LlamaConfig
    cfg = LlamaConfig.from_path(Path(model_dir))
    if cfg.bos_token_id is None:
        raise ValueError("--score-file: config.json names no bos_token_id")
    tok, _ = _tokenizer(str(model_dir))
    text = Path(path).read_text(encoding="utf-8")
    return [int(cfg.bos_token_id), *tok.encode(text, add_special_tokens=False).ids]


def encode_score_file(req: str) -> str:
    """{"model", "path", "max_seq"} -> {"ids": [...], "windows": [[start, end], ...]}"""
    r = json.loads(req)
    ids = score_file_tokens(r["model"], r["path"])
    return json.dumps({"ids": ids, "windows": score_windows(len(ids), int(r["max_seq"]))})


def score_summary(n_tokens: int, parts: list) -> dict:
    """The ``--score-file`` result line from the per-window (tokens, ScoreResult) pairs:
    ``nll`` is the mean over all scored tokens."""
    import math
    scored = sum(len(t) - 1 for t, _ in parts)
    total = sum(float(-r.logprobs.sum()) for _, r in parts)
    hits = sum(round(r.top1 * (len(t) - 1)) for t, r in parts)
    nll = total / scored if scored else float("nan")
    return {"tokens": n_tokens, "scored": scored, "windows": len(parts), "nll": nll,
            "ppl": math.exp(nll) if scored else float("nan"),
            "top1": hits / scored if scored else float("nan")}
