"""REST API (cake-core/src/cake/api/{mod,text,image}.rs).

* ``POST /api/v1/chat/completions`` — OpenAI-shaped, one JSON response
  ``{id (uuid4), object: "chat.completion", created, model: "llama3",
  choices: [{index: 0, message: {role, content}}]}`` (text.rs:16-52,54-96).
  One request at a time (the reference's global write lock, text.rs:67):
  reset → add messages → generate.  Superset (Appendix E Q4/Q5): honours
  ``max_tokens``, ``stream`` (server-sent events) and per-request
  ``temperature`` / ``top_p`` / ``top_k`` / ``seed`` (the server's CLI values
  when absent; on the device path they are read by the decode graph from device
  memory, no recapture), adds a ``usage`` block
  and lowercase ``role`` (``CAKE_API_REFERENCE_ROLES=1`` restores the
  capitalised reference serialisation).  ``logprobs: true`` with ``top_logprobs`` in
  [0, 20] (the native engine) adds ``choices[0].logprobs.content``: one entry per
  emitted token, ``{token, id, logprob, bytes, top_logprobs: [{token, id, logprob,
  bytes}]}``; a non-finite log-prob is sent as -9999.0.  ``presence_penalty`` /
  ``frequency_penalty`` in [-2, 2], ``logit_bias`` (``{"<token id>": bias}``, at most 300
  entries, bias in [-100, 100]) and ``min_p`` in [0, 1] (the native engine) act on the
  logits before token selection (``engine.LogitControls``); absent or neutral values change
  nothing, and a generator that cannot honour them answers 400 instead of ignoring them.
  ``n`` in [1, 8] (the native engine on one GPU, 16-bit formats) returns ``n`` choices decoded
  as one lock-step batch, choice ``i`` drawing with ``seed + i``, ``usage`` summed; 400 for an
  out-of-range ``n`` and for ``n > 1`` with ``stream``, ``logprobs``, the logit controls or an
  engine that does not batch; an absent ``n`` or ``n = 1`` is the single-sequence path.
* ``POST /api/v1/image`` — body ``{"image_args": {...sd-* keys...}}``,
  returns ``{"images": [base64 PNG, ...]}`` (image.rs:15-68).
* anything else → 404 with body ``nope`` (mod.rs:19-21,40).
"""


import base64
import io
import json
import logging
import os
import threading
import time
import uuid

log = logging.getLogger("cake.api")


def _reference_roles() -> bool:
    return os.environ.get("CAKE_API_REFERENCE_ROLES", "0") == "1"


def request_sampling(body: dict, default):
    """SamplingConfig of one chat request: the server default with the request's
    temperature / top_p / top_k / seed.  ValueError on an invalid value."""
    import dataclasses
    over = {}
    if body.get("temperature") is not None:
        t = float(body["temperature"])
        if not t >= 0.0:
            raise ValueError("temperature must be >= 0")
        over["temperature"] = t
    if body.get("top_p") is not None:
        p = float(body["top_p"])
        if not 0.0 < p <= 1.0:
            raise ValueError("top_p must be in (0, 1]")
        over["top_p"] = None if p >= 1.0 else p
    if body.get("top_k") is not None:
        k = body["top_k"]
        if isinstance(k, bool) or not isinstance(k, int) or k < 0:
            raise ValueError("top_k must be a non-negative integer")
        over["top_k"] = k or None
    if body.get("seed") is not None:
        sd = body["seed"]
        if isinstance(sd, bool) or not isinstance(sd, int):
            raise ValueError("seed must be an integer")
        over["seed"] = sd & 0xFFFFFFFFFFFFFFFF
    return dataclasses.replace(default, **over)


LOGPROBS_MAX_TOP = 20
LOGPROB_FLOOR = -9999.0   # JSON has no -Infinity


def request_logprobs(body: dict) -> int | None:
    """The request's log-prob setting: None (not asked) or the number of alternatives per
    token.  ValueError on an invalid combination."""
    want = body.get("logprobs")
    if want is not None and not isinstance(want, bool):
        raise ValueError("logprobs must be a boolean")
    top = body.get("top_logprobs")
    if top is not None:
        if isinstance(top, bool) or not isinstance(top, int) or not 0 <= top <= LOGPROBS_MAX_TOP:
            raise ValueError(f"top_logprobs must be an integer in [0, {LOGPROBS_MAX_TOP}]")
        if not want:
            raise ValueError("top_logprobs needs logprobs: true")
    return (top or 0) if want else None


N_MAX = 8   # completions of one request: the engine's lock-step batch (engine.MAX_BATCH)


def request_n(body: dict) -> int:
    """The request's ``n`` (completions): 1 when absent, else an integer in [1, 8].
    ValueError on anything else."""
    n = body.get("n")
    if n is None:
        return 1
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= N_MAX:
        raise ValueError(f"n must be an integer in [1, {N_MAX}]")
    return n


def batch_refusal(body: dict, llm, want_lp, controls) -> str | None:
    """Why a request with n > 1 cannot be served (never ignored), or None."""
    if body.get("stream"):
        return "n > 1 cannot be streamed"
    if want_lp is not None:
        return "n > 1 does not return logprobs"
    if controls is not None:
        return ("n > 1 does not apply presence_penalty, frequency_penalty, logit_bias or "
                "min_p")
    if not hasattr(llm, "generate_n"):
        return ("n > 1 needs the native engine (a GPU, f16 / bf16, graphs on, "
                "CAKE_NATIVE != 0)")
    return llm.batch_refusal()


def request_logit_controls(body: dict, vocab_size: int | None = None):
    """The request's ``engine.LogitControls`` (presence_penalty, frequency_penalty, logit_bias
    in OpenAI's shape ``{"<token id>": bias}``, min_p), or None when every field is absent or
    neutral.  ValueError on an invalid value."""
    from ..engine import LogitControls
    bias = body.get("logit_bias")
    if bias is not None:
        if not isinstance(bias, dict):
            raise ValueError("logit_bias must be an object of token id -> bias")
        ids = {}
        for k, v in bias.items():
            # OpenAI's keys are the ids as decimal strings
            if not isinstance(k, str) or not k.isascii() or not k.isdigit():
                raise ValueError(f"logit_bias keys must be token ids (non-negative integers), "
                                 f"got {k!r}")
            ids[int(k)] = v
        if len(ids) != len(bias):
            raise ValueError("logit_bias names a token id twice")
        bias = ids

    def field(name):
        v = body.get(name)
        return 0.0 if v is None else v

    c = LogitControls(field("presence_penalty"), field("frequency_penalty"), bias,
                      body.get("min_p"))
    if vocab_size is not None:
        c.check_vocab(vocab_size)
    return None if c.neutral else c


def logprob_entry(llm, tok) -> dict:
    """One ``logprobs.content`` entry of an emitted Token."""
    import math

    def one(tid: int, lp, text=None) -> dict:
        if text is None:
            try:
                text = llm.tokenizer.decode([tid], skip_special_tokens=False) or ""
            except Exception:  # noqa: BLE001  (an id the tokenizer cannot render)
                text = ""
        v = float(lp) if lp is not None and math.isfinite(lp) else LOGPROB_FLOOR
        return {"token": text, "id": int(tid), "logprob": v, "bytes": list(text.encode("utf-8"))}

    e = one(tok.id, tok.logprob, tok.text or "")
    e["top_logprobs"] = [one(i, lp) for i, lp in (tok.top_logprobs or [])]
    return e


def create_app(master):
    from fastapi import FastAPI, Request
    from fastapi.responses import JSONResponse, PlainTextResponse, StreamingResponse

    from ..models.chat import Message

    app = FastAPI(title="cake_amd", docs_url=None, redoc_url=None, openapi_url=None)
    lock = threading.Lock()  # one generation at a time (text.rs:67)

    @app.post("/api/v1/chat/completions")
    async def chat(request: Request):
        body = await request.json()
        client = request.client.host if request.client else "?"
        log.info("starting chat for %s ...", client)
        if master.llm is None:
            return JSONResponse({"error": "LLM model not found"}, status_code=400)
        try:
            messages = [Message.from_dict(m) for m in body["messages"]]
        except (KeyError, TypeError, ValueError) as e:
            return JSONResponse({"error": f"bad request: {e}"}, status_code=400)
        max_tokens = body.get("max_tokens")
        default = getattr(master.ctx, "sampling", None)
        sampling = None
        if default is not None and hasattr(master.llm, "set_sampling"):
            try:
                sampling = request_sampling(body, default)
                check = getattr(master.llm, "check_sampling", None)
                if check is not None:
                    check(sampling)  # a generator may support only part of the space
            except (TypeError, ValueError) as e:
                return JSONResponse({"error": f"bad request: {e}"}, status_code=400)
        try:
            want_lp = request_logprobs(body)
        except ValueError as e:
            return JSONResponse({"error": f"bad request: {e}"}, status_code=400)
        if want_lp is not None and not hasattr(master.llm, "set_logprobs"):
            return JSONResponse({"error": "bad request: logprobs need the native engine (a "
                                          "GPU, f16 / bf16, graphs on, CAKE_NATIVE != 0)"},
                                status_code=400)
        try:
            controls = request_logit_controls(
                body, getattr(getattr(master.llm, "eng", None), "vocab_size", None))
        except ValueError as e:
            return JSONResponse({"error": f"bad request: {e}"}, status_code=400)
        if controls is not None and not hasattr(master.llm, "set_logit_controls"):
            return JSONResponse({"error": "bad request: presence_penalty, frequency_penalty, "
                                          "logit_bias and min_p need the native engine (a GPU, "
                                          "f16 / bf16, graphs on, CAKE_NATIVE != 0)"},
                                status_code=400)
        try:
            n = request_n(body)
        except ValueError as e:
            return JSONResponse({"error": f"bad request: {e}"}, status_code=400)
        model_name = master.llm.MODEL_NAME
        rid, created = str(uuid.uuid4()), int(time.time())
        role = "Assistant" if _reference_roles() else "assistant"
        if n > 1:  # n completions on one lock-step batch; n = 1 is the path below, untouched
            why = batch_refusal(body, master.llm, want_lp, controls)
            if why is not None:
                return JSONResponse({"error": f"bad request: {why}"}, status_code=400)

            def run_n():
                with lock:
                    master.reset()
                    if sampling is not None:
                        master.llm.set_sampling(sampling)
                    for m in messages:
                        master.llm.add_message(m)
                    want = max_tokens if max_tokens is not None else master.ctx.args.sample_len
                    return master.llm.generate_n(n, want)
            import anyio
            try:
                outs = await anyio.to_thread.run_sync(run_n)
            except RuntimeError as e:  # the engine's own refusal
                return JSONResponse({"error": f"bad request: {e}"}, status_code=400)
            return JSONResponse({
                "id": rid, "object": "chat.completion", "created": created, "model": model_name,
                "choices": [{"index": i, "message": {"role": role, "content": text},
                             "finish_reason": "stop"} for i, (text, _) in enumerate(outs)],
                "usage": {"completion_tokens": sum(c for _, c in outs)},
            })

        def run(sink, on_token=None):
            with lock:
                master.reset()
                if hasattr(master.llm, "set_logprobs"):
                    master.llm.set_logprobs(want_lp)
                if hasattr(master.llm, "set_logit_controls"):
                    master.llm.set_logit_controls(controls)
                # a new configuration, or an explicit seed (restart its stream)
                if sampling is not None and (body.get("seed") is not None or
                                             sampling != getattr(master.llm, "sampling", None)):
                    master.llm.set_sampling(sampling)
                for m in messages:
                    master.llm.add_message(m)
                if on_token is None:
                    return master.generate_text(sink, max_tokens=max_tokens)
                return master.generate_text(sink, max_tokens=max_tokens, on_token=on_token)

        if body.get("stream"):
            import queue
            q: queue.Queue = queue.Queue()

            def worker():
                try:
                    if want_lp is None:
                        run(lambda s: q.put(s))
                    else:  # the text sink runs first: pair each text with its token's entry
                        last: list[str] = []
                        run(last.append,
                            lambda t: q.put((last.pop(), logprob_entry(master.llm, t))))
                finally:
                    q.put(None)
            threading.Thread(target=worker, daemon=True).start()

            def events():
                while True:
                    s = q.get()
                    if s is None:
                        break
                    entry = None
                    if want_lp is not None:
                        s, entry = s
                    chunk = {"id": rid, "object": "chat.completion.chunk", "created": created,
                             "model": model_name,
                             "choices": [{"index": 0, "delta": {"content": s}, "finish_reason": None}]}
                    if entry is not None:
                        chunk["choices"][0]["logprobs"] = {"content": [entry]}
                    yield f"data: {json.dumps(chunk)}\n\n"
                yield "data: [DONE]\n\n"
            return StreamingResponse(events(), media_type="text/event-stream")

        import anyio
        parts: list[str] = []
        entries: list[dict] = []
        if want_lp is None:
            stats = await anyio.to_thread.run_sync(lambda: run(parts.append))
        else:
            stats = await anyio.to_thread.run_sync(lambda: run(
                parts.append, lambda t: entries.append(logprob_entry(master.llm, t))))
        text = "".join(parts)
        choice = {"index": 0, "message": {"role": role, "content": text}, "finish_reason": "stop"}
        if want_lp is not None:
            choice["logprobs"] = {"content": entries}
        return JSONResponse({
            "id": rid, "object": "chat.completion", "created": created, "model": model_name,
            "choices": [choice],
            "usage": {"completion_tokens": stats.get("generated", 0)},
        })

    @app.post("/api/v1/image")
    async def image(request: Request):
        body = await request.json()
        if master.sd is None:
            return JSONResponse({"error": "image model not found"}, status_code=400)
        from ..models.sd.args import ImageGenerationArgs
        args = ImageGenerationArgs.from_json(body.get("image_args", {}))
        out: list[str] = []

        def cb(images):
            for img in images:
                buf = io.BytesIO()
                img.save(buf, format="PNG")
                out.append(base64.b64encode(buf.getvalue()).decode())

        import anyio

        def run():
            with lock:
                master.generate_image(args, cb)
        await anyio.to_thread.run_sync(run)
        return JSONResponse({"images": out})

    @app.api_route("/{path:path}", methods=["GET", "POST", "PUT", "DELETE", "PATCH"])
    async def nope(path: str):
        return PlainTextResponse("nope", status_code=404)

    return app


def start(master, address: str) -> None:
    import uvicorn
    host, _, port = address.rpartition(":")
    log.info("starting api on http://%s:%s ...", host, port)
    uvicorn.run(create_app(master), host=host or "0.0.0.0", port=int(port), log_level="warning")
