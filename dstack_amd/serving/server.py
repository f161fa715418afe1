"""OpenAI-compatible HTTP server of the serving engine (what a ``type: service`` replica runs).

Routes: ``GET /health``, ``GET /v1/models``, ``POST /v1/completions``, ``POST /v1/chat/completions``
(both with SSE streaming), ``GET /metrics`` (Prometheus text: running/waiting sequences, KV-cache
usage, token counters, TTFT) — the gateway / in-server model proxy
(``dstack_amd/proxy/lib/model_proxy.py``) forwards OpenAI requests here, and the service
autoscaler reads replica load next to amdsmi GPU utilisation.  Reference parity: the reference's
services run vLLM/TGI and its model proxy speaks the same OpenAI API
(reference ``src/dstack/_internal/proxy/lib/routers/model_proxy.py:27-102``).

The engine loop runs in its own thread; each HTTP request gets an asyncio queue that the engine
thread feeds through ``loop.call_soon_threadsafe``.
"""

from __future__ import annotations

import asyncio
import collections
import json
import threading
import time
import uuid

from fastapi import FastAPI, HTTPException, Request
from fastapi.responses import JSONResponse, PlainTextResponse, StreamingResponse

from dstack_amd.ops.serving import TOP_LOGPROBS_MAX
from dstack_amd.serving.engine import LLMEngine, SamplingParams, check_penalties
from dstack_amd.serving import guided
from dstack_amd.serving.tokenizer import load_tokenizer

GUIDE_CACHE_SIZE = 64  # compiled grammars the server keeps, least recently used out first
GUIDE_FIELDS = ("response_format", "guided_json", "guided_regex", "guided_choice")


class _Stream:
    """Incremental detokenization with stop strings for one engine request."""

    def __init__(self, tok, stop):
        self.tok = tok
        self.stop = [s for s in (stop or []) if s]
        self.ids: list[int] = []
        self.text = ""
        self.stopped = False

    def push(self, token) -> str:
        if token is None or self.stopped:
            return ""
        self.ids.append(token)
        full = self.tok.decode(self.ids)
        if full.endswith("�"):  # an incomplete UTF-8 sequence: wait for the next token
            return ""
        for s in self.stop:
            i = full.find(s)
            if i >= 0:
                full = full[:i]
                self.stopped = True
                break
        delta = full[len(self.text):]
        self.text = full
        return delta


def create_app(engine: LLMEngine, served_model_name: str, tokenizer=None) -> FastAPI:
    tok = tokenizer or load_tokenizer(engine.model.spec.path, engine.model.cfg.vocab_size)
    if not engine.eos_token_ids:
        engine.eos_token_ids = tuple(tok.eos_token_ids)
    if served_model_name in engine.lora_slots:
        raise ValueError(f"LoRA adapter {served_model_name!r} has the served model's name")
    def _usage(prompt_tokens: int, completion_tokens: int, reqs) -> dict:
        u = {"prompt_tokens": prompt_tokens, "completion_tokens": completion_tokens,
             "total_tokens": prompt_tokens + completion_tokens}
        if engine.prefix_caching:  # prompt tokens served from the prefix cache (OpenAI's field for it)
            u["prompt_tokens_details"] = {"cached_tokens": sum(r.cached_tokens for r in reqs)}
        return u

    state = dict(requests=0, ttft_sum=0.0, ttft_n=0, gen_tokens=0, prompt_tokens=0, started=time.time(),
                 guide_compile_s=0.0)
    guide_cache: collections.OrderedDict = collections.OrderedDict()  # canonical JSON of the constraint -> Guide
    guide_lock = threading.Lock()

    from contextlib import asynccontextmanager

    @asynccontextmanager
    async def lifespan(app):
        engine.start()
        try:
            yield
        finally:
            engine.stop()

    app = FastAPI(title="dstack-amd serving", lifespan=lifespan)

    def _check_model(name):
        """``(name to echo, adapter or None)`` for a request's ``model``: the base model's name (or
        none) runs the base model, a loaded LoRA adapter's name runs that adapter."""
        if not name or name == served_model_name:
            return served_model_name, None
        if name in engine.lora_slots:
            return name, name
        raise HTTPException(404, detail={"message": f"model {name!r} does not exist", "type": "invalid_request_error",
                                         "code": "model_not_found"})

    def _bad(msg: str):
        return HTTPException(400, detail={"message": msg, "type": "invalid_request_error"})

    def _num(body: dict, key: str, kind, default):
        v = body.get(key)
        if v is None:
            return default
        if isinstance(v, bool) or not isinstance(v, (int, float)) or (kind is int and v != int(v)):
            raise _bad(f"{key} must be {'an integer' if kind is int else 'a number'}")
        return kind(v)

    def _top_logprobs(body: dict, chat: bool) -> int:
        """How many alternatives per position the request asks for: ``logprobs: N`` on
        /v1/completions, ``logprobs: true`` + ``top_logprobs: N`` on /v1/chat/completions."""
        if chat:
            n = _num(body, "top_logprobs", int, 0)
            if n and not body.get("logprobs"):
                raise _bad("top_logprobs requires logprobs: true")
        else:
            n = 0 if isinstance(body.get("logprobs"), bool) else _num(body, "logprobs", int, 0)
        if not 0 <= n <= TOP_LOGPROBS_MAX:
            raise _bad(f"{'top_logprobs' if chat else 'logprobs'} must be between 0 and {TOP_LOGPROBS_MAX}")
        return n

    def _constraint(body: dict):
        """``(field, kind, value)`` of the request's structured-output constraint, or None.  At most
        one of ``response_format`` (other than ``text``) and ``guided_json / _regex / _choice``."""
        given = [f for f in GUIDE_FIELDS if body.get(f) is not None]
        rf = body.get("response_format")
        if rf is not None:
            if not isinstance(rf, dict) or rf.get("type") not in ("text", "json_object", "json_schema"):
                raise _bad("response_format.type must be one of text, json_object, json_schema")
            if rf["type"] == "text":
                given.remove("response_format")
        if len(given) > 1:
            raise _bad(f"at most one structured-output field may be given, got {' and '.join(given)}")
        if not given:
            return None
        field = given[0]
        if field == "response_format":
            if rf["type"] == "json_object":
                return field, "json_object", None
            js = rf.get("json_schema")
            if not isinstance(js, dict) or not isinstance(js.get("schema"), dict):
                raise _bad("response_format.json_schema.schema must be a JSON schema object")
            return field, "json", js["schema"]
        return field, field[len("guided_"):], body[field]

    def _compile_guide(field: str, kind: str, value):
        """The compiled grammar of a constraint, from the cache or compiled here (the calling thread is
        a worker of the request handler, never the engine loop)."""
        try:
            key = json.dumps([kind, value], sort_keys=True, separators=(",", ":"))
        except (TypeError, ValueError):
            raise ValueError(f"{field} is not JSON-serialisable") from None
        with guide_lock:
            g = guide_cache.get(key)
            if g is not None:
                guide_cache.move_to_end(key)
        if g is None:
            t0 = time.perf_counter()
            try:
                if kind == "json_object":
                    g = guided.compile_json_object()
                elif kind == "json":
                    g = guided.compile_json_schema(value)
                elif kind == "regex":
                    g = guided.compile_regex(value)
                else:
                    g = guided.compile_choice(value)
            except ValueError as e:
                g = e  # a refusal is remembered too: asking again must not compile again
            with guide_lock:
                state["guide_compile_s"] += time.perf_counter() - t0
                guide_cache[key] = g
                while len(guide_cache) > GUIDE_CACHE_SIZE:
                    guide_cache.popitem(last=False)
        if isinstance(g, ValueError):
            raise ValueError(str(g))
        return g

    async def _guide(body: dict):
        """The request's compiled grammar or None; every refusal is a 400 that names the field."""
        c = _constraint(body)
        if c is None:
            return None
        if engine.guide_error:
            raise _bad(f"{c[0]}: {engine.guide_error}")
        if body.get("ignore_eos"):
            raise _bad(f"ignore_eos cannot be combined with {c[0]}: the grammar ends the output with EOS")
        try:
            return await asyncio.get_running_loop().run_in_executor(None, _compile_guide, *c)
        except ValueError as e:
            raise _bad(f"{c[0]}: {e}") from e

    def _params(body: dict, prompt_len: int, default_max: int, chat: bool = False, guide=None) -> SamplingParams:
        max_ctx = engine.model.max_model_len
        if prompt_len >= max_ctx:
            raise HTTPException(400, detail={"message": f"prompt has {prompt_len} tokens; this model's maximum "
                                             f"context length is {max_ctx}", "type": "invalid_request_error"})
        mt = body.get("max_tokens") or body.get("max_completion_tokens") or default_max
        mt = max(1, min(int(mt), max_ctx - prompt_len))
        stop_ids = tuple(body.get("stop_token_ids") or ())
        t = body.get("temperature")
        min_p = _num(body, "min_p", float, 0.0)
        if not 0.0 <= min_p <= 1.0:
            raise _bad("min_p must be between 0 and 1")
        sp = SamplingParams(max_tokens=mt, temperature=1.0 if t is None else float(t),
                            top_p=float(body.get("top_p") or 1.0), top_k=int(body.get("top_k") or 0),
                            min_p=min_p, top_logprobs=_top_logprobs(body, chat),
                            seed=body.get("seed"), ignore_eos=bool(body.get("ignore_eos", False)),
                            stop_token_ids=stop_ids,
                            presence_penalty=_num(body, "presence_penalty", float, 0.0),
                            frequency_penalty=_num(body, "frequency_penalty", float, 0.0),
                            repetition_penalty=_num(body, "repetition_penalty", float, 1.0),
                            logit_bias=body.get("logit_bias"), guide=guide)
        try:
            sp.logit_bias = check_penalties(sp, engine.model.cfg.vocab_size) or None
        except ValueError as e:
            raise _bad(str(e)) from e
        return sp

    def _submit(ids, params, stop, lora=None):
        loop = asyncio.get_running_loop()
        q: asyncio.Queue = asyncio.Queue()

        def on_event(req, token, finished):
            loop.call_soon_threadsafe(q.put_nowait, (token, finished, req.finish_reason))

        try:
            req = engine.add_request(ids, params, on_event=on_event, lora=lora)
        except ValueError as e:
            raise HTTPException(400, detail={"message": str(e), "type": "invalid_request_error"}) from e
        state["requests"] += 1
        state["prompt_tokens"] += len(ids)
        return req, q, _Stream(tok, stop)

    async def _drain(req, q, st):
        """Yields (delta_text, finish_reason or None) until the request finishes.  A consumer that
        goes away early (client disconnect: GeneratorExit / CancelledError in the streaming body or
        the awaiting handler) aborts the request, so it stops decoding and frees its KV pages."""
        t0 = time.perf_counter()
        first = True
        done = False
        try:
            while True:
                token, finished, reason = await q.get()
                if first and token is not None:
                    state["ttft_sum"] += time.perf_counter() - t0
                    state["ttft_n"] += 1
                    first = False
                if token is not None:
                    state["gen_tokens"] += 1
                delta = st.push(token)
                if st.stopped and not finished:
                    engine.abort(req.id)
                    done = True
                    yield delta, "stop"
                    return
                if finished:
                    done = True
                    if reason == "abort":
                        reason = "stop"
                    if reason and reason.startswith("error"):
                        raise HTTPException(500, detail={"message": reason, "type": "server_error"})
                    yield delta, reason
                    return
                if delta:
                    yield delta, None
        finally:
            if not done:
                engine.abort(req.id)

    def _abort_all(subs):
        for _, (req, _q, _st) in subs:
            if not req.finished:
                engine.abort(req.id)

    def _prompts(body):
        p = body.get("prompt")
        if p is None:
            raise HTTPException(400, detail={"message": "prompt is required", "type": "invalid_request_error"})
        if isinstance(p, str):
            return [tok.encode(p)]
        if isinstance(p, list) and p and all(isinstance(x, int) for x in p):
            return [p]
        if isinstance(p, list) and all(isinstance(x, str) for x in p):
            return [tok.encode(x) for x in p]
        if isinstance(p, list) and all(isinstance(x, list) for x in p):
            return p
        raise HTTPException(400, detail={"message": "unsupported prompt format", "type": "invalid_request_error"})

    def _alternatives(req, i):
        """[(token string, logprob)] of output position i, most likely first."""
        return [(tok.decode([t]), lp) for t, lp in req.top_logprobs[i]] if req.params.top_logprobs else []

    def _chat_logprob(req, i):
        """OpenAI's ``choices[].logprobs.content[]`` entry of output position i."""
        def entry(text, lp):
            return {"token": text, "logprob": lp, "bytes": list(text.encode("utf-8"))}

        e = entry(tok.decode([req.output_ids[i]]), req.logprobs[i])
        e["top_logprobs"] = [entry(text, lp) for text, lp in _alternatives(req, i)]
        return e

    def _stop(body):
        s = body.get("stop")
        return [s] if isinstance(s, str) else list(s or [])

    @app.get("/health")
    async def health():
        return {"status": "ok"}

    @app.get("/v1/models")
    async def models():
        card = {"object": "model", "created": int(state["started"]), "owned_by": "dstack-amd",
                "max_model_len": engine.model.max_model_len}
        return {"object": "list", "data": [dict(card, id=served_model_name)] + [
            dict(card, id=name, parent=served_model_name) for name in engine.lora_slots]}

    @app.post("/v1/completions")
    async def completions(request: Request):
        body = await request.json()
        model_name, lora = _check_model(body.get("model"))
        prompts = _prompts(body)
        guide = await _guide(body)
        n = int(body.get("n") or 1)
        rid = f"cmpl-{uuid.uuid4().hex[:24]}"
        created = int(time.time())
        # validate every prompt before submitting any: a 400 for prompt k must not leave prompts
        # 0..k-1 decoding with no consumer
        planned = []
        for p in prompts:
            for k in range(n):
                params = _params(body, len(p), 16, guide=guide)
                if params.seed is not None and n > 1:
                    params.seed = int(params.seed) + k
                planned.append((p, params))
        subs = []
        try:
            for p, params in planned:
                subs.append((p, _submit(p, params, _stop(body), lora)))
        except BaseException:
            _abort_all(subs)
            raise
        want_lp = body.get("logprobs") is not None

        if body.get("stream"):
            async def gen():
                usage = {"prompt_tokens": 0, "completion_tokens": 0}
                try:
                    for idx, (p, (req, q, st)) in enumerate(subs):
                        async for delta, reason in _drain(req, q, st):
                            ch = {"index": idx, "text": delta, "logprobs": None, "finish_reason": reason}
                            yield "data: " + json.dumps({"id": rid, "object": "text_completion", "created": created,
                                                         "model": model_name, "choices": [ch]}) + "\n\n"
                        usage["prompt_tokens"] += len(p)
                        usage["completion_tokens"] += len(req.output_ids)
                finally:
                    _abort_all(subs)  # the client left mid-stream: later choices were never read
                if (body.get("stream_options") or {}).get("include_usage"):
                    usage = _usage(usage["prompt_tokens"], usage["completion_tokens"], [s[1][0] for s in subs])
                    yield "data: " + json.dumps({"id": rid, "object": "text_completion", "created": created,
                                                 "model": model_name, "choices": [], "usage": usage}) + "\n\n"
                yield "data: [DONE]\n\n"

            return StreamingResponse(gen(), media_type="text/event-stream")

        choices, pt, ct = [], 0, 0
        try:
            for idx, (p, (req, q, st)) in enumerate(subs):
                text, reason = "", None
                async for delta, r in _drain(req, q, st):
                    text += delta
                    reason = r or reason
                lp = None
                if want_lp:
                    lp = {"tokens": [tok.decode([t]) for t in req.output_ids], "token_logprobs": list(req.logprobs)}
                    if req.params.top_logprobs:
                        lp["top_logprobs"] = []
                        for i in range(len(req.output_ids)):
                            alts: dict = {}
                            for alt, v in _alternatives(req, i):
                                alts.setdefault(alt, v)  # two ids with one string: the likelier one
                            lp["top_logprobs"].append(alts)
                choices.append({"index": idx, "text": text, "logprobs": lp, "finish_reason": reason})
                pt += len(p)
                ct += len(req.output_ids)
        finally:
            _abort_all(subs)
        return {"id": rid, "object": "text_completion", "created": created, "model": model_name,
                "choices": choices, "usage": _usage(pt, ct, [s[1][0] for s in subs])}

    @app.post("/v1/chat/completions")
    async def chat(request: Request):
        body = await request.json()
        model_name, lora = _check_model(body.get("model"))
        msgs = body.get("messages")
        if not isinstance(msgs, list) or not msgs:
            raise HTTPException(400, detail={"message": "messages must be a non-empty list", "type": "invalid_request_error"})
        ids = tok.encode(tok.apply_chat_template(msgs, add_generation_prompt=True), add_bos=True)
        params = _params(body, len(ids), engine.model.max_model_len - len(ids), chat=True, guide=await _guide(body))
        want_lp = bool(body.get("logprobs"))
        req, q, st = _submit(ids, params, _stop(body), lora)
        rid = f"chatcmpl-{uuid.uuid4().hex[:24]}"
        created = int(time.time())

        if body.get("stream"):
            async def gen():
                head = {"id": rid, "object": "chat.completion.chunk", "created": created, "model": model_name}
                yield "data: " + json.dumps(dict(head, choices=[{"index": 0, "delta": {"role": "assistant", "content": ""},
                                                                "finish_reason": None}])) + "\n\n"
                sent = 0  # output positions whose logprob entries went out already
                async for delta, reason in _drain(req, q, st):
                    d = {"content": delta} if delta else {}
                    ch = {"index": 0, "delta": d, "finish_reason": reason}
                    if want_lp:  # the tokens pushed since the previous chunk
                        ch["logprobs"] = {"content": [_chat_logprob(req, i) for i in range(sent, len(st.ids))]}
                        sent = len(st.ids)
                    yield "data: " + json.dumps(dict(head, choices=[ch])) + "\n\n"
                if (body.get("stream_options") or {}).get("include_usage"):
                    u = _usage(len(ids), len(req.output_ids), [req])
                    yield "data: " + json.dumps(dict(head, choices=[], usage=u)) + "\n\n"
                yield "data: [DONE]\n\n"

            return StreamingResponse(gen(), media_type="text/event-stream")

        text, reason = "", None
        async for delta, r in _drain(req, q, st):
            text += delta
            reason = r or reason
        choice = {"index": 0, "message": {"role": "assistant", "content": text}, "finish_reason": reason}
        if want_lp:
            choice["logprobs"] = {"content": [_chat_logprob(req, i) for i in range(len(st.ids))]}
        return {"id": rid, "object": "chat.completion", "created": created, "model": model_name,
                "choices": [choice],
                "usage": _usage(len(ids), len(req.output_ids), [req])}

    @app.get("/metrics")
    async def metrics():
        m = engine.metrics()
        lines = []

        def g(name, help_, val, kind="gauge"):
            lines.extend([f"# HELP {name} {help_}", f"# TYPE {name} {kind}", f"{name} {val}"])

        g("dstack_serving_running", "sequences in the running batch", m["running"])
        g("dstack_serving_waiting", "sequences waiting for admission", m["waiting"])
        g("dstack_serving_kv_usage", "fraction of KV-cache pages in use", round(m["kv_usage"], 6))
        g("dstack_serving_kv_pages_total", "KV-cache pages (64 tokens each)", m["kv_pages_total"])
        g("dstack_serving_requests_total", "requests received", state["requests"], "counter")
        g("dstack_serving_prompt_tokens_total", "prompt tokens received", state["prompt_tokens"], "counter")
        g("dstack_serving_generation_tokens_total", "tokens generated", state["gen_tokens"], "counter")
        g("dstack_serving_preemptions_total", "sequences preempted (recomputed)", m["preemptions"], "counter")
        if engine.lora_slots:
            name = "dstack_serving_lora_requests_total"
            lines.extend([f"# HELP {name} requests received per LoRA adapter", f"# TYPE {name} counter"])
            for adapter, n in engine.lora_requests.items():
                lines.append(f'{name}{{adapter="{adapter}"}} {n}')
        if engine.prefix_caching:
            g("dstack_serving_prefix_cache_hit_tokens_total", "prompt tokens served from the prefix cache",
              m["prefix_hit_tokens"], "counter")
            g("dstack_serving_prefix_cache_query_tokens_total", "prompt tokens looked up in the prefix cache",
              m["prefix_query_tokens"], "counter")
            g("dstack_serving_prefix_cached_pages", "KV-cache pages registered for prefix reuse (64 tokens each)",
              m["prefix_cached_pages"])
        if engine.spec_k:
            g("dstack_serving_spec_steps_total", "verify steps run (n-gram speculative decoding)", m["spec_steps"],
              "counter")
            g("dstack_serving_spec_draft_tokens_total", "draft tokens proposed and verified", m["spec_drafted"], "counter")
            g("dstack_serving_spec_accepted_tokens_total", "draft tokens accepted", m["spec_accepted"], "counter")
        if engine.max_guides:
            g("dstack_serving_guided_requests_total", "requests with a structured-output constraint",
              m["guided_requests"], "counter")
            g("dstack_serving_guided_grammars_resident", "compiled grammars resident on the device",
              m["guided_grammars_resident"])
            g("dstack_serving_guided_compile_seconds_total", "time spent compiling grammars",
              round(state["guide_compile_s"], 6), "counter")
        ttft = state["ttft_sum"] / state["ttft_n"] if state["ttft_n"] else 0.0
        g("dstack_serving_ttft_mean_seconds", "mean time to first token", round(ttft, 6))
        return PlainTextResponse("\n".join(lines) + "\n")

    @app.exception_handler(HTTPException)
    async def _http_error(request, exc: HTTPException):
        detail = exc.detail if isinstance(exc.detail, dict) else {"message": str(exc.detail)}
        return JSONResponse({"error": detail}, status_code=exc.status_code)

    return app
