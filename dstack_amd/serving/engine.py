"""Continuous-batching inference engine (one process, one GPU, one model replica).

Step loop: the native scheduler (``_sched.Scheduler``, C++) plans a PREFILL step (newly admitted
prompts, packed) or a DECODE step (one token for every running sequence); the model runs it; the
fused sampler picks tokens; finished sequences release their KV pages.  Decode steps run from
hipGraphs captured once per batch bucket (padding rows are inert), so a small-batch step costs one
graph launch instead of ~10 kernel launches per layer.

Offline use::

    eng = LLMEngine.from_model("llama-3-8b")
    outs = eng.generate([[1, 2, 3]], SamplingParams(max_tokens=32))

Online use: ``start()`` runs the loop in a background thread; ``add_request`` takes an ``on_event``
callback that receives ``(request, token_id, finished)`` from that thread (the HTTP server turns it
into an asyncio queue).

Tensor parallel (``ServingLlama(tp_group=...)``, one process per GPU under torchrun): rank 0 is the
leader — scheduler, requests, sampling, HTTP — and broadcasts every step's inputs (one packed int64
tensor) to the followers, which run ``follow()``: the same model step on their shard, joining the
step's all-reduces and the logits all-gather.
"""

from __future__ import annotations

import itertools
import threading
import time
from dataclasses import dataclass, field

import numpy as np
import torch
import torch.distributed as dist

from dstack_amd.ops import serving as sops
from dstack_amd.serving.model import ServingLlama, check_awq, load_spec


@dataclass
class SamplingParams:
    max_tokens: int = 16
    temperature: float = 1.0
    top_p: float = 1.0
    top_k: int = 0
    min_p: float = 0.0  # keep tokens whose probability is at least min_p times the most likely one's
    top_logprobs: int = 0  # also return the N most likely tokens (<= 20) of every output position
    seed: int | None = None
    ignore_eos: bool = False
    stop_token_ids: tuple = ()
    # adjustments of the logits in front of truncation and the draw (ops.serving.apply_penalties)
    presence_penalty: float = 0.0  # subtracted from tokens generated so far; [-2, 2]
    frequency_penalty: float = 0.0  # times the token's count among the generated tokens; [-2, 2]
    repetition_penalty: float = 1.0  # divides (x > 0) or multiplies the logits of prompt and generated tokens; (0, 2]
    logit_bias: dict | None = None  # {token id: bias in [-100, 100]}, at most LOGIT_BIAS_MAX entries
    # structured output: a compiled grammar (serving.guided.Guide); every token's bytes must keep its DFA alive
    guide: object = None

    @property
    def wants_penalties(self) -> bool:
        return (self.presence_penalty != 0.0 or self.frequency_penalty != 0.0 or self.repetition_penalty != 1.0
                or bool(self.logit_bias))


def check_penalties(params: SamplingParams, vocab: int) -> dict:
    """Validate the penalty fields of ``params`` (ValueError outside the accepted ranges) and return
    its ``logit_bias`` as ``{int token id: float}``."""
    def num(name, lo, hi, open_lo=False):
        v = getattr(params, name)
        ok = not isinstance(v, bool) and isinstance(v, (int, float)) and (lo < v if open_lo else lo <= v) and v <= hi
        if not ok:
            raise ValueError(f"{name} must be in {'(' if open_lo else '['}{lo}, {hi}], got {v!r}")

    num("presence_penalty", -2, 2)
    num("frequency_penalty", -2, 2)
    num("repetition_penalty", 0, 2, open_lo=True)
    return sops.check_logit_bias(params.logit_bias, vocab)


@dataclass
class Request:
    id: int
    prompt_ids: list
    params: SamplingParams
    output_ids: list = field(default_factory=list)
    logprobs: list = field(default_factory=list)
    top_logprobs: list = field(default_factory=list)  # per output token: [(token_id, logprob), ...]
    finished: bool = False
    finish_reason: str | None = None
    arrival: float = field(default_factory=time.perf_counter)
    first_token_at: float | None = None
    finished_at: float | None = None
    on_event: object = None
    seed: int = 0
    cached_tokens: int = 0  # prompt tokens taken from the prefix cache at admission
    logit_bias: dict = field(default_factory=dict)  # params.logit_bias, validated: {int token id: float}
    lora: str | None = None  # the adapter the request asked for (add_request(..., lora=name))
    lora_slot: int = -1  # its slot in the model's adapter stacks; -1: the base model
    guide_state: int = 1  # the DFA state of params.guide after the tokens emitted so far (1: the start)

    @property
    def all_ids(self):
        return self.prompt_ids + self.output_ids


VERIFY_MAX_ROWS = 256  # the largest row count of a verify step (the decode GEMMs are tuned up to it)


def _buckets(max_batch: int):
    out, b = [], 1
    while b < max_batch:
        out.append(b)
        b = b * 2 if b < 32 else b + 32
    out.append(max_batch)
    return sorted(set(out))


class LLMEngine:
    def __init__(self, model: ServingLlama, max_batch: int = 256, max_prefill_tokens: int = 16384,
                 num_pages: int | None = None, use_graphs: bool | None = None, gpu_memory_utilization: float = 0.90,
                 eos_token_ids=(), enable_prefix_caching: bool = False, lora_modules: dict | None = None,
                 max_lora_rank: int = 64, speculative_ngram: int = 0, ngram_max: int = 3, ngram_min: int = 1,
                 speculative_max_batch: int = 32, max_guides: int = 16, token_bytes=None):
        from dstack_amd.serving import _native

        if isinstance(max_guides, bool) or not isinstance(max_guides, int) or max_guides < 0:
            raise ValueError(f"max_guides must be an integer >= 0, got {max_guides!r}")
        self.max_guides, self._token_bytes = max_guides, token_bytes

        if enable_prefix_caching and model.tp > 1:
            raise ValueError("prefix caching is not supported with tensor parallel yet")
        _check_speculative(speculative_ngram, ngram_max, ngram_min, speculative_max_batch,
                           model.tp > 1, lora_modules)
        # n-gram speculative decoding: K drafts per sequence, T = K + 1 rows of a verify step
        self.spec_k, self.spec_T = int(speculative_ngram), int(speculative_ngram) + 1
        self.ngram_max, self.ngram_min, self.spec_max_batch = int(ngram_max), int(ngram_min), int(speculative_max_batch)
        self._propose = _native.ngram_propose
        # LoRA adapters ({name: PEFT directory}): every adapter gets its own slot of the model's
        # stacks, loaded here -- before the KV cache is sized -- and kept for the engine's life
        self.lora_slots: dict[str, int] = {}
        if lora_modules:
            _check_lora(model.quantization, model.tp_group if model.tp > 1 else None)
            model.enable_lora(len(lora_modules), max_lora_rank)
            for slot, (name, path) in enumerate(lora_modules.items()):
                model.load_lora(slot, path)
                self.lora_slots[name] = slot
        self.lora_requests = {name: 0 for name in self.lora_slots}  # requests admitted per adapter
        self.prefix_caching = bool(enable_prefix_caching)
        self.model = model
        self.device = model.device
        self.tp, self.tp_group = model.tp, model.tp_group
        self.leader = model.tp_rank == 0
        if self.tp > 1:
            self._src = dist.get_global_rank(self.tp_group, 0)
        if self.device.type == "cuda":
            from dstack_amd.ops import gemm_tuning

            # hipBLASLt solutions tuned offline for the decode GEMMs (tools/tune_serving_gemms.py)
            self.gemm_tuning = gemm_tuning.setup(device_index=self.device.index or 0, kind="serving")
        if not model.k_cache:
            model.allocate_kv(num_pages, gpu_memory_utilization=gpu_memory_utilization)
        self.max_batch = max_batch
        self.sched = _native.Scheduler(num_pages=model.num_pages, page_size=sops.PAGE, max_batch=max_batch,
                                       max_prefill_tokens=max(max_prefill_tokens, model.max_model_len),
                                       max_model_len=model.max_model_len, pad_to=128,
                                       enable_prefix_caching=self.prefix_caching)
        self.width = self.sched.table_width
        self.eos_token_ids = tuple(eos_token_ids)
        self.requests: dict[int, Request] = {}
        self._ids = itertools.count()
        self._lock = threading.Lock()
        self._pending: list[Request] = []
        self._wake = threading.Event()
        self._thread = None
        self._stop = False
        # (tensor parallel: eager steps, so every rank issues the same RCCL collectives in order)
        self.use_graphs = (self.device.type == "cuda" and self.tp == 1) if use_graphs is None else use_graphs
        self.buckets = _buckets(max_batch)
        # decode graphs: bucket -> graph of the plain step; with adapters loaded also (bucket, "lora")
        # -> graph of the step with the LoRA kernels (a step whose rows all run the base model
        # replays the plain one)
        self._graphs: dict = {}
        # verify steps (speculative decoding): n sequences take n * T rows, padded to the smallest row
        # count of the bucket series -- every GEMM then runs at a row count the decode step already
        # has a tuned path for; with captured graphs also ("verify", R) -> graph
        self.verify_buckets = []
        if self.spec_k:
            series = [r for r in _buckets(VERIFY_MAX_ROWS)]
            want = {next((r for r in series if r >= n * self.spec_T), None)
                    for n in range(1, min(self.spec_max_batch, max_batch) + 1)}
            self.verify_buckets = sorted(r for r in want if r is not None)
        self._alloc_static()
        self.stats = dict(prefill_tokens=0, decode_tokens=0, steps=0, preemptions=0, prefill_s=0.0, decode_s=0.0)
        if self.max_guides:
            self.stats.update(guided_requests=0)
        if self.spec_k:
            self.stats.update(spec_steps=0, spec_drafted=0, spec_accepted=0)
        if self.prefix_caching:
            # (prefill_tokens counts computed tokens: an admitted prompt is its hit + computed tokens)
            self.stats.update(prefix_hit_tokens=0, prefix_query_tokens=0, prefix_cached_pages=0)

    @classmethod
    def from_model(cls, model: str, device=None, max_model_len: int | None = None, seed: int = 0, tp_group=None,
                   quantization: str | None = None, kv_cache_dtype: str = "auto", **kw):
        if kw.get("enable_prefix_caching") and tp_group is not None:
            raise ValueError("prefix caching is not supported with tensor parallel yet")
        if kw.get("lora_modules"):
            _check_lora(quantization, tp_group)  # before any weight is loaded
        _check_speculative(kw.get("speculative_ngram", 0), kw.get("ngram_max", 3), kw.get("ngram_min", 1),
                           kw.get("speculative_max_batch", 32), tp_group is not None, kw.get("lora_modules"))
        if quantization == "mxfp4" and tp_group is not None:
            raise ValueError("quantization=\"mxfp4\" is not supported with tensor parallel yet")
        spec = load_spec(model)
        if spec.awq is not None or quantization == "awq":  # an AWQ checkpoint selects the mode by itself
            check_awq(spec, quantization)
            quantization = "awq"
            if kw.get("lora_modules"):
                _check_lora(quantization, tp_group)
            if tp_group is not None:
                raise ValueError("quantization=\"awq\" is not supported with tensor parallel yet")
        device = device or ("cuda" if torch.cuda.is_available() else "cpu")
        m = ServingLlama(spec, device, max_model_len=max_model_len, tp_group=tp_group, quantization=quantization,
                         kv_cache_dtype=kv_cache_dtype)
        if spec.path:
            m.load_hf()  # (an AWQ checkpoint arrives 4-bit: nothing to quantize below)
        else:
            m.init_random(seed)
        if quantization == "fp8":
            m.quantize_fp8()  # before the KV cache is sized: the freed bf16 bytes become KV pages
        elif quantization == "mxfp4":
            m.quantize_mxfp4()
        elif quantization == "awq" and not spec.path:
            m.quantize_awq()  # built-in random weights: min/max rounding, so the benchmarks run without a checkpoint
        return cls(m, eos_token_ids=spec.eos_token_ids, **kw)

    # ------------------------------------------------------------------------------------------
    def _alloc_static(self):
        dev, B, W = self.device, self.max_batch, self.width
        # rows of the per-row buffers: a verify step (speculative decoding) has T rows per sequence
        N = self.rows_max = max([B] + self.verify_buckets)
        i32 = dict(dtype=torch.int32, device=dev)
        self.s_tokens = torch.zeros(N, dtype=torch.int64, device=dev)
        self.s_pos = torch.zeros(N, **i32)
        self.s_slots = torch.full((N,), -1, **i32)
        self.s_tables = torch.zeros(B, W, **i32)
        self.s_ctx = torch.zeros(B, **i32)
        self.s_temps = torch.zeros(N, dtype=torch.float32, device=dev)
        self.s_seeds = torch.zeros(N, dtype=torch.int64, device=dev)
        self.s_steps = torch.zeros(N, **i32)
        self.s_out_tok = torch.zeros(N, **i32)
        self.s_out_lp = torch.zeros(N, dtype=torch.float32, device=dev)
        # truncation and top-N log-probabilities (padding rows: k = 0, p = 1, min_p = 0, top_n = 0)
        self.s_top_k = torch.zeros(N, **i32)
        self.s_top_p = torch.ones(N, dtype=torch.float32, device=dev)
        self.s_min_p = torch.zeros(N, dtype=torch.float32, device=dev)
        self.s_top_n = torch.zeros(N, **i32)
        self.s_tau = torch.zeros(N, dtype=torch.float32, device=dev)
        self.s_top_ids = torch.full((N, sops.TOP_LOGPROBS_MAX), -1, **i32)
        self.s_top_lps = torch.full((N, sops.TOP_LOGPROBS_MAX), float("-inf"), dtype=torch.float32, device=dev)
        self._filter_rows_set = 0  # leading rows of the four parameter buffers that may hold a request's values
        # penalties and logit_bias: one state row and bias list per running sequence that asked (a
        # request takes a slot when its prompt is sampled and gives it back when it finishes or is
        # preempted), and per-row parameters (padding rows and rows that ask for nothing: slot -1)
        # (tensor parallel: only the leader samples, so only the leader holds state)
        self.p_state, self.p_bias_ids, self.p_bias_vals, self.p_bias_n = sops.alloc_penalty_state(
            B if self.leader else 1, self.model.cfg.vocab_size, dev)
        self.s_pen_slot = torch.full((N,), -1, **i32)
        self.s_pen = torch.empty(4, N, dtype=torch.float32, device=dev)  # rows: rep, 1 / rep, freq, pres
        self._reset_penalty_rows(N)
        self._pen_free = list(range(B - 1, -1, -1))
        self._pen_slots: dict[int, int] = {}  # request id -> slot
        self._alloc_guides(N)
        # LoRA: every row's adapter slot (padding rows and base-model rows: -1)
        self.s_lora_idx = torch.full((B,), -1, **i32)
        self._lora_rows_set = 0  # leading rows of s_lora_idx that may hold a slot
        self._ws = {b: sops.DecodeWorkspace(b, self.model.H, self.model.KVH, W, dev) for b in self.buckets}
        if self.spec_k:
            self.s_qlens = torch.zeros(B, **i32)  # rows in use per sequence of a verify step
            self._vws = {r: sops.VerifyWorkspace(r, self.spec_T, self.model.H, self.model.KVH, W, dev)
                         for r in self.verify_buckets}

    def _alloc_guides(self, N: int):
        """Structured outputs: a pool of ``max_guides`` grammars (16-bit transitions [G, 4096, 256] and
        uint8 acceptance [G, 4096]: 2 MiB + 4 KiB each), the tokenizer's byte table, the EOS ids and
        per-row (grammar slot, DFA state); padding rows and rows that ask for nothing: slot -1.
        Allocated after the KV cache is sized; only the leader samples, so only the leader holds it."""
        self.guide_error = None  # why guided requests are refused (None: they are accepted)
        self._guide_slot: dict[str, int] = {}  # content hash -> pool slot (resident grammars)
        self._guide_refs: dict[str, int] = {}  # content hash -> live requests that hold it
        self._guide_lru: dict[str, None] = {}  # resident, unreferenced hashes, least recently used first
        self._guide_free: list[int] = []
        self._guide_held: dict[int, str] = {}  # request id -> content hash
        self._guide_rows_set = 0
        self._eos_staged = None
        if not self.max_guides:
            self.guide_error = "structured outputs are disabled (max_guides = 0)"
            return
        if not self.leader:
            self.max_guides = 0
            return
        from dstack_amd.serving import guided
        from dstack_amd.serving.tokenizer import load_tokenizer

        dev, V, G = self.device, self.model.cfg.vocab_size, self.max_guides
        try:
            table = self._token_bytes
            if table is None:
                table = load_tokenizer(self.model.spec.path, V).token_bytes()
            off, blob = guided.pack_token_bytes(table, V)
        except Exception as e:  # noqa: BLE001 - an unsupported tokenizer refuses guided requests, nothing else
            self.guide_error, self.max_guides = f"structured outputs are not available: {e}", 0
            return
        self.token_bytes = [bytes(b) for b in table][:V] + [b""] * max(0, V - len(table))
        self.g_trans = torch.zeros(G, sops.GUIDE_MAX_STATES, 256, dtype=torch.int16, device=dev)
        self.g_accept = torch.zeros(G, sops.GUIDE_MAX_STATES, dtype=torch.uint8, device=dev)
        self.g_tok_off = torch.from_numpy(off).to(dev)
        self.g_tok_bytes = torch.from_numpy(blob).to(dev)
        self.g_eos = torch.full((sops.GUIDE_EOS_MAX,), -1, dtype=torch.int32, device=dev)
        self.g_n_eos = torch.zeros(1, dtype=torch.int32, device=dev)
        self.s_guide = torch.full((N,), -1, dtype=torch.int32, device=dev)
        self.s_guide_state = torch.zeros(N, dtype=torch.int32, device=dev)
        self._guide_free = list(range(G - 1, -1, -1))

    def _apply_guide(self, logits, guide, state):
        return sops.apply_guide(logits, guide, state, self.g_trans, self.g_accept, self.g_tok_off, self.g_tok_bytes,
                                self.g_eos, self.g_n_eos)

    def _reset_penalty_rows(self, m: int):
        self.s_pen_slot[:m].fill_(-1)
        self.s_pen[:2, :m].fill_(1.0)
        self.s_pen[2:, :m].zero_()
        self._pen_rows_set = 0  # leading rows of the penalty parameter buffers that may hold a request's values

    def _apply_penalties(self, logits, slot, pen):
        return sops.apply_penalties(logits, self.p_state, slot, pen[0], pen[1], pen[2], pen[3], self.p_bias_ids,
                                    self.p_bias_vals, self.p_bias_n)

    def _decode_body(self, b: int, lora: bool = False):
        logits = self.model.decode(self.s_tokens[:b], self.s_pos[:b], self.s_slots[:b], self.s_tables[:b],
                                   self.s_ctx[:b], ws=self._ws[b], **(dict(lora_idx=self.s_lora_idx[:b]) if lora else {}))
        self._apply_penalties(logits, self.s_pen_slot[:b], self.s_pen[:, :b])
        if self.max_guides:
            self._apply_guide(logits, self.s_guide[:b], self.s_guide_state[:b])
        sops.sample_filtered(logits, self.s_temps[:b], self.s_seeds[:b], self.s_steps[:b], self.s_top_k[:b],
                             self.s_top_p[:b], self.s_min_p[:b], self.s_out_tok[:b], self.s_out_lp[:b],
                             top_n=self.s_top_n[:b], top_ids=self.s_top_ids[:b], top_lps=self.s_top_lps[:b],
                             tau=self.s_tau[:b])
        sops.penalties_update(self.p_state, self.s_pen_slot[:b], self.s_out_tok[:b])
        return logits

    def _verify_seqs(self, R: int) -> int:
        """Sequences a verify step of R rows holds (its block-table rows)."""
        return min(R // self.spec_T, self.max_batch)

    def _verify_body(self, R: int):
        """The decode body over R rows, T per sequence, with the verify attention."""
        nb = self._verify_seqs(R)
        logits = self.model.verify(self.s_tokens[:R], self.s_pos[:R], self.s_slots[:R], self.s_tables[:nb],
                                   self.s_ctx[:nb], self.s_qlens[:nb], self.spec_T, ws=self._vws[R])
        self._apply_penalties(logits, self.s_pen_slot[:R], self.s_pen[:, :R])
        if self.max_guides:
            self._apply_guide(logits, self.s_guide[:R], self.s_guide_state[:R])
        sops.sample_filtered(logits, self.s_temps[:R], self.s_seeds[:R], self.s_steps[:R], self.s_top_k[:R],
                             self.s_top_p[:R], self.s_min_p[:R], self.s_out_tok[:R], self.s_out_lp[:R],
                             top_n=self.s_top_n[:R], top_ids=self.s_top_ids[:R], top_lps=self.s_top_lps[:R],
                             tau=self.s_tau[:R])
        sops.penalties_update(self.p_state, self.s_pen_slot[:R], self.s_out_tok[:R])
        return logits

    def capture_graphs(self):
        """One hipGraph per batch bucket (largest first, sharing one memory pool)."""
        if not self.use_graphs or self._graphs:
            return
        self.s_slots.fill_(-1)
        self.s_ctx.zero_()
        self.s_temps.zero_()
        self.s_top_k.zero_()
        self.s_top_p.fill_(1.0)
        self.s_min_p.zero_()
        self.s_top_n.zero_()
        self._filter_rows_set = 0
        self._reset_penalty_rows(self.rows_max)
        if self.max_guides:
            self.s_guide.fill_(-1)
            self._guide_rows_set = 0
        self.s_lora_idx.fill_(-1)
        self._lora_rows_set = 0
        if self.spec_k:
            self.s_qlens.zero_()
        variants = [False, True] if self.lora_slots else [False]
        torch.cuda.synchronize(self.device)
        s = torch.cuda.Stream(self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            # warm-up of every bucket: each row count may take a different GEMM path (HIP GEMV up to
            # 4 rows, the in-tree fp8 GEMM, hipBLASLt) and hipBLASLt may not set up a kernel inside
            # a capture ('operation not permitted when stream is capturing')
            for b in self.buckets:
                for lora in variants:
                    self._decode_body(b, lora)
            for r in self.verify_buckets:
                self._verify_body(r)
        torch.cuda.current_stream(self.device).wait_stream(s)
        pool = torch.cuda.graph_pool_handle()
        self._graph_logits = {}
        for b in reversed(self.buckets):
            for lora in variants:
                key = (b, "lora") if lora else b
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, pool=pool):
                    self._graph_logits[key] = self._decode_body(b, lora)
                self._graphs[key] = g
        for r in reversed(self.verify_buckets):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=pool):
                self._graph_logits["verify", r] = self._verify_body(r)
            self._graphs["verify", r] = g
        torch.cuda.synchronize(self.device)

    # ------------------------------------------------------------------------------------------
    def add_request(self, prompt_ids, params: SamplingParams | None = None, on_event=None,
                    lora: str | None = None) -> Request:
        params = params or SamplingParams()
        if lora is not None and lora not in self.lora_slots:
            raise ValueError(f"unknown LoRA adapter {lora!r} (loaded: {', '.join(self.lora_slots) or 'none'})")
        if not prompt_ids:
            raise ValueError("empty prompt")
        if len(prompt_ids) >= self.model.max_model_len:
            raise ValueError(f"prompt of {len(prompt_ids)} tokens does not fit max_model_len {self.model.max_model_len}")
        vocab = self.model.cfg.vocab_size
        if min(prompt_ids) < 0 or max(prompt_ids) >= vocab:
            raise ValueError(f"token ids must be in [0, {vocab})")
        if not 0.0 <= params.min_p <= 1.0:
            raise ValueError(f"min_p must be in [0, 1], got {params.min_p}")
        if not 0 <= params.top_logprobs <= sops.TOP_LOGPROBS_MAX:
            raise ValueError(f"top_logprobs must be in [0, {sops.TOP_LOGPROBS_MAX}], got {params.top_logprobs}")
        logit_bias = check_penalties(params, vocab)
        if params.guide is not None:
            self._check_guide(params)
        rid = next(self._ids)
        seed = params.seed if params.seed is not None else (rid * 7919 + 17)
        req = Request(rid, list(prompt_ids), params, on_event=on_event, seed=int(seed), logit_bias=logit_bias,
                      lora=lora, lora_slot=self.lora_slots[lora] if lora is not None else -1)
        with self._lock:
            if lora is not None:
                self.lora_requests[lora] += 1
            if params.guide is not None:
                self.stats["guided_requests"] += 1
            self.requests[rid] = req
            self._pending.append(req)
        self._wake.set()
        return req

    def abort(self, rid: int):
        with self._lock:
            req = self.requests.get(rid)
            if req is not None and not req.finished:
                req.finished, req.finish_reason = True, "abort"
                req.finished_at = time.perf_counter()
                self._aborted = getattr(self, "_aborted", set()) | {rid}
        self._wake.set()

    def has_work(self) -> bool:
        return bool(self._pending) or self.sched.num_running > 0 or self.sched.num_waiting > 0

    # ------------------------------------------------------------------------------------------
    def _admit_pending(self):
        with self._lock:
            pending, self._pending = self._pending, []
            aborted, self._aborted = getattr(self, "_aborted", set()), set()
        held = []
        for req in pending:
            if req.finished:
                continue
            if req.params.guide is not None and not self._take_guide(req):
                held.append(req)  # every grammar slot is referenced: wait for one (never dropped)
                continue
            if self.prefix_caching:
                # (the salt keeps the cached K/V of one adapter from serving another's prompt)
                self.sched.add(req.id, len(req.prompt_ids), len(req.prompt_ids) + req.params.max_tokens,
                               np.asarray(req.prompt_ids, dtype=np.int32), salt=req.lora_slot + 1)
            else:
                self.sched.add(req.id, len(req.prompt_ids), len(req.prompt_ids) + req.params.max_tokens)
        if held:
            with self._lock:
                self._pending[:0] = held
        for rid in aborted:
            self.sched.finish(rid)
            self._release_penalty_slot(rid)
            self._release_guide(rid)
            self._emit(self.requests.pop(rid, None), None, True)

    def _emit(self, req, token, finished):
        if req is not None and req.on_event is not None:
            req.on_event(req, token, finished)

    def step(self) -> int:
        """Run one scheduled step; returns the number of tokens produced."""
        self._admit_pending()
        if self.spec_k and 0 < self.sched.num_running <= self.spec_max_batch:
            plan = self.sched.schedule(False, self.spec_k)  # a decode plan then grants lookahead slots
        else:
            plan = self.sched.schedule(False)
        for rid in plan["preempted"]:
            self.stats["preemptions"] += 1
            self._release_penalty_slot(rid)  # rebuilt when its recompute prefill is sampled
        kind = plan["kind"]
        if kind == "idle":
            return 0
        ids = list(plan["seq_ids"])
        reqs = [self.requests[i] for i in ids]
        t0 = time.perf_counter()
        runs = drafts = None
        if kind == "decode" and "lookahead" in plan and self._verify_rows(len(reqs)) is not None:
            drafts = [self._drafts(r, int(g)) for r, g in zip(reqs, plan["lookahead"])]
        if kind == "prefill":
            toks = np.zeros(plan["rows"], dtype=np.int64)
            for r, off, n, st in zip(reqs, plan["offsets"], plan["lens"], plan["starts"]):
                toks[off : off + n] = r.all_ids[st : st + n]
                if not r.output_ids:  # (a readmission after preemption also hits generated tokens)
                    r.cached_tokens = int(st)
            if self.tp > 1:
                self._bcast_prefill(toks, plan["positions"], plan["slots"], plan["offsets"], plan["lens"])
            dev = self.device
            extra = dict(starts=plan["starts"], block_tables=plan["block_tables"]) if self.prefix_caching else {}
            if any(r.lora_slot >= 0 for r in reqs):
                # every row of a prompt's segment (its padding too, so neighbours of one adapter merge)
                lora_idx = np.full(plan["rows"], -1, dtype=np.int32)
                ends = list(plan["offsets"][1:]) + [plan["rows"]]
                for r, off, end in zip(reqs, plan["offsets"], ends):
                    lora_idx[off:end] = r.lora_slot
                extra["lora_idx"] = torch.from_numpy(lora_idx)
            logits = self.model.prefill(torch.from_numpy(toks).to(dev), torch.from_numpy(plan["positions"]).to(dev),
                                        torch.from_numpy(plan["slots"]).to(dev), plan["offsets"], plan["lens"], **extra)
            tokens, lps, tops = self._sample(logits, reqs)
            self.stats["prefill_tokens"] += int(sum(plan["lens"]))
            if self.prefix_caching:
                self.stats.update(prefix_hit_tokens=self.sched.prefix_hit_tokens,
                                  prefix_query_tokens=self.sched.prefix_query_tokens)
            self.stats["prefill_s"] += time.perf_counter() - t0
        elif drafts is not None and any(drafts):
            tokens, lps, tops, runs = self._verify(plan, reqs, drafts)
            self.stats["decode_s"] += time.perf_counter() - t0
        else:
            if "lookahead" in plan:  # (no sequence has a draft, or too many rows: the plain step)
                plan["positions"] = np.ascontiguousarray(plan["positions"][:, 0])
                plan["slots"] = np.ascontiguousarray(plan["slots"][:, 0])
            tokens, lps, tops = self._decode(plan, reqs)
            self.stats["decode_tokens"] += len(reqs)
            self.stats["decode_s"] += time.perf_counter() - t0
        self.stats["steps"] += 1
        if self.prefix_caching:
            self.stats["prefix_cached_pages"] = self.sched.cached_pages
        now = time.perf_counter()
        # the rows of the step's outputs that each request emits, in order: one, or (verify step) the
        # rows of its accepted drafts and the one after them
        verify = runs is not None
        if not verify:
            runs = [(i,) for i in range(len(reqs))]
        emitted = 0
        for req, rows in zip(reqs, runs):
            for i in rows:
                # (a verify step: the K/V of an accepted draft counts as cached once its token is kept)
                self.sched.mark_computed(req.id)
                if req.finished:  # aborted while the step ran
                    break
                tok = int(tokens[i])
                req.output_ids.append(tok)
                req.logprobs.append(float(lps[i]))
                if req.params.top_logprobs > 0:
                    req.top_logprobs.append([(t, l) for t, l in zip(tops[0][i], tops[1][i]) if t >= 0])
                if req.first_token_at is None:
                    req.first_token_at = now
                if self.prefix_caching:
                    self.sched.append(req.id, tok)
                else:
                    self.sched.append(req.id)
                emitted += 1
                if req.params.guide is not None:
                    # the host is the single source of truth of the DFA state
                    if tok not in self.eos_token_ids:
                        req.guide_state = self._guide_advance(req, tok)
                    elif not req.params.guide.accept[req.guide_state]:
                        raise RuntimeError(f"structured output: the mask let EOS {tok} through in state "
                                           f"{req.guide_state}, where the grammar of request {req.id} does not "
                                           "accept (a bug, not a request error)")
                reason = None
                if len(req.output_ids) >= req.params.max_tokens:
                    reason = "length"
                elif not req.params.ignore_eos and (tok in self.eos_token_ids or tok in req.params.stop_token_ids):
                    reason = "stop"
                elif len(req.all_ids) >= self.model.max_model_len:
                    reason = "length"
                if reason:
                    req.finished, req.finish_reason, req.finished_at = True, reason, now
                    self.sched.finish(req.id)
                    self._release_penalty_slot(req.id)
                    self._release_guide(req.id)
                self._emit(req, tok, req.finished)
                if req.finished:  # the tokens after a finishing one are dropped
                    self.requests.pop(req.id, None)
                    break
        if verify:
            self.stats["decode_tokens"] += emitted
            return emitted
        return len(reqs)

    def _seed_rows(self, reqs):
        temps = torch.tensor([r.params.temperature for r in reqs], dtype=torch.float32)
        seeds = torch.tensor([r.seed for r in reqs], dtype=torch.int64)
        steps = torch.tensor([len(r.output_ids) for r in reqs], dtype=torch.int32)
        return temps, seeds, steps

    def _filter_rows(self, reqs, rows: int | None = None):
        """top_k, top_p, min_p, top_n of the requests, padded with inert rows up to ``rows``."""
        pad = max(0, (rows or 0) - len(reqs))
        top_k = torch.tensor([r.params.top_k for r in reqs] + [0] * pad, dtype=torch.int32)
        top_p = torch.tensor([r.params.top_p for r in reqs] + [1.0] * pad, dtype=torch.float32)
        min_p = torch.tensor([r.params.min_p for r in reqs] + [0.0] * pad, dtype=torch.float32)
        top_n = torch.tensor([r.params.top_logprobs for r in reqs] + [0] * pad, dtype=torch.int32)
        return top_k, top_p, min_p, top_n

    def _stage_filters(self, reqs, b: int):
        """Stage truncation / top-N parameters into the static buffers.  Steps where no request asks
        for any (the common case) touch nothing: the buffers already hold inert rows."""
        p = [r.params for r in reqs]
        if any(q.top_k > 0 or q.top_p < 1.0 or q.min_p > 0.0 or q.top_logprobs > 0 for q in p):
            m = max(b, self._filter_rows_set)
            for buf, host in zip((self.s_top_k, self.s_top_p, self.s_min_p, self.s_top_n), self._filter_rows(reqs, m)):
                buf[:m].copy_(host, non_blocking=True)
            self._filter_rows_set = len(reqs)
        elif self._filter_rows_set:
            m, self._filter_rows_set = self._filter_rows_set, 0
            self.s_top_k[:m].zero_()
            self.s_top_p[:m].fill_(1.0)
            self.s_min_p[:m].zero_()
            self.s_top_n[:m].zero_()

    def _release_penalty_slot(self, rid: int):
        slot = self._pen_slots.pop(rid, None)
        if slot is not None:
            self._pen_free.append(slot)

    def _take_penalty_slot(self, req) -> int:
        """A free slot for ``req``, its state row and bias list rebuilt from the request (a
        readmission after preemption also counts the tokens generated so far)."""
        slot = self._pen_free.pop()  # at most max_batch sequences run and there are max_batch slots
        self._pen_slots[req.id] = slot
        sops.penalties_fill(self.p_state, self.p_bias_ids, self.p_bias_vals, self.p_bias_n, slot, req.prompt_ids,
                            req.output_ids, req.logit_bias)
        return slot

    def _penalty_rows(self, reqs, rows: int | None = None):
        """slot int32 [m] and (rep, 1 / rep, freq, pres) fp32 [4, m] of the requests, padded with inert
        rows up to ``rows``; a request without a slot asks for nothing."""
        pad = max(0, (rows or 0) - len(reqs))
        held = [r is not None and r.id in self._pen_slots for r in reqs]  # (None: a row that asks for nothing)
        slot = torch.tensor([self._pen_slots[r.id] if h else -1 for r, h in zip(reqs, held)] + [-1] * pad,
                            dtype=torch.int32)
        p = [r.params if h else SamplingParams() for r, h in zip(reqs, held)]
        rep = torch.tensor([q.repetition_penalty for q in p] + [1.0] * pad, dtype=torch.float32)
        freq = torch.tensor([q.frequency_penalty for q in p] + [0.0] * pad, dtype=torch.float32)
        pres = torch.tensor([q.presence_penalty for q in p] + [0.0] * pad, dtype=torch.float32)
        return slot, torch.stack([rep, sops.inv_rep_of(rep), freq, pres])

    def _stage_penalties(self, reqs, b: int):
        """Stage penalty slots and parameters into the static buffers, as ``_stage_filters`` does:
        steps where no request holds a slot (the common case) copy nothing."""
        if self._pen_slots and any(r is not None and r.id in self._pen_slots for r in reqs):
            m = max(b, self._pen_rows_set)
            slot, pen = self._penalty_rows(reqs, m)
            self.s_pen_slot[:m].copy_(slot, non_blocking=True)
            self.s_pen[:, :m].copy_(pen, non_blocking=True)
            self._pen_rows_set = len(reqs)
        elif self._pen_rows_set:
            self._reset_penalty_rows(self._pen_rows_set)

    def _stage_lora(self, reqs, b: int) -> bool:
        """Stage the rows' adapter slots into ``s_lora_idx``, as ``_stage_penalties`` does: steps where
        no request has an adapter copy nothing.  Returns whether the step needs the LoRA kernels."""
        if self.lora_slots and any(r.lora_slot >= 0 for r in reqs):
            m = max(b, self._lora_rows_set)
            idx = torch.tensor([r.lora_slot for r in reqs] + [-1] * (m - len(reqs)), dtype=torch.int32)
            self.s_lora_idx[:m].copy_(idx, non_blocking=True)
            self._lora_rows_set = len(reqs)
            return True
        if self._lora_rows_set:
            self.s_lora_idx[: self._lora_rows_set].fill_(-1)
            self._lora_rows_set = 0
        return False

    # ------------------------------------------------------------------------------------------
    # structured outputs
    # ------------------------------------------------------------------------------------------
    def _check_guide(self, params):
        from dstack_amd.serving.guided import Guide

        if self.guide_error:
            raise ValueError(self.guide_error)
        g = params.guide
        if not isinstance(g, Guide) or g.states > sops.GUIDE_MAX_STATES:
            raise ValueError("guide must be a compiled grammar (dstack_amd.serving.guided)")
        if params.ignore_eos:
            raise ValueError("ignore_eos cannot be combined with a structured output (guide): the grammar ends "
                             "the output with EOS")
        if not self.eos_token_ids:
            raise ValueError("a structured output needs an EOS token id to end with; the engine has none")

    def _take_guide(self, req) -> bool:
        """Reference the request's grammar, uploading it when it is not resident (into a free slot or
        over the least recently used unreferenced one).  False: every slot is referenced."""
        g = req.params.guide
        if req.id in self._guide_held:
            return True
        if g.key not in self._guide_slot:
            if self._guide_free:
                slot = self._guide_free.pop()
            elif self._guide_lru:
                old = next(iter(self._guide_lru))
                del self._guide_lru[old]
                slot = self._guide_slot.pop(old)
            else:
                return False
            S = g.states
            self.g_trans[slot].zero_()
            self.g_accept[slot].zero_()
            self.g_trans[slot, :S].copy_(torch.from_numpy(g.trans.view(np.int16)))
            self.g_accept[slot, :S].copy_(torch.from_numpy(g.accept))
            self._guide_slot[g.key] = slot
        self._guide_lru.pop(g.key, None)
        self._guide_refs[g.key] = self._guide_refs.get(g.key, 0) + 1
        self._guide_held[req.id] = g.key
        return True

    def _release_guide(self, rid: int):
        key = self._guide_held.pop(rid, None)
        if key is None:
            return
        self._guide_refs[key] -= 1
        if self._guide_refs[key] == 0:
            del self._guide_refs[key]
            self._guide_lru[key] = None  # stays resident until its slot is needed

    def _guide_advance(self, req, tok: int, state: int | None = None) -> int:
        from dstack_amd.serving.guided import advance

        s = advance(req.params.guide, req.guide_state if state is None else state, self.token_bytes[tok])
        if state is None and (s == 0 or not self.token_bytes[tok]):
            raise RuntimeError(f"structured output: the mask let token {tok} through, which the grammar of request "
                               f"{req.id} refuses in state {req.guide_state} (a bug, not a request error)")
        return s

    def _guide_rows(self, rows):
        """slot and state int32 tensors of ``rows``: per row ``(request, state)`` or None (nothing asked)."""
        slot = [self._guide_slot[self._guide_held[r[0].id]] if r is not None else -1 for r in rows]
        state = [r[1] if r is not None else 0 for r in rows]
        return torch.tensor(slot, dtype=torch.int32), torch.tensor(state, dtype=torch.int32)

    def _stage_eos(self):
        if self._eos_staged != self.eos_token_ids:
            ids = [int(e) for e in self.eos_token_ids][: sops.GUIDE_EOS_MAX]
            self.g_eos.copy_(torch.tensor(ids + [-1] * (sops.GUIDE_EOS_MAX - len(ids)), dtype=torch.int32))
            self.g_n_eos.fill_(len(ids))
            self._eos_staged = self.eos_token_ids

    def _stage_guides(self, rows, b: int):
        """Stage grammar slots and DFA states into the static buffers, as ``_stage_penalties`` does:
        steps where no row is guided (the common case) copy nothing."""
        if not self.max_guides:
            return
        if any(r is not None for r in rows):
            self._stage_eos()
            m = max(b, self._guide_rows_set)
            slot, state = self._guide_rows(list(rows) + [None] * (m - len(rows)))
            self.s_guide[:m].copy_(slot, non_blocking=True)
            self.s_guide_state[:m].copy_(state, non_blocking=True)
            self._guide_rows_set = len(rows)
        elif self._guide_rows_set:
            self.s_guide[: self._guide_rows_set].fill_(-1)
            self._guide_rows_set = 0

    @staticmethod
    def _tops(reqs, ids, lps):
        """The top-N outputs on the host, copied only in steps where some request asked for them."""
        if not any(r.params.top_logprobs > 0 for r in reqs):
            return None
        return ids.tolist(), lps.tolist()

    def _sample(self, logits, reqs):
        temps, seeds, steps = (t.to(self.device) for t in self._seed_rows(reqs))
        top_k, top_p, min_p, top_n = (t.to(self.device) for t in self._filter_rows(reqs))
        # the prefill path: a request that asks for a penalty or a bias takes its slot here, and the
        # same adjustment as in the decode graph runs eagerly around the sampler
        for r in reqs:
            if r.params.wants_penalties and r.id not in self._pen_slots:
                self._take_penalty_slot(r)
        slot = None
        if any(r.id in self._pen_slots for r in reqs):
            slot, pen = (t.to(self.device) for t in self._penalty_rows(reqs))
            self._apply_penalties(logits, slot, pen)
        if self.max_guides and any(r.params.guide is not None for r in reqs):
            self._stage_eos()
            gslot, gstate = self._guide_rows([(r, r.guide_state) if r.params.guide is not None else None for r in reqs])
            self._apply_guide(logits, gslot.to(self.device), gstate.to(self.device))
        tok, lp, ids, tlp = sops.sample_filtered(logits, temps, seeds, steps, top_k, top_p, min_p, top_n=top_n)
        if slot is not None:
            sops.penalties_update(self.p_state, slot, tok)
        return tok.tolist(), lp.tolist(), self._tops(reqs, ids, tlp)

    def _decode(self, plan, reqs):
        n = len(reqs)
        b = next(x for x in self.buckets if x >= n)
        temps, seeds, steps = self._seed_rows(reqs)
        last = torch.tensor([r.all_ids[-1] for r in reqs], dtype=torch.int64)
        nb = torch.from_numpy
        with torch.no_grad():
            # stage the step's inputs into the static buffers (padding rows: inert)
            self.s_tokens[:n].copy_(last, non_blocking=True)
            self.s_pos[:n].copy_(nb(plan["positions"]), non_blocking=True)
            self.s_slots[:n].copy_(nb(plan["slots"]), non_blocking=True)
            self.s_tables[:n].copy_(nb(plan["block_tables"]), non_blocking=True)
            self.s_ctx[:n].copy_(nb(plan["ctx_lens"]), non_blocking=True)
            self.s_temps[:n].copy_(temps, non_blocking=True)
            self.s_seeds[:n].copy_(seeds, non_blocking=True)
            self.s_steps[:n].copy_(steps, non_blocking=True)
            self._stage_filters(reqs, b)
            self._stage_penalties(reqs, b)
            self._stage_guides([(r, r.guide_state) if r.params.guide is not None else None for r in reqs], b)
            lora = self._stage_lora(reqs, b)
            if b > n:
                self.s_slots[n:b].fill_(-1)
                self.s_ctx[n:b].zero_()
                self.s_temps[n:b].zero_()
            if self.tp > 1:
                self._bcast_decode(b)
            key = (b, "lora") if lora else b
            if self._graphs and key in self._graphs:
                self._graphs[key].replay()
            else:
                self._decode_body(b, lora)
            return (self.s_out_tok[:n].tolist(), self.s_out_lp[:n].tolist(),
                    self._tops(reqs, self.s_top_ids[:n], self.s_top_lps[:n]))

    # ------------------------------------------------------------------------------------------
    # n-gram speculative decoding
    # ------------------------------------------------------------------------------------------
    def _verify_rows(self, n: int):
        """The row bucket of a verify step of n sequences, or None when it takes too many rows."""
        return next((r for r in self.verify_buckets if r >= n * self.spec_T), None) if n <= self.spec_max_batch else None

    def _drafts(self, req, grant: int):
        """The draft tokens of ``req`` for a step: the n-gram proposal over its tokens so far, at most
        ``grant`` of them.  None for a request that asks for a penalty or a logit_bias (it holds a state slot, whose
        counts depend on every earlier token)."""
        if grant <= 0 or req.params.wants_penalties:
            return []
        d = self._propose(np.asarray(req.all_ids, dtype=np.int32), grant, self.ngram_max, self.ngram_min).tolist()
        if req.params.guide is not None:
            # walk the drafts through the grammar and cut them at the first token it refuses
            s = req.guide_state
            for j, t in enumerate(d):
                s = self._guide_advance(req, t, s) if self.token_bytes[t] else 0
                if s == 0:
                    return d[:j]
        return d

    def _verify(self, plan, reqs, drafts):
        """One verify step: row ``b*T`` carries sequence b's last token and rows ``b*T + 1 ..`` its
        drafts; every row is sampled as the plain step would sample that position, and a draft is
        accepted iff it is the token drawn from the row before it.  Returns the step's flat outputs
        and, per request, the rows it emits (its accepted drafts' rows and the one after them)."""
        n, T = len(reqs), self.spec_T
        R = self._verify_rows(n)
        nb = self._verify_seqs(R)
        tokens, pos = np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.int32)
        slots = np.full(R, -1, dtype=np.int32)
        temps, seeds, steps = np.zeros(R, dtype=np.float32), np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.int32)
        ctx, qlens = np.zeros(nb, dtype=np.int32), np.zeros(nb, dtype=np.int32)
        for b, (r, d) in enumerate(zip(reqs, drafts)):
            q = 1 + len(d)
            rows = slice(b * T, b * T + q)
            tokens[rows] = [r.all_ids[-1]] + d
            pos[rows] = plan["positions"][b, :q]
            slots[rows] = plan["slots"][b, :q]
            temps[rows] = r.params.temperature
            seeds[rows] = r.seed
            steps[rows] = len(r.output_ids) + np.arange(q)
            ctx[b] = plan["ctx_lens"][b] + len(d)
            qlens[b] = q
        # per-row sampler inputs: a sequence's filters on all of its rows, its penalty slot on its first
        row_reqs = [r for r in reqs for _ in range(T)]
        pen_reqs = [r if j == 0 else None for r in reqs for j in range(T)]
        guide_rows = []  # row j of a guided sequence: the state after its drafts [:j]
        for r, d in zip(reqs, drafts):
            if r.params.guide is None:
                guide_rows += [None] * T
                continue
            s = r.guide_state
            for j in range(T):
                guide_rows.append((r, s) if j <= len(d) else None)
                if j < len(d):
                    s = self._guide_advance(r, d[j], s)
        nbf = torch.from_numpy
        with torch.no_grad():
            self.s_tokens[:R].copy_(nbf(tokens), non_blocking=True)
            self.s_pos[:R].copy_(nbf(pos), non_blocking=True)
            self.s_slots[:R].copy_(nbf(slots), non_blocking=True)
            self.s_tables[:n].copy_(nbf(plan["block_tables"]), non_blocking=True)
            self.s_ctx[:nb].copy_(nbf(ctx), non_blocking=True)
            self.s_qlens[:nb].copy_(nbf(qlens), non_blocking=True)
            self.s_temps[:R].copy_(nbf(temps), non_blocking=True)
            self.s_seeds[:R].copy_(nbf(seeds), non_blocking=True)
            self.s_steps[:R].copy_(nbf(steps), non_blocking=True)
            self._stage_filters(row_reqs, R)
            self._stage_penalties(pen_reqs, R)
            self._stage_guides(guide_rows, R)
            if ("verify", R) in self._graphs:
                self._graphs["verify", R].replay()
            else:
                self._verify_body(R)
            out_tok, out_lp = self.s_out_tok[:R].tolist(), self.s_out_lp[:R].tolist()
            tops = self._tops(reqs, self.s_top_ids[:R], self.s_top_lps[:R])
        runs = []
        for b, d in enumerate(drafts):
            a = 0
            while a < len(d) and out_tok[b * T + a] == d[a]:
                a += 1
            runs.append(tuple(range(b * T, b * T + a + 1)))
            self.stats["spec_drafted"] += len(d)
            self.stats["spec_accepted"] += a
        self.stats["spec_steps"] += 1
        return out_tok, out_lp, tops, runs

    # ------------------------------------------------------------------------------------------
    # tensor parallel: the leader broadcasts each step's inputs, followers replay them
    # ------------------------------------------------------------------------------------------
    _STOP, _PREFILL, _DECODE = 0, 1, 2

    def _bcast(self, header, payload=None):
        hdr = torch.tensor(header + [0] * (4 - len(header)), dtype=torch.int64, device=self.device)
        dist.broadcast(hdr, src=self._src, group=self.tp_group)
        if payload is not None:
            dist.broadcast(payload, src=self._src, group=self.tp_group)

    def _bcast_prefill(self, toks, positions, slots, offsets, lens):
        parts = [np.asarray(a, dtype=np.int64) for a in (toks, positions, slots, offsets, lens)]
        payload = torch.from_numpy(np.concatenate(parts)).to(self.device)
        self._bcast([self._PREFILL, len(lens), len(toks)], payload)

    def _bcast_decode(self, b: int):
        payload = torch.cat([self.s_tokens[:b], self.s_pos[:b].long(), self.s_slots[:b].long(), self.s_ctx[:b].long(),
                             self.s_tables[:b].long().flatten()])
        self._bcast([self._DECODE, b, b, self.width], payload)

    @torch.no_grad()
    def follow(self):
        """Follower rank loop: run the leader's steps on this rank's shard until it stops."""
        assert self.tp > 1 and not self.leader
        dev = self.device
        while True:
            hdr = torch.empty(4, dtype=torch.int64, device=dev)
            dist.broadcast(hdr, src=self._src, group=self.tp_group)
            kind, n, rows, width = hdr.tolist()
            if kind == self._STOP:
                return
            if kind == self._PREFILL:
                payload = torch.empty(3 * rows + 2 * n, dtype=torch.int64, device=dev)
                dist.broadcast(payload, src=self._src, group=self.tp_group)
                toks, pos, slots, offsets, lens = payload.split([rows, rows, rows, n, n])
                self.model.prefill(toks, pos.int(), slots.int(), offsets.tolist(), lens.tolist())
            else:
                b = n
                payload = torch.empty(4 * b + b * width, dtype=torch.int64, device=dev)
                dist.broadcast(payload, src=self._src, group=self.tp_group)
                toks, pos, slots, ctx, tables = payload.split([b, b, b, b, b * width])
                self.s_tokens[:b].copy_(toks)
                self.s_pos[:b].copy_(pos)
                self.s_slots[:b].copy_(slots)
                self.s_ctx[:b].copy_(ctx)
                self.s_tables[:b].copy_(tables.view(b, width))
                self.model.decode(self.s_tokens[:b], self.s_pos[:b], self.s_slots[:b], self.s_tables[:b],
                                  self.s_ctx[:b], ws=self._ws[b])

    def shutdown(self):
        """Leader: release the followers (tensor parallel) and stop the loop thread."""
        self.stop()
        if self.tp > 1 and self.leader and not getattr(self, "_released", False):
            self._released = True
            self._bcast([self._STOP])

    # ------------------------------------------------------------------------------------------
    def generate(self, prompts, params: SamplingParams | list | None = None, lora=None) -> list[Request]:
        """Offline batch generation: returns the finished requests in prompt order.  ``lora``: an
        adapter name for every prompt, or a list with one name (or None: the base model) per prompt."""
        ps = params if isinstance(params, list) else [params or SamplingParams()] * len(prompts)
        ls = lora if isinstance(lora, (list, tuple)) else [lora] * len(prompts)
        reqs = [self.add_request(p, sp, lora=l) for p, sp, l in zip(prompts, ps, ls)]
        while any(not r.finished for r in reqs):
            self.step()
        return reqs

    # ------------------------------------------------------------------------------------------
    def start(self):
        if self._thread is not None:
            return
        self._stop = False
        self._thread = threading.Thread(target=self._loop, name="dstack-amd-engine", daemon=True)
        self._thread.start()

    def stop(self):
        self._stop = True
        self._wake.set()
        if self._thread is not None:
            self._thread.join(timeout=30)
            self._thread = None

    def _loop(self):
        if self.device.type == "cuda":
            torch.cuda.set_device(self.device)
        while not self._stop:
            if not self.has_work():
                self._wake.wait(timeout=0.5)
                self._wake.clear()
                continue
            try:
                self.step()
            except Exception as e:  # noqa: BLE001 - fail every in-flight request, keep serving
                import logging

                logging.getLogger(__name__).exception("engine step failed")
                with self._lock:
                    victims = list(self.requests.values())
                    self.requests.clear()
                    self._pending.clear()
                for r in victims:
                    self.sched.finish(r.id)
                    self._release_penalty_slot(r.id)
                    self._release_guide(r.id)
                    r.finished, r.finish_reason = True, f"error: {e}"
                    self._emit(r, None, True)

    def metrics(self) -> dict:
        if self.prefix_caching:
            self.stats["prefix_cached_pages"] = self.sched.cached_pages
        if self.max_guides:
            self.stats["guided_grammars_resident"] = len(self._guide_slot)
        return dict(self.stats, running=self.sched.num_running, waiting=self.sched.num_waiting + len(self._pending),
                    kv_pages_free=self.sched.free_pages, kv_pages_total=self.sched.num_pages,
                    kv_usage=1.0 - self.sched.free_pages / max(1, self.sched.num_pages))


def _check_lora(quantization, tp_group):
    """The combinations LoRA adapters are refused with (see ``ServingLlama.enable_lora``)."""
    if quantization == "fp8":
        raise ValueError("LoRA adapters are not supported with quantization=\"fp8\": the fp8 projections take e4m3 "
                         "inputs and hand on unscaled outputs, so an adapter has neither a bf16 input nor a "
                         "finished output to add to (an fp8 KV cache is fine)")
    if quantization == "mxfp4":
        raise ValueError("LoRA adapters are not supported with quantization=\"mxfp4\": the decode GEMM takes e4m3 "
                         "activations against FP4 weights, and the adapter kernels are written for bf16 "
                         "projections (an fp8 KV cache is fine)")
    if quantization == "awq":
        raise ValueError("LoRA adapters are not supported with quantization=\"awq\" yet (an fp8 KV cache is fine)")
    if tp_group is not None:
        raise ValueError("LoRA adapters are not supported with tensor parallel yet")


def _check_speculative(speculative_ngram, ngram_max, ngram_min, speculative_max_batch, tensor_parallel, lora_modules):
    """The option values and combinations n-gram speculative decoding is refused with."""
    k = speculative_ngram
    if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k <= sops.VERIFY_MAX_T - 1:
        raise ValueError(f"speculative_ngram must be 0 (off) or in [1, {sops.VERIFY_MAX_T - 1}], got {k!r}")
    for name, v in (("ngram_min", ngram_min), ("ngram_max", ngram_max), ("speculative_max_batch", speculative_max_batch)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"{name} must be an integer >= 1, got {v!r}")
    if ngram_min > ngram_max:
        raise ValueError(f"ngram_min must not exceed ngram_max, got ngram_min={ngram_min}, ngram_max={ngram_max}")
    if k == 0:
        return
    if tensor_parallel:
        raise ValueError("speculative_ngram is not supported with tensor parallel yet")
    if lora_modules:
        raise ValueError("speculative_ngram is not supported with lora_modules (--lora-modules) yet: a verify step "
                         "runs without the adapter kernels")


def _filter_top_k_top_p(logits: torch.Tensor, reqs) -> torch.Tensor:
    """Mask logits outside each row's top-k / nucleus (top-p) set to -inf (rows that ask for it)."""
    if not any(r.params.top_p < 1.0 or r.params.top_k > 0 for r in reqs):
        return logits
    out = logits.clone()
    for i, r in enumerate(reqs):
        k, p = r.params.top_k, r.params.top_p
        if k <= 0 and p >= 1.0:
            continue
        row = out[i].float()
        if r.params.temperature > 0:
            row = row / r.params.temperature
        if k > 0:
            kth = torch.topk(row, min(k, row.numel())).values[-1]
            out[i][row < kth] = float("-inf")
            row = row.masked_fill(row < kth, float("-inf"))
        if p < 1.0:
            srt, idx = torch.sort(row, descending=True)
            cum = torch.softmax(srt, dim=-1).cumsum(-1)
            drop = cum - torch.softmax(srt, dim=-1) > p  # keep the smallest prefix reaching p
            out[i][idx[drop]] = float("-inf")
    return out
