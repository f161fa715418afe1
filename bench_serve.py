#!/usr/bin/env python3
"""Serving benchmark of the MI355X-native engine (``dstack_amd.serving``): offline throughput and
latency of one model replica on one GPU, random-init weights, synthetic prompts.

    python bench_serve.py --model llama-3-70b --num-prompts 256 --input-len 1024 --output-len 256
    python bench_serve.py --model llama-3-70b --latency --input-len 32000 --output-len 128
    python bench_serve.py --model llama-3-8b --num-prompts 64 --input-len 2048 --output-len 16 \
        --shared-prefix-len 1536 --enable-prefix-caching
    python bench_serve.py --model llama-3-8b --num-loras 8 --lora-rank 16      # requests round-robin over 8 adapters
    python bench_serve.py --model llama-3-8b --num-loras 8 --lora-idle         # adapters loaded, none requested

Throughput mode submits every prompt at t=0 (like ``vllm benchmark_throughput``) and reports
output and total tokens/s, TTFT / time-per-output-token percentiles, and the engine's prefill and
decode rates.  Latency mode runs single requests back to back (the reference's "single large
prompt" figure, BASELINE.md: ≈11.25 s for a ≈32k-token prompt, Llama 3.1 405B FP8 on 8×MI300X with
vLLM — a different model and GPU count, quoted for scale only).  Prints one JSON line.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _pct(xs, q):
    if not xs:
        return None
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(round(q / 100 * (len(xs) - 1))))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama-3-70b")
    ap.add_argument("--num-prompts", type=int, default=256)
    ap.add_argument("--input-len", type=int, default=1024)
    ap.add_argument("--output-len", type=int, default=256)
    ap.add_argument("--max-batch", type=int, default=256)
    ap.add_argument("--max-prefill-tokens", type=int, default=16384)
    ap.add_argument("--max-model-len", type=int, default=None)
    ap.add_argument("--latency", action="store_true", help="single requests back to back")
    ap.add_argument("--repeats", type=int, default=3, help="latency mode: requests")
    ap.add_argument("--no-graphs", action="store_true")
    ap.add_argument("--temperature", type=float, default=0.0)
    ap.add_argument("--top-p", type=float, default=1.0, help="nucleus sampling (1 = off)")
    ap.add_argument("--top-k", type=int, default=0, help="top-k sampling (0 = off)")
    ap.add_argument("--min-p", type=float, default=0.0, help="min-p sampling (0 = off)")
    ap.add_argument("--presence-penalty", type=float, default=0.0, help="on every request (0 = off)")
    ap.add_argument("--frequency-penalty", type=float, default=0.0, help="on every request (0 = off)")
    ap.add_argument("--repetition-penalty", type=float, default=1.0, help="on every request (1 = off)")
    ap.add_argument("--quantization", choices=["fp8", "mxfp4", "awq"], default=None)
    ap.add_argument("--kv-cache-dtype", choices=["auto", "fp8"], default="auto")
    ap.add_argument("--enable-prefix-caching", action="store_true",
                    help="reuse cached KV pages of a shared prompt prefix (dstack_amd.serving --enable-prefix-caching)")
    ap.add_argument("--shared-prefix-len", type=int, default=0,
                    help="the first N tokens of every prompt are identical (a system prompt / template); the rest "
                         "differ per prompt")
    ap.add_argument("--num-loras", type=int, default=0,
                    help="serve N random LoRA adapters (written to a temporary directory) and assign the requests "
                         "to them round-robin")
    ap.add_argument("--lora-rank", type=int, default=16, help="rank of the random adapters")
    ap.add_argument("--lora-idle", action="store_true",
                    help="with --num-loras: load the adapters but send every request to the base model")
    ap.add_argument("--speculative-ngram", type=int, default=0, metavar="K",
                    help="n-gram speculative decoding with K drafts (dstack_amd.serving --speculative-ngram)")
    ap.add_argument("--ngram-max", type=int, default=3)
    ap.add_argument("--ngram-min", type=int, default=1)
    ap.add_argument("--speculative-max-batch", type=int, default=32)
    ap.add_argument("--guided", choices=["json_object"], default=None,
                    help="every request carries this structured-output constraint (a built-in config decodes "
                         "with the byte tokenizer; a request ends with EOS when its document closes, or at "
                         "--output-len)")
    ap.add_argument("--max-guides", type=int, default=16, help="grammar slots (0: structured outputs off)")
    args = ap.parse_args()
    if args.lora_idle and not args.num_loras:
        ap.error("--lora-idle needs --num-loras")
    if not 0 <= args.shared_prefix_len <= args.input_len:
        ap.error("--shared-prefix-len must be within --input-len")

    import numpy as np
    import torch

    from dstack_amd.serving.engine import LLMEngine, SamplingParams

    max_len = args.max_model_len or max(args.input_len + args.output_len + 64, 2048)
    lora_modules, lora_dir = None, None
    if args.num_loras:
        import tempfile

        from dstack_amd.serving.lora import write_random_adapter
        from dstack_amd.serving.model import load_spec

        lora_dir = tempfile.TemporaryDirectory(prefix="bench_serve_lora_")
        cfg = load_spec(args.model).cfg
        lora_modules = {f"lora-{i}": write_random_adapter(os.path.join(lora_dir.name, f"lora-{i}"), cfg,
                                                          args.lora_rank, seed=i) for i in range(args.num_loras)}
    t0 = time.perf_counter()
    eng = LLMEngine.from_model(args.model, max_model_len=max_len, max_batch=1 if args.latency else args.max_batch,
                               max_prefill_tokens=args.max_prefill_tokens, use_graphs=not args.no_graphs and None,
                               quantization=args.quantization, kv_cache_dtype=args.kv_cache_dtype,
                               enable_prefix_caching=args.enable_prefix_caching, lora_modules=lora_modules,
                               max_lora_rank=max(args.lora_rank, 8), speculative_ngram=args.speculative_ngram,
                               ngram_max=args.ngram_max, ngram_min=args.ngram_min,
                               speculative_max_batch=args.speculative_max_batch, max_guides=args.max_guides)
    if lora_dir is not None:
        lora_dir.cleanup()  # the adapters are in HBM now
    t_load = time.perf_counter() - t0
    t0 = time.perf_counter()
    eng.capture_graphs()
    t_graph = time.perf_counter() - t0
    m = eng.model
    vocab = m.cfg.vocab_size
    rng = np.random.default_rng(0)
    sp = SamplingParams(max_tokens=args.output_len, temperature=args.temperature, top_p=args.top_p, top_k=args.top_k,
                        min_p=args.min_p, ignore_eos=True, presence_penalty=args.presence_penalty,
                        frequency_penalty=args.frequency_penalty, repetition_penalty=args.repetition_penalty)

    if args.guided:
        from dstack_amd.serving import guided
        from dstack_amd.serving.tokenizer import load_tokenizer

        if not eng.eos_token_ids:
            eng.eos_token_ids = tuple(load_tokenizer(m.spec.path, vocab).eos_token_ids)
        sp.ignore_eos, sp.guide = False, guided.compile_json_object()

    shared = rng.integers(10, vocab - 10, size=args.shared_prefix_len).tolist() if args.shared_prefix_len else []

    def prompts(n):
        return [shared + rng.integers(10, vocab - 10, size=args.input_len - len(shared)).tolist() for _ in range(n)]

    # warm-up: one short request through prefill and decode (hipBLASLt heuristics, allocator)
    eng.generate([prompts(1)[0][:128]], SamplingParams(max_tokens=4, ignore_eos=True))
    for k in eng.stats:
        eng.stats[k] = 0 if isinstance(eng.stats[k], int) else 0.0
    hit0 = eng.sched.prefix_hit_tokens  # (the scheduler's totals include the warm-up request)
    torch.cuda.synchronize() if torch.cuda.is_available() else None

    n = args.repeats if args.latency else args.num_prompts
    names = list(lora_modules) if lora_modules and not args.lora_idle else [None]
    lora = [names[i % len(names)] for i in range(n)]
    t0 = time.perf_counter()
    if args.latency:
        reqs = []
        for p, l in zip(prompts(n), lora):
            reqs += eng.generate([p], sp, lora=l)
    else:
        reqs = eng.generate(prompts(n), sp, lora=lora)
    elapsed = time.perf_counter() - t0
    out_tokens = sum(len(r.output_ids) for r in reqs)
    in_tokens = sum(len(r.prompt_ids) for r in reqs)
    ttft = [r.first_token_at - r.arrival for r in reqs]
    e2e = [r.finished_at - r.arrival for r in reqs]
    tpot = [(r.finished_at - r.first_token_at) / max(1, len(r.output_ids) - 1) for r in reqs]
    st = eng.stats
    hits = eng.sched.prefix_hit_tokens - hit0
    res = {
        "metric": "serving latency (s)" if args.latency else "serving output tokens/s",
        "value": round(_pct(e2e, 50), 4) if args.latency else round(out_tokens / elapsed, 1),
        "unit": "s" if args.latency else "tokens/s",
        "higher_is_better": not args.latency,
        "model": args.model, "dtype": str(m.dtype).replace("torch.", ""), "quantization": args.quantization,
        "kv_cache_dtype": args.kv_cache_dtype, "n_gpus": 1,
        "data": "synthetic prompts (uniform random token ids), random-init weights",
        "num_prompts": n, "input_len": args.input_len, "output_len": args.output_len,
        "temperature": args.temperature, "top_p": args.top_p, "top_k": args.top_k, "min_p": args.min_p,
        "presence_penalty": args.presence_penalty, "frequency_penalty": args.frequency_penalty,
        "repetition_penalty": args.repetition_penalty,
        "max_batch": eng.max_batch, "elapsed_s": round(elapsed, 3),
        "output_tokens_per_s": round(out_tokens / elapsed, 1),
        "total_tokens_per_s": round((in_tokens + out_tokens) / elapsed, 1),
        "ttft_p50_s": round(_pct(ttft, 50), 4), "ttft_p99_s": round(_pct(ttft, 99), 4),
        "tpot_p50_ms": round(_pct(tpot, 50) * 1e3, 3), "e2e_p50_s": round(_pct(e2e, 50), 4),
        "prefill_tokens_per_s": round(st["prefill_tokens"] / st["prefill_s"], 1) if st["prefill_s"] else None,
        # prompt tokens admitted (computed + served from the prefix cache) per second of prefill steps
        "prompt_tokens_per_prefill_s": round((st["prefill_tokens"] + hits) / st["prefill_s"], 1) if st["prefill_s"] else None,
        "guided": args.guided, "max_guides": eng.max_guides,
        "finished_stop": sum(r.finish_reason == "stop" for r in reqs),
        "num_loras": args.num_loras, "lora_rank": args.lora_rank if args.num_loras else None,
        "lora_idle": args.lora_idle, "lora_requests": sum(eng.lora_requests.values()),
        "prefix_caching": args.enable_prefix_caching, "shared_prefix_len": args.shared_prefix_len,
        "prefix_hit_tokens": hits, "prefill_s": round(st["prefill_s"], 4),
        "decode_tokens_per_s": round(st["decode_tokens"] / st["decode_s"], 1) if st["decode_s"] else None,
        "engine_steps": st["steps"], "preemptions": st["preemptions"],
        "weights_gb": round(m.weight_bytes() / 1e9, 1), "kv_pages": m.num_pages, "kv_tokens": m.num_pages * 64,
        "load_s": round(t_load, 1), "graph_capture_s": round(t_graph, 1), "graphs": len(eng._graphs),
        "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else "cpu",
    }
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
