#!/usr/bin/env python3
"""Sampler microbenchmark: what truncated sampling costs per decode step, R rows of V bf16 logits.

    python tools/bench_sampler.py [--rows 1 32 256] [--vocab 128256] [--top-p 0.9] [--iters 20]

Per row count it times (GPU time, hip events, median of ``--iters`` after warm-up):

- ``python_filter``: the per-row PyTorch filter (``engine._filter_top_k_top_p``: topk / sort / softmax /
  mask per row) followed by ``ops.serving.sample`` -- the path the engine took before the in-graph
  sampler;
- ``filtered``: ``ops.serving.sample_filtered`` with top-p on every row (threshold + masked draw +
  the idle top-N kernel, as the decode graph runs them);
- ``unfiltered`` against ``sample``: ``sample_filtered`` with nothing asked for, and the plain
  ``sample`` kernel.

Prints one JSON line per row count.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 32, 256])
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--top-p", type=float, default=0.9)
    ap.add_argument("--temperature", type=float, default=0.8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--python-iters", type=int, default=3, help="iterations of the (slow) per-row PyTorch filter")
    args = ap.parse_args()

    import torch

    from dstack_amd.ops import serving as sops
    from dstack_amd.serving.engine import SamplingParams, _filter_top_k_top_p

    dev = torch.device("cuda", 0)

    def gpu_ms(fn, iters):
        fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b))
        return statistics.median(times)

    class Req:
        def __init__(self, params):
            self.params = params

    for R in args.rows:
        torch.manual_seed(R)
        logits = (torch.randn(R, args.vocab, device=dev) * 3).to(torch.bfloat16)
        temps = torch.full((R,), args.temperature, device=dev)
        seeds = torch.arange(R, device=dev, dtype=torch.int64)
        steps = torch.zeros(R, device=dev, dtype=torch.int32)
        zero_i = torch.zeros(R, device=dev, dtype=torch.int32)
        ones, zeros = torch.ones(R, device=dev), torch.zeros(R, device=dev)
        top_p = torch.full((R,), args.top_p, device=dev)
        out = dict(tokens=torch.empty(R, device=dev, dtype=torch.int32), logprobs=torch.empty(R, device=dev),
                   top_n=zero_i, top_ids=torch.empty(R, sops.TOP_LOGPROBS_MAX, device=dev, dtype=torch.int32),
                   top_lps=torch.empty(R, sops.TOP_LOGPROBS_MAX, device=dev), tau=torch.empty(R, device=dev))
        reqs = [Req(SamplingParams(temperature=args.temperature, top_p=args.top_p)) for _ in range(R)]

        def python_filter():
            sops.sample(_filter_top_k_top_p(logits, reqs), temps, seeds, steps, out["tokens"], out["logprobs"])

        res = {
            "rows": R, "vocab": args.vocab, "top_p": args.top_p, "temperature": args.temperature,
            "python_filter_ms": round(gpu_ms(python_filter, args.python_iters), 4),
            "filtered_ms": round(gpu_ms(lambda: sops.sample_filtered(logits, temps, seeds, steps, zero_i, top_p, zeros,
                                                                     **out), args.iters), 4),
            "unfiltered_ms": round(gpu_ms(lambda: sops.sample_filtered(logits, temps, seeds, steps, zero_i, ones, zeros,
                                                                       **out), args.iters), 4),
            "sample_ms": round(gpu_ms(lambda: sops.sample(logits, temps, seeds, steps, out["tokens"], out["logprobs"]),
                                      args.iters), 4),
            "threshold_ms": round(gpu_ms(lambda: sops.sample_threshold(logits, temps, zero_i, top_p, zeros,
                                                                       out=out["tau"]), args.iters), 4),
            "device": torch.cuda.get_device_name(0),
        }
        res["filtered_speedup"] = round(res["python_filter_ms"] / res["filtered_ms"], 1)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
