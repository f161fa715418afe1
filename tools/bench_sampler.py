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
  ``sample`` kernel;
- ``idle_chain``: what the decode graph runs when no request asks for a penalty -- ``apply_penalties``
  with every slot -1, ``sample_filtered`` with nothing asked for, ``penalties_update`` -- to set beside
  ``unfiltered``; ``noop_launch``: one launch that does nothing (``penalties_update``, every slot -1);
- ``penalised``: ``apply_penalties`` alone with every row penalised (repetition, frequency, presence),
  without and with 300 ``logit_bias`` entries per row, and the rate it reaches counting 8 B per
  element (2 B + 4 B read, 2 B written); ``penalised_chain``: the same in front of the sampler.

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

        # penalties / logit_bias in front of the sampler (csrc/penalties.hip), as the decode graph chains them
        V = args.vocab
        state, bias_ids, bias_vals, bias_n = sops.alloc_penalty_state(R, V, dev)
        state.copy_(torch.randint(0, 4, (R, V), device=dev, dtype=torch.int32))
        bias_ids.copy_(torch.stack([torch.randperm(V, device=dev)[: sops.LOGIT_BIAS_MAX] for _ in range(R)]))
        bias_vals.uniform_(-5, 5)
        idle = torch.full((R,), -1, device=dev, dtype=torch.int32)
        slot = torch.arange(R, device=dev, dtype=torch.int32).flip(0)
        rep = torch.full((R,), 1.1, device=dev)
        freq, pres = torch.full((R,), 0.5, device=dev), torch.full((R,), 0.25, device=dev)
        pen = logits.clone()  # (rewritten in place by every call; the time does not depend on the values)

        inv = sops.inv_rep_of(rep)

        def apply(s):
            sops.apply_penalties(pen, state, s, rep, inv, freq, pres, bias_ids, bias_vals, bias_n)

        def chain(s):
            apply(s)
            sops.sample_filtered(pen, temps, seeds, steps, zero_i, ones, zeros, **out)
            sops.penalties_update(state, s, out["tokens"])

        res["idle_chain_ms"] = round(gpu_ms(lambda: chain(idle), args.iters), 4)
        res["noop_launch_ms"] = round(gpu_ms(lambda: sops.penalties_update(state, idle, out["tokens"]), args.iters), 4)
        res["penalised_ms"] = round(gpu_ms(lambda: apply(slot), args.iters), 4)
        res["penalised_chain_ms"] = round(gpu_ms(lambda: chain(slot), args.iters), 4)
        bias_n.fill_(sops.LOGIT_BIAS_MAX)
        res["penalised_bias300_ms"] = round(gpu_ms(lambda: apply(slot), args.iters), 4)
        for k in ("penalised_ms", "penalised_bias300_ms"):  # 2 B + 4 B read, 2 B written per element
            res[k.replace("_ms", "_tbps")] = round(R * V * 8 / (res[k] * 1e-3) / 1e12, 3)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
