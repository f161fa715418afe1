#!/usr/bin/env python3
"""Batched LoRA kernel microbenchmark (``ops/csrc/lora.hip``): microseconds per ``lora_shrink`` and
``lora_expand`` launch at the four projection shapes of a Llama model, next to the time the bytes
each launch has to move would take at HBM bandwidth.

    python tools/bench_lora.py [--models llama-3-8b llama-3-70b] [--rows 1 32 256] [--ranks 16 64]
                               [--adapters 1 8] [--iters 50]

Per (model, projection, rows, rank, distinct adapters): GPU time from hip events, the median of
``--iters`` launches after a warm-up, rows dealt to the adapters round-robin.  The bound counts what
must come from memory at least once: for shrink the rows of ``x`` (T K bf16), the ``A`` of each
distinct adapter (L K bf16) and ``t`` written (T L fp32); for expand ``t`` read, the ``B`` of each
distinct adapter (N R bf16) and ``y`` read and written (2 T N bf16) -- at 8 TB/s.  Rows that share
an adapter re-read its weights through L2, so the kernels' own traffic is T times the weights; the
ratio to the bound says what a kernel that grouped rows could still gain.  Prints one JSON line
per case and a table at the end."""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BPS = 8.0e12


def projections(cfg):
    """(name, K, slice_ends) of the four base projections."""
    hd, d, f = cfg.head_dim, cfg.dim, cfg.ffn_dim
    H, KVH = cfg.n_heads * hd, cfg.n_kv_heads * hd
    return [("wqkv", d, (H, H + KVH, H + 2 * KVH)), ("wo", H, (d,)), ("wgu", d, (f, 2 * f)), ("wdown", f, (d,))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=["llama-3-8b", "llama-3-70b"])
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 32, 256])
    ap.add_argument("--ranks", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--adapters", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()

    import torch

    from dstack_amd.models.llama import CONFIGS
    from dstack_amd.ops import serving as sops

    if not torch.cuda.is_available():
        sys.exit("bench_lora.py needs a ROCm GPU")
    dev = torch.device("cuda", 0)

    def gpu_us(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b) * 1e3)
        return statistics.median(times)

    table = []
    S = max(args.adapters)
    for model in args.models:
        for name, K, ends in projections(CONFIGS[model]):
            N, nsl = ends[-1], len(ends)
            for R in args.ranks:
                L = nsl * R
                g = torch.Generator(device=dev).manual_seed(K + N + R)
                A = (torch.randn(S, L, K, device=dev, generator=g) * 0.02).to(torch.bfloat16)
                B = (torch.randn(S, N, R, device=dev, generator=g) * 0.02).to(torch.bfloat16)
                for T in args.rows:
                    x = torch.randn(T, K, device=dev, generator=g).to(torch.bfloat16)
                    y = torch.randn(T, N, device=dev, generator=g).to(torch.bfloat16)
                    t = torch.zeros(T, L, device=dev)
                    for n_ad in args.adapters:
                        idx = (torch.arange(T, device=dev) % n_ad).to(torch.int32)
                        used = min(n_ad, T)
                        shrink_us = gpu_us(lambda: sops.lora_shrink(x, A, idx, out=t))
                        expand_us = gpu_us(lambda: sops.lora_expand(t, B, idx, ends, y))
                        shrink_b = T * K * 2 + used * L * K * 2 + T * L * 4
                        expand_b = T * L * 4 + used * N * R * 2 + 2 * T * N * 2
                        res = {"model": model, "proj": name, "K": K, "N": N, "slices": nsl, "R": R, "rows": T,
                               "adapters": n_ad, "shrink_us": round(shrink_us, 2),
                               "shrink_bound_us": round(shrink_b / HBM_BPS * 1e6, 2),
                               "expand_us": round(expand_us, 2), "expand_bound_us": round(expand_b / HBM_BPS * 1e6, 2)}
                        print(json.dumps(res), flush=True)
                        table.append(res)
                del A, B
    cols = ["model", "proj", "R", "rows", "adapters", "shrink_us", "shrink_bound_us", "expand_us", "expand_bound_us"]
    print(" ".join(f"{c:>15}" for c in cols))
    for r in table:
        print(" ".join(f"{r[c]!s:>15}" for c in cols))
    print(f"device: {torch.cuda.get_device_name(0)}")


if __name__ == "__main__":
    main()
