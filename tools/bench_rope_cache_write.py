#!/usr/bin/env python3
"""RoPE + cache-write microbenchmark: what the q/k-norm form (Qwen3) costs over the plain form.

    python tools/bench_rope_cache_write.py [--rows 256 16384] [--heads 32] [--kv-heads 8] [--iters 50]

Per row count and cache type (bf16, e4m3) it times ``ops.serving.rope_cache_write`` without and with
norm weights on the same tensors, the two alternating: GPU time of one eager launch (hip events,
median of ``--iters`` after warm-up).  The comparison is against the un-normed form of the same
kernel, not against a separate norm pass.  Under ``rocprofv3 --kernel-trace --stats`` the same run
gives the kernels' own times.  Prints one JSON line per row count and cache type.
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
    ap.add_argument("--rows", type=int, nargs="+", default=[256, 16384])
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--kv-heads", type=int, default=8)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()

    import torch

    from dstack_amd.ops import serving as sops
    from dstack_amd.serving.model import rope_tables

    dev = torch.device("cuda", 0)
    H, KVH = args.heads, args.kv_heads
    cos, sin = rope_tables(max(args.rows) + 64, 128, 1e6, None, dev)
    norm = dict(q_norm=torch.rand(128, device=dev) + 0.5, k_norm=torch.rand(128, device=dev) + 0.5, eps=1e-6)
    for T in args.rows:
        torch.manual_seed(T)
        qkv = torch.randn(T, (H + 2 * KVH) * 128, device=dev).to(torch.bfloat16)
        pos = torch.arange(T, device=dev, dtype=torch.int32)
        slots = torch.randperm(T, device=dev).int()
        for cache_dtype in (torch.bfloat16, torch.float8_e4m3fn):
            kc, vc = sops.alloc_cache((T + 63) // 64, KVH, cache_dtype, dev)
            times = {"plain": [], "qk_norm": []}
            for it in range(args.iters + 3):  # (qkv is rewritten in place; the time does not depend on the values)
                for name, kw in (("plain", {}), ("qk_norm", norm)):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    sops.rope_cache_write(qkv, pos, slots, cos, sin, kc, vc, H, KVH, **kw)
                    b.record()
                    torch.cuda.synchronize()
                    if it >= 3:
                        times[name].append(a.elapsed_time(b) * 1e3)
            med = {k: statistics.median(v) for k, v in times.items()}
            print(json.dumps({"rows": T, "heads": H, "kv_heads": KVH, "cache": str(cache_dtype).split(".")[-1],
                              "plain_us": round(med["plain"], 2), "qk_norm_us": round(med["qk_norm"], 2),
                              "ratio": round(med["qk_norm"] / med["plain"], 3),
                              "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
