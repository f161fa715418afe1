"""Paged-prefix prefill attention in isolation: time of ``sops.paged_prefill`` for one or more
segments of ``len`` new tokens over ``start`` cached ones (random page placement, what a
long-running server ends up with), with ``flash_attn_fwd`` over S = start + len rows beside it for
scale -- the work the engine does for the same prompt without the prefix cache.

    python tools/bench_paged_prefill.py                      # the default grid: 8B / 70B heads, bf16 / fp8
    python tools/bench_paged_prefill.py --start 1536 --len 512 --heads 32 --kv-heads 8 --cache-dtype fp8

Prints one JSON line per case.  Attention FLOPs are counted for the causal pairs only
(4 * 128 * pairs * H); device time from events around ``--iters`` launches after a warm-up."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, iters):
    import torch

    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e-3


def bench(start, n, H, KVH, cache_dtype, batch, iters):
    import torch

    from dstack_amd.ops import _ext
    from dstack_amd.ops import serving as sops

    dev = "cuda"
    fp8 = cache_dtype == "fp8"
    per_seq = (start + n + 63) // 64
    pages = batch * per_seq
    k, v = sops.alloc_cache(pages, KVH, torch.float8_e4m3fn if fp8 else torch.bfloat16, dev)
    if fp8:
        k.copy_(torch.randn(k.shape, device=dev).clamp(-4, 4).to(k.dtype))
        v.copy_(torch.randn(v.shape, device=dev).clamp(-4, 4).to(v.dtype))
    else:
        k.normal_()
        v.normal_()
    rows = (n + 127) // 128 * 128
    tables = torch.randperm(pages, device=dev).view(batch, per_seq).int().contiguous()
    i32 = dict(dtype=torch.int32, device=dev)
    offsets = torch.arange(batch, **i32) * rows
    starts = torch.full((batch,), start, **i32)
    lens = torch.full((batch,), n, **i32)
    qkv = torch.randn(batch * rows, (H + 2 * KVH) * 128, device=dev).to(torch.bfloat16)
    out = torch.zeros(batch * rows, H * 128, dtype=torch.bfloat16, device=dev)
    t = _time(lambda: sops.paged_prefill(qkv, k, v, tables, offsets, starts, lens, H, KVH, out=out, max_len=n), iters)
    pairs = batch * (n * start + n * (n + 1) // 2)
    S = start + n
    full = torch.randn(batch, S, (H + 2 * KVH) * 128, device=dev).to(torch.bfloat16)
    C = _ext.require()
    t_full = _time(lambda: C.flash_attn_fwd(full, H, KVH, True), iters)
    full_pairs = batch * S * (S + 1) // 2
    return {"start": start, "len": n, "H": H, "KVH": KVH, "cache": cache_dtype, "batch": batch,
            "paged_prefill_us": round(t * 1e6, 1), "paged_prefill_tflops": round(4 * 128 * pairs * H / t / 1e12, 1),
            "flash_attn_fwd_S": S, "flash_attn_fwd_us": round(t_full * 1e6, 1),
            "flash_attn_fwd_tflops": round(4 * 128 * full_pairs * H / t_full / 1e12, 1),
            "speedup_vs_full": round(t_full / t, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--start", type=int, default=None, help="cached tokens per segment")
    ap.add_argument("--len", type=int, default=512, help="new tokens per segment")
    ap.add_argument("--heads", type=int, default=None)
    ap.add_argument("--kv-heads", type=int, default=8)
    ap.add_argument("--cache-dtype", choices=["bf16", "fp8"], default=None)
    ap.add_argument("--batch", type=int, default=8, help="segments per launch")
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_paged_prefill needs a ROCm GPU")
    for start in ([a.start] if a.start is not None else [1536, 7680]):
        for H in ([a.heads] if a.heads else [32, 64]):  # Llama-3 8B / 70B query heads (8 KV heads)
            for cd in ([a.cache_dtype] if a.cache_dtype else ["bf16", "fp8"]):
                print(json.dumps(bench(start, a.len, H, a.kv_heads, cd, a.batch, a.iters)), flush=True)


if __name__ == "__main__":
    main()
