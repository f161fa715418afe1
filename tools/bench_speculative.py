"""N-gram speculative decoding in isolation.

    python tools/bench_speculative.py kernel          # paged_verify (T = 5) vs paged_decode vs paged_prefill
    python tools/bench_speculative.py step --model llama-3-8b [--quantization fp8] [--kv-cache-dtype fp8]
                                                      # captured verify step (K = 4) vs captured decode step

``kernel``: Llama-3-8B (32 / 8) and -70B (64 / 8) heads, bf16 and e4m3 caches, batch 1 x 32k context
and batch 32 x 1k, random page placement.  All three kernels read the same K/V bytes; ``TBps`` is
those bytes over the time.  ``step``: the engine's own hipGraphs at 1, 4, 8, 16 and 32 sequences of
about 1k context, timed with device events; ``ratio`` - 1 is the number of accepted drafts per step
at which speculation breaks even.  Two passes of every measurement, alternating, so the spread is
in the output."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, iters, warmup=5):
    import torch

    for _ in range(warmup):
        fn()
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    beg.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return beg.elapsed_time(end) * 1e-3 / iters


def kernel(args):
    import torch

    from dstack_amd.ops import serving as sops

    dev, T = "cuda", args.T
    g = torch.Generator(device="cpu").manual_seed(0)
    for H, KVH in ((32, 8), (64, 8)):
        for dtype in (torch.bfloat16, torch.float8_e4m3fn):
            for B, ctx in ((1, 32768), (32, 1024)):
                npg = ctx // sops.PAGE
                pages_total = B * npg + 64
                k, v = sops.alloc_cache(pages_total, KVH, torch.bfloat16, dev)
                k.normal_()
                v.normal_()
                k, v = k.to(dtype), v.to(dtype)
                W = npg
                tables = torch.randperm(pages_total, generator=g)[: B * npg].view(B, npg).int().to(dev)
                i32 = dict(dtype=torch.int32, device=dev)
                ctx_t = torch.full((B,), ctx, **i32)
                q1 = torch.randn(B, (H + 2 * KVH) * 128, device=dev).to(torch.bfloat16)
                qT = torch.randn(B * T, (H + 2 * KVH) * 128, device=dev).to(torch.bfloat16)
                o1 = torch.empty(B, H * 128, dtype=torch.bfloat16, device=dev)
                oT = torch.empty(B * T, H * 128, dtype=torch.bfloat16, device=dev)
                dws = sops.DecodeWorkspace(B, H, KVH, W, dev)
                vws = sops.VerifyWorkspace(B * T, T, H, KVH, W, dev)
                q_lens = torch.full((B,), T, **i32)
                offs, starts = torch.arange(B, **i32) * T, ctx_t - T
                fns = {
                    "paged_decode": lambda: sops.paged_decode(q1, k, v, tables, ctx_t, H, KVH, out=o1, ws=dws),
                    "paged_verify": lambda: sops.paged_verify(qT, k, v, tables, ctx_t, q_lens, T, H, KVH, out=oT, ws=vws),
                    "paged_prefill": lambda: sops.paged_prefill(qT, k, v, tables, offs, starts, q_lens, H, KVH, out=oT,
                                                                max_len=T),
                }
                kv_bytes = B * ctx * KVH * 128 * 2 * k.element_size()
                us = {n: [] for n in fns}
                for _ in range(2):
                    for n, fn in fns.items():
                        us[n].append(round(_time(fn, args.iters) * 1e6, 1))
                best = {n: min(t) for n, t in us.items()}
                print(json.dumps({"H": H, "KVH": KVH, "cache": str(dtype).replace("torch.", ""), "B": B, "ctx": ctx, "T": T,
                                  "decode_plan": [dws.nsplit, dws.pps], "verify_plan": [vws.nsplit, vws.pps], "us": us,
                                  "TBps": {n: round(kv_bytes / (t * 1e-6) / 1e12, 2) for n, t in best.items()},
                                  "verify_over_decode": round(best["paged_verify"] / best["paged_decode"], 2),
                                  "prefill_over_verify": round(best["paged_prefill"] / best["paged_verify"], 2)}),
                      flush=True)


def step(args):
    import torch

    from dstack_amd.ops import serving as sops
    from dstack_amd.serving.engine import LLMEngine

    K, ctx = args.K, args.ctx
    eng = LLMEngine.from_model(args.model, max_model_len=2048, max_batch=32, quantization=args.quantization,
                               kv_cache_dtype=args.kv_cache_dtype, speculative_ngram=K, speculative_max_batch=32)
    eng.capture_graphs()
    T, npg = K + 1, (ctx + K) // sops.PAGE + 1
    i32 = dict(dtype=torch.int32, device=eng.device)
    rows = []
    for n in (1, 4, 8, 16, 32):
        b = next(x for x in eng.buckets if x >= n)
        R = eng._verify_rows(n)
        pages = torch.arange(n * npg, **i32).view(n, npg)
        eng.s_tables.zero_()
        eng.s_tables[:n, :npg] = pages

        def slot(pos):  # of position `pos` of every sequence
            return pages[:, pos // sops.PAGE] * sops.PAGE + pos % sops.PAGE

        def stage_decode():
            eng.s_slots.fill_(-1)
            eng.s_ctx.zero_()
            eng.s_pos[:n] = ctx - 1
            eng.s_slots[:n] = slot(ctx - 1)
            eng.s_ctx[:n] = ctx

        def stage_verify():
            eng.s_slots.fill_(-1)
            eng.s_ctx.zero_()
            eng.s_qlens.zero_()
            for j in range(T):
                eng.s_pos[j : n * T : T] = ctx - 1 + j
                eng.s_slots[j : n * T : T] = slot(ctx - 1 + j)
            eng.s_ctx[:n] = ctx + K
            eng.s_qlens[:n] = T

        ms = {"decode": [], "verify": []}
        for _ in range(2):
            stage_decode()
            ms["decode"].append(round(_time(eng._graphs[b].replay, args.iters) * 1e3, 3))
            stage_verify()
            ms["verify"].append(round(_time(eng._graphs["verify", R].replay, args.iters) * 1e3, 3))
        ratio = min(ms["verify"]) / min(ms["decode"])
        rows.append({"model": args.model, "quantization": args.quantization, "kv_cache_dtype": args.kv_cache_dtype,
                     "K": K, "ctx": ctx, "seqs": n, "decode_rows": b, "verify_rows": R, "ms": ms,
                     "ratio": round(ratio, 3), "break_even_accepted_per_step": round(ratio - 1, 3)})
        print(json.dumps(rows[-1]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    k = sub.add_parser("kernel")
    k.add_argument("-T", type=int, default=5)
    k.add_argument("--iters", type=int, default=50)
    s = sub.add_parser("step")
    s.add_argument("--model", default="llama-3-8b")
    s.add_argument("--quantization", default=None)
    s.add_argument("--kv-cache-dtype", default="auto")
    s.add_argument("-K", type=int, default=4)
    s.add_argument("--ctx", type=int, default=1024)
    s.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_speculative needs a ROCm GPU")
    {"kernel": kernel, "step": step}[args.cmd](args)


if __name__ == "__main__":
    main()
