"""The in-tree 256x256-tile GEMM in its e4m3 form (csrc/gemm_nt.hip, F8: scaled 16x16x128 MFMA over
the bf16 kernel's LDS-DMA ring) against hipBLASLt's fp8 GEMM with scalar unit scales
(torch._scaled_mm) -- both give the raw product that the serving engine's deferred-scale consumers
take -- on the Llama-3-70B projections at a decode batch (M = 256) and a prefill batch (M = 16384).

    python tools/bench_fp8_nt.py            # ROWS=256,16384
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dstack_amd.ops import _ext  # noqa: E402

SHAPES = {"qkv": (10240, 8192), "o": (8192, 8192), "gate_up": (57344, 8192), "down": (8192, 28672)}


def timed(fn, iters=20):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def main():
    C = _ext.require()
    rows = [int(m) for m in os.getenv("ROWS", "256,16384").split(",")]
    only = os.getenv("ONLY")
    one = torch.ones((), device="cuda", dtype=torch.float32)
    res = {}
    for M in rows:
        for name, (N, K) in SHAPES.items():
            if only and name not in only.split(","):
                continue
            torch.manual_seed(0)
            xq = (torch.randn(M, K, device="cuda") * 2).to(torch.float8_e4m3fn)
            wq = (torch.randn(N, K, device="cuda") * 2).to(torch.float8_e4m3fn)
            out = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
            ours = lambda: C.gemm_nt_f8(xq.view(torch.uint8), wq.view(torch.uint8), out)  # noqa: E731
            lib = lambda: torch._scaled_mm(xq, wq.t(), scale_a=one, scale_b=one, out_dtype=torch.bfloat16)  # noqa: E731
            ours()
            y1 = lib()
            err = ((out.float() - y1.float()).norm() / y1.float().norm()).item()
            to, tl = [], []
            for _ in range(5):
                to.append(timed(ours))
                tl.append(timed(lib))
            fl = 2.0 * M * N * K
            r = {"M": M, "N": N, "K": K, "ours_us": statistics.median(to) * 1e3, "lib_us": statistics.median(tl) * 1e3,
                 "rel_diff": err}
            r["ours_pf"] = fl / r["ours_us"] / 1e9
            r["lib_pf"] = fl / r["lib_us"] / 1e9
            r["ours_tb_s"] = N * K / r["ours_us"] / 1e6
            r["speedup"] = r["lib_us"] / r["ours_us"]
            res[f"{name}_m{M}"] = r
            print(f"{name}_m{M}", json.dumps({k: round(v, 4) if isinstance(v, float) else v for k, v in r.items()}),
                  flush=True)
            del xq, wq, out, y1
            torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
