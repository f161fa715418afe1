"""The W4A16 decode GEMM (csrc/w4.hip, ``--quantization awq``) against the bf16 GEMM it replaces (what
the unquantized model runs for the same projection and rows, ``ServingLlama._mm``: the HIP GEMV at one
row, hipBLASLt above) and against ``mxfp4_gemm`` (csrc/mxfp4.hip, kernel alone, e4m3 activations
quantized beforehand), on the Llama-3-8B and -70B projections at decode batches.  ``w4_gemm`` takes the
bf16 activations as they are, so the kernel is the model's whole call.  Weight GB/s counts what the
kernel streams: codes + scales + zero bytes (W4), codes + scales (MXFP4), 2 bytes per weight (bf16).

Every call takes the next of several copies of the weight (more than the 256 MB of last-level
cache in total), so no call finds its weights cached.  The three paths alternate, REPS times after a
warm-up; the spread is the min..max of a path's repetitions.

    python tools/bench_w4.py            # ROWS=1,16,64,256 REPS=5 ITERS=20 G=128
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dstack_amd.ops import _ext  # noqa: E402
from dstack_amd.ops import serving as sops  # noqa: E402
from dstack_amd.serving.model import ServingLlama, load_spec  # noqa: E402

SHAPES = {"8b_qkv": (6144, 4096), "8b_o": (4096, 4096), "8b_gate_up": (28672, 4096), "8b_down": (4096, 14336),
          "70b_qkv": (10240, 8192), "70b_o": (8192, 8192), "70b_gate_up": (57344, 8192), "70b_down": (8192, 28672)}
FOOTPRINT = 768 << 20  # bytes of weight copies cycled through per path


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters * 1e3  # us


class Cycle:
    def __init__(self, items):
        self.items, self.i = items, 0

    def next(self):
        self.i = (self.i + 1) % len(self.items)
        return self.items[self.i]


def main():
    C = _ext.require()
    rows = [int(r) for r in os.getenv("ROWS", "1,16,64,256").split(",")]
    reps, iters, g = int(os.getenv("REPS", "5")), int(os.getenv("ITERS", "20")), int(os.getenv("G", "128"))
    names = os.getenv("SHAPES", ",".join(SHAPES)).split(",")
    bf = ServingLlama(load_spec("llama-3-70b"), "cuda")  # (no weights allocated: only its _mm dispatch is used)
    print(f"# {torch.cuda.get_device_name(0)}; us per call, median of {reps} x {iters} calls (min..max); group size {g}; "
          f"bf16: the unquantized model's call; w4, mxfp4: the kernels alone (mxfp4 without its activation quantization)")
    print("# shape            N      K    M  form split |  bf16 us (spread)        GB/s |    w4 us (spread)        GB/s | "
          "bf16/w4 | mxfp4 us   GB/s | mxfp4/w4")
    gen = torch.Generator(device="cuda").manual_seed(0)
    for name in names:
        N, K = SHAPES[name]
        bytes_bf, bytes_w4, bytes_mx = N * K * 2, N * K // 2 + N * K // g * 3, N * K // 2 + N * K // 32
        wbf = [torch.randn(N, K, device="cuda", dtype=torch.bfloat16, generator=gen) * 0.02
               for _ in range(max(2, FOOTPRINT // bytes_bf))]
        w4, wmx = [], []
        for _ in range(max(2, FOOTPRINT // bytes_w4)):
            c = torch.randint(0, 256, (N, K // 2), dtype=torch.uint8, device="cuda", generator=gen)
            z = torch.randint(0, 16, (N, K // g), dtype=torch.uint8, device="cuda", generator=gen)
            s = (torch.rand(N, K // g, device="cuda", generator=gen) * 0.01 + 0.001).half()
            w4.append(sops.w4_shuffle(c, z, s, g))
            sc = torch.randint(118, 124, (N, K // 32), dtype=torch.uint8, device="cuda", generator=gen)
            wmx.append(sops.mxfp4_shuffle(c, sc))
            del c, z, s, sc
        cbf, c4, cmx = Cycle(wbf), Cycle(w4), Cycle(wmx)
        for M in rows:
            x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16, generator=gen)
            xq, xs = C.quant_fp8_rows(x)
            xq = xq.view(torch.uint8)
            runs = (lambda: bf._mm(x, cbf.next()), lambda: C.w4_gemm(x, *c4.next(), N, K, g),
                    lambda: C.mxfp4_gemm(xq, xs, *cmx.next(), N, K))
            for fn in runs:
                timed(fn, max(3, len(wbf), len(w4)))  # warm-up: every copy once
            ts = ([], [], [])
            for _ in range(reps):
                for t, fn in zip(ts, runs):
                    t.append(timed(fn, iters))
            mbf, m4, mmx = (statistics.median(t) for t in ts)
            print(f"{name:12s} {N:6d} {K:6d} {M:4d}  {C.w4_gemm_form(M):4d} {C.w4_gemm_split(M, N, K):5d} | "
                  f"{mbf:8.1f} ({min(ts[0]):7.1f}..{max(ts[0]):7.1f}) {bytes_bf / mbf / 1e3:6.0f} | "
                  f"{m4:8.1f} ({min(ts[1]):7.1f}..{max(ts[1]):7.1f}) {bytes_w4 / m4 / 1e3:6.0f} | {mbf / m4:7.2f} | "
                  f"{mmx:8.1f} {bytes_mx / mmx / 1e3:6.0f} | {mmx / m4:8.2f}", flush=True)
        del wbf, w4, wmx
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
