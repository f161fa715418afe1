"""The block-scaled FP4 decode GEMM (csrc/mxfp4.hip, ``--quantization mxfp4``) against what the fp8
model runs for the same projection and rows (``ServingLlama._mm_fp8``: the fp8 GEMV up to 4 rows, the
in-tree rows / weight-streaming GEMMs or hipBLASLt above), on the Llama-3-70B projections at decode
batches.  Both sides are timed as the model calls them, activation quantization included; the
MXFP4 kernel is also timed alone (its achieved weight GB/s counts codes + scales).

Every call takes the next of several copies of the weight (more than the 256 MB of last-level
cache in total), so no call finds its weights cached.  The two paths alternate, REPS times after a
warm-up; the spread is the min..max of a path's repetitions.

    python tools/bench_mxfp4.py            # ROWS=1,16,64,128,256 REPS=5 ITERS=20
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dstack_amd.ops import _ext  # noqa: E402
from dstack_amd.ops import serving as sops  # noqa: E402
from dstack_amd.serving.model import Fp8Weight, Mxfp4Weight, ServingLlama, load_spec  # noqa: E402

SHAPES = {"qkv": ("wqkv", 10240, 8192), "o": ("wo", 8192, 8192), "gate_up": ("wgu", 57344, 8192),
          "down": ("wdown", 8192, 28672)}
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
    rows = [int(r) for r in os.getenv("ROWS", "1,16,64,128,256").split(",")]
    reps, iters = int(os.getenv("REPS", "5")), int(os.getenv("ITERS", "20"))
    names = os.getenv("SHAPES", ",".join(SHAPES)).split(",")
    spec = load_spec("llama-3-70b")
    f8 = ServingLlama(spec, "cuda", quantization="fp8")
    mx = ServingLlama(spec, "cuda", quantization="mxfp4")
    print(f"# {torch.cuda.get_device_name(0)}; us per call, median of {reps} x {iters} calls (min..max); "
          f"fp8 / mxfp4: the model's call, activation quantization included; kernel: mxfp4_gemm alone")
    print("# shape        N      K    M  form split |   fp8 us (spread)        | mxfp4 us (spread)        | "
          "fp8/mxfp4 | kernel us  weight GB/s")
    g = torch.Generator(device="cuda").manual_seed(0)
    for name in names:
        key, N, K = SHAPES[name]
        nf8 = max(2, FOOTPRINT // (N * K))
        nmx = max(2, FOOTPRINT // (N * K // 2))
        w8 = []
        for _ in range(nf8):
            q = torch.randint(0, 120, (N, K), dtype=torch.uint8, device="cuda", generator=g)  # finite e4m3 bytes
            w8.append(Fp8Weight(q, torch.full((N,), 1e-3, device="cuda"), f8._stream_copy(key, q)))
        w4 = []
        for _ in range(nmx):
            c = torch.randint(0, 256, (N, K // 2), dtype=torch.uint8, device="cuda", generator=g)
            s = torch.randint(118, 124, (N, K // 32), dtype=torch.uint8, device="cuda", generator=g)
            w4.append(Mxfp4Weight(*sops.mxfp4_shuffle(c, s), N, K))
        mx._mx_scratch = torch.empty(N * K, dtype=torch.bfloat16, device="cuda")
        c8, c4 = Cycle(w8), Cycle(w4)
        wbytes = N * K // 2 + N * K // 32
        for M in rows:
            x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16, generator=g)
            xq, xs = C.quant_fp8_rows(x)
            xq = xq.view(torch.uint8)
            run8 = lambda: f8._mm(x, c8.next())  # noqa: E731
            run4 = lambda: mx._mm(x, c4.next())  # noqa: E731

            def kern():
                w = c4.next()
                return C.mxfp4_gemm(xq, xs, w.codes, w.scales, N, K)

            for fn in (run8, run4, kern):
                timed(fn, max(3, len(w8), len(w4)))  # warm-up: every copy once
            t8, t4, tk = [], [], []
            for _ in range(reps):
                t8.append(timed(run8, iters))
                t4.append(timed(run4, iters))
                tk.append(timed(kern, iters))
            m8, m4, mk = (statistics.median(t) for t in (t8, t4, tk))
            print(f"{name:8s} {N:6d} {K:6d} {M:4d}  {C.mxfp4_gemm_form(M):4d} {C.mxfp4_gemm_split(M, N, K):5d} | "
                  f"{m8:8.1f} ({min(t8):7.1f}..{max(t8):7.1f}) | {m4:8.1f} ({min(t4):7.1f}..{max(t4):7.1f}) | "
                  f"{m8 / m4:9.2f} | {mk:9.1f} {wbytes / mk / 1e3:11.0f}", flush=True)
        del w8, w4
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
