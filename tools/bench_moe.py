"""The MoE MLP of a decode step (csrc/moe.hip: route, grouped gate/up GEMM, SwiGLU, grouped down GEMM,
combine) at Mixtral-8x7B's shapes (hidden 4096, FFN 14336, 8 experts, top-2) against the eager path
(``ops.serving.moe_mlp_eager``: one library GEMM pair per non-empty expert and a host read of the
counts -- the plain implementation, which cannot be captured), on the same inputs and hence the same
routing.  Also ``moe_gemm`` alone on the gate/up weights: its achieved HBM rate over the bytes of the
experts that the rows chose (N K 2 bytes each; the activations and partials are not counted).

Every call takes the next of several inputs, so consecutive calls choose other experts; one call's
chosen experts (at least 0.7 GB) exceed the 256 MB last-level cache.  The two paths alternate, REPS
times after a warm-up; the spread is the min..max of a path's repetitions.

    python tools/bench_moe.py [--out FILE]         # ROWS=1,16,64,256 REPS=5 ITERS=20
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dstack_amd.ops import serving as sops  # noqa: E402

E, TOPK, D, F = 8, 2, 4096, 14336


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(iters):
        fn(i)
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters * 1e3  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    rows = [int(r) for r in os.getenv("ROWS", "1,16,64,256").split(",")]
    reps, iters = int(os.getenv("REPS", "5")), int(os.getenv("ITERS", "20"))
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)

    def draw(*shape, sd):
        return torch.empty(*shape, dtype=torch.bfloat16, device=dev).normal_(0.0, sd, generator=g)

    router, wgu, wdown = draw(E, D, sd=0.02), draw(E, 2 * F, D, sd=0.02), draw(E, D, F, sd=0.02)
    ws = sops.MoeWorkspace(E, TOPK, D, F, dev)
    lines = [f"# {torch.cuda.get_device_name(0)}; Mixtral-8x7B MoE MLP (hidden {D}, FFN {F}, {E} experts, top-{TOPK}); us per "
             f"call, median of {reps} x {iters} calls (min..max)",
             "# rows form split(gu,down) experts/call | gate/up moe_gemm us (spread)   GB/s | kernels MLP us (spread) | "
             "eager MLP us (spread) | eager/kernels"]
    for R in rows:
        hs = [draw(R, D, sd=1.0) for _ in range(8)]
        live = torch.ones(R, dtype=torch.int32, device=dev)
        routed = [tuple(t.clone() for t in sops.moe_route(h, router, live, TOPK)) for h in hs]
        chosen = statistics.mean(int((c > 0).sum()) for _, _, c, _ in routed)
        s1, s2 = ws.split[R]
        part = ws.part[: s1 * R * TOPK * 2 * F].view(s1, R * TOPK, 2 * F)
        paths = {
            "gemm": lambda i: sops.moe_gemm(hs[i % 8], TOPK, wgu, routed[i % 8][2], routed[i % 8][3], s1, part=part),
            "kernels": lambda i: sops.moe_mlp(hs[i % 8], router, wgu, wdown, TOPK, live, ws),
            "eager": lambda i: sops.moe_mlp_eager(hs[i % 8], router, wgu, wdown, TOPK, live),
        }
        for fn in paths.values():  # warm-up: code objects, library algorithm choice
            timed(fn, 8)
        t = {name: [] for name in paths}
        for _ in range(reps):
            for name, fn in paths.items():
                t[name].append(timed(fn, iters))
        med = {name: statistics.median(v) for name, v in t.items()}
        sp = {name: f"({min(v):.0f}..{max(v):.0f})" for name, v in t.items()}
        gbs = chosen * 2 * F * D * 2 / med["gemm"] / 1e3
        lines.append(f"{R:6d} {sops._ext.require().moe_gemm_form(R):4d} {s1:5d},{s2:<5d} {chosen:12.1f} | "
                     f"{med['gemm']:12.1f} {sp['gemm']:>14} {gbs:7.0f} | {med['kernels']:10.1f} {sp['kernels']:>14} | "
                     f"{med['eager']:10.1f} {sp['eager']:>14} | {med['eager'] / med['kernels']:.2f}x")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
