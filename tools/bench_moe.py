"""The MoE MLP of a decode step (csrc/moe.hip: route, grouped gate/up GEMM, SwiGLU, grouped down GEMM,
combine) at Mixtral-8x7B's shapes (hidden 4096, FFN 14336, 8 experts, top-2) against the eager path
(``ops.serving.moe_mlp_eager``: one library GEMM pair per non-empty expert and a host read of the
counts -- the plain implementation, which cannot be captured), on the same inputs and hence the same
routing.  Also ``moe_gemm`` alone on the gate/up weights: its achieved HBM rate over the bytes of the
experts that the rows chose (N K 2 bytes each; the activations and partials are not counted).

Every call takes the next of several inputs, so consecutive calls choose other experts; one call's
chosen experts (at least 0.7 GB) exceed the 256 MB last-level cache.  The two paths alternate, REPS
times after a warm-up; the spread is the min..max of a path's repetitions.

``--w4``: the same shapes and rows with the experts as W4 (``quant_w4`` at g = 128, csrc/moe_w4.hip):
``moe_w4_gemm`` beside the bf16 ``moe_gemm`` on the same routing, for the gate/up and the down GEMM, and
the whole MLP of both, alternating under the same protocol.

``--fine 30b`` / ``--fine 235b``: ``moe_fine_gemm`` (csrc/moe_fine.hip) at Qwen3-30B-A3B's shapes (hidden 2048,
FFN 768, 128 experts, top-8) or at Qwen3-235B-A22B's (hidden 4096, FFN 1536) with 64 experts, top-8, which
``moe_gemm`` can run too: there it runs beside ``moe_fine_gemm`` on the same routing.  Gate/up and down GEMM,
the weight GB/s of the chosen experts, the whole MLP on the kernels against ``moe_mlp_eager``.

``--prefill``: the MLP of a prefill of 384 .. 4096 rows at Qwen3-30B-A3B's shapes on ``moe_prefill_mlp``
(csrc/moe_prefill.hip, the tiled grouped GEMM) against ``moe_fine_mlp`` over 256-row slices, µs and TFLOP/s.

    python tools/bench_moe.py [--w4 | --fine 30b|235b | --prefill] [--out FILE]  # ROWS=1,16,64,256 REPS=5 ITERS=20
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


def measure(paths, reps, iters):
    """Every path warmed up (code objects, library algorithm choice), then the paths alternating, ``reps`` times:
    name -> the us per call of each repetition, name -> their median."""
    for fn in paths.values():
        timed(fn, 8)
    t = {name: [] for name in paths}
    for _ in range(reps):
        for name, fn in paths.items():
            t[name].append(timed(fn, iters))
    return t, {name: statistics.median(v) for name, v in t.items()}


def w4_table(dev, draw, router, wgu, wdown, ws, rows, reps, iters, g=128):
    from dstack_amd.ops import reference as ref

    def quant(w):  # stacked stored form, expert by expert
        return tuple(torch.stack(t) for t in zip(*(sops.w4_shuffle(*ref.quant_w4(w[e], g), g) for e in range(E))))

    qgu, qdown = quant(wgu), quant(wdown)
    ws4 = sops.MoeWorkspace(E, TOPK, D, F, dev, w4_group=g)
    lines = [f"# {torch.cuda.get_device_name(0)}; Mixtral-8x7B MoE MLP (hidden {D}, FFN {F}, {E} experts, top-{TOPK}), W4 "
             f"experts (g = {g}) beside bf16; us per call, median of {reps} x {iters} calls (min..max)",
             "# rows form | split bf16(gu,down) w4(gu,down) | gate/up: bf16 us, w4 us, bf16/w4 | down: bf16 us, w4 us, "
             "bf16/w4 | MLP: bf16 us, w4 us, bf16/w4"]
    for R in rows:
        hs = [draw(R, D, sd=1.0) for _ in range(8)]
        acts = [draw(R * TOPK, F, sd=1.0) for _ in range(8)]
        live = torch.ones(R, dtype=torch.int32, device=dev)
        routed = [tuple(t.clone() for t in sops.moe_route(h, router, live, TOPK)) for h in hs]
        (b1, b2), (s1, s2) = ws.split[R], ws4.split[R]
        P = R * TOPK

        def part(w, s, n):
            return w.part[: s * P * n].view(s, P, n)

        paths = {
            "gu": lambda i: sops.moe_gemm(hs[i % 8], TOPK, wgu, *routed[i % 8][2:], b1, part=part(ws, b1, 2 * F)),
            "gu4": lambda i: sops.moe_w4_gemm(hs[i % 8], TOPK, qgu, g, *routed[i % 8][2:], s1, part=part(ws4, s1, 2 * F)),
            "dn": lambda i: sops.moe_gemm(acts[i % 8], 1, wdown, *routed[i % 8][2:], b2, part=part(ws, b2, D)),
            "dn4": lambda i: sops.moe_w4_gemm(acts[i % 8], 1, qdown, g, *routed[i % 8][2:], s2, part=part(ws4, s2, D)),
            "mlp": lambda i: sops.moe_mlp(hs[i % 8], router, wgu, wdown, TOPK, live, ws),
            "mlp4": lambda i: sops.moe_w4_mlp(hs[i % 8], router, qgu, qdown, g, TOPK, live, ws4),
        }
        t, med = measure(paths, reps, iters)
        cell = {name: f"{med[name]:8.1f} ({min(v):.0f}..{max(v):.0f})" for name, v in t.items()}
        lines.append(f"{R:6d} {sops._ext.require().moe_w4_gemm_form(R):4d} | {b1},{b2} {s1},{s2} | "
                     + " | ".join(f"{cell[a]} {cell[a + '4']} {med[a] / med[a + '4']:.2f}x" for a in ("gu", "dn", "mlp")))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    return text


FINE_SHAPES = {"30b": (128, 8, 2048, 768), "235b": (64, 8, 4096, 1536)}  # experts, top-k, hidden, FFN


def fine_table(dev, draw, shape, rows, reps, iters):
    E, TOPK, D, F = FINE_SHAPES[shape]
    router, wgu, wdown = draw(E, D, sd=0.02), draw(E, 2 * F, D, sd=0.02), draw(E, D, F, sd=0.02)
    ws = sops.MoeWorkspace(E, TOPK, D, F, dev, fine=True)
    old = sops.MoeWorkspace(E, TOPK, D, F, dev) if E <= sops.MOE_MAX_EXPERTS else None  # moe_gemm beside it
    lines = [f"# {torch.cuda.get_device_name(0)}; Qwen3-MoE MLP (hidden {D}, FFN {F}, {E} experts, top-{TOPK}); us per "
             f"call, median of {reps} x {iters} calls (min..max)",
             "# rows split(gu,down) experts/call | gate/up: fine us, GB/s" + (", moe_gemm us" if old else "")
             + " | down: fine us, GB/s" + (", moe_gemm us" if old else "") + " | MLP: fine us"
             + (", moe_gemm us" if old else "") + ", eager us, eager/fine"]
    for R in rows:
        hs = [draw(R, D, sd=1.0) for _ in range(8)]
        acts = [draw(R * TOPK, F, sd=1.0) for _ in range(8)]
        live = torch.ones(R, dtype=torch.int32, device=dev)
        routed = [tuple(t.clone() for t in sops.moe_route(h, router, live, TOPK)) for h in hs]
        chosen = statistics.mean(int((c > 0).sum()) for _, _, c, _ in routed)
        P = R * TOPK

        def part(w, s, n):
            return w.part[: s * P * n].view(s, P, n)

        s1, s2 = ws.split[R]
        paths = {
            "gu": lambda i: sops.moe_fine_gemm(hs[i % 8], TOPK, wgu, *routed[i % 8][2:], s1, part=part(ws, s1, 2 * F)),
            "dn": lambda i: sops.moe_fine_gemm(acts[i % 8], 1, wdown, *routed[i % 8][2:], s2, part=part(ws, s2, D)),
            "mlp": lambda i: sops.moe_fine_mlp(hs[i % 8], router, wgu, wdown, TOPK, live, ws),
            "eager": lambda i: sops.moe_mlp_eager(hs[i % 8], router, wgu, wdown, TOPK, live),
        }
        if old:
            b1, b2 = old.split[R]
            paths["gu0"] = lambda i: sops.moe_gemm(hs[i % 8], TOPK, wgu, *routed[i % 8][2:], b1, part=part(old, b1, 2 * F))
            paths["dn0"] = lambda i: sops.moe_gemm(acts[i % 8], 1, wdown, *routed[i % 8][2:], b2, part=part(old, b2, D))
            paths["mlp0"] = lambda i: sops.moe_mlp(hs[i % 8], router, wgu, wdown, TOPK, live, old)
        t, med = measure(paths, reps, iters)
        cell = {name: f"{med[name]:7.1f} ({min(v):.0f}..{max(v):.0f})" for name, v in t.items()}
        gbs = {"gu": chosen * 2 * F * D * 2 / med["gu"] / 1e3, "dn": chosen * F * D * 2 / med["dn"] / 1e3}
        lines.append(f"{R:6d} {s1},{s2} {chosen:6.1f} | "
                     + " | ".join(f"{cell[a]} {gbs[a]:5.0f}" + (f" {cell[a + '0']}" if old else "") for a in ("gu", "dn"))
                     + f" | {cell['mlp']}" + (f" {cell['mlp0']}" if old else "")
                     + f" {cell['eager']} {med['eager'] / med['mlp']:.2f}x")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    return text


def prefill_table(dev, draw, rows, reps, iters):
    """The whole MLP of a prefill of R rows on ``moe_prefill_mlp`` (slices of 2048 rows, as the engine runs it)
    against ``moe_fine_mlp`` over 256-row slices, the path it replaces; TFLOP/s over the 6 R k D F flops of the
    routed pairs."""
    E, TOPK, D, F = FINE_SHAPES["30b"]
    router, wgu, wdown = draw(E, D, sd=0.02), draw(E, 2 * F, D, sd=0.02), draw(E, D, F, sd=0.02)
    ws, pws = sops.MoeWorkspace(E, TOPK, D, F, dev, fine=True), sops.MoePrefillWorkspace(E, TOPK, D, F, dev)
    lines = [f"# {torch.cuda.get_device_name(0)}; Qwen3-MoE MLP of a prefill (hidden {D}, FFN {F}, {E} experts, top-{TOPK}); "
             f"us per call, median of {reps} x {iters} calls (min..max)",
             "# rows tile | moe_prefill_mlp us, TFLOP/s | moe_fine_mlp in 256-row slices us, TFLOP/s | slices/prefill"]

    def run(mlp, w, n, h, live):
        return torch.cat([mlp(h[i : i + n], router, wgu, wdown, TOPK, live[i : i + n], w) for i in range(0, h.shape[0], n)])

    for R in rows:
        hs = [draw(R, D, sd=1.0) for _ in range(4)]
        live = torch.ones(R, dtype=torch.int32, device=dev)
        paths = {"prefill": lambda i: run(sops.moe_prefill_mlp, pws, sops.MOE_PREFILL_MAX_ROWS, hs[i % 4], live),
                 "slices": lambda i: run(sops.moe_fine_mlp, ws, sops.MOE_MAX_ROWS, hs[i % 4], live)}
        t, med = measure(paths, reps, iters)
        cell = {name: f"{med[name]:8.1f} ({min(v):.0f}..{max(v):.0f}) {6 * R * TOPK * D * F / med[name] / 1e6:6.1f}"
                for name, v in t.items()}
        lines.append(f"{R:6d} {sops.moe_prefill_tile(min(R, sops.MOE_PREFILL_MAX_ROWS), TOPK, E):4d} | {cell['prefill']} | "
                     f"{cell['slices']} | {med['slices'] / med['prefill']:.2f}x")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    return text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--fine", choices=sorted(FINE_SHAPES), default=None,
                    help="moe_fine_gemm at Qwen3-30B-A3B's shapes, or at Qwen3-235B's with 64 experts beside moe_gemm")
    ap.add_argument("--w4", action="store_true", help="W4 experts (moe_w4_gemm) beside the bf16 kernels")
    ap.add_argument("--prefill", action="store_true",
                    help="moe_prefill_mlp beside moe_fine_mlp in 256-row slices at Qwen3-30B-A3B's shapes (ROWS defaults to "
                         "384,512,1024,2048,4096)")
    args = ap.parse_args()
    rows = [int(r) for r in os.getenv("ROWS", "384,512,1024,2048,4096" if args.prefill else "1,16,64,256").split(",")]
    reps, iters = int(os.getenv("REPS", "5")), int(os.getenv("ITERS", "20"))
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)

    def draw(*shape, sd):
        return torch.empty(*shape, dtype=torch.bfloat16, device=dev).normal_(0.0, sd, generator=g)

    if args.prefill:
        text = prefill_table(dev, draw, rows, reps, iters)
    elif args.fine:
        text = fine_table(dev, draw, args.fine, rows, reps, iters)
    else:
        router, wgu, wdown = draw(E, D, sd=0.02), draw(E, 2 * F, D, sd=0.02), draw(E, D, F, sd=0.02)
        ws = sops.MoeWorkspace(E, TOPK, D, F, dev)
    if args.w4 and not args.fine and not args.prefill:
        text = w4_table(dev, draw, router, wgu, wdown, ws, rows, reps, iters)
    if args.w4 or args.fine or args.prefill:
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(text)
        return
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
        t, med = measure(paths, reps, iters)
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
