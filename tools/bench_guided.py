#!/usr/bin/env python3
"""Structured-output mask microbenchmark: what ``apply_guide`` costs per decode step, R rows of V bf16
logits, next to ``apply_penalties`` on the same shapes as the yardstick.

    python tools/bench_guided.py [--rows 1 16 256] [--vocab 128256] [--iters 20] [--tokenizer DIR]

Grammars: ``json_object`` (the largest one in everyday use) and a small flat schema.  States: the
start state (one byte is legal, so nearly every token dies on its first byte: the walk is one read of
the hot row ``trans[g][s]``) and a state in the middle of a string (nearly every byte is legal, so
every token walks all of its bytes through the table: the gather-bound case).  All rows guided, in the
same state (``same``) or spread over the states a document passes through (``spread``).

The token table is the tokenizer's of ``--tokenizer`` (a checkpoint directory) or, without one, a
synthetic ByteLevel-like table of ``--vocab`` tokens: the 256 bytes, then words of letters, digits and
JSON punctuation with the length distribution of a 128k BPE vocabulary (mean about 6.5 bytes, a few of
up to 40).  Prints one JSON line per row count.
"""

from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCHEMA = {"type": "object", "required": ["name", "age", "tags"], "properties": {
    "name": {"type": "string", "maxLength": 32}, "age": {"type": "integer"}, "email": {"type": "string"},
    "tags": {"type": "array", "items": {"type": "string"}, "maxItems": 8}, "active": {"type": "boolean"}}}


def synthetic_tokens(vocab: int, seed: int = 0) -> list:
    rng = random.Random(seed)
    letters = "etaoinshrdlucmfwypvbgkqjxz"
    out = [bytes([b]) for b in range(256)]
    seen = set(out)
    while len(out) < vocab - 256:  # the last 256 ids: special tokens, no bytes
        n = min(40, max(1, int(rng.lognormvariate(1.7, 0.55))))
        kind = rng.random()
        if kind < 0.70:
            w = "".join(rng.choice(letters) for _ in range(n))
            w = (" " + w[:-1] if rng.random() < 0.5 and n > 1 else w)
            w = w.capitalize() if rng.random() < 0.15 else w
        elif kind < 0.80:
            w = "".join(rng.choice("0123456789") for _ in range(min(n, 3)))
        elif kind < 0.92:
            w = "".join(rng.choice(' {}[]":,.-_()/\\\n\t=;') for _ in range(min(n, 6)))
        else:
            w = "".join(rng.choice("éüñ日本語中文кирил") for _ in range(max(1, n // 3)))
        b = w.encode()
        if b not in seen:
            seen.add(b)
            out.append(b)
    return out + [b""] * 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--tokenizer", default=None, help="checkpoint directory with a tokenizer.json")
    args = ap.parse_args()

    import numpy as np
    import torch

    from dstack_amd.ops import serving as sops
    from dstack_amd.serving import guided

    dev = torch.device("cuda", 0)
    V = args.vocab
    if args.tokenizer:
        from dstack_amd.serving.tokenizer import HFTokenizer

        tokens = HFTokenizer(args.tokenizer).token_bytes()
    else:
        tokens = synthetic_tokens(V)
    off, blob = guided.pack_token_bytes(tokens, V)
    off, blob = torch.from_numpy(off).to(dev), torch.from_numpy(blob).to(dev)
    grammars = {"json_object": guided.compile_json_object(), "schema": guided.compile_json_schema(SCHEMA)}
    trans = torch.zeros(len(grammars), sops.GUIDE_MAX_STATES, 256, dtype=torch.int16, device=dev)
    accept = torch.zeros(len(grammars), sops.GUIDE_MAX_STATES, dtype=torch.uint8, device=dev)
    docs = {"json_object": b'{"name": "Ada Lovelace", "tags": ["x", {"k": 1.5e3}], "note": "a \\n b"}',
            "schema": b'{"name": "Ada Lovelace", "age": 36, "tags": ["math", "engines"], "active": true}'}
    states = {}
    for i, (name, g) in enumerate(grammars.items()):
        trans[i, : g.states] = torch.from_numpy(g.trans.view(np.int16)).to(dev)
        accept[i, : g.states] = torch.from_numpy(g.accept).to(dev)
        assert g.matches(docs[name]), name
        path = [guided.walk(g, 1, docs[name][:k]) for k in range(len(docs[name]))]
        states[name] = dict(start=1, mid_string=guided.walk(g, 1, b'{"name": "Ad'), path=path)
    eos = torch.tensor([V - 256, V - 255], dtype=torch.int32, device=dev)
    n_eos = torch.tensor([2], dtype=torch.int32, device=dev)

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

    for R in args.rows:
        torch.manual_seed(R)
        src = (torch.randn(R, V, device=dev) * 3).to(torch.bfloat16)
        x = src.clone()
        res = {"rows": R, "vocab": V, "token_bytes_mean": round(float(blob.numel()) / V, 2),
               "token_table": args.tokenizer or "synthetic", "device": torch.cuda.get_device_name(0)}
        for gi, name in enumerate(grammars):
            res[f"{name}_states"] = grammars[name].states
            guide = torch.full((R,), gi, dtype=torch.int32, device=dev)
            for label in ("start", "mid_string", "spread"):
                if label == "spread":
                    path = states[name]["path"]
                    st = torch.tensor([path[(r * 7) % len(path)] for r in range(R)], dtype=torch.int32, device=dev)
                else:
                    st = torch.full((R,), states[name][label], dtype=torch.int32, device=dev)

                def run():
                    # (masks in place: a masked logit stays masked, the walk does not look at the logits)
                    sops.apply_guide(x, guide, st, trans, accept, off, blob, eos, n_eos)

                x.copy_(src)
                res[f"{name}_{label}_ms"] = round(gpu_ms(run, args.iters), 4)
                if label != "spread":
                    res[f"{name}_{label}_kept"] = int((~torch.isneginf(x[0].float())).sum())
        idle = torch.full((R,), -1, dtype=torch.int32, device=dev)
        zero = torch.zeros(R, dtype=torch.int32, device=dev)
        res["idle_ms"] = round(gpu_ms(lambda: sops.apply_guide(x, idle, zero, trans, accept, off, blob, eos, n_eos),
                                      args.iters), 4)
        # the yardstick: apply_penalties with every row penalised, same shapes
        state, bias_ids, bias_vals, bias_n = sops.alloc_penalty_state(R, V, dev)
        state.copy_(torch.randint(0, 4, (R, V), device=dev, dtype=torch.int32))
        slot = torch.arange(R, device=dev, dtype=torch.int32)
        rep = torch.full((R,), 1.1, device=dev)
        freq, pres = torch.full((R,), 0.5, device=dev), torch.full((R,), 0.25, device=dev)
        inv = sops.inv_rep_of(rep)
        pen = src.clone()
        res["apply_penalties_ms"] = round(gpu_ms(lambda: sops.apply_penalties(pen, state, slot, rep, inv, freq, pres, bias_ids,
                                                                              bias_vals, bias_n), args.iters), 4)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
