"""``python -m dstack_amd.serving --model llama-3-70b --port 8000``: one OpenAI-compatible model
replica on one GPU (the process a ``type: service`` run starts; see
``examples/llama3-70b-service/service.dstack.yml``)."""

from __future__ import annotations

import argparse
import logging
import os
import time


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m dstack_amd.serving")
    ap.add_argument("--model", default=os.environ.get("MODEL", "llama-3-8b"),
                    help="built-in config (random weights) or an HF Llama checkpoint directory")
    ap.add_argument("--served-model-name", default=None)
    ap.add_argument("--host", default="0.0.0.0")
    ap.add_argument("--port", type=int, default=int(os.environ.get("PORT", "8000")))
    ap.add_argument("--max-model-len", type=int, default=None)
    ap.add_argument("--max-batch", type=int, default=256)
    ap.add_argument("--max-prefill-tokens", type=int, default=16384)
    ap.add_argument("--gpu-memory-utilization", type=float, default=0.90)
    ap.add_argument("--no-graphs", action="store_true", help="run decode steps eagerly (no hipGraph capture)")
    ap.add_argument("--seed", type=int, default=0, help="random-init seed for built-in configs")
    ap.add_argument("--quantization", choices=["fp8", "mxfp4", "awq"], default=None,
                    help="fp8: e4m3 projection weights with per-channel scales, per-token activation scales; "
                         "mxfp4: OCP MXFP4 projection weights (e2m1, one E8M0 scale per 32), e4m3 activations "
                         "on the block-scaled FP4 decode GEMM; awq: an AutoAWQ 4-bit checkpoint (qweight / qzeros / "
                         "scales, GEMM packing) on the W4A16 decode GEMM with bf16 activations -- selected by "
                         "itself when the checkpoint's config.json says so")
    ap.add_argument("--kv-cache-dtype", choices=["auto", "fp8"], default="auto",
                    help="fp8: e4m3 paged KV cache (half the bytes per decode step, twice the tokens)")
    ap.add_argument("--enable-prefix-caching", action="store_true",
                    help="reuse the cached KV pages of a prompt's prefix (64-token pages, LRU eviction); "
                         "not with tensor parallel")
    ap.add_argument("--lora-modules", nargs="+", default=[], metavar="NAME=PATH",
                    help="LoRA adapters (PEFT directories) to serve next to the base model; a request picks one "
                         "by its `model`; not with --quantization fp8 / mxfp4 / awq or tensor parallel")
    ap.add_argument("--max-lora-rank", type=int, default=64,
                    help="largest adapter rank accepted (the adapter stacks are padded to 8, 16, 32 or 64)")
    ap.add_argument("--speculative-ngram", type=int, default=0, metavar="K",
                    help="n-gram speculative decoding: verify up to K (1..7) draft tokens per sequence and step, "
                         "copied from the latest earlier occurrence of the sequence's last tokens; outputs are the "
                         "plain engine's; not with --lora-modules or tensor parallel")
    ap.add_argument("--ngram-max", type=int, default=3, help="longest suffix the proposal matches")
    ap.add_argument("--ngram-min", type=int, default=1, help="shortest suffix the proposal matches")
    ap.add_argument("--speculative-max-batch", type=int, default=32,
                    help="decode steps with more running sequences than this run without drafts")
    ap.add_argument("--max-guides", type=int, default=16, metavar="N",
                    help="structured outputs (response_format, guided_json / _regex / _choice): grammars resident "
                         "on the device at once (2 MiB each); 0 allocates nothing and refuses such requests")
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s")
    log = logging.getLogger("dstack_amd.serving")

    import torch
    import uvicorn

    from dstack_amd.serving.engine import LLMEngine
    from dstack_amd.serving.lora import parse_lora_modules
    from dstack_amd.serving.server import create_app

    try:
        lora_modules = parse_lora_modules(args.lora_modules)
    except ValueError as e:
        ap.error(str(e))

    if torch.cuda.is_available():
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    t0 = time.time()
    eng = LLMEngine.from_model(args.model, max_model_len=args.max_model_len, seed=args.seed, max_batch=args.max_batch,
                               max_prefill_tokens=args.max_prefill_tokens, use_graphs=not args.no_graphs and None,
                               gpu_memory_utilization=args.gpu_memory_utilization, quantization=args.quantization,
                               kv_cache_dtype=args.kv_cache_dtype, enable_prefix_caching=args.enable_prefix_caching,
                               lora_modules=lora_modules or None, max_lora_rank=args.max_lora_rank,
                               speculative_ngram=args.speculative_ngram, ngram_max=args.ngram_max,
                               ngram_min=args.ngram_min, speculative_max_batch=args.speculative_max_batch,
                               max_guides=args.max_guides)
    eng.capture_graphs()
    m = eng.model
    log.info("model %s: %.1f GB weights, %d KV pages (%d tokens), max_model_len %d, %d decode graphs, ready in %.1fs",
             args.model, m.weight_bytes() / 1e9, m.num_pages, m.num_pages * 64, m.max_model_len, len(eng._graphs),
             time.time() - t0)
    if lora_modules:
        log.info("LoRA adapters: %s (rank padded to %d)", ", ".join(lora_modules), m.lora_rank)
    if eng.guide_error and args.max_guides:
        log.warning("%s", eng.guide_error)
    name = args.served_model_name or os.path.basename(os.path.normpath(args.model))
    uvicorn.run(create_app(eng, name), host=args.host, port=args.port, log_level="info")


if __name__ == "__main__":
    main()
