"""LoRA adapters for the serving engine: reading a PEFT adapter directory (``adapter_config.json`` +
``adapter_model.safetensors``, as ``examples/fine-tuning/qlora`` and
``dstack_amd/api/huggingface/sft_train.py`` write them) without ``peft`` installed.

An adapter holds, for any subset of the seven Llama projections, ``lora_A`` [r, in] and ``lora_B``
[out, r]; the served projection is ``W x + scale * B (A x)`` with ``scale = lora_alpha / r``
(``lora_alpha / sqrt(r)`` with ``use_rslora``).  ``ServingLlama.load_lora`` stacks them per slot in
the layout of ``ops/csrc/lora.hip``: q/k/v become the three slices of the fused ``wqkv`` and gate/up
the two of ``wgu``, the rank is zero-padded to the stack's, and ``scale`` is multiplied into ``B`` in
fp32 before the one rounding to the model's dtype.  Everything this loader does not implement is
refused with a ValueError that names the field, never ignored.
"""

from __future__ import annotations

import json
import math
import os
import re
from dataclasses import dataclass, field

import torch

# PEFT module name -> (fused weight of the serving model, slice inside it)
TARGETS = {
    "q_proj": ("wqkv", 0), "k_proj": ("wqkv", 1), "v_proj": ("wqkv", 2), "o_proj": ("wo", 0),
    "gate_proj": ("wgu", 0), "up_proj": ("wgu", 1), "down_proj": ("wdown", 0),
}
_KEY = re.compile(r"^base_model\.model\.model\.layers\.(\d+)\.(?:self_attn|mlp)\.(\w+)\.lora_([AB])\.weight$")
_PARENT = {"q_proj": "self_attn", "k_proj": "self_attn", "v_proj": "self_attn", "o_proj": "self_attn",
           "gate_proj": "mlp", "up_proj": "mlp", "down_proj": "mlp"}


@dataclass
class LoraAdapter:
    """One adapter on the host: ``tensors[(layer, target)] = (A [r, in] fp32, B [out, r] fp32)`` with
    ``scale`` still to be applied to ``B``."""

    rank: int
    scale: float
    tensors: dict = field(default_factory=dict)


def padded_rank(rank: int) -> int:
    """The smallest rank the kernels take (8, 16, 32, 64) that holds ``rank``."""
    from dstack_amd.ops.serving import LORA_RANKS

    for r in LORA_RANKS:
        if rank <= r:
            return r
    raise ValueError(f"max_lora_rank {rank} is above the largest supported rank {LORA_RANKS[-1]}")


def read_adapter(path: str, n_layers: int, shapes: dict, max_rank: int) -> LoraAdapter:
    """Read and validate the PEFT adapter in ``path`` for a base model of ``n_layers`` layers whose
    projections have ``shapes[target] = (out, in)`` (the seven keys of ``TARGETS``)."""
    from safetensors import safe_open

    cfg_path = os.path.join(path, "adapter_config.json")
    st_path = os.path.join(path, "adapter_model.safetensors")
    for p in (cfg_path, st_path):
        if not os.path.exists(p):
            raise ValueError(f"LoRA adapter {path}: {os.path.basename(p)} not found")
    with open(cfg_path) as f:
        cfg = json.load(f)

    def bad(fld, why):
        return ValueError(f"LoRA adapter {path}: {fld} {why}")

    if str(cfg.get("peft_type", "LORA")).upper() != "LORA":
        raise bad("peft_type", f"{cfg.get('peft_type')!r} is not supported (LORA only)")
    if cfg.get("use_dora"):
        raise bad("use_dora", "is not supported")
    if cfg.get("bias", "none") != "none":
        raise bad("bias", f"{cfg.get('bias')!r} is not supported (\"none\" only)")
    if cfg.get("fan_in_fan_out"):
        raise bad("fan_in_fan_out", "is not supported")
    for fld in ("modules_to_save", "rank_pattern", "alpha_pattern"):
        if cfg.get(fld):
            raise bad(fld, f"{cfg[fld]!r} is not supported (must be empty)")
    rank = cfg.get("r")
    if isinstance(rank, bool) or not isinstance(rank, int) or rank < 1:
        raise bad("r", f"must be a positive integer, got {rank!r}")
    if rank > max_rank:
        raise bad("r", f"{rank} is above max_lora_rank {max_rank}")
    alpha = cfg.get("lora_alpha", rank)
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)):
        raise bad("lora_alpha", f"must be a number, got {alpha!r}")
    tm = cfg.get("target_modules") or []
    if isinstance(tm, str):
        raise bad("target_modules", f"{tm!r} must be a list of module names, not a pattern")
    outside = sorted(set(m.split(".")[-1] for m in tm) - set(TARGETS))
    if outside:
        raise bad("target_modules", f"{outside} are not supported (only {', '.join(TARGETS)})")
    scale = alpha / math.sqrt(rank) if cfg.get("use_rslora") else alpha / rank

    halves: dict = {}
    with safe_open(st_path, framework="pt") as st:
        for name in st.keys():
            m = _KEY.match(name)
            if not m or m.group(2) not in TARGETS or _PARENT[m.group(2)] not in name or int(m.group(1)) >= n_layers:
                raise ValueError(f"LoRA adapter {path}: unexpected tensor {name}")
            layer, target, half = int(m.group(1)), m.group(2), m.group(3)
            t = st.get_tensor(name).to(torch.float32)
            out_f, in_f = shapes[target]
            want = (rank, in_f) if half == "A" else (out_f, rank)
            if tuple(t.shape) != want:
                raise ValueError(f"LoRA adapter {path}: {name} has shape {tuple(t.shape)}, "
                                 f"the base model needs {want}")
            halves.setdefault((layer, target), {})[half] = t
    ad = LoraAdapter(rank, float(scale))
    for (layer, target), h in sorted(halves.items()):
        if set(h) != {"A", "B"}:
            have = "lora_" + next(iter(h))
            raise ValueError(f"LoRA adapter {path}: layer {layer} {target} has {have} but not its other half")
        ad.tensors[(layer, target)] = (h["A"], h["B"])
    if not ad.tensors:
        raise ValueError(f"LoRA adapter {path}: no LoRA tensors found")
    return ad


def parse_lora_modules(items) -> dict:
    """``["name=path", ...]`` (the ``--lora-modules`` option) as ``{name: path}``."""
    out = {}
    for it in items or ():
        name, sep, path = it.partition("=")
        if not sep or not name or not path:
            raise ValueError(f"--lora-modules takes name=path, got {it!r}")
        if name in out:
            raise ValueError(f"--lora-modules names {name!r} twice")
        out[name] = path
    return out


def write_random_adapter(path: str, cfg, rank: int, seed: int = 0, std: float = 0.02, targets=tuple(TARGETS),
                         dtype=torch.bfloat16) -> str:
    """Write a PEFT-format adapter of ``rank`` with A, B ~ N(0, std) on ``targets`` for a model of
    config ``cfg`` (``LlamaConfig``) into ``path`` (benchmarks and tests: no trained adapter needed)."""
    from safetensors.torch import save_file

    hd, d, f = cfg.head_dim, cfg.dim, cfg.ffn_dim
    shapes = {"q_proj": (cfg.n_heads * hd, d), "k_proj": (cfg.n_kv_heads * hd, d), "v_proj": (cfg.n_kv_heads * hd, d),
              "o_proj": (d, cfg.n_heads * hd), "gate_proj": (f, d), "up_proj": (f, d), "down_proj": (d, f)}
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i in range(cfg.n_layers):
        for t in targets:
            out_f, in_f = shapes[t]
            base = f"base_model.model.model.layers.{i}.{_PARENT[t]}.{t}"
            sd[f"{base}.lora_A.weight"] = (torch.randn(rank, in_f, generator=g) * std).to(dtype)
            sd[f"{base}.lora_B.weight"] = (torch.randn(out_f, rank, generator=g) * std).to(dtype)
    os.makedirs(path, exist_ok=True)
    save_file(sd, os.path.join(path, "adapter_model.safetensors"))
    with open(os.path.join(path, "adapter_config.json"), "w") as fh:
        json.dump({"peft_type": "LORA", "r": rank, "lora_alpha": 2 * rank, "target_modules": list(targets),
                   "bias": "none", "task_type": "CAUSAL_LM"}, fh)
    return path
