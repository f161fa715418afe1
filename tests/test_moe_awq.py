"""AWQ Mixtral checkpoints: the W4A16 routed expert GEMM of ``csrc/moe_w4.hip`` against fp64 references on
exact integer data, the loader against transformers, the engine in captured graphs."""

import functools
import json
import os

import pytest
import torch

from dstack_amd.ops import reference as ref
from dstack_amd.ops import serving as sops
from dstack_amd.serving.engine import LLMEngine, SamplingParams
from dstack_amd.serving.model import Awq4Experts, Awq4Weight
from tests.test_awq import _exact_case, pack_awq
from tests.test_moe import GPU_KW, PROMPTS, _mlp64, _mlp_equals_its_steps, _patterns, _tiny_mixtral


def _experts(gpu, E, M, N, K, g, seed, long_k=False):
    """E experts of ``test_awq._exact_case`` data: (stacked stored weight, fp32 (q - z) s [E, N, K], x [M, K])."""
    cases = [_exact_case(gpu, M, N, K, g, seed + e, long_k) for e in range(E)]
    stored = tuple(torch.stack(t) for t in zip(*(sops.w4_shuffle(c, z, s, g) for c, z, s, _, _ in cases)))
    return stored, torch.stack([ref.dequant_w4(c, z, s, g) for c, z, s, _, _ in cases]).cpu(), cases[0][3].bfloat16()


@pytest.mark.gpu
@pytest.mark.parametrize("E,k,N,K,g", [(8, 2, 256, 512, 128), (8, 2, 512, 1024, 32), (16, 4, 256, 512, 64)])
@pytest.mark.parametrize("R", [1, 5, 16, 17, 100, 256])
def test_gpu_gemm_exact(gpu, R, E, k, N, K, g):
    """Integer data on which every fp32 sum of the kernel is exact (``test_awq._exact_case``): the partials
    summed over the K slices equal the fp64 product with the dequantized expert in every element of
    every live pair, gathered per token (``src_div = k``) and per pair (``src_div = 1``), under the four
    routing patterns of ``test_moe``; ``moe_combine`` with weights of 1 gives its bf16 rounding and exact
    zeros for dead rows from an output pre-filled with NaN."""
    W, Wd, x = _experts(gpu, E, R * k, N, K, g, seed=R * 1000 + N + E)
    xs = {k: x[:R].contiguous(), 1: x}
    split = sops.moe_w4_gemm_split(R, k, E, N, K)
    assert split >= 1
    gen = torch.Generator().manual_seed(R + E)
    for name, (topk_e, live) in _patterns(R, E, k, gen).items():
        topk_e, live = topk_e.to(gpu, torch.int32).contiguous(), live.to(gpu)
        counts, lists = sops.moe_lists(topk_e, live, E)
        alive = (live > 0).repeat_interleave(k).cpu()
        for src_div, xd in xs.items():
            part = sops.moe_w4_gemm(xd, src_div, W, g, counts, lists, split)
            want = sops.moe_gemm_ref(xd.cpu(), src_div, Wd, counts.cpu(), lists.cpu(), 1)[0].double()
            assert torch.equal(part.sum(0).cpu().double()[alive], want[alive]), (name, src_div)
        y = torch.full((R, N), float("nan"), dtype=torch.bfloat16, device=gpu)
        sops.moe_combine(part, torch.ones(R, k, device=gpu), live, out=y)
        assert torch.equal(y.cpu(), want.view(R, k, N).sum(1).to(torch.bfloat16)), name


@pytest.mark.gpu
def test_gpu_gemm_split_k(gpu):
    """K = 8192 in 1 and 4 slices and in as many as the split rule gives: exact, and the same bits from
    run to run (no atomics)."""
    R, E, k, N, K, g = 17, 8, 2, 256, 8192, 128
    W, Wd, x = _experts(gpu, E, R, N, K, g, seed=3, long_k=True)
    topk_e, live = _patterns(R, E, k, torch.Generator().manual_seed(1))["random"]
    counts, lists = sops.moe_lists(topk_e.to(gpu, torch.int32).contiguous(), live.to(gpu), E)
    want = sops.moe_gemm_ref(x.cpu(), k, Wd, counts.cpu(), lists.cpu(), 1)[0].double()
    rule = sops.moe_w4_gemm_split(R, k, E, N, K)
    assert rule >= 1 and K % (512 * rule) == 0
    for split in (1, 4, rule):
        part = sops.moe_w4_gemm(x, k, W, g, counts, lists, split)
        assert part.shape[0] == split and torch.equal(part.sum(0).cpu().double(), want), split
        assert torch.equal(sops.moe_w4_gemm(x, k, W, g, counts, lists, split), part), split


@pytest.mark.gpu
@pytest.mark.parametrize("R", [17, 256])
def test_gpu_mlp_no_worse_than_the_bf16_kernels(gpu, R, capsys):
    """Gaussian data, D = F = 512, 8 experts, top-2, g = 128, weights ``quant_w4`` of Gaussian ones.  Against
    ``ref.moe_mlp`` in fp64 on the exact fp32 ``(q - z) s`` the RMS error of ``moe_w4_mlp`` does not exceed
    that of the bf16 ``moe_mlp`` kernels on the bf16 rounding of the same weights: that path rounds every
    weight by 2^-9 relative, the W4 path applies fp32 scales to exact integers and adds about 2e-6 relative
    (``w4.hip``).  No margin.  Measured on an MI355X: see docs/reference/performance.md."""
    gen = torch.Generator().manual_seed(R)
    E, k, D, F, g = 8, 2, 512, 512, 128
    h = torch.randn(R, D, generator=gen).to(gpu, torch.bfloat16)
    router = torch.randn(E, D, generator=gen).to(gpu, torch.bfloat16)
    live = torch.ones(R, dtype=torch.int32, device=gpu)
    stored, deq = [], []
    for N, K in ((2 * F, D), (D, F)):
        canon = [ref.quant_w4(torch.randn(N, K, generator=gen) / K ** 0.5, g) for _ in range(E)]
        stored.append(tuple(torch.stack(t).to(gpu) for t in zip(*(sops.w4_shuffle(*c, g) for c in canon))))
        deq.append(torch.stack([ref.dequant_w4(*c, g) for c in canon]))
    want = _mlp64(h.cpu(), router.cpu(), deq[0], deq[1], k)
    got = sops.moe_w4_mlp(h, router, stored[0], stored[1], g, k, live, sops.MoeWorkspace(E, k, D, F, gpu, w4_group=g))
    bf16 = sops.moe_mlp(h, router, deq[0].to(gpu, torch.bfloat16), deq[1].to(gpu, torch.bfloat16), k, live,
                        sops.MoeWorkspace(E, k, D, F, gpu))
    err, err_bf16 = ((t.cpu().double() - want).pow(2).mean().sqrt().item() for t in (got, bf16))
    with capsys.disabled():
        print(f"\nmoe_w4_mlp R={R}: rms error W4 kernels {err:.3e}, bf16 kernels on bf16((q - z) s) {err_bf16:.3e}, rms of "
              f"the result {want.pow(2).mean().sqrt().item():.3e}")
    assert err <= err_bf16


@pytest.mark.gpu
def test_gpu_mlp_equals_its_steps(gpu):
    gen = torch.Generator().manual_seed(0)
    E, k, D, F, g = 8, 2, 512, 512, 128
    router = torch.randn(E, D, generator=gen).to(gpu, torch.bfloat16)
    wgu, wdown = (tuple(torch.stack(t).to(gpu) for t in zip(*(
        sops.w4_shuffle(*ref.quant_w4(torch.randn(N, K, generator=gen) / K ** 0.5, g), g) for _ in range(E))))
        for N, K in ((2 * F, D), (D, F)))
    _mlp_equals_its_steps(gpu, lambda h, r, u, d, *a: sops.moe_w4_mlp(h, r, u, d, g, *a),
                          lambda x, src_div, W, *a: sops.moe_w4_gemm(x, src_div, W, g, *a),
                          lambda: sops.MoeWorkspace(E, k, D, F, gpu, w4_group=g), router, wgu, wdown, k)


# ---------------------------------------------------------------------------------------------
# checkpoints
# ---------------------------------------------------------------------------------------------
def _write(root, hidden, ffn, g, skip=("gate",)):
    """A tiny Mixtral whose projections and experts are ``quant_w4`` of random weights, written as an AutoAWQ
    checkpoint (its packing and names; the router and the rest in fp16) and as the unquantized checkpoint
    holding ``dequant_w4`` of the same tensors.  Returns (AWQ dir, plain dir, {tensor name: canonical W4})."""
    from safetensors.torch import load_file, save_file

    _, dirs = _tiny_mixtral(os.path.join(root, "src"), hidden, ffn)
    sd = load_file(os.path.join(dirs["saved"], "model.safetensors"))
    awq, plain, canon = {}, {}, {}
    for name, t in sd.items():
        pre = name[: -len(".weight")]
        if pre.endswith(("_proj", ".w1", ".w2", ".w3")):
            c, z, s = canon[pre] = ref.quant_w4(t, g)
            q = torch.stack([c & 15, c >> 4], -1).reshape(t.shape)
            awq[pre + ".qweight"], awq[pre + ".qzeros"], awq[pre + ".scales"] = pack_awq(q.t()), pack_awq(z.t()), s.t().contiguous()
            plain[name] = ref.dequant_w4(c, z, s, g)
        else:
            awq[name], plain[name] = t.half(), t.half().float()
    with open(os.path.join(dirs["saved"], "config.json")) as f:
        cfg = json.load(f)
    qc = dict(quant_method="awq", bits=4, group_size=g, version="GEMM", zero_point=True, modules_to_not_convert=list(skip))
    for sub, tensors, c in (("awq", awq, {**cfg, "quantization_config": qc}), ("plain", plain, cfg)):
        os.makedirs(os.path.join(root, sub))
        save_file(tensors, os.path.join(root, sub, "model.safetensors"))
        with open(os.path.join(root, sub, "config.json"), "w") as f:
            json.dump(c, f)
    return os.path.join(root, "awq"), os.path.join(root, "plain"), canon


CPU_KW = dict(device="cpu", max_model_len=64, max_batch=2, num_pages=8)


@pytest.mark.parametrize("g", [64, 128])
def test_cpu_engine_on_an_awq_mixtral_checkpoint(tmp_path, g):
    """Greedy, 10 tokens, token for token: the engine on the AWQ directory (no flag), the engine on the
    dequantized checkpoint and transformers' Mixtral on the dequantized weights."""
    from transformers import MixtralForCausalLM

    awq_path, plain_path, canon = _write(str(tmp_path), 256, 512, g)
    prompt = [3, 17, 42, 99, 5, 64]
    sp = SamplingParams(max_tokens=10, temperature=0, ignore_eos=True)
    eng = LLMEngine.from_model(awq_path, **CPU_KW)
    base = LLMEngine.from_model(plain_path, **CPU_KW)
    m = eng.model
    assert m.quantization == "awq" and base.model.quantization is None
    L = m.layers[1]
    assert isinstance(L["wgu"], Awq4Experts) and isinstance(L["wdown"], Awq4Experts) and isinstance(L["wo"], Awq4Weight)
    assert L["wgu"].shape == (8, 1024, 256) and L["wdown"].shape == (8, 256, 512) and L["wgu"].g == g
    pre = "model.layers.1.block_sparse_moe.experts.5."
    for got, gate, up in zip(L["wgu"].canonical(5), canon[pre + "w1"], canon[pre + "w3"]):
        assert torch.equal(got, torch.cat([gate, up]))
    for got, want in zip(L["wdown"].canonical(5), canon[pre + "w2"]):
        assert torch.equal(got, want)
    # 4 + 24 / g bits per projection weight against fp32 here; the embedding, head and norms are the same bytes
    rest = sum(t.numel() * 4 for t in (m.embed, m.lm_head, m.norm))
    assert m.weight_bytes() - rest < 0.45 * (base.model.weight_bytes() - rest) / 2
    hf = MixtralForCausalLM.from_pretrained(plain_path, dtype=torch.float32).eval()
    with torch.no_grad():
        want = hf.generate(torch.tensor([prompt]), max_new_tokens=10, do_sample=False)[0, len(prompt):].tolist()
    assert eng.generate([prompt], sp)[0].output_ids == want
    assert base.generate([prompt], sp)[0].output_ids == want


def _drop(name):
    return lambda sd: sd.pop(name)


@pytest.mark.parametrize("family,skip,damage,kw,match", [
    ("mixtral", ["gate", "w2"], None, {}, "modules_to_not_convert"),
    ("llama", ["gate"], None, {}, "modules_to_not_convert"),
    ("mixtral", ["gate"], _drop("model.layers.1.block_sparse_moe.experts.3.w3.qzeros"), {},
     r"missing 1 tensors.*experts\.3\.w3\.qzeros"),
    ("mixtral", ["gate"], lambda sd: sd.update({"model.layers.0.block_sparse_moe.experts.2.w1.weight": torch.zeros(512, 256)}),
     {}, r"unexpected tensor model\.layers\.0\.block_sparse_moe\.experts\.2\.w1\.weight.*AWQ"),
    ("mixtral", ["gate"], None, dict(quantization="fp8"), "--quantization"),
])
def test_refusals(tmp_path, family, skip, damage, kw, match):
    from safetensors.torch import load_file, save_file

    awq_path, _, _ = _write(str(tmp_path), 256, 512, 128, skip=skip)
    cfg = json.load(open(os.path.join(awq_path, "config.json")))
    cfg["model_type"] = family
    json.dump(cfg, open(os.path.join(awq_path, "config.json"), "w"))
    if damage:
        sd = load_file(os.path.join(awq_path, "model.safetensors"))
        damage(sd)
        save_file(sd, os.path.join(awq_path, "model.safetensors"))
    with pytest.raises(ValueError, match=match):
        LLMEngine.from_model(awq_path, **CPU_KW, **kw)


# ---------------------------------------------------------------------------------------------
# engine on the GPU
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gpu_case(root):
    """(AWQ checkpoint directory, eager greedy tokens) of a tiny Mixtral with hidden 512 and FFN 512."""
    awq_path, _, _ = _write(root, 512, 512, 128)
    eager = LLMEngine.from_model(awq_path, use_graphs=False, **GPU_KW)
    sp = SamplingParams(max_tokens=12, temperature=0, ignore_eos=True)
    return awq_path, [o.output_ids for o in eager.generate(PROMPTS, sp)]


@pytest.mark.gpu
@pytest.mark.parametrize("speculative", [0, 3])
def test_gpu_engine_graphs_equal_eager(gpu, tmp_path_factory, speculative):
    """Decode steps -- and with n-gram speculation the verify steps -- in captured graphs emit the eager
    engine's greedy tokens."""
    path, want = _gpu_case(str(tmp_path_factory.getbasetemp() / "moe_awq_gpu"))
    eng = LLMEngine.from_model(path, speculative_ngram=speculative, **GPU_KW)
    assert isinstance(eng.model.layers[0]["wgu"], Awq4Experts)
    eng.capture_graphs()
    got = [o.output_ids for o in eng.generate(PROMPTS, SamplingParams(max_tokens=12, temperature=0, ignore_eos=True))]
    assert got == want and (not speculative or eng.stats["spec_steps"] > 0)


@pytest.mark.gpu
def test_gpu_long_prefill_dequantizes_expert_by_expert(gpu, tmp_path_factory):
    """One 512-row prefill runs the eager dequant path.  The dequant is exact and the GEMMs are the same,
    so the logits equal, bit for bit, those of the same model with its experts replaced by
    ``bf16((q - z) s)`` tensors on ``moe_mlp_eager``."""
    path, _ = _gpu_case(str(tmp_path_factory.getbasetemp() / "moe_awq_gpu"))
    tokens = torch.arange(1, 513, device=gpu) % 100
    pos = torch.arange(256, dtype=torch.int32, device=gpu).repeat(2)
    slots = torch.arange(512, dtype=torch.int32, device=gpu)
    a = LLMEngine.from_model(path, use_graphs=False, **dict(GPU_KW, num_pages=128)).model
    got = a.prefill(tokens, pos, slots, [0, 256], [256, 256])
    for L in a.layers:
        for key in ("wgu", "wdown"):
            L[key] = L[key].dequantized().to(gpu, torch.bfloat16)
    want = a.prefill(tokens, pos, slots, [0, 256], [256, 256])
    assert got.abs().max() > 0.1 and torch.equal(got, want)
