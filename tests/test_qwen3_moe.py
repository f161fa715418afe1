"""Qwen3-MoE serving: ``moe_fine_gemm`` (``csrc/moe_fine.hip``) and the 128-expert router against fp64
references on exact integer data, the loader against transformers, the engine in captured graphs."""

import functools
import json
import os

import pytest
import torch

from dstack_amd.ops import reference as ref
from dstack_amd.ops import serving as sops
from dstack_amd.serving.engine import LLMEngine, SamplingParams
from tests.test_moe import _mlp64, _mlp_equals_its_steps, _patterns


def _tiny_qwen3_moe(root, hidden, ffn, experts, per_tok):
    """A random fp32 Qwen3-MoE (``hidden / 128`` heads, 1 KV head, 2 layers) saved as the installed
    transformers writes it ("saved"), under the other spelling of the expert tensors (fused ``mlp.experts``
    tensors / the Hub's per-expert projections: "resaved") and with the other spelling of the config key
    that counts the experts ("rekeyed").  Returns (model, {name: dir})."""
    from safetensors.torch import load_file, save_file
    from transformers import Qwen3MoeConfig, Qwen3MoeForCausalLM

    torch.manual_seed(0)
    cfg = Qwen3MoeConfig(hidden_size=hidden, num_attention_heads=hidden // 128, num_key_value_heads=1, head_dim=128,
                         intermediate_size=2 * ffn, moe_intermediate_size=ffn, num_experts=experts,
                         num_experts_per_tok=per_tok, norm_topk_prob=True, num_hidden_layers=2, vocab_size=128,
                         max_position_embeddings=512, tie_word_embeddings=False)
    model = Qwen3MoeForCausalLM(cfg).float().eval()
    dirs = {s: os.path.join(root, s) for s in ("saved", "resaved", "rekeyed")}
    model.save_pretrained(dirs["saved"], safe_serialization=True)
    sd = load_file(os.path.join(dirs["saved"], "model.safetensors"))
    other = {n: t for n, t in sd.items() if ".mlp.experts." not in n}
    for name in [n for n in sd if n.endswith(".mlp.gate.weight")]:
        pre = name[: -len(".gate.weight")]
        if f"{pre}.experts.gate_up_proj" in sd:  # fused -> per-expert
            for e in range(experts):
                g, u = sd[f"{pre}.experts.gate_up_proj"][e].chunk(2)
                for w, v in (("gate_proj", g), ("up_proj", u), ("down_proj", sd[f"{pre}.experts.down_proj"][e])):
                    other[f"{pre}.experts.{e}.{w}.weight"] = v.contiguous()
        else:  # per-expert -> fused: gate rows first
            ex = [[sd[f"{pre}.experts.{e}.{w}.weight"] for e in range(experts)] for w in ("gate_proj", "up_proj", "down_proj")]
            other[f"{pre}.experts.gate_up_proj"] = torch.stack([torch.cat([g, u]) for g, u in zip(ex[0], ex[1])])
            other[f"{pre}.experts.down_proj"] = torch.stack(ex[2])
    with open(os.path.join(dirs["saved"], "config.json")) as f:
        hf = json.load(f)
    a, b = ("num_experts", "num_local_experts") if "num_experts" in hf else ("num_local_experts", "num_experts")
    rekeyed = {**{k: v for k, v in hf.items() if k != a}, b: hf[a]}
    for name, tensors, conf in (("resaved", other, hf), ("rekeyed", sd, rekeyed)):
        os.makedirs(dirs[name])
        save_file(tensors, os.path.join(dirs[name], "model.safetensors"))
        with open(os.path.join(dirs[name], "config.json"), "w") as f:
            json.dump(conf, f)
    return model, dirs


# ---------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cpu_case(root):
    model, dirs = _tiny_qwen3_moe(root, 256, 128, 16, 4)
    prompt = [3, 17, 42, 99, 5, 64]
    with torch.no_grad():
        want = model.generate(torch.tensor([prompt]), max_new_tokens=10, do_sample=False)[0, len(prompt):].tolist()
    return dirs, prompt, want


@pytest.mark.parametrize("spelling", ["saved", "resaved", "rekeyed"])
def test_cpu_engine_equals_transformers(tmp_path_factory, spelling):
    """Greedy, 10 tokens, token for token, for both spellings of the expert tensors and of the expert count
    (seed 0: the engine and transformers agree on every token on the CPU, so no router near-tie decides one)."""
    dirs, prompt, want = _cpu_case(str(tmp_path_factory.getbasetemp() / "qwen3_moe_cpu"))
    eng = LLMEngine.from_model(dirs[spelling], device="cpu", max_model_len=64, max_batch=2, num_pages=8)
    assert eng.model.spec.family == "qwen3_moe" and eng.model.spec.qk_norm and (eng.model.E, eng.model.topk) == (16, 4)
    assert eng.model.layers[0]["wgu"].shape == (16, 256, 256) and eng.model.layers[0]["wdown"].shape == (16, 256, 128)
    got = eng.generate([prompt], SamplingParams(max_tokens=10, temperature=0, ignore_eos=True))[0].output_ids
    assert got == want


@pytest.mark.parametrize("cfg,kw,match", [
    (dict(norm_topk_prob=False), {}, "norm_topk_prob"),
    (dict(mlp_only_layers=[0]), {}, "mlp_only_layers"),
    (dict(decoder_sparse_step=2), {}, "decoder_sparse_step"),
    (dict(num_experts=129), {}, "num_experts"),
    ({}, dict(quantization="fp8"), "quantization"),
    ({}, dict(quantization="mxfp4"), "quantization"),
    ({}, dict(quantization="awq"), "quantization"),
    ({}, dict(tp_group=object()), "tp_group"),
    ({}, dict(lora_modules={"a": "nowhere"}), "lora_modules"),
])
def test_refused_at_start(tmp_path, cfg, kw, match):
    hf = {**dict(model_type="qwen3_moe", hidden_size=512, num_attention_heads=4, num_key_value_heads=1, head_dim=128,
                 intermediate_size=1024, moe_intermediate_size=768, num_hidden_layers=2, vocab_size=128,
                 num_experts=128, num_experts_per_tok=8), **cfg}
    (tmp_path / "config.json").write_text(json.dumps(hf))
    with pytest.raises(ValueError, match=match):
        LLMEngine.from_model(str(tmp_path), device="cpu", **kw)


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
def _exact_case(gpu, R, E, k, N, K, split, patterns=None):
    """``test_moe.py::test_gpu_gemm_exact``'s method on ``moe_fine_gemm`` with ``split`` K slices."""
    g = torch.Generator().manual_seed(R * 1000 + N + E)
    Wc = (torch.randint(0, 2, (E, N, K), generator=g) * 2 - 1).to(torch.bfloat16)
    W = Wc.to(gpu)
    xs = {k: torch.randint(-1, 2, (R, K), generator=g).to(gpu, torch.bfloat16),
          1: torch.randint(-1, 2, (R * k, K), generator=g).to(gpu, torch.bfloat16)}
    for name, (topk_e, live) in _patterns(R, E, k, g).items():
        if patterns and name not in patterns:
            continue
        topk_e, live = topk_e.to(gpu, torch.int32).contiguous(), live.to(gpu)
        counts, lists = sops.moe_lists(topk_e, live, E)
        rc, rl = ref.moe_lists(topk_e.cpu(), live.cpu(), E)
        assert counts.cpu().tolist() == rc.tolist() and lists.cpu().tolist() == rl.tolist(), name
        alive = (live > 0).repeat_interleave(k).cpu()
        for src_div, x in xs.items():
            part = sops.moe_fine_gemm(x, src_div, W, counts, lists, split)
            want = sops.moe_gemm_ref(x.cpu(), src_div, Wc, rc, rl, 1)[0].double()  # (fp64 sums, zeros for dead pairs)
            assert part.shape[0] == split and torch.equal(part.sum(0).cpu().double()[alive], want[alive]), (name, src_div)
        y = torch.full((R, N), float("nan"), dtype=torch.bfloat16, device=gpu)
        sops.moe_combine(part, torch.ones(R, k, device=gpu), live, out=y)
        assert torch.equal(y.cpu(), want.view(R, k, N).sum(1).to(torch.bfloat16)), name


@pytest.mark.gpu
@pytest.mark.parametrize("E,k,N,K", [(128, 8, 128, 768), (128, 8, 256, 512), (16, 4, 384, 1280)])
@pytest.mark.parametrize("R", [1, 17, 100, 256])
def test_gpu_fine_gemm_exact(gpu, R, E, k, N, K):
    """x in {-1, 0, 1}, W in {-1, +1}: every summation order is exact, so the partials summed over the K
    slices equal the fp64 product in every element, per token (``src_div = k``) and per pair (``src_div =
    1``), and dead rows come out of ``moe_combine`` as exact zeros from a NaN-filled output.  Six K-steps
    (the tail), the minimum K, ten steps; "all to the first k" gives an expert R pairs: four passes at
    R = 256, two with a ragged last block at R = 100."""
    split = sops.moe_fine_gemm_split(R, k, E, N, K)
    assert split >= 1
    _exact_case(gpu, R, E, k, N, K, split)


@pytest.mark.gpu
@pytest.mark.parametrize("K,split", [(2048, 1), (2048, 4), (1536, 2)])
def test_gpu_fine_gemm_forced_split(gpu, K, split):
    """Slices of 16, 4 and 6 steps (the last: every slice ends in the six-step tail)."""
    _exact_case(gpu, 100, 16, 4, 256, K, split, patterns=("all to the first k", "every third row dead"))


@pytest.mark.gpu
@pytest.mark.parametrize("R,E,k", [(1, 128, 8), (17, 128, 8), (256, 128, 8)])
def test_gpu_route_exact_128(gpu, R, E, k):
    """``test_moe.py::test_gpu_route_exact``'s construction with two experts per lane: the planted tie of
    row 0 is between experts 0 and 127 (lane 0's first and lane 63's second).  Experts, counts and lists
    equal the reference exactly; the weights match the fp64 softmax within 1e-5 relative (about ten fp32
    operations of at most 2 ulp).  A NaN row stays in range."""
    g = torch.Generator().manual_seed(R + E)
    h = torch.zeros(R, 512)
    h[torch.arange(R), torch.arange(R)] = (torch.randint(0, 2, (R,), generator=g) * 2 - 1).float()
    h[:, 256:] = torch.randint(-1, 2, (R, 256), generator=g).float()
    gate = torch.zeros(E, 512)
    gate[:, :R] = (torch.rand(R, E, generator=g).argsort(dim=1).t() - E // 2).float()
    gate[:, 256:] = torch.randint(-1, 2, (256,), generator=g).float()
    gate[E - 1, 0] = gate[0, 0]  # the tie (row 0)
    live = (torch.arange(R) % 5 != 3).int()
    hg, gg = h.to(gpu, torch.bfloat16), gate.to(gpu, torch.bfloat16)
    topk_e, topk_w, counts, lists = sops.moe_route(hg, gg, live.to(gpu), k)
    re, rw, rc, rl = ref.moe_route(h, gate, live, k)
    assert topk_e.cpu().tolist() == re.tolist() and counts.cpu().tolist() == rc.tolist() and lists.cpu().tolist() == rl.tolist()
    p64 = torch.softmax(h.double() @ gate.double().t(), -1).gather(1, re.long())
    torch.testing.assert_close(topk_w.cpu().double(), p64 / p64.sum(-1, keepdim=True), rtol=1e-5, atol=0)
    hg[R // 2, 300] = float("nan")
    topk_e, _, counts, lists = sops.moe_route(hg, gg, live.to(gpu), k)
    assert 0 <= int(topk_e.min()) and int(topk_e.max()) < E and int(counts.sum()) == int(live.sum()) * k
    assert -1 <= int(lists.min()) and int(lists.max()) < R * k


@pytest.mark.gpu
@pytest.mark.parametrize("R", [17, 256])
def test_gpu_fine_mlp_no_worse_than_library_path(gpu, R, capsys):
    """Gaussian data, D 512, F 768, 128 experts, top-8: the kernel path's RMS error against the fp64
    reference is no larger than that of the eager bf16 library path, which rounds the gate/up and down
    products to bf16 where the kernels keep fp32 (no margin, as in ``test_moe.py``)."""
    g = torch.Generator().manual_seed(R)
    E, k, D, F = 128, 8, 512, 768
    h = torch.randn(R, D, generator=g).to(gpu, torch.bfloat16)
    router = torch.randn(E, D, generator=g).to(gpu, torch.bfloat16)
    wgu = (torch.randn(E, 2 * F, D, generator=g) / D ** 0.5).to(gpu, torch.bfloat16)
    wdown = (torch.randn(E, D, F, generator=g) / F ** 0.5).to(gpu, torch.bfloat16)
    live = torch.ones(R, dtype=torch.int32, device=gpu)
    want = _mlp64(h.cpu(), router.cpu(), wgu.cpu(), wdown.cpu(), k)
    got = sops.moe_fine_mlp(h, router, wgu, wdown, k, live, sops.MoeWorkspace(E, k, D, F, gpu, fine=True))
    eager = sops.moe_mlp_eager(h, router, wgu, wdown, k, live)
    err, err_eager = ((t.cpu().double() - want).pow(2).mean().sqrt().item() for t in (got, eager))
    with capsys.disabled():
        print(f"\nmoe_fine_mlp R={R}: rms error kernels {err:.3e}, eager library path {err_eager:.3e}, rms of the "
              f"result {want.pow(2).mean().sqrt().item():.3e}")
    assert err <= err_eager


@pytest.mark.gpu
def test_gpu_fine_mlp_equals_its_steps(gpu):
    """72 experts: past 64, so the router's two-per-lane form runs."""
    g = torch.Generator().manual_seed(0)
    E, k, D, F = 72, 8, 512, 512
    router = torch.randn(E, D, generator=g).to(gpu, torch.bfloat16)
    wgu = (torch.randn(E, 2 * F, D, generator=g) / D ** 0.5).to(gpu, torch.bfloat16)
    wdown = (torch.randn(E, D, F, generator=g) / F ** 0.5).to(gpu, torch.bfloat16)
    _mlp_equals_its_steps(gpu, sops.moe_fine_mlp, sops.moe_fine_gemm, lambda: sops.MoeWorkspace(E, k, D, F, gpu, fine=True),
                          router, wgu, wdown, k)


GPU_KW = dict(device="cuda", max_model_len=512, max_batch=8, num_pages=64)
PROMPTS = [[1, 2, 3, 4, 5, 1, 2, 3, 4, 5, 1, 2, 3], list(range(7, 90))]


@functools.lru_cache(maxsize=None)
def _gpu_case(root):
    """(checkpoint directory, eager greedy tokens) of a tiny Qwen3-MoE: hidden 512, F 768, 128 experts top-8."""
    _, dirs = _tiny_qwen3_moe(root, 512, 768, 128, 8)
    eager = LLMEngine.from_model(dirs["saved"], use_graphs=False, **GPU_KW)
    sp = SamplingParams(max_tokens=12, temperature=0, ignore_eos=True)
    return dirs["saved"], [o.output_ids for o in eager.generate(PROMPTS, sp)]


@pytest.mark.gpu
@pytest.mark.parametrize("speculative", [0, 3])
def test_gpu_engine_graphs_equal_eager(gpu, tmp_path_factory, speculative):
    path, want = _gpu_case(str(tmp_path_factory.getbasetemp() / "qwen3_moe_gpu"))
    eng = LLMEngine.from_model(path, speculative_ngram=speculative, **GPU_KW)
    eng.capture_graphs()
    got = [o.output_ids for o in eng.generate(PROMPTS, SamplingParams(max_tokens=12, temperature=0, ignore_eos=True))]
    assert got == want and (not speculative or eng.stats["spec_steps"] > 0)


@pytest.mark.gpu
def test_gpu_long_prefill_stays_on_the_kernels(gpu, tmp_path_factory, monkeypatch):
    path, _ = _gpu_case(str(tmp_path_factory.getbasetemp() / "qwen3_moe_gpu"))
    calls = []
    monkeypatch.setattr(sops, "moe_mlp_eager", lambda *a, **kw: calls.append(a[0].shape[0]))
    eng = LLMEngine.from_model(path, use_graphs=False, **GPU_KW)
    out = eng.generate([[5 + i % 100 for i in range(300)]], SamplingParams(max_tokens=2, temperature=0, ignore_eos=True))
    assert len(out[0].output_ids) == 2 and calls == []
