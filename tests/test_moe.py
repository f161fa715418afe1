"""Mixtral sparse-MoE serving: the router and grouped-GEMM kernels of ``csrc/moe.hip`` against fp64
references on exact integer data, the loader against transformers, the engine in captured graphs."""

import functools
import json
import math
import os

import pytest
import torch

from dstack_amd.ops import reference as ref
from dstack_amd.ops import serving as sops
from dstack_amd.serving.engine import LLMEngine, SamplingParams


def _tiny_mixtral(root, hidden, ffn, experts=8, per_tok=2):
    """A random fp32 Mixtral (``hidden / 128`` heads, 1 KV head, 2 layers) saved twice: as the installed
    transformers writes it and under the other spelling of the expert tensors (the Hub's per-expert
    ``block_sparse_moe`` names / the fused ``mlp.experts`` tensors).  Returns (model, {spelling: dir})."""
    from safetensors.torch import load_file, save_file
    from transformers import MixtralConfig, MixtralForCausalLM

    torch.manual_seed(0)
    cfg = MixtralConfig(hidden_size=hidden, num_attention_heads=hidden // 128, num_key_value_heads=1, head_dim=128,
                        intermediate_size=ffn, num_local_experts=experts, num_experts_per_tok=per_tok,
                        num_hidden_layers=2, vocab_size=128, max_position_embeddings=512, sliding_window=None,
                        tie_word_embeddings=False)
    model = MixtralForCausalLM(cfg).float().eval()
    dirs = {s: os.path.join(root, s) for s in ("saved", "resaved")}
    model.save_pretrained(dirs["saved"], safe_serialization=True)
    sd = load_file(os.path.join(dirs["saved"], "model.safetensors"))
    other = {}
    for name, t in sd.items():
        pre = name.split(".block_sparse_moe.")[0].split(".mlp.")[0]
        if name.endswith("block_sparse_moe.gate.weight"):  # per-expert -> fused: gate rows first
            ex = [[sd[f"{pre}.block_sparse_moe.experts.{e}.{w}.weight"] for e in range(experts)] for w in ("w1", "w3", "w2")]
            other[f"{pre}.mlp.gate.weight"] = t
            other[f"{pre}.mlp.experts.gate_up_proj"] = torch.stack([torch.cat([g, u]) for g, u in zip(ex[0], ex[1])])
            other[f"{pre}.mlp.experts.down_proj"] = torch.stack(ex[2])
        elif name.endswith("mlp.gate.weight"):  # fused -> per-expert
            other[f"{pre}.block_sparse_moe.gate.weight"] = t
            for e in range(experts):
                g, u = sd[f"{pre}.mlp.experts.gate_up_proj"][e].chunk(2)
                for w, v in (("w1", g), ("w3", u), ("w2", sd[f"{pre}.mlp.experts.down_proj"][e])):
                    other[f"{pre}.block_sparse_moe.experts.{e}.{w}.weight"] = v.contiguous()
        elif ".block_sparse_moe." not in name and ".mlp." not in name:
            other[name] = t
    os.makedirs(dirs["resaved"])
    save_file(other, os.path.join(dirs["resaved"], "model.safetensors"))
    with open(os.path.join(dirs["saved"], "config.json")) as f, open(os.path.join(dirs["resaved"], "config.json"), "w") as g:
        g.write(f.read())
    return model, dirs


def _mlp64(h, router, wgu, wdown, k, live=None):
    return ref.moe_mlp(h.double(), router.double(), wgu.double(), wdown.double(), k, live)


# ---------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------
def test_reference_router_and_mlp_by_hand():
    """Row 0 ties experts 0 and 1 at the top (order 0, 1, weights 1/2 each); row 1 picks expert 2, then
    the tie of experts 0 and 1 goes to expert 0, weights e/(e+1) and 1/(e+1)."""
    h = torch.tensor([[2.0, 0.0], [0.0, 1.0]])
    router = torch.tensor([[1.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
    wgu = torch.tensor([[[1.0, 0.0], [1.0, 1.0]], [[0.0, 1.0], [1.0, 0.0]], [[0.0, 2.0], [0.0, 1.0]]])  # gate row, up row
    wdown = torch.tensor([[[1.0], [0.0]], [[0.0], [1.0]], [[1.0], [1.0]]])
    live = torch.ones(2, dtype=torch.int32)
    topk_e, topk_w, counts, lists = ref.moe_route(h, router, live, 2)
    e = math.e
    assert topk_e.tolist() == [[0, 1], [2, 0]]
    torch.testing.assert_close(topk_w, torch.tensor([[0.5, 0.5], [e / (e + 1), 1 / (e + 1)]]))
    assert counts.tolist() == [2, 1, 1] and lists.tolist() == [[0, 3], [1, -1], [2, -1]]
    silu2 = 2 / (1 + math.exp(-2))
    # row 0: expert 0 gives silu(2) * 2 on column 0, expert 1 has gate 0; row 1: expert 2 gives silu(2) on both, expert 0 has gate 0
    want = torch.tensor([[0.5 * silu2 * 2, 0.0], [e / (e + 1) * silu2, e / (e + 1) * silu2]])
    torch.testing.assert_close(ref.moe_mlp(h, router, wgu, wdown, 2), want)
    dead = ref.moe_mlp(h, router, wgu, wdown, 2, torch.tensor([1, 0], dtype=torch.int32))
    torch.testing.assert_close(dead, torch.stack([want[0], torch.zeros(2)]))


@functools.lru_cache(maxsize=None)
def _cpu_case(root):
    model, dirs = _tiny_mixtral(root, 256, 512)
    prompt = [3, 17, 42, 99, 5, 64]
    with torch.no_grad():
        want = model.generate(torch.tensor([prompt]), max_new_tokens=10, do_sample=False)[0, len(prompt):].tolist()
    return dirs, prompt, want


@pytest.mark.parametrize("spelling", ["saved", "resaved"])
def test_cpu_engine_equals_transformers(tmp_path_factory, spelling):
    """Greedy, 10 tokens, token for token, for both spellings of the expert tensors (seed 0: the engine
    and transformers agree on every token on the CPU, so no router near-tie decides one)."""
    dirs, prompt, want = _cpu_case(str(tmp_path_factory.getbasetemp() / "moe_cpu"))
    eng = LLMEngine.from_model(dirs[spelling], device="cpu", max_model_len=64, max_batch=2, num_pages=8)
    assert eng.model.layers[0]["wgu"].shape == (8, 1024, 256) and eng.model.layers[0]["wdown"].shape == (8, 256, 512)
    got = eng.generate([prompt], SamplingParams(max_tokens=10, temperature=0, ignore_eos=True))[0].output_ids
    assert got == want


@pytest.mark.parametrize("spelling", ["saved", "resaved"])
def test_missing_expert_tensor_is_refused(tmp_path_factory, tmp_path, spelling):
    from safetensors.torch import load_file, save_file

    dirs, _, _ = _cpu_case(str(tmp_path_factory.getbasetemp() / "moe_cpu"))
    sd = load_file(os.path.join(dirs[spelling], "model.safetensors"))
    sd.pop(next(n for n in sorted(sd) if ".experts." in n))
    save_file(sd, str(tmp_path / "model.safetensors"))
    (tmp_path / "config.json").write_text(open(os.path.join(dirs[spelling], "config.json")).read())
    with pytest.raises(ValueError, match="missing 1 tensors"):
        LLMEngine.from_model(str(tmp_path), device="cpu", max_model_len=64, max_batch=2, num_pages=8)


@pytest.mark.parametrize("cfg,kw,match", [
    ({}, dict(quantization="fp8"), "--quantization"),
    ({}, dict(quantization="mxfp4"), "--quantization"),
    ({}, dict(quantization="awq"), "--quantization"),
    ({}, dict(tp_group=object()), "tensor parallel"),
    ({}, dict(lora_modules={"a": "nowhere"}), "--lora-modules"),
    (dict(num_local_experts=65), {}, "num_local_experts"),
    (dict(num_experts_per_tok=9, num_local_experts=16), {}, "num_experts_per_tok"),
])
def test_refused_at_start(tmp_path, cfg, kw, match):
    hf = {**dict(model_type="mixtral", hidden_size=512, num_attention_heads=4, num_key_value_heads=1,
                 intermediate_size=1024, num_hidden_layers=2, vocab_size=128, num_local_experts=8,
                 num_experts_per_tok=2, sliding_window=None), **cfg}
    (tmp_path / "config.json").write_text(json.dumps(hf))
    with pytest.raises(ValueError, match=match):
        LLMEngine.from_model(str(tmp_path), device="cpu", **kw)


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
def _patterns(R, E, k, g):
    """name -> (topk_e [R, k] of distinct experts per row, live [R])"""
    rand = torch.rand(R, E, generator=g).argsort(dim=1)[:, :k]
    no3 = (torch.rand(R, E - 1, generator=g).argsort(dim=1)[:, :k] + 4) % E  # nobody picks expert 3
    ones = torch.ones(R, dtype=torch.int32)
    return {"random": (rand, ones), "all to the first k": (torch.arange(k).repeat(R, 1), ones), "expert 3 empty": (no3, ones),
            "every third row dead": (rand, (torch.arange(R) % 3 != 2).int())}


@pytest.mark.gpu
@pytest.mark.parametrize("E,k,N,K", [(8, 2, 256, 512), (8, 2, 512, 1024), (16, 4, 256, 512)])
@pytest.mark.parametrize("R", [1, 5, 16, 17, 100, 256])
def test_gpu_gemm_exact(gpu, R, E, k, N, K):
    """x in {-1, 0, 1}, W in {-1, +1}: every summation order is exact, so the partials summed over the K
    slices equal the fp64 product in every element -- with the rows gathered per token (``src_div = k``)
    and per pair (``src_div = 1``) -- and ``moe_combine`` with weights of 1 equals its bf16 rounding;
    dead rows come out as exact zeros from an output pre-filled with NaN."""
    g = torch.Generator().manual_seed(R * 1000 + N + E)
    Wc = (torch.randint(0, 2, (E, N, K), generator=g) * 2 - 1).to(torch.bfloat16)
    W = Wc.to(gpu)
    xs = {k: torch.randint(-1, 2, (R, K), generator=g).to(gpu, torch.bfloat16),
          1: torch.randint(-1, 2, (R * k, K), generator=g).to(gpu, torch.bfloat16)}
    split = sops.moe_gemm_split(R, k, E, N, K)
    assert split >= 1
    for name, (topk_e, live) in _patterns(R, E, k, g).items():
        topk_e, live = topk_e.to(gpu, torch.int32).contiguous(), live.to(gpu)
        counts, lists = sops.moe_lists(topk_e, live, E)
        rc, rl = ref.moe_lists(topk_e.cpu(), live.cpu(), E)
        assert counts.cpu().tolist() == rc.tolist() and lists.cpu().tolist() == rl.tolist(), name
        alive = (live > 0).repeat_interleave(k).cpu()
        for src_div, x in xs.items():
            part = sops.moe_gemm(x, src_div, W, counts, lists, split)
            want = sops.moe_gemm_ref(x.cpu(), src_div, Wc, rc, rl, 1)[0].double()  # (fp64 sums, zeros for dead pairs)
            assert torch.equal(part.sum(0).cpu().double()[alive], want[alive]), (name, src_div)
        y = torch.full((R, N), float("nan"), dtype=torch.bfloat16, device=gpu)
        sops.moe_combine(part, torch.ones(R, k, device=gpu), live, out=y)
        assert torch.equal(y.cpu(), want.view(R, k, N).sum(1).to(torch.bfloat16)), name


@pytest.mark.gpu
@pytest.mark.parametrize("split", [1, 4])
def test_gpu_gemm_forced_split(gpu, split):
    g = torch.Generator().manual_seed(split)
    R, E, k, N, K = 17, 8, 2, 256, 2048
    W = (torch.randint(0, 2, (E, N, K), generator=g) * 2 - 1).to(torch.bfloat16)
    x = torch.randint(-1, 2, (R, K), generator=g).to(torch.bfloat16)
    topk_e, live = _patterns(R, E, k, g)["all to the first k"]
    topk_e = topk_e.to(torch.int32).contiguous()
    part = sops.moe_gemm(x.to(gpu), k, W.to(gpu), *sops.moe_lists(topk_e.to(gpu), live.to(gpu), E), split)
    want = sops.moe_gemm_ref(x, k, W, *ref.moe_lists(topk_e, live, E), 1)[0]
    assert part.shape[0] == split and torch.equal(part.sum(0).cpu().double(), want.double())


@pytest.mark.gpu
@pytest.mark.parametrize("R,E,k", [(1, 8, 2), (17, 8, 2), (100, 16, 4), (256, 64, 8)])
def test_gpu_route_exact(gpu, R, E, k):
    """Integer logits, distinct within a row but for one planted tie: a signed one-hot half of ``h``
    picks a column of distinct gate values, the other half adds the same integer to every expert's
    logit.  Experts, counts and lists equal the reference exactly; the weights match the fp64 softmax
    within 1e-5 relative (about ten fp32 operations of at most 2 ulp).  A NaN row stays in range."""
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
def test_gpu_mlp_no_worse_than_library_path(gpu, R, capsys):
    """Gaussian data, D = F = 512, 8 experts, top-2: the kernel path's RMS error against the fp64
    reference is no larger than that of the eager bf16 library path (which rounds the gate/up and down
    products to bf16 where the kernels keep fp32).  RMS, not the maximum: both paths end in the same
    bf16 rounding, which alone decides the largest single error."""
    g = torch.Generator().manual_seed(R)
    E, k, D, F = 8, 2, 512, 512
    h = torch.randn(R, D, generator=g).to(gpu, torch.bfloat16)
    router = torch.randn(E, D, generator=g).to(gpu, torch.bfloat16)
    wgu = (torch.randn(E, 2 * F, D, generator=g) / D ** 0.5).to(gpu, torch.bfloat16)
    wdown = (torch.randn(E, D, F, generator=g) / F ** 0.5).to(gpu, torch.bfloat16)
    live = torch.ones(R, dtype=torch.int32, device=gpu)
    want = _mlp64(h.cpu(), router.cpu(), wgu.cpu(), wdown.cpu(), k)
    got = sops.moe_mlp(h, router, wgu, wdown, k, live, sops.MoeWorkspace(E, k, D, F, gpu))
    eager = sops.moe_mlp_eager(h, router, wgu, wdown, k, live)
    err, err_eager = ((t.cpu().double() - want).pow(2).mean().sqrt().item() for t in (got, eager))
    with capsys.disabled():
        print(f"\nmoe_mlp R={R}: rms error kernels {err:.3e}, eager library path {err_eager:.3e}, rms of the result "
              f"{want.pow(2).mean().sqrt().item():.3e}")
    assert err <= err_eager


ROWS = (1, 16, 17, 64, 128, 256)
SHAPES = {"mixtral-8x7b": (8, 2, 4096, 14336), "mixtral-8x22b": (8, 2, 6144, 16384),
          "qwen3-30b-a3b": (128, 8, 2048, 768)}  # experts, per token, hidden, FFN
# (rule, model) -> K slices of the gate/up GEMM and of the down GEMM at ROWS, recorded from the build of the commit
# before the three rules were merged into one (128 experts are past the limit of the first two: 0)
SPLITS = {
    ("moe_gemm_split", "mixtral-8x7b"): ([2, 1, 1, 1, 1, 1], [14, 4, 4, 4, 4, 4]),
    ("moe_gemm_split", "mixtral-8x22b"): ([2, 1, 1, 1, 1, 1], [8, 2, 2, 2, 2, 2]),
    ("moe_gemm_split", "qwen3-30b-a3b"): ([0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0]),
    ("moe_w4_gemm_split", "mixtral-8x7b"): ([2, 1, 1, 1, 1, 1], [14, 4, 4, 4, 4, 2]),
    ("moe_w4_gemm_split", "mixtral-8x22b"): ([2, 1, 1, 1, 1, 1], [8, 2, 2, 2, 2, 2]),
    ("moe_w4_gemm_split", "qwen3-30b-a3b"): ([0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0]),
    ("moe_fine_gemm_split", "mixtral-8x7b"): ([1, 1, 1, 1, 1, 1], [8, 2, 2, 2, 2, 2]),
    ("moe_fine_gemm_split", "mixtral-8x22b"): ([1, 1, 1, 1, 1, 1], [4, 1, 1, 1, 1, 1]),
    ("moe_fine_gemm_split", "qwen3-30b-a3b"): ([4, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1]),
}


@pytest.mark.gpu
def test_gpu_split_rules_give_the_recorded_slices(gpu):
    """The K slices decide speed only (every exact-GEMM test passes at any of them), so the three rules are held
    to what they gave at the served models' shapes; a shape a kernel does not run gives 0 (K % 512, N % 256,
    K < 512)."""
    for (rule, model), want in SPLITS.items():
        E, k, D, F = SHAPES[model]
        got = ([getattr(sops, rule)(R, k, E, 2 * F, D) for R in ROWS], [getattr(sops, rule)(R, k, E, D, F) for R in ROWS])
        assert got == want, (rule, model)
    assert sops.moe_gemm_split(16, 2, 8, 512, 768) == 0 and sops.moe_w4_gemm_split(16, 2, 8, 384, 1024) == 0
    assert sops.moe_fine_gemm_split(16, 8, 128, 512, 384) == 0


def _mlp_equals_its_steps(gpu, mlp, gemm, workspace, router, wgu, wdown, k, D=512):
    """``mlp(h, router, wgu, wdown, k, live, ws)`` returns the bits of the five public calls it stands for --
    ``moe_route``, ``gemm(x, src_div, W, counts, lists, split)`` with the workspace's split, ``moe_swiglu``, ``gemm``,
    ``moe_combine`` -- composed here on freshly allocated buffers: for one row; for 17 rows (a second, partly
    filled token block) of which row 5 is dead; for the same rows as a column slice whose row stride is no
    multiple of 16 bytes, which the MLP has to copy; and for one row through a workspace that 17 rows went
    through before, none of whose stale rows may be read."""
    wide = torch.randn(17, D + 4, generator=torch.Generator().manual_seed(k)).to(gpu, torch.bfloat16)
    live = torch.ones(17, dtype=torch.int32, device=gpu)
    live[5] = 0

    def steps(h, live):
        topk_e, topk_w, counts, lists = sops.moe_route(h, router, live, k)
        s1, s2 = workspace().split[h.shape[0]]
        a = sops.moe_swiglu(gemm(h, k, wgu, counts, lists, s1), live)
        return sops.moe_combine(gemm(a, 1, wdown, counts, lists, s2), topk_w, live)

    h17 = wide[:, :D].contiguous()
    h1 = h17[:1]
    want17, want1 = steps(h17, live), steps(h1, live[:1])
    assert want17[4].any() and not want17[5].any() and want1.any()
    assert not wide[:, :D].is_contiguous() and wide.stride(0) % 8
    assert torch.equal(mlp(h1, router, wgu, wdown, k, live[:1], workspace()), want1)
    ws = workspace()
    assert torch.equal(mlp(h17, router, wgu, wdown, k, live, workspace()), want17)
    assert torch.equal(mlp(wide[:, :D], router, wgu, wdown, k, live, ws), want17)
    assert torch.equal(mlp(h1, router, wgu, wdown, k, live[:1], ws), want1)


@pytest.mark.gpu
def test_gpu_mlp_equals_its_steps(gpu):
    g = torch.Generator().manual_seed(0)
    E, k, D, F = 8, 2, 512, 512
    router = torch.randn(E, D, generator=g).to(gpu, torch.bfloat16)
    wgu = (torch.randn(E, 2 * F, D, generator=g) / D ** 0.5).to(gpu, torch.bfloat16)
    wdown = (torch.randn(E, D, F, generator=g) / F ** 0.5).to(gpu, torch.bfloat16)
    _mlp_equals_its_steps(gpu, sops.moe_mlp, sops.moe_gemm, lambda: sops.MoeWorkspace(E, k, D, F, gpu), router, wgu, wdown, k)


GPU_KW = dict(device="cuda", max_model_len=512, max_batch=8, num_pages=64)
PROMPTS = [[1, 2, 3, 4, 5, 1, 2, 3, 4, 5, 1, 2, 3], list(range(7, 90))]


@functools.lru_cache(maxsize=None)
def _gpu_case(root):
    """(checkpoint directory, eager greedy tokens) of a tiny Mixtral with hidden 512 and FFN 1024."""
    _, dirs = _tiny_mixtral(root, 512, 1024)
    eager = LLMEngine.from_model(dirs["saved"], use_graphs=False, **GPU_KW)
    sp = SamplingParams(max_tokens=12, temperature=0, ignore_eos=True)
    return dirs["saved"], [o.output_ids for o in eager.generate(PROMPTS, sp)]


@pytest.mark.gpu
@pytest.mark.parametrize("speculative", [0, 3])
def test_gpu_engine_graphs_equal_eager(gpu, tmp_path_factory, speculative):
    """Decode steps -- and with n-gram speculation the verify steps -- in captured graphs emit the eager
    engine's greedy tokens: the MoE MLP reads its routing from device memory only."""
    path, want = _gpu_case(str(tmp_path_factory.getbasetemp() / "moe_gpu"))
    eng = LLMEngine.from_model(path, speculative_ngram=speculative, **GPU_KW)
    eng.capture_graphs()
    got = [o.output_ids for o in eng.generate(PROMPTS, SamplingParams(max_tokens=12, temperature=0, ignore_eos=True))]
    assert got == want and (not speculative or eng.stats["spec_steps"] > 0)


@pytest.mark.gpu
def test_gpu_long_prefill_runs_eagerly_and_small_hidden_is_refused(gpu, tmp_path_factory, monkeypatch):
    path, _ = _gpu_case(str(tmp_path_factory.getbasetemp() / "moe_gpu"))
    calls = []
    eager = sops.moe_mlp_eager
    monkeypatch.setattr(sops, "moe_mlp_eager", lambda h, *a: calls.append(h.shape[0]) or eager(h, *a))
    eng = LLMEngine.from_model(path, use_graphs=False, **GPU_KW)
    out = eng.generate([[5 + i % 100 for i in range(300)]], SamplingParams(max_tokens=2, temperature=0, ignore_eos=True))
    assert len(out[0].output_ids) == 2 and calls == [384, 384]  # 300 tokens in 128-row segments, 2 layers
    dirs, _, _ = _cpu_case(str(tmp_path_factory.getbasetemp() / "moe_cpu"))
    with pytest.raises(ValueError, match="hidden size 256"):
        LLMEngine.from_model(dirs["saved"], **GPU_KW)
