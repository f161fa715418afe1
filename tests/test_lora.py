"""Multi-LoRA serving: the PEFT adapter loader, parity of the engine with HF models that have the
adapters merged into their weights (mixed batches of adapters and the base model, preemption,
prefix caching), the HTTP surface (CPU), and the batched LoRA kernels and the graph-captured decode
step with adapters (GPU).

Parity source: ``transformers.LlamaForCausalLM`` with ``W + (alpha / r) B A`` merged in fp32 -- what
``peft``'s ``merge_and_unload`` computes (peft is not installed and is not needed)."""

import copy
import json
import math

import pytest
import torch

from dstack_amd.ops import serving as sops
from dstack_amd.serving.engine import LLMEngine, SamplingParams
from dstack_amd.serving.lora import TARGETS, parse_lora_modules, read_adapter
from dstack_amd.serving.model import ServingLlama, load_spec

ALL = tuple(TARGETS)
_HF_PARENT = {"q_proj": "self_attn", "k_proj": "self_attn", "v_proj": "self_attn", "o_proj": "self_attn",
              "gate_proj": "mlp", "up_proj": "mlp", "down_proj": "mlp"}


def _shapes(dim, heads, kv_heads, ffn):
    return {"q_proj": (heads * 128, dim), "k_proj": (kv_heads * 128, dim), "v_proj": (kv_heads * 128, dim),
            "o_proj": (dim, heads * 128), "gate_proj": (ffn, dim), "up_proj": (ffn, dim), "down_proj": (dim, ffn)}


TINY = _shapes(256, 2, 1, 512)  # the _hf_tiny recipe
LLAMA_TINY = _shapes(512, 4, 2, 1024)  # the built-in llama-tiny config


def _write_adapter(path, shapes, rank, seed, targets=ALL, layers=2, std=0.08, tensors=None, **cfg):
    """A PEFT adapter directory with A, B ~ N(0, std) and lora_alpha = 2 r; returns its tensors
    ``{(layer, target): (A, B)}``.  ``cfg`` overrides adapter_config.json fields."""
    from safetensors.torch import save_file

    g = torch.Generator().manual_seed(seed)
    out, sd = {}, {}
    for i in range(layers):
        for t in targets:
            o, k = shapes[t]
            a = torch.randn(rank, k, generator=g) * std
            b = torch.randn(o, rank, generator=g) * std
            out[(i, t)] = (a, b)
            base = f"base_model.model.model.layers.{i}.{_HF_PARENT[t]}.{t}"
            sd[f"{base}.lora_A.weight"] = a
            sd[f"{base}.lora_B.weight"] = b
    if tensors is not None:
        tensors(sd)
    path.mkdir(parents=True, exist_ok=True)
    save_file(sd, str(path / "adapter_model.safetensors"))
    conf = dict(peft_type="LORA", r=rank, lora_alpha=2 * rank, target_modules=list(targets), bias="none",
                use_rslora=False, use_dora=False, fan_in_fan_out=False, modules_to_save=None, rank_pattern={},
                alpha_pattern={}, lora_dropout=0.05, task_type="CAUSAL_LM")
    conf.update(cfg)
    (path / "adapter_config.json").write_text(json.dumps(conf))
    return out


def _hf_tiny(tmp_path):
    transformers = pytest.importorskip("transformers")
    cfg = transformers.LlamaConfig(
        hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1,
        vocab_size=512, max_position_embeddings=1024, rope_theta=500000.0, head_dim=128, eos_token_id=2,
        bos_token_id=1)
    torch.manual_seed(0)
    m = transformers.LlamaForCausalLM(cfg).eval()
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 2:
                p.normal_(0, 0.08)
    path = tmp_path / "hf"
    m.save_pretrained(str(path))
    return m, str(path)


def _merged(hf, tensors, scale=2.0):
    """A copy of ``hf`` with W + scale * B A (fp32) in place of every adapted weight."""
    m = copy.deepcopy(hf)
    with torch.no_grad():
        for (i, t), (a, b) in tensors.items():
            w = getattr(getattr(m.model.layers[i], _HF_PARENT[t]), t).weight
            w.add_(scale * (b.float() @ a.float()))
    return m


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    """The tiny HF model, the two adapters of the parity tests (rank 8 seed 1, rank 16 seed 2, all
    seven targets) and the HF models with each merged in.  Shared and never modified."""
    tmp = tmp_path_factory.mktemp("lora")
    hf, path = _hf_tiny(tmp)
    t0 = _write_adapter(tmp / "a0", TINY, 8, 1)
    t1 = _write_adapter(tmp / "a1", TINY, 16, 2)
    mods = {"a0": str(tmp / "a0"), "a1": str(tmp / "a1")}
    return dict(hf=hf, path=path, mods=mods, merged={None: hf, "a0": _merged(hf, t0), "a1": _merged(hf, t1)},
                tensors={"a0": t0, "a1": t1})


PROMPTS = [[1, 5, 9, 33, 7, 100, 2, 45, 61], [1, 300, 301, 302]]


def _hf_greedy(hf, p, n):
    with torch.no_grad():
        return hf.generate(torch.tensor([p]), max_new_tokens=n, do_sample=False, eos_token_id=None,
                           pad_token_id=0)[0, len(p):].tolist()


# ------------------------------------------------------------------------------------------------
# 1. loader
# ------------------------------------------------------------------------------------------------
def _model(path="llama-tiny"):
    m = ServingLlama(load_spec(path), "cpu", max_model_len=256)
    m.init_random(0) if path == "llama-tiny" else m.load_hf()
    return m


def test_loader_roundtrip_slices_padding_and_scaling(tmp_path):
    m = _model().enable_lora(3, 16)
    assert m.lora_rank == 16
    t = _write_adapter(tmp_path / "a", LLAMA_TINY, 8, 3)
    before = m.weight_bytes()
    m.load_lora(1, str(tmp_path / "a"))
    assert m.weight_bytes() == before  # the stacks are counted from enable_lora on
    per_slot = 16 * sum(o + k for o, k in LLAMA_TINY.values()) * 2 * 4  # R * (in + out) per target, 2 layers, fp32
    assert before - _model().weight_bytes() == 3 * per_slot
    H, KVH, F, R = 4 * 128, 2 * 128, 1024, 16
    for i in range(2):
        A, B = m.lora[i]["wqkv"]
        assert A.shape == (3, 3 * R, 512) and B.shape == (3, H + 2 * KVH, R)
        for j, (name, lo, hi) in enumerate([("q_proj", 0, H), ("k_proj", H, H + KVH), ("v_proj", H + KVH, H + 2 * KVH)]):
            a, b = t[(i, name)]
            assert torch.equal(A[1, j * R : j * R + 8], a) and not A[1, j * R + 8 : (j + 1) * R].any()
            assert torch.equal(B[1, lo:hi, :8], b * 2.0) and not B[1, lo:hi, 8:].any()
        A, B = m.lora[i]["wgu"]
        assert A.shape == (3, 2 * R, 512) and B.shape == (3, 2 * F, R)
        for j, name in enumerate(["gate_proj", "up_proj"]):
            a, b = t[(i, name)]
            assert torch.equal(A[1, j * R : j * R + 8], a) and torch.equal(B[1, j * F : (j + 1) * F, :8], b * 2.0)
        for key, name in (("wo", "o_proj"), ("wdown", "down_proj")):
            A, B = m.lora[i][key]
            a, b = t[(i, name)]
            assert torch.equal(A[1, :8], a) and torch.equal(B[1, :, :8], b * 2.0) and not A[1, 8:].any()
        for A, B in m.lora[i].values():  # the other slots stay empty
            assert not A[0].any() and not A[2].any() and not B[0].any() and not B[2].any()


def test_loader_rslora_and_target_subset(tmp_path):
    m = _model().enable_lora(1, 8)
    t = _write_adapter(tmp_path / "a", LLAMA_TINY, 8, 4, targets=("q_proj", "down_proj"), use_rslora=True)
    m.load_lora(0, str(tmp_path / "a"))
    scale = 16 / math.sqrt(8)
    for i in range(2):
        a, b = t[(i, "q_proj")]
        A, B = m.lora[i]["wqkv"]
        assert torch.equal(A[0, :8], a) and torch.equal(B[0, :512], b * scale)
        assert not A[0, 8:].any() and not B[0, 512:].any()  # k and v: absent, zero
        assert torch.equal(m.lora[i]["wdown"][1][0], t[(i, "down_proj")][1] * scale)
        for key in ("wo", "wgu"):
            assert not m.lora[i][key][0].any() and not m.lora[i][key][1].any()
    # loading another adapter into the slot replaces all of it
    _write_adapter(tmp_path / "b", LLAMA_TINY, 4, 5, targets=("o_proj",))
    m.load_lora(0, str(tmp_path / "b"))
    assert not m.lora[0]["wqkv"][0].any() and m.lora[0]["wo"][0][0, :4].any() and not m.lora[0]["wo"][0][0, 4:].any()


def _drop(name):
    return lambda sd: sd.pop(name)


Q0 = "base_model.model.model.layers.0.self_attn.q_proj"


@pytest.mark.parametrize("match,kw", [
    ("peft_type", dict(peft_type="IA3")),
    ("use_dora", dict(use_dora=True)),
    ("bias", dict(bias="all")),
    ("modules_to_save", dict(modules_to_save=["lm_head"])),
    ("rank_pattern", dict(rank_pattern={"q_proj": 4})),
    ("alpha_pattern", dict(alpha_pattern={"q_proj": 4})),
    ("fan_in_fan_out", dict(fan_in_fan_out=True)),
    ("target_modules", dict(target_modules=["q_proj", "embed_tokens"])),
    ("target_modules", dict(target_modules=["lm_head"])),
    ("max_lora_rank 16", dict(rank=32)),
    ("has shape", dict(shapes=dict(LLAMA_TINY, q_proj=(512, 256)))),
    ("has shape", dict(shapes=dict(LLAMA_TINY, down_proj=(256, 1024)))),
    ("unexpected tensor", dict(tensors=lambda sd: sd.update({"base_model.model.lm_head.lora_A.weight": torch.zeros(8, 512)}))),
    ("unexpected tensor", dict(layers=3)),
    ("other half", dict(tensors=_drop(Q0 + ".lora_B.weight"))),
    ("other half", dict(tensors=_drop(Q0 + ".lora_A.weight"))),
])
def test_loader_rejections(tmp_path, match, kw):
    m = _model().enable_lora(1, 16)
    kw = dict(kw)
    shapes, rank = kw.pop("shapes", LLAMA_TINY), kw.pop("rank", 8)
    _write_adapter(tmp_path / "a", shapes, rank, 6, **kw)
    with pytest.raises(ValueError, match=match):
        m.load_lora(0, str(tmp_path / "a"))


def test_loader_needs_both_files_and_cli_option(tmp_path):
    with pytest.raises(ValueError, match="adapter_config.json"):
        read_adapter(str(tmp_path), 2, LLAMA_TINY, 16)
    assert parse_lora_modules(["a=/x", "b=/y=z"]) == {"a": "/x", "b": "/y=z"}
    for bad in (["a"], ["=x"], ["a=/x", "a=/y"]):
        with pytest.raises(ValueError, match="lora-modules"):
            parse_lora_modules(bad)
    with pytest.raises(ValueError, match="max_lora_rank"):
        _model().enable_lora(1, 128)


def test_lora_refused_with_fp8_and_tensor_parallel(tmp_path):
    _write_adapter(tmp_path / "a", LLAMA_TINY, 8, 1)
    mods = {"a": str(tmp_path / "a")}
    with pytest.raises(ValueError, match="quantization=\"fp8\""):
        LLMEngine.from_model("llama-tiny", device="cpu", quantization="fp8", lora_modules=mods)
    with pytest.raises(ValueError, match="tensor parallel"):
        LLMEngine.from_model("llama-tiny", device="cpu", tp_group=object(), lora_modules=mods)
    m = ServingLlama(load_spec("llama-tiny"), "cpu", quantization="fp8")
    with pytest.raises(ValueError, match="quantization=\"fp8\""):
        m.enable_lora(1, 8)
    # an fp8 KV cache is fine
    eng = LLMEngine.from_model("llama-tiny", device="cpu", kv_cache_dtype="fp8", max_model_len=256, max_batch=4,
                               num_pages=16, lora_modules=mods)
    out = eng.generate([[1, 2, 3]], SamplingParams(max_tokens=3, temperature=0), lora="a")
    assert len(out[0].output_ids) == 3
    with pytest.raises(ValueError, match="unknown LoRA adapter"):
        eng.add_request([1, 2, 3], lora="nope")


# ------------------------------------------------------------------------------------------------
# 2. parity with merged weights
# ------------------------------------------------------------------------------------------------
def test_reference_kernels_match_merged_matmul():
    """The CPU references of the two kernels against one dense matmul with the merged update."""
    g = torch.Generator().manual_seed(0)
    S, R, K, ends = 3, 8, 64, (32, 48, 64)
    x = torch.randn(5, K, generator=g)
    A = torch.randn(S, 3 * R, K, generator=g)
    B = torch.randn(S, 64, R, generator=g)
    y0 = torch.randn(5, 64, generator=g)
    idx = torch.tensor([0, -1, 2, 2, 1], dtype=torch.int32)
    t = sops.lora_shrink(x, A, idx)
    y = sops.lora_expand(t, B, idx, ends, y0.clone())
    z = y0.clone()
    sops.lora_runs(x, A, B, [(0, 0, 1), (2, 2, 4), (1, 4, 5)], ends, z)
    for r, s in enumerate(idx.tolist()):
        if s < 0:
            assert torch.equal(y[r], y0[r]) and not t[r].any()
            continue
        want, lo = y0[r].clone(), 0
        for j, hi in enumerate(ends):
            want[lo:hi] += B[s, lo:hi] @ (A[s, j * R : (j + 1) * R] @ x[r])
            lo = hi
        torch.testing.assert_close(y[r], want, atol=1e-4, rtol=1e-5)
        torch.testing.assert_close(z[r], want, atol=1e-4, rtol=1e-5)


def _prefill_two(m, lora_idx):
    toks = torch.zeros(256, dtype=torch.int64)
    toks[:9] = torch.tensor(PROMPTS[0])
    toks[128:132] = torch.tensor(PROMPTS[1])
    pos = torch.cat([torch.arange(128), torch.arange(128)]).int()
    pos[9:128] = 0
    pos[132:] = 0
    slots = torch.full((256,), -1, dtype=torch.int32)
    slots[:9] = torch.arange(9)
    slots[128:132] = torch.arange(4) + 64
    return m.prefill(toks, pos, slots, [0, 128], [9, 4], lora_idx=lora_idx)


def test_hf_parity_with_merged_adapters(tiny):
    eng = LLMEngine.from_model(tiny["path"], device="cpu", max_model_len=512, max_batch=8, num_pages=64,
                               lora_modules=tiny["mods"], max_lora_rank=16)
    assert eng.lora_slots == {"a0": 0, "a1": 1} and eng.model.lora_rank == 16
    merged = tiny["merged"]
    # prefill logits: (adapter of prompt 0, adapter of prompt 1) in one packed call
    for n0, n1 in [("a0", "a1"), ("a1", None), (None, "a0"), ("a1", "a1")]:
        idx = torch.full((256,), -1, dtype=torch.int32)
        idx[:128] = eng.lora_slots.get(n0, -1)
        idx[128:] = eng.lora_slots.get(n1, -1)
        logits = _prefill_two(eng.model, idx)
        with torch.no_grad():
            for i, (p, name) in enumerate(zip(PROMPTS, (n0, n1))):
                want = merged[name](torch.tensor([p])).logits[0, -1]
                torch.testing.assert_close(logits[i], want, atol=2e-4, rtol=2e-4)
    # greedy decode: each adapter and the base, both prompts, in one batch (slots 0, 1 and -1 mixed)
    names = ["a0", "a1", None]
    prompts = [p for _ in names for p in PROMPTS]
    lora = [n for n in names for _ in PROMPTS]
    outs = eng.generate(prompts, SamplingParams(max_tokens=12, temperature=0, ignore_eos=True), lora=lora)
    got = {(r.lora, tuple(r.prompt_ids)): r.output_ids for r in outs}
    for name in names:
        for p in PROMPTS:
            assert got[(name, tuple(p))] == _hf_greedy(merged[name], p, 12), (name, p)
            if name is not None:  # the precondition: the adapter changes the very first token
                assert got[(name, tuple(p))][0] != got[(None, tuple(p))][0], (name, p)
    assert eng.lora_requests == {"a0": 2, "a1": 2}


# ------------------------------------------------------------------------------------------------
# 3. preemption
# ------------------------------------------------------------------------------------------------
def test_engine_preemption_with_adapters_keeps_greedy_outputs(tmp_path):
    _write_adapter(tmp_path / "a", LLAMA_TINY, 8, 1)
    _write_adapter(tmp_path / "b", LLAMA_TINY, 16, 2, targets=("q_proj", "v_proj", "down_proj"))
    mods = {"a": str(tmp_path / "a"), "b": str(tmp_path / "b")}
    kw = dict(device="cpu", max_model_len=256, max_batch=8, lora_modules=mods, max_lora_rank=16)
    prompts = [[1 + i, 2, 3, 4 + i] * (5 + i) for i in range(4)]
    lora = ["a", None, "b", "a"]
    sp = SamplingParams(max_tokens=60, temperature=0, ignore_eos=True)
    big = LLMEngine.from_model("llama-tiny", num_pages=64, **kw).generate(prompts, sp, lora=lora)
    small_eng = LLMEngine.from_model("llama-tiny", num_pages=5, **kw)
    small = small_eng.generate(prompts, sp, lora=lora)
    assert small_eng.stats["preemptions"] > 0
    assert [r.output_ids for r in small] == [r.output_ids for r in big]
    base = LLMEngine.from_model("llama-tiny", num_pages=64, device="cpu", max_model_len=256, max_batch=8)
    plain = base.generate(prompts, sp)
    assert plain[1].output_ids == big[1].output_ids  # the base-model row of the mixed batch
    assert all(plain[i].output_ids != big[i].output_ids for i in (0, 2, 3))


# ------------------------------------------------------------------------------------------------
# 4. prefix caching never shares KV across adapters (the scheduler side: test_prefix_cache_salt.py)
# ------------------------------------------------------------------------------------------------
def test_prefix_cache_is_per_adapter(tiny):
    eng = LLMEngine.from_model(tiny["path"], device="cpu", max_model_len=512, max_batch=8, num_pages=64,
                               lora_modules=tiny["mods"], max_lora_rank=16, enable_prefix_caching=True)
    p = list(range(1, 200))  # three full pages
    sp = SamplingParams(max_tokens=6, temperature=0, ignore_eos=True)
    for name, cached in [(None, 0), ("a0", 0), ("a1", 0), ("a0", 192), (None, 192), ("a1", 192)]:
        r = eng.generate([p], sp, lora=name)[0]
        assert r.cached_tokens == cached, (name, r.cached_tokens)
        assert r.output_ids == _hf_greedy(tiny["merged"][name], p, 6), name


# ------------------------------------------------------------------------------------------------
# 5. HTTP API
# ------------------------------------------------------------------------------------------------
def test_api_routes_by_model_name(tmp_path):
    from fastapi.testclient import TestClient

    from dstack_amd.serving.server import create_app

    _write_adapter(tmp_path / "a", LLAMA_TINY, 8, 1)
    _write_adapter(tmp_path / "b", LLAMA_TINY, 8, 2)
    eng = LLMEngine.from_model("llama-tiny", device="cpu", max_model_len=256, max_batch=8, num_pages=32,
                               lora_modules={"sql": str(tmp_path / "a"), "chat-ft": str(tmp_path / "b")})
    body = {"prompt": [1, 2, 3, 4, 5], "max_tokens": 8, "temperature": 0, "ignore_eos": True, "logprobs": 0}
    with TestClient(create_app(eng, served_model_name="llama-tiny")) as api:
        models = api.get("/v1/models").json()["data"]
        assert [m["id"] for m in models] == ["llama-tiny", "sql", "chat-ft"]
        assert "parent" not in models[0] and models[1]["parent"] == models[2]["parent"] == "llama-tiny"
        base = api.post("/v1/completions", json=dict(body, model="llama-tiny")).json()
        sql = api.post("/v1/completions", json=dict(body, model="sql")).json()
        ft = api.post("/v1/completions", json=dict(body, model="chat-ft")).json()
        assert (base["model"], sql["model"], ft["model"]) == ("llama-tiny", "sql", "chat-ft")
        toks = [r["choices"][0]["logprobs"]["tokens"] for r in (base, sql, ft)]
        assert toks[0] != toks[1] and toks[0] != toks[2] and toks[1] != toks[2]
        assert api.post("/v1/completions", json=dict(body)).json()["choices"][0]["logprobs"]["tokens"] == toks[0]
        chat = api.post("/v1/chat/completions", json={"model": "sql", "max_tokens": 2, "temperature": 0,
                                                      "messages": [{"role": "user", "content": "hi"}]})
        assert chat.status_code == 200 and chat.json()["model"] == "sql"
        for route, extra in (("/v1/completions", {"prompt": [1, 2]}),
                             ("/v1/chat/completions", {"messages": [{"role": "user", "content": "hi"}]})):
            r = api.post(route, json=dict(extra, model="nope"))
            assert r.status_code == 404 and r.json()["error"]["code"] == "model_not_found"
        metrics = api.get("/metrics").text
    assert 'dstack_serving_lora_requests_total{adapter="sql"} 2' in metrics
    assert 'dstack_serving_lora_requests_total{adapter="chat-ft"} 1' in metrics


# ------------------------------------------------------------------------------------------------
# GPU: the kernels
# ------------------------------------------------------------------------------------------------
IDX = [0, -1, 2, 2, 1]


def _rel(got, want):
    return ((got.double() - want).norm() / want.norm()).item()


@pytest.mark.gpu
@pytest.mark.parametrize("K,nsl,R", [(256, 3, 8), (4096, 2, 64), (28672, 1, 64), (4104, 1, 16)])
def test_gpu_lora_shrink_matches_fp64(gpu, K, nsl, R):
    """bf16 inputs, x with a padded row stride, fp32 output against an fp64 matmul: K below one
    512-column wave step, a K of several steps per wave, and a K that is no multiple of 512.
    Bound 1e-5: strictly sequential fp32 accumulation, the worst order, gives 2.2e-6 at K = 28672;
    a single dropped 8-column chunk gives 1.5e-2."""
    g = torch.Generator(device=gpu).manual_seed(K + R)
    S, L, T = 3, nsl * R, len(IDX)
    x = torch.randn(T, K + 64, device=gpu, generator=g).to(torch.bfloat16)[:, :K]
    A = (torch.randn(S, L, K, device=gpu, generator=g) * 0.02).to(torch.bfloat16)
    idx = torch.tensor(IDX, dtype=torch.int32, device=gpu)
    t = torch.full((T, L), 123.0, device=gpu)
    assert sops.lora_shrink(x, A, idx, out=t) is t
    live = [r for r, s in enumerate(IDX) if s >= 0]
    want = torch.stack([x[r].double().cpu() @ A[IDX[r]].double().cpu().t() for r in live])
    err = _rel(t[live].cpu(), want)
    print(f"shrink K={K} nsl={nsl} R={R}: rel err {err:.3e}")
    assert err < 1e-5, err
    assert bool((t[1] == 123.0).all())  # the row without an adapter is not written
    torch.testing.assert_close(sops.lora_shrink_ref(x, A, idx)[live].cpu(), want.float(), atol=1e-3, rtol=1e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("zero_y", [True, False])
@pytest.mark.parametrize("N,ends,R", [(512, (256, 384, 512), 8), (1024, (512, 1024), 64), (8192, (8192,), 16)])
def test_gpu_lora_expand_matches_fp64(gpu, N, ends, R, zero_y):
    """t ~ N(0, 1), B ~ N(0, 1/64): the delta and y0 ~ N(0, 1) have comparable norms.  Bound 5e-3
    (that of test_gemv_matches_fp32) against float(y0) + delta in fp64: one correct bf16 rounding
    measures 1.6e-3, a missing delta 0.69.  Rows without an adapter stay bitwise."""
    g = torch.Generator(device=gpu).manual_seed(N + R)
    S, T, nsl = 3, len(IDX), len(ends)
    t = torch.randn(T, nsl * R, device=gpu, generator=g)
    B = (torch.randn(S, N, R, device=gpu, generator=g) / 8).to(torch.bfloat16)
    y0 = torch.randn(T, N, device=gpu, generator=g).to(torch.bfloat16)
    if zero_y:
        y0.zero_()
    idx = torch.tensor(IDX, dtype=torch.int32, device=gpu)
    y = y0.clone()
    assert sops.lora_expand(t, B, idx, ends, y) is y
    live = [r for r, s in enumerate(IDX) if s >= 0]
    want = []
    for r in live:
        w, lo = y0[r].double().cpu(), 0
        for j, hi in enumerate(ends):
            w[lo:hi] += B[IDX[r], lo:hi].double().cpu() @ t[r, j * R : (j + 1) * R].double().cpu()
            lo = hi
        want.append(w)
    err = _rel(y[live].cpu(), torch.stack(want))
    print(f"expand N={N} R={R} zero_y={zero_y}: rel err {err:.3e}")
    assert err < 5e-3, err
    assert torch.equal(y[1], y0[1])
    ref = sops.lora_expand_ref(t, B, idx, ends, y0)
    assert _rel(ref[live].cpu(), torch.stack(want)) < 5e-3 and torch.equal(ref[1], y0[1])


@pytest.mark.gpu
def test_gpu_lora_kernels_are_bitwise_deterministic(gpu):
    g = torch.Generator(device=gpu).manual_seed(0)
    T, S, K, R, ends = 64, 3, 4096, 16, (4096, 5120, 6144)
    x = torch.randn(T, K, device=gpu, generator=g).to(torch.bfloat16)
    A = (torch.randn(S, 3 * R, K, device=gpu, generator=g) * 0.02).to(torch.bfloat16)
    B = (torch.randn(S, ends[-1], R, device=gpu, generator=g) / 8).to(torch.bfloat16)
    idx = (torch.arange(T, device=gpu) % (S + 1) - 1).to(torch.int32)  # -1, 0, 1, 2, -1, ...
    y0 = torch.randn(T, ends[-1], device=gpu, generator=g).to(torch.bfloat16)
    t1, t2 = (sops.lora_shrink(x, A, idx, out=torch.zeros(T, 3 * R, device=gpu)) for _ in range(2))
    assert torch.equal(t1, t2) and bool(t1[1].any()) and not bool(t1[0].any())
    y1, y2 = (sops.lora_expand(t1, B, idx, ends, y0.clone()) for _ in range(2))
    assert torch.equal(y1, y2) and not torch.equal(y1, y0)


# ------------------------------------------------------------------------------------------------
# GPU: the engine on the HIP path
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_engine_with_adapters_matches_graphs_and_merged_hf(gpu, tiny):
    """Base, adapter 0 and adapter 1 over three prompts in one batch: hipGraph and eager steps give
    the same tokens, every first token is its merged fp32 HF model's argmax up to bf16 near-ties,
    and a base-only batch on the adapter-loaded engine replays the plain graphs: the tokens of an
    engine built without adapters."""
    prompts3 = [[1, 5, 9, 33, 7, 100, 2, 45, 61], [1, 300, 301, 302], list(range(1, 200))]
    names = [None, "a0", "a1"]
    prompts = [p for _ in names for p in prompts3]
    lora = [n for n in names for _ in prompts3]
    sp = SamplingParams(max_tokens=20, temperature=0, ignore_eos=True)
    kw = dict(device="cuda", max_model_len=512, max_batch=16, num_pages=96)
    g = LLMEngine.from_model(tiny["path"], lora_modules=tiny["mods"], max_lora_rank=16, **kw)
    g.capture_graphs()
    assert set(g._graphs) == set(g.buckets) | {(b, "lora") for b in g.buckets}
    out_g = [r.output_ids for r in g.generate(prompts, sp, lora=lora)]
    ng = LLMEngine.from_model(tiny["path"], lora_modules=tiny["mods"], max_lora_rank=16, use_graphs=False, **kw)
    out_ng = [r.output_ids for r in ng.generate(prompts, sp, lora=lora)]
    assert out_g == out_ng
    with torch.no_grad():
        for p, n, o in zip(prompts, lora, out_g):
            ref = tiny["merged"][n](torch.tensor([p])).logits[0, -1]
            assert ref[o[0]] >= ref.max() - 0.02 * (ref.max() - ref.min()), (n, p[:4])
    assert out_g[:3] != out_g[3:6] and out_g[:3] != out_g[6:]
    # the plain-graph rule
    plain = LLMEngine.from_model(tiny["path"], **kw)
    plain.capture_graphs()
    assert set(plain._graphs) == set(plain.buckets)
    want = [r.output_ids for r in plain.generate(prompts3, sp)]
    assert [r.output_ids for r in g.generate(prompts3, sp)] == want
