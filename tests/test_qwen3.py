"""Qwen3: the per-head q/k RMSNorm inside the RoPE + cache-write kernel, the loader and the engine."""

import pytest
import torch
from safetensors.torch import load_file, save_file

from dstack_amd.ops import serving as sops
from dstack_amd.serving.engine import LLMEngine, SamplingParams
from dstack_amd.serving.model import ServingLlama, load_spec, rope_tables

E4M3 = torch.float8_e4m3fn
PROMPTS = [[1, 5, 9, 33, 7, 100, 2, 45, 61], [1, 300, 301, 302]]


@pytest.mark.gpu
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "rs_cs"])
@pytest.mark.parametrize("cache_dtype", [torch.bfloat16, E4M3], ids=["bf16", "e4m3"])
@pytest.mark.parametrize("T,H,KVH", [(1, 1, 1), (5, 4, 2), (70, 8, 2)])
def test_gpu_qk_norm_rope_cache_write(gpu, T, H, KVH, cache_dtype, scaled):
    """Every q / k element against fp64 (scales -> norm -> rotation, one rounding): half a bf16 ulp plus 2e-5 of
    the rotation pair (fp32: a 128-term sum <= 128 * 2^-24, halved by the root, a few ulps for rsqrt and the rotation,
    < 1e-5, doubled as ``got`` rounds the fp32 value); v, caches and sentinel bit for bit.  With one token there is
    no zero row and no padding token: they would leave nothing of the partial wave to check."""
    torch.manual_seed(T)
    NH, QK, pages, ks, vs = H + 2 * KVH, H + KVH, 3, 0.5, 2.0
    cos, sin = rope_tables(4096, 128, 1e6, None, gpu)
    x = torch.randn(T, NH, 128, device=gpu) * (2.0 ** (torch.arange(NH, device=gpu) % 5 - 2))[None, :, None]
    pos = torch.randint(0, 4000, (T,), device=gpu, dtype=torch.int32)
    slots = torch.randperm(pages * 64, device=gpu)[:T].int()
    if T > 1:
        x[1, 0], x[2, H], slots[3] = 0, 0, -1
    j = torch.arange(128, device=gpu, dtype=torch.float32)
    qw, kw = 0.5 + j / 128, 1.5 - j / 128
    inp, sc = (x * (300 if scaled else 1)).to(torch.bfloat16).view(T, -1), {}
    if scaled:
        sc = dict(rs=torch.rand(T, device=gpu) * 1e-2 + 1e-3, cs=torch.rand(NH * 128, device=gpu) * 1e-2 + 1e-3)
    xin = ((inp.float() * sc["rs"][:, None] * sc["cs"][None, :]).to(torch.bfloat16) if scaled else inp).view(T, NH, 128)
    bits = torch.uint8 if cache_dtype == E4M3 else torch.int16
    caches = [sops.alloc_cache(pages, KVH, cache_dtype, gpu) for _ in range(3)]
    kc, vc = (t.view(bits).fill_(0x5A) for t in caches[0])  # bit views of the sentinel-filled caches
    got = sops.rope_cache_write(inp.clone(), pos, slots, cos, sin, *caches[0], H, KVH, ks, vs, q_norm=qw, k_norm=kw,
                                eps=1e-6, **sc).view(T, NH, 128)
    xd, w = xin[:, :QK].double(), torch.cat([qw.expand(H, -1), kw.expand(KVH, -1)]).double()
    n = xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + 1e-6) * w
    c, s = cos[pos.long()].double()[:, None], sin[pos.long()].double()[:, None]
    n1, n2 = n[..., :64], n[..., 64:]
    want = torch.cat([n1 * c - n2 * s, n2 * c + n1 * s], -1)
    err = (got[:, :QK].double() - want).abs()
    bound = 2.0 ** -8 * want.abs() + 2e-5 * (n1.abs() + n2.abs()).repeat(1, 1, 2)
    print(f"max err / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert (err <= bound).all()
    assert T == 1 or ((got[1, 0] == 0).all() and (got[2, H] == 0).all())
    assert torch.equal(got[:, QK:], xin[:, QK:])
    page, off = slots[slots >= 0].long() // 64, slots[slots >= 0].long() % 64
    k, v = got[slots >= 0][:, H:QK], got[slots >= 0][:, QK:]
    if cache_dtype == E4M3:
        k, v = (k.float() / ks).clamp(-448, 448).to(E4M3), (v.float() / vs).clamp(-448, 448).to(E4M3)
    assert torch.equal(kc[page, :, off, :], k.contiguous().view(bits)), "k rows of the cache"
    assert torch.equal(vc[page, :, :, off], v.contiguous().view(bits)), "v columns of the cache"
    kc[page, :, off, :] = vc[page, :, :, off] = 0x5A
    assert (kc == 0x5A).all() and (vc == 0x5A).all()
    # without norm weights: the call as it always was (this only guards the dispatch)
    a = sops.rope_cache_write(inp.clone(), pos, slots, cos, sin, *caches[1], H, KVH, ks, vs, q_norm=None, k_norm=None, **sc)
    b = sops.rope_cache_write(inp.clone(), pos, slots, cos, sin, *caches[2], H, KVH, ks, vs, **sc)
    assert torch.equal(a, b) and all(torch.equal(p.view(bits), q.view(bits)) for p, q in zip(caches[1], caches[2]))


def _tiny(tmp_path, family="qwen3"):
    """Two random layers: Qwen3, 4 x 128 attention dims on a hidden size of 256, q/k norm weights off ones; or Llama."""
    import transformers

    common = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_key_value_heads=2, vocab_size=512,
                  max_position_embeddings=1024, rope_theta=1000000.0, eos_token_id=2, bos_token_id=1)
    if family == "qwen3":
        hf = transformers.Qwen3ForCausalLM(transformers.Qwen3Config(num_attention_heads=4, head_dim=128, **common))
    else:
        hf = transformers.LlamaForCausalLM(transformers.LlamaConfig(num_attention_heads=2, **common))
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for name, p in hf.named_parameters():
            if p.dim() == 2:
                p.normal_(0, 0.08, generator=g)
            elif "_norm.weight" in name:
                p.uniform_(0.5, 1.5, generator=g)
    hf.eval().save_pretrained(str(tmp_path / family))
    return hf, str(tmp_path / family)


def test_qwen3_hf_parity_and_loader(tmp_path):
    hf, path = _tiny(tmp_path)
    spec = load_spec(path)
    assert (spec.family, spec.qk_norm, spec.qkv_bias, spec.head_dim) == ("qwen3", True, False, 128)
    eng = LLMEngine.from_model(path, device="cpu", max_model_len=256, max_batch=4, num_pages=32)
    outs = eng.generate(PROMPTS, SamplingParams(max_tokens=10, temperature=0, ignore_eos=True))
    for p, r in zip(PROMPTS, outs):
        with torch.no_grad():
            ref = hf.generate(torch.tensor([p]), max_new_tokens=10, do_sample=False, eos_token_id=None, pad_token_id=0)
        assert r.output_ids == ref[0, len(p):].tolist()
    sd = load_file(f"{path}/model.safetensors")
    w = sd.pop(name := "model.layers.0.self_attn.k_norm.weight")
    save_file(sd, f"{path}/model.safetensors")
    with pytest.raises(ValueError, match="missing 1 tensors"):
        ServingLlama(spec, "cpu").load_hf()
    _, llama = _tiny(tmp_path, "llama")
    save_file({**load_file(f"{llama}/model.safetensors"), name: w}, f"{llama}/model.safetensors")
    with pytest.raises(ValueError, match=f"unexpected tensor {name}"):
        ServingLlama(load_spec(llama), "cpu").load_hf()


@pytest.mark.gpu
@pytest.mark.parametrize("quantization", [None, "fp8"])
@pytest.mark.parametrize("kv_cache_dtype", ["auto", "fp8"])
def test_gpu_qwen3_engine_graphs_match_eager(gpu, tmp_path, kv_cache_dtype, quantization):
    """Greedy tokens of captured decode graphs equal the eager engine's.  fp8: the 300-token prompt's
    prefill (past ``fp8_defer_rows``) hands the raw qkv product and its scales to the norm form."""
    _, path = _tiny(tmp_path)
    prompts, outs = PROMPTS + [[1 + i % 500 for i in range(300)]], []
    for graphs in (True, False):
        eng = LLMEngine.from_model(path, device="cuda", max_model_len=512, max_batch=8, num_pages=64, use_graphs=graphs,
                                   kv_cache_dtype=kv_cache_dtype, quantization=quantization)
        eng.model.fp8_defer_rows = 128
        if graphs:
            eng.capture_graphs()
        assert bool(eng._graphs) == graphs
        outs.append([r.output_ids for r in eng.generate(prompts, SamplingParams(max_tokens=12, temperature=0, ignore_eos=True))])
    assert outs[0] == outs[1]
