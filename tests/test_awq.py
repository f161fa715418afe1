"""AWQ 4-bit checkpoints (``--quantization awq``): the AutoAWQ "GEMM" packing, the canonical and the
stored layout, the min/max quantizer of the built-in models, the W4A16 decode GEMM and dequantizer
(``ops/csrc/w4.hip``), the checkpoint loader and the engine built on them."""

import functools
import json

import pytest
import torch

from dstack_amd.ops import reference as ref
from dstack_amd.ops import serving as sops
from dstack_amd.serving.engine import LLMEngine, SamplingParams
from dstack_amd.serving.model import Awq4Weight, ServingLlama, load_spec

ORDER = [0, 2, 4, 6, 1, 3, 5, 7]


def pack_awq(ints: torch.Tensor) -> torch.Tensor:
    """AutoAWQ's ``WQLinear_GEMM.from_linear`` packing loop on an integer matrix [rows, cols] (values
    0..15): dword ``col`` of a row ORs ``ints[:, col * 8 + order_map[i]] << (i * 4)`` for i = 0..7.
    Done in int64 and wrapped to int32 (a nibble of 8 or more in position 7 sets the sign bit)."""
    rows, cols = ints.shape
    out = torch.zeros(rows, cols // 8, dtype=torch.int64)
    for col in range(cols // 8):
        for i in range(8):
            out[:, col] |= ints[:, col * 8 + ORDER[i]].to(torch.int64) << (i * 4)
    return ((out + 2 ** 31) % 2 ** 32 - 2 ** 31).to(torch.int32)


def _random_layer(K, N, g, seed):
    gen = torch.Generator().manual_seed(seed)
    q = torch.randint(0, 16, (K, N), generator=gen)
    z = torch.randint(0, 16, (K // g, N), generator=gen)
    s = (torch.rand(K // g, N, generator=gen) * 0.015 + 0.005).to(torch.float16)
    return q, z, s


# ------------------------------------------------------------------------------------------------
# packing
# ------------------------------------------------------------------------------------------------
def test_unpack_hand_check_and_negative_dwords():
    # 0x75316420: nibbles 0, 2, 4, 6, 1, 3, 5, 7 from the low end -> columns 0..7 hold 0..7
    qw = torch.tensor([[0x75316420]], dtype=torch.int32).repeat(2, 1)  # K = 2 rows
    qz = torch.tensor([[0x75316420]], dtype=torch.int32)
    codes, zeros, scales = ref.unpack_awq(qw, qz, torch.ones(1, 8, dtype=torch.float16))
    assert codes.shape == (8, 1) and zeros.shape == (8, 1) and scales.shape == (8, 1)
    assert codes[:, 0].tolist() == [n | (n << 4) for n in range(8)]  # k = 0 low nibble, k = 1 high nibble
    assert zeros[:, 0].tolist() == list(range(8))
    # a dword with its sign bit set: nibble 7 (column 7) is 0xF, nibble 3 (column 6) is 0x8
    neg = torch.tensor([[-(2 ** 31) + 0x70008000]], dtype=torch.int32).repeat(2, 1)  # 0xF0008000
    assert int(neg[0, 0]) < 0
    codes, _, _ = ref.unpack_awq(neg, qz, torch.ones(1, 8, dtype=torch.float16))
    assert (codes[:, 0] & 15).tolist() == [0, 0, 0, 0, 0, 0, 8, 15]
    assert pack_awq(torch.tensor([[0, 0, 0, 0, 0, 0, 8, 15]]))[0, 0] == neg[0, 0]  # the packer agrees


@pytest.mark.parametrize("K,N,g", [(128, 8, 32), (512, 1024, 128), (1024, 512, 64)])
def test_unpack_inverts_the_autoawq_packer(K, N, g):
    q, z, s = _random_layer(K, N, g, seed=K + N)
    codes, zeros, scales = ref.unpack_awq(pack_awq(q), pack_awq(z), s)
    assert codes.dtype == zeros.dtype == torch.uint8 and scales.dtype == torch.float16
    nib = torch.stack([codes & 15, codes >> 4], dim=-1).reshape(N, K)
    assert torch.equal(nib.long(), q.t()) and torch.equal(zeros.long(), z.t()) and torch.equal(scales, s.t())
    w = ref.dequant_w4(codes, zeros, scales, g)
    want = (q.t() - z.t().repeat_interleave(g, dim=1)).float() * s.t().float().repeat_interleave(g, dim=1)
    assert w.dtype == torch.float32 and torch.equal(w, want)
    with pytest.raises(ValueError, match="unpack_awq"):
        ref.unpack_awq(pack_awq(q), pack_awq(z)[:, :-1], s)


# ------------------------------------------------------------------------------------------------
# quantizer and dequantizer
# ------------------------------------------------------------------------------------------------
def _group(vals, g=32):
    x = torch.empty(1, g)
    x[0] = torch.tensor(vals, dtype=torch.float32).repeat(g // len(vals) + 1)[:g]
    return x


def test_quantizer_on_hand_made_groups():
    # a constant group: s = 1, z = 0, q = clamp(round(w), 0, 15) -- 3.2 -> 3 (not 0), -2 -> 0, 40 -> 15
    for val, q in ((3.2, 3), (-2.0, 0), (40.0, 15), (0.0, 0)):
        c, z, s = ref.quant_w4(_group([val]), 32)
        assert float(s[0, 0]) == 1.0 and int(z[0, 0]) == 0 and (c == (q | (q << 4))).all(), val
    # a group spanning exactly 0..15: s = 1, z = 0, codes = values, dequantized exactly
    vals = [float(v) for v in range(16)]
    c, z, s = ref.quant_w4(_group(vals), 32)
    assert float(s[0, 0]) == 1.0 and int(z[0, 0]) == 0
    assert c[0, :8].tolist() == [(2 * j) | ((2 * j + 1) << 4) for j in range(8)]
    assert torch.equal(ref.dequant_w4(c, z, s, 32), _group(vals))
    # negative only, -7.5 .. 0: s = 0.5, z = round(7.5 / 0.5) = 15, -7.5 -> code 0, 0 -> code 15
    vals = [-0.5 * v for v in range(16)]
    c, z, s = ref.quant_w4(_group(vals), 32)
    assert float(s[0, 0]) == 0.5 and int(z[0, 0]) == 15
    assert c[0, :8].tolist() == [(15 - 2 * j) | ((15 - 2 * j - 1) << 4) for j in range(8)]
    assert torch.equal(ref.dequant_w4(c, z, s, 32), _group(vals))
    # negative only and away from 0, -4 and -1: s = fp16(0.2), -min / s = 20 clamps to z = 15; then
    # -4 -> round(-20) + 15 < 0 -> code 0 and -1 -> round(-5) + 15 = 10
    c, z, s = ref.quant_w4(_group([-4.0, -1.0]), 32)
    assert int(z[0, 0]) == 15 and (c[0] == (0 | (10 << 4))).all()
    with pytest.raises(ValueError, match="group size"):
        ref.quant_w4(torch.zeros(4, 96), 64)
    with pytest.raises(ValueError, match="group size"):
        ref.quant_w4(torch.zeros(4, 96), 48)


@pytest.mark.parametrize("g", [32, 128])
def test_requantizing_the_dequantized_weight_returns_the_same_codes(g):
    """quant(dequant(c, z, s)) == (c, z, s) is a property of groups whose codes span 0..15: then
    max - min = 15 s exactly, so the scale is found again, -min / s = z and w / s + z = q are
    integers.  (A group whose codes span less gets a smaller scale the second time.)  Random codes
    with a 0 and a 15 planted in every group; then Gaussian weights, compared on the groups that
    span 0..15 after the first pass -- nearly all of them."""
    gen = torch.Generator().manual_seed(g)
    N, K = 64, 1024
    q = torch.randint(0, 16, (N, K // g, g), generator=gen)
    q[..., 0], q[..., 1] = 0, 15
    q = q.reshape(N, K // 2, 2).to(torch.uint8)
    c = q[..., 0] | (q[..., 1] << 4)
    z = torch.randint(0, 16, (N, K // g), generator=gen).to(torch.uint8)
    s = (torch.rand(N, K // g, generator=gen) * 0.02 + 0.001).to(torch.float16)
    c2, z2, s2 = ref.quant_w4(ref.dequant_w4(c, z, s, g), g)
    assert torch.equal(c2, c) and torch.equal(z2, z) and torch.equal(s2, s)
    w = torch.randn(N, K, generator=gen) * 0.02
    c, z, s = ref.quant_w4(w, g)
    d = ref.dequant_w4(c, z, s, g)
    rel = ((d - w).norm() / w.norm()).item()
    # 16 levels over the group's range: about +-2.6 sigma for 128 Gaussian values (step 0.35 sigma, rms
    # error step / sqrt(12) = 0.10 sigma), +-2.1 sigma for 32 (0.08 sigma)
    assert rel < (0.13 if g == 128 else 0.10), rel
    c2, z2, _ = ref.quant_w4(d, g)
    nib = torch.stack([c & 15, c >> 4], dim=-1).reshape(N, K // g, g)
    full = (nib.amin(-1) == 0) & (nib.amax(-1) == 15)
    assert full.float().mean() > 0.9
    same = (torch.stack([c2 & 15, c2 >> 4], dim=-1).reshape(N, K // g, g) == nib).all(-1)
    assert same[full].all() and torch.equal(z2[full], z[full])


# ------------------------------------------------------------------------------------------------
# stored layout
# ------------------------------------------------------------------------------------------------
def _random_canonical(N, K, g, seed, device="cpu"):
    gen = torch.Generator(device=device).manual_seed(seed)
    c = torch.randint(0, 256, (N, K // 2), dtype=torch.uint8, device=device, generator=gen)
    z = torch.randint(0, 16, (N, K // g), dtype=torch.uint8, device=device, generator=gen)
    s = (torch.rand(N, K // g, device=device, generator=gen) * 0.02 + 0.001).to(torch.float16)
    return c, z, s


@pytest.mark.parametrize("g", [32, 128])
@pytest.mark.parametrize("K", [512, 1024])
@pytest.mark.parametrize("N", [16, 256, 1024])
def test_shuffle_roundtrip(N, K, g):
    c, z, s = _random_canonical(N, K, g, seed=N + K + g)
    sc, sz, ss = sops.w4_shuffle(c, z, s, g)
    assert sc.shape == c.shape and sz.shape == z.shape and ss.shape == s.shape
    assert sc.is_contiguous() and sz.is_contiguous() and ss.is_contiguous()
    uc, uz, us = sops.w4_unshuffle(sc, sz, ss, g)
    assert torch.equal(uc, c) and torch.equal(uz, z) and torch.equal(us, s)


@pytest.mark.parametrize("g", [32, 64, 128])
def test_shuffle_is_the_kernels_lane_order(g):
    """Lane r + 16 gq of 16-row block b holds, of K-step t, row 16 b + r: its 16 code bytes at
    ((b * steps + t) * 64 + lane) * 16, dword kk of them the elements 128 t + 32 kk + 8 gq + j with j =
    (0, 2, 4, 6, 1, 3, 5, 7)[p] in nibble p; the scale and the zero byte (128 + z) of row 16 b + 4 gq + e
    and group G of the step at element ((b * steps + t) * 4 + gq) * (128 / g) * 4 + 4 G + e.  A K that is
    no multiple of 128 is padded with zero codes."""
    N, K = 32, 640 if g == 128 else 576  # (576 = 4.5 K-steps; with g = 128 every K is whole K-steps)
    c, z, s = _random_canonical(N, K, g, seed=g)
    sc, sz, ss = sops.w4_shuffle(c, z, s, g)
    Kp = 640
    assert sc.shape == (N, Kp // 2) and sz.shape == (N, Kp // g) and ss.shape == (N, Kp // g)
    steps, GS = Kp // 128, 128 // g
    nib = torch.stack([c & 15, c >> 4], dim=-1).reshape(N, K)
    fc, fz, fs = sc.flatten(), sz.flatten(), ss.flatten()
    for b, r, gq, t in [(0, 0, 0, 0), (1, 5, 3, 3), (0, 15, 2, 1), (1, 9, 1, 2), (1, 12, 0, 3)]:
        o = ((b * steps + t) * 64 + r + 16 * gq) * 16
        for kk in range(4):
            dword = sum(int(fc[o + 4 * kk + i]) << (8 * i) for i in range(4))
            k0 = 128 * t + 32 * kk + 8 * gq
            assert [(dword >> (4 * p)) & 15 for p in range(8)] == [int(nib[16 * b + r, k0 + j]) for j in ORDER], (b, r, gq, t)
        for G in range(GS):
            for e in range(4):
                at = ((b * steps + t) * 4 + gq) * GS * 4 + 4 * G + e
                assert int(fz[at]) == 128 + int(z[16 * b + 4 * gq + e, t * GS + G])
                assert fs[at] == s[16 * b + 4 * gq + e, t * GS + G]
    if K < Kp:  # elements 576..639 are MFMA steps 2 and 3 of K-step 4: zero codes, zero scales, z = 0
        o = ((1 * steps + 4) * 64 + 7 + 16 * 3) * 16
        assert (fc[o + 8 : o + 16] == 0).all() and (fc[o : o + 8] != 0).any()
        at = ((1 * steps + 4) * 4 + 3) * GS * 4
        assert (fz[at + 4 * (GS // 2) : at + 4 * GS] == 128).all() and (fs[at + 4 * (GS // 2) : at + 4 * GS] == 0).all()
    uc, uz, us = sops.w4_unshuffle(sc, sz, ss, g, K)
    assert torch.equal(uc, c) and torch.equal(uz, z) and torch.equal(us, s)


# ------------------------------------------------------------------------------------------------
# engine on a written AWQ checkpoint (the shape of the built-in llama-tiny)
# ------------------------------------------------------------------------------------------------
CPU_KW = dict(device="cpu", max_model_len=256, max_batch=4, num_pages=16)
DIM, LAYERS, HEADS, KV_HEADS, FFN, VOCAB = 512, 2, 4, 2, 1024, 1024
PROJ = {"self_attn.q_proj": (HEADS * 128, DIM), "self_attn.k_proj": (KV_HEADS * 128, DIM),
        "self_attn.v_proj": (KV_HEADS * 128, DIM), "self_attn.o_proj": (DIM, HEADS * 128),
        "mlp.gate_proj": (FFN, DIM), "mlp.up_proj": (FFN, DIM), "mlp.down_proj": (DIM, FFN)}


def _config(family, g=None, **quant):
    cfg = dict(architectures=[{"llama": "LlamaForCausalLM", "qwen2": "Qwen2ForCausalLM"}[family]], model_type=family,
               hidden_size=DIM, intermediate_size=FFN, num_hidden_layers=LAYERS, num_attention_heads=HEADS,
               num_key_value_heads=KV_HEADS, vocab_size=VOCAB, max_position_embeddings=256, rope_theta=500000.0,
               rms_norm_eps=1e-5, hidden_act="silu", tie_word_embeddings=False, bos_token_id=1, eos_token_id=2,
               torch_dtype="float16")
    if g is not None:
        cfg["quantization_config"] = dict(dict(quant_method="awq", bits=4, group_size=g, version="GEMM",
                                               zero_point=True, modules_to_not_convert=None), **quant)
    return cfg


def write_checkpoints(root, family, g, **quant):
    """An AWQ checkpoint directory and the unquantized one holding ``dequant_w4`` of the same tensors
    (fp32 ``.weight``); norms, embedding, head and Qwen2's biases are shared.  Returns both paths."""
    from safetensors.torch import save_file

    gen = torch.Generator().manual_seed(7)
    shared = {"model.embed_tokens.weight": torch.randn(VOCAB, DIM, generator=gen) * 0.08,
              "model.norm.weight": 1 + 0.1 * torch.randn(DIM, generator=gen),
              "lm_head.weight": torch.randn(VOCAB, DIM, generator=gen) * 0.08}
    awq, plain = {}, {}
    for i in range(LAYERS):
        p = f"model.layers.{i}."
        shared[p + "input_layernorm.weight"] = 1 + 0.1 * torch.randn(DIM, generator=gen)
        shared[p + "post_attention_layernorm.weight"] = 1 + 0.1 * torch.randn(DIM, generator=gen)
        if family == "qwen2":
            for name in ("q", "k", "v"):
                shared[p + f"self_attn.{name}_proj.bias"] = torch.randn(PROJ[f"self_attn.{name}_proj"][0], generator=gen) * 0.5
        for j, (name, (N, K)) in enumerate(PROJ.items()):
            q, z, s = _random_layer(K, N, g, seed=100 * i + j)
            awq[p + name + ".qweight"], awq[p + name + ".qzeros"], awq[p + name + ".scales"] = pack_awq(q), pack_awq(z), s
            plain[p + name + ".weight"] = ((q.t() - z.t().repeat_interleave(g, dim=1)).float()
                                           * s.t().float().repeat_interleave(g, dim=1)).contiguous()
    paths = []
    for sub, tensors, cfg in (("awq", awq, _config(family, g, **quant)), ("plain", plain, _config(family))):
        d = root / sub
        d.mkdir()
        # (norms and the other unquantized tensors of an AWQ checkpoint are fp16 on disk)
        half = {k: v.half().float() for k, v in shared.items()}
        save_file({**{k: (v.half() if sub == "awq" else v) for k, v in half.items()}, **tensors},
                  str(d / "model.safetensors"))
        (d / "config.json").write_text(json.dumps(cfg))
        paths.append(str(d))
    return paths


@pytest.mark.parametrize("family,g", [("llama", 128), ("qwen2", 64)])
def test_engine_on_an_awq_checkpoint(tmp_path, family, g):
    awq_path, plain_path = write_checkpoints(tmp_path, family, g)
    spec = load_spec(awq_path)
    assert spec.awq is not None and spec.awq.group_size == g and spec.family == family
    eng = LLMEngine.from_model(awq_path, **CPU_KW)  # no flag: the checkpoint's config selects the mode
    m = eng.model
    assert m.quantization == "awq"
    assert all(isinstance(L[k], Awq4Weight) and L[k].g == g for L in m.layers for k in m.FP8_KEYS)
    assert not isinstance(m.lm_head, Awq4Weight) and not isinstance(m.embed, Awq4Weight)
    assert all(L[k].dtype == m.dtype for L in m.layers for k in ("attn_norm", "ffn_norm")) and m.norm.dtype == m.dtype
    assert ("bqkv" in m.layers[0]) == (family == "qwen2")
    # stored bytes of a projection: N K / 2 of codes, per group an fp16 scale and a whole byte for
    # the zero point (128 + z, not a nibble): N K / g * (2 + 1)
    w = m.layers[0]["wgu"]
    assert tuple(w.shape) == (2 * FFN, DIM) and w.nbytes() == 2 * FFN * DIM // 2 + 2 * FFN * DIM // g * 3
    shapes = [(HEADS + 2 * KV_HEADS) * 128 * DIM, DIM * HEADS * 128, 2 * FFN * DIM, DIM * FFN]
    rest = (2 * VOCAB * DIM + DIM + LAYERS * (2 * DIM + ((HEADS + 2 * KV_HEADS) * 128 if family == "qwen2" else 0))) * 4
    assert m.weight_bytes() == LAYERS * sum(nk // 2 + nk // g * 3 for nk in shapes) + rest
    same = LLMEngine.from_model(awq_path, quantization="awq", **CPU_KW)  # the flag says the same
    assert torch.equal(same.model.layers[1]["wdown"].codes, m.layers[1]["wdown"].codes)
    # the canonical form of a fused weight is the checkpoint's tensors, q/k/v along N
    c, z, s = m.layers[0]["wqkv"].canonical()
    qs = [_random_layer(DIM, PROJ[f"self_attn.{n}_proj"][0], g, seed=j) for j, n in enumerate("qkv")]
    assert torch.equal(torch.stack([c & 15, c >> 4], -1).reshape(c.shape[0], -1).long(), torch.cat([q.t() for q, _, _ in qs]))
    assert torch.equal(z.long(), torch.cat([z_.t() for _, z_, _ in qs])) and torch.equal(s, torch.cat([s_.t() for _, _, s_ in qs]))
    # prefill logits against the unquantized engine holding dequant_w4 of the same tensors.  On the CPU
    # both multiply identical fp32 values: the W4 products (ref.w4_linear) and the other engine's
    # _mm accumulate in fp64 and round once, the other engine's prefill qkv product is the library's
    # fp32 GEMM.  So the two differ by one fp32 summation order per layer (relative error K 2^-24 of
    # the sum of magnitudes at worst) -- the difference test_serving.py allows between this engine
    # and transformers' fp32 model, and the same bound.
    base = LLMEngine.from_model(plain_path, **CPU_KW)
    assert base.model.quantization is None and not isinstance(base.model.layers[0]["wo"], Awq4Weight)
    prompt = torch.tensor(list(range(1, 129)))
    pos = torch.arange(128, dtype=torch.int32)
    slots = torch.arange(128, dtype=torch.int32)
    a = base.model.prefill(prompt, pos, slots, [0], [128])
    b = m.prefill(prompt, pos, slots, [0], [128])
    assert a.abs().max() > 0.5  # not flat
    torch.testing.assert_close(b, a, atol=2e-4, rtol=2e-4)
    # greedy generation: speculative decoding changes nothing
    sp = SamplingParams(max_tokens=24, temperature=0, ignore_eos=True)
    prompts = [[1, 2, 3, 4, 5, 1, 2, 3, 4, 5, 1, 2], list(range(7, 60))]
    plain = [o.output_ids for o in eng.generate(prompts, sp)]
    spec_eng = LLMEngine.from_model(awq_path, speculative_ngram=3, **CPU_KW)
    assert [o.output_ids for o in spec_eng.generate(prompts, sp)] == plain and spec_eng.stats["spec_steps"] > 0


def test_builtin_model_with_awq_generates():
    base = LLMEngine.from_model("llama-tiny", **CPU_KW)
    eng = LLMEngine.from_model("llama-tiny", quantization="awq", **CPU_KW)
    assert all(isinstance(L[k], Awq4Weight) and L[k].g == 128 for L in eng.model.layers for k in eng.model.FP8_KEYS)
    assert eng.model.weight_bytes() < 0.45 * base.model.weight_bytes()  # 4.19 bits per projection weight
    out = eng.generate([[1, 2, 3, 4, 5]], SamplingParams(max_tokens=8, temperature=0, ignore_eos=True))
    assert len(out[0].output_ids) == 8
    # the stored weight is quant_w4 of the random weight
    w = base.model.layers[0]["wo"]
    for got, want in zip(eng.model.layers[0]["wo"].canonical(), ref.quant_w4(w, 128)):
        assert torch.equal(got, want)


@pytest.mark.parametrize("field,value", [("quant_method", "gptq"), ("bits", 8), ("version", "gemv"),
                                         ("zero_point", False), ("group_size", -1),
                                         ("modules_to_not_convert", ["lm_head", "mlp.down_proj"])])
def test_bad_quantization_config_fields_are_named(tmp_path, field, value):
    (tmp_path / "config.json").write_text(json.dumps(_config("llama", 128, **{field: value})))
    with pytest.raises(ValueError, match=field):
        load_spec(str(tmp_path))


def test_quantization_config_spellings(tmp_path):
    (tmp_path / "config.json").write_text(json.dumps(_config("llama", 64, version="gemm", modules_to_not_convert=[])))
    assert load_spec(str(tmp_path)).awq.group_size == 64


def test_refusals(tmp_path):
    from safetensors.torch import load_file, save_file

    awq_path, plain_path = write_checkpoints(tmp_path, "llama", 128)
    with pytest.raises(ValueError, match="quantization=\"awq\".*no quantization_config"):
        LLMEngine.from_model(plain_path, quantization="awq", **CPU_KW)  # no calibrator here
    with pytest.raises(ValueError, match="quantization='fp8' on an AWQ checkpoint"):
        LLMEngine.from_model(awq_path, quantization="fp8", **CPU_KW)
    with pytest.raises(ValueError, match="quantization='mxfp4' on an AWQ checkpoint"):
        ServingLlama(load_spec(awq_path), "cpu", quantization="mxfp4")
    mods = {"a": "/nonexistent/adapter"}
    for model in ("llama-tiny", awq_path):
        with pytest.raises(ValueError, match="LoRA.*quantization=\"awq\""):
            LLMEngine.from_model(model, quantization=None if model == awq_path else "awq", lora_modules=mods, **CPU_KW)
        with pytest.raises(ValueError, match="awq.*tensor parallel"):
            LLMEngine.from_model(model, device="cpu", quantization="awq", tp_group=object())
    with pytest.raises(ValueError, match="awq.*tensor parallel"):
        ServingLlama(load_spec(awq_path), "cpu", tp_group=object())
    with pytest.raises(ValueError, match="LoRA.*quantization=\"awq\""):
        ServingLlama(load_spec("llama-tiny"), "cpu", quantization="awq").enable_lora(1, 8)
    with pytest.raises(ValueError, match="quantization.*fp8, mxfp4, awq"):
        ServingLlama(load_spec("llama-tiny"), "cpu", quantization="int3")
    # damaged checkpoints: each error names the tensor
    sd = load_file(f"{awq_path}/model.safetensors")

    def broken(change):
        d = dict(sd)
        change(d)
        save_file(d, f"{awq_path}/model.safetensors")
        return ServingLlama(load_spec(awq_path), "cpu")

    with pytest.raises(ValueError, match=r"missing 1 tensors.*layers\.1\.mlp\.up_proj\.qzeros"):
        broken(lambda d: d.pop("model.layers.1.mlp.up_proj.qzeros")).load_hf()
    with pytest.raises(ValueError, match=r"unexpected tensor model\.layers\.0\.self_attn\.o_proj\.weight.*AWQ"):
        broken(lambda d: d.update({"model.layers.0.self_attn.o_proj.weight": torch.zeros(DIM, DIM)})).load_hf()
    with pytest.raises(ValueError, match=r"layers\.0\.mlp\.down_proj\.qweight: expected torch\.int32 \[1024, 64\]"):
        broken(lambda d: d.update({"model.layers.0.mlp.down_proj.qweight":
                                   d["model.layers.0.mlp.down_proj.qweight"][:512].contiguous()})).load_hf()
    with pytest.raises(ValueError, match=r"layers\.1\.self_attn\.k_proj\.scales: expected torch\.float16"):
        broken(lambda d: d.update({"model.layers.1.self_attn.k_proj.scales":
                                   d["model.layers.1.self_attn.k_proj.scales"].float()})).load_hf()
    # and an AWQ tensor in an unquantized checkpoint
    sd = load_file(f"{plain_path}/model.safetensors")
    sd["model.layers.0.mlp.up_proj.qweight"] = torch.zeros(DIM, FFN // 8, dtype=torch.int32)
    save_file(sd, f"{plain_path}/model.safetensors")
    with pytest.raises(ValueError, match=r"unexpected tensor model\.layers\.0\.mlp\.up_proj\.qweight"):
        ServingLlama(load_spec(plain_path), "cpu").load_hf()
    # a built-in projection whose K has no whole groups
    m = ServingLlama(load_spec("llama-tiny"), "cpu", quantization="awq").init_random(0)
    m.layers[0]["wo"] = torch.zeros(512, 192)
    with pytest.raises(ValueError, match="quantization=\"awq\".*K % 128"):
        m.quantize_awq()


# ------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("g", [32, 64, 128])
def test_gpu_dequant_is_exact(gpu, g):
    from dstack_amd.ops import _ext

    C = _ext.require()
    N, K = 256, 512
    c, z, s = _random_canonical(N, K, g, seed=g, device=gpu)
    out = torch.full((N, K), float("nan"), dtype=torch.bfloat16, device=gpu)
    C.w4_dequant(*sops.w4_shuffle(c, z, s, g), N, K, g, out)
    assert torch.equal(out, ref.dequant_w4(c, z, s, g).bfloat16())


def _exact_case(gpu, M, N, K, g, seed, long_k):
    """Integer data on which the kernel's every sum is exact in fp32 in any order.  The kernel does not
    sum x (q - z) s: per group it sums P = sum x (128 + q) and X = sum x by MFMA, forms P - (128 + z) X
    in one fma and adds s times that to the accumulator.  K <= 1024 (x in -8..8, s in 2^-2..2^1):
    |P| <= 8 * 143 * 128 < 2^18 and |X| <= 2^10 are integers, (128 + z) X < 2^18 too, so the fma's
    result x-sum (q - z) (|.| <= 8 * 15 * 128 < 2^14) is exact; the accumulator holds multiples of 2^-2
    below 15 * 2 * 8 * 1024 < 2^18: 20 bits.  K = 8192 (x in -2..2, s in 2^-1..2^1): the same with
    smaller groups sums and an accumulator of multiples of 2^-1 below 15 * 2 * 2 * 8192 < 2^19; the
    fp32 partials and their sum are exact as well."""
    gen = torch.Generator(device=gpu).manual_seed(seed)
    c = torch.randint(0, 256, (N, K // 2), dtype=torch.uint8, device=gpu, generator=gen)
    z = torch.randint(0, 16, (N, K // g), dtype=torch.uint8, device=gpu, generator=gen)
    lo, hi, amax = (-1, 2, 2) if long_k else (-2, 2, 8)
    s = torch.ldexp(torch.ones(N, K // g, device=gpu), torch.randint(lo, hi, (N, K // g), device=gpu, generator=gen))
    s = s.to(torch.float16)
    x = torch.randint(-amax, amax + 1, (M, K), device=gpu, generator=gen).float()
    want = (x.double() @ ref.dequant_w4(c, z, s, g).double().t()).to(torch.bfloat16)
    return c, z, s, x, want


# which instantiation (16-row token blocks) runs M rows: 1 (M <= 16), 4 (<= 64), 8 (<= 128), 16 (<= 256)
FORMS = {1: 1, 3: 1, 5: 1, 16: 1, 17: 4, 100: 8, 256: 16}


@pytest.mark.gpu
@pytest.mark.parametrize("g", [32, 128])
@pytest.mark.parametrize("stride_pad", [0, 64])
@pytest.mark.parametrize("N,K", [(256, 512), (1024, 1024)])
@pytest.mark.parametrize("M", [1, 5, 16, 17, 100, 256])
def test_gpu_gemm_exact(gpu, M, N, K, stride_pad, g):
    """bf16(fp64 product) exactly, in every instantiation (M 1, 5, 16: 1 token block; 17: 4; 100: 8;
    256: 16), with an activation row stride of K and of K + 64, with one and with four groups per
    K-step."""
    from dstack_amd.ops import _ext

    C = _ext.require()
    assert C.w4_gemm_supported(M, N, K, g) and C.w4_gemm_form(M) == FORMS[M] and C.w4_gemm_split(M, N, K) >= 1
    c, z, s, x, want = _exact_case(gpu, M, N, K, g, seed=M * 7 + N + g, long_k=False)
    buf = torch.zeros(M, K + stride_pad, dtype=torch.bfloat16, device=gpu)
    xb = buf[:, :K]
    xb.copy_(x)
    y = C.w4_gemm(xb, *sops.w4_shuffle(c, z, s, g), N, K, g)
    assert y.shape == (M, N) and y.dtype == torch.bfloat16
    assert torch.equal(y, want), (y.float() - want.float()).abs().max().item()


@pytest.mark.gpu
@pytest.mark.parametrize("M", [3, 256])
def test_gpu_gemm_exact_split_k(gpu, M):
    """(N, K) = (256, 8192) runs as several K slices: fp32 partials and the reduce kernel, still exact,
    and the same bits from run to run (no atomics)."""
    from dstack_amd.ops import _ext

    C = _ext.require()
    N, K, g = 256, 8192, 128
    assert C.w4_gemm_split(M, N, K) > 1 and C.w4_gemm_form(M) == FORMS[M]
    c, z, s, x, want = _exact_case(gpu, M, N, K, g, seed=M, long_k=True)
    stored = sops.w4_shuffle(c, z, s, g)
    y = C.w4_gemm(x.bfloat16(), *stored, N, K, g)
    assert torch.equal(y, want), (y.float() - want.float()).abs().max().item()
    assert torch.equal(C.w4_gemm(x.bfloat16(), *stored, N, K, g), y)


@pytest.mark.gpu
def test_gpu_shapes_and_the_models_fallback(gpu):
    """``w4_gemm_supported`` covers every projection of the built-in models at 1 and 256 rows and
    rejects 257 rows and K = 640; the model then dequantizes the weight and runs the bf16 GEMM --
    integer data and power-of-two scales, so bf16((q - z) s) and the product are still exact."""
    from dstack_amd.ops import _ext

    C = _ext.require()
    M, N, K, g = 5, 256, 640, 128
    assert not C.w4_gemm_supported(M, N, K, g) and not C.w4_gemm_supported(257, 256, 512, g)
    assert not C.w4_gemm_supported(1, 256, 512, 16) and not C.w4_gemm_supported(1, 128, 512, g)
    assert all(C.w4_gemm_supported(m, 256, 512, gg) for m in range(1, 257) for gg in (32, 64, 128))
    for n, k in [(1024, 512), (512, 512), (2048, 512), (512, 1024),          # llama-tiny
                 (3072, 2048), (2048, 2048), (16384, 2048), (2048, 8192),    # 1B
                 (6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336),   # 8B
                 (10240, 8192), (8192, 8192), (57344, 8192), (8192, 28672)]:  # 70B
        assert C.w4_gemm_supported(1, n, k, g) and C.w4_gemm_supported(256, n, k, g), (n, k)
    c, z, s, x, want = _exact_case(gpu, M, N, K, g, seed=11, long_k=False)
    m = ServingLlama(load_spec("llama-tiny"), "cuda", quantization="awq")
    m._w4_scratch = torch.empty(N * K, dtype=torch.bfloat16, device=gpu)
    y = m._mm(x.bfloat16(), Awq4Weight(*sops.w4_shuffle(c, z, s, g), N, K, g))
    assert torch.equal(y, want)


@pytest.mark.gpu
def test_gpu_gemm_random_is_as_close_as_the_bf16_gemm(gpu):
    """Gaussian data: the error of ``w4_gemm`` against the fp64 product with the dequantized weight is
    at most twice that of torch's bf16 ``x @ Wdeq.T`` on the same inputs -- both accumulate in fp32 and
    round to bf16 once; the factor covers the summation order and the cancellation of 128 + q.
    Measured on an MI355X: 1.645e-3 for ``w4_gemm``, 2.337e-3 for the bf16 GEMM (which also rounds the
    weight to bf16)."""
    from dstack_amd.ops import _ext

    C = _ext.require()
    M, N, K, g = 7, 1024, 4096, 128
    gen = torch.Generator(device=gpu).manual_seed(5)
    x = torch.randn(M, K, device=gpu, generator=gen).bfloat16()
    w = torch.randn(N, K, device=gpu, generator=gen) * 0.02
    c, z, s = ref.quant_w4(w, g)
    wd = ref.dequant_w4(c, z, s, g)
    want = x.double() @ wd.double().t()
    y = C.w4_gemm(x, *sops.w4_shuffle(c, z, s, g), N, K, g)
    lib = x @ wd.bfloat16().t()
    err = ((y.double() - want).norm() / want.norm()).item()
    err_lib = ((lib.double() - want).norm() / want.norm()).item()
    print(f"w4_gemm relative error {err:.3e}, bf16 library GEMM {err_lib:.3e}")
    assert y.shape == (M, N) and err <= 2 * err_lib, (err, err_lib)


GPU_KW = dict(device="cuda", max_model_len=512, max_batch=8, num_pages=128)


def _with_dequantized_projections(engine):
    for L in engine.model.layers:
        for k in engine.model.FP8_KEYS:
            w = L[k]
            L[k] = ref.dequant_w4(*ref.quant_w4(w, 128), 128).to(w.dtype)
    return engine


@pytest.mark.gpu
def test_gpu_engine_prefill_through_the_dequant_path(gpu):
    """Two 256-token prompts in one prefill step are 512 rows: past the decode GEMM's 256, so every
    projection is dequantized into the scratch and multiplied by the bf16 GEMM.  Against the bf16
    engine holding the dequantized weights only the bf16 rounding of the weights and the summation
    order differ: the bound of the MXFP4 test of the same name."""
    base = _with_dequantized_projections(LLMEngine.from_model("llama-tiny", **GPU_KW))
    eng = LLMEngine.from_model("llama-tiny", quantization="awq", **GPU_KW)
    assert all(isinstance(L[k], Awq4Weight) for L in eng.model.layers for k in eng.model.FP8_KEYS)
    tokens = torch.arange(1, 513, device=gpu) % 1000
    pos = torch.arange(256, dtype=torch.int32, device=gpu).repeat(2)
    slots = torch.arange(512, dtype=torch.int32, device=gpu)
    a = base.model.prefill(tokens, pos, slots, [0, 256], [256, 256])
    b = eng.model.prefill(tokens, pos, slots, [0, 256], [256, 256])
    cos = torch.nn.functional.cosine_similarity(a.float(), b.float(), dim=-1)
    assert cos.shape == (2,) and cos.min().item() > 0.999, cos


@functools.lru_cache(maxsize=None)
def _eager_tokens(kv_cache_dtype):
    sp = SamplingParams(max_tokens=16, temperature=0, ignore_eos=True)
    eager = LLMEngine.from_model("llama-tiny", quantization="awq", kv_cache_dtype=kv_cache_dtype, use_graphs=False,
                                 **GPU_KW)
    return [o.output_ids for o in eager.generate(PROMPTS, sp)]


PROMPTS = [[1, 2, 3, 4, 5, 1, 2, 3, 4, 5, 1, 2, 3], list(range(7, 90))]


@pytest.mark.gpu
@pytest.mark.parametrize("kv_cache_dtype", ["auto", "fp8"])
def test_gpu_engine_decode_in_graphs_equals_eager(gpu, kv_cache_dtype):
    """The decode path (1-token-block GEMM form, split-K workspaces) inside captured graphs gives the
    token ids of the same engine without graphs: the kernels are deterministic."""
    sp = SamplingParams(max_tokens=16, temperature=0, ignore_eos=True)
    graphs = LLMEngine.from_model("llama-tiny", quantization="awq", kv_cache_dtype=kv_cache_dtype, **GPU_KW)
    graphs.capture_graphs()
    got = [o.output_ids for o in graphs.generate(PROMPTS, sp)]
    assert all(len(ids) == 16 for ids in got) and got == _eager_tokens(kv_cache_dtype)


@pytest.mark.gpu
def test_gpu_engine_verify_steps_in_graphs(gpu):
    """Speculative decoding's verify steps (4 rows per sequence: ``w4_gemm`` too) run in captured
    graphs and emit the plain engine's greedy tokens."""
    sp = SamplingParams(max_tokens=16, temperature=0, ignore_eos=True)
    eng = LLMEngine.from_model("llama-tiny", quantization="awq", speculative_ngram=3, **GPU_KW)
    eng.capture_graphs()
    got = [o.output_ids for o in eng.generate(PROMPTS, sp)]
    assert got == _eager_tokens("auto") and eng.stats["spec_steps"] > 0
