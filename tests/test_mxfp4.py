"""MXFP4 projection weights (``--quantization mxfp4``): the OCP MX v1.0 quantizer rule, the stored
layout, the block-scaled FP4 decode GEMM (``ops/csrc/mxfp4.hip``) and the engine built on them."""

import pytest
import torch

from dstack_amd.ops import reference as ref
from dstack_amd.ops import serving as sops
from dstack_amd.serving.engine import LLMEngine, SamplingParams
from dstack_amd.serving.model import Mxfp4Weight, ServingLlama, load_spec


def _block(vals):
    x = torch.zeros(1, 32)
    x[0, : len(vals)] = torch.tensor(vals, dtype=torch.float32)
    return x


# (first values of a 32-element block (the rest zero), expected scale byte, expected first code bytes)
HAND_BLOCKS = [
    # amax exactly a power of two: 4 = 1.0 * 2^2 -> e = 0, 4 -> code 6; 1 -> 2; -2 -> 8 | 4; 0.5 -> 1
    ([4.0, 1.0, -2.0, 0.5], 127, [0x26, 0x1C]),
    # amax 1.0 -> e = -2: 1.0 / 2^-2 = 4 -> code 6; 0.375 / 0.25 = 1.5 -> 3
    ([1.0, 0.375], 125, [0x36]),
    # 7.9 saturates to 6 at scale 1 (e = floor(log2 7.9) - 2 = 0); ties to even: 2.5 -> 2 (code 4),
    # 3.5 -> 4 (6), 0.25 -> 0 (0), 0.75 -> 1 (2)
    ([7.9, 2.5, 3.5, 0.25, 0.75], 127, [0x47, 0x06, 0x02]),
    # more ties at e = 0: 5 -> 4 (code 6, not 6.0 = code 7), 1.25 -> 1 (2), 1.75 -> 2 (4), 7 -> 8 -> 6 (7)
    ([5.0, 1.25, 1.75, 7.0], 127, [0x26, 0x74]),
    # an all-zero block: e = -127 (byte 0), codes 0
    ([], 0, [0x00, 0x00]),
    # -0.0 keeps its sign bit; so does a value that rounds to zero (-0.2 at e = 0: 0.2 < 0.25 -> 0)
    ([4.0, -0.0, -0.2, 0.2], 127, [0x86, 0x08]),
    # tiny values: amax 3e-39 < 2^-127 -> e = -130 clamps to -127 (byte 0); 3e-39 * 2^127 = 0.51 -> 0.5
    # (code 1, negative: 9), 1e-40 * 2^127 = 0.017 -> 0
    ([1e-40, -3e-39], 0, [0x90]),
    # large values: amax 2^100 -> e = 98 (byte 225), 2^100 / 2^98 = 4 -> code 6, -2^99 -> 8 | 4
    ([2.0 ** 100, -(2.0 ** 99)], 225, [0xC6]),
]


@pytest.mark.parametrize("vals,scale,codes", HAND_BLOCKS)
def test_quantizer_rule_on_hand_made_blocks(vals, scale, codes):
    c, s = ref.quant_mxfp4(_block(vals))
    assert c.shape == (1, 16) and s.shape == (1, 1) and c.dtype == s.dtype == torch.uint8
    assert int(s[0, 0]) == scale
    assert c[0, : len(codes)].tolist() == codes
    assert (c[0, len(codes):] == 0).all()


def test_requantizing_the_dequantized_weight_returns_the_same_bytes():
    torch.manual_seed(0)
    w = (torch.randn(64, 1024) * torch.rand(64, 1) * 3).bfloat16()
    c, s = ref.quant_mxfp4(w)
    assert int(s.max()) < 255
    d = ref.dequant_mxfp4(c, s)
    assert d.dtype == torch.float32 and d.shape == w.shape
    rel = ((d - w.float()).norm() / w.float().norm()).item()
    assert 0.08 < rel < 0.14, rel  # 11.5 % on Gaussian data: the format's error, not the code's
    c2, s2 = ref.quant_mxfp4(d)
    assert torch.equal(c, c2) and torch.equal(s, s2)
    c3, s3 = ref.quant_mxfp4(w.float())  # fp32 input: the same rule
    assert torch.equal(c, c3) and torch.equal(s, s3)
    with pytest.raises(ValueError, match="32"):
        ref.quant_mxfp4(torch.zeros(4, 48))


@pytest.mark.parametrize("N", [16, 256, 1024])
@pytest.mark.parametrize("K", [512, 1024])
def test_shuffle_roundtrip(N, K):
    g = torch.Generator().manual_seed(N + K)
    c = torch.randint(0, 256, (N, K // 2), dtype=torch.uint8, generator=g)
    s = torch.randint(0, 255, (N, K // 32), dtype=torch.uint8, generator=g)
    sc, ss = sops.mxfp4_shuffle(c, s)
    assert sc.shape == c.shape and ss.shape == s.shape and sc.is_contiguous() and ss.is_contiguous()
    uc, us = sops.mxfp4_unshuffle(sc, ss)
    assert torch.equal(uc, c) and torch.equal(us, s)


def test_shuffle_is_the_kernels_lane_order():
    """Lane r + 16 g of 16-row block b holds row 16 b + r, K elements [128 t + 32 g, + 32) of K-step t:
    its 16 code bytes at ((b * steps + t) * 64 + lane) * 16, and byte t % 4 of its scale dword at
    ((b * groups + t / 4) * 64 + lane) * 4.  A K that is no multiple of 512 is padded with zero codes."""
    N, K = 32, 640
    g = torch.Generator().manual_seed(1)
    c = torch.randint(0, 256, (N, K // 2), dtype=torch.uint8, generator=g)
    s = torch.randint(0, 255, (N, K // 32), dtype=torch.uint8, generator=g)
    sc, ss = sops.mxfp4_shuffle(c, s)
    assert sc.shape == (N, 512) and ss.shape == (N, 32)  # Kp = 1024
    steps, groups = 8, 2
    fc, fs = sc.flatten(), ss.flatten()
    for b, r, gq, t in [(0, 0, 0, 0), (1, 5, 3, 4), (0, 15, 2, 3), (1, 9, 1, 1)]:
        lane = r + 16 * gq
        o = ((b * steps + t) * 64 + lane) * 16
        assert torch.equal(fc[o : o + 16], c[16 * b + r, 64 * t + 16 * gq : 64 * t + 16 * gq + 16])
        assert fs[((b * groups + t // 4) * 64 + lane) * 4 + t % 4] == s[16 * b + r, 4 * t + gq]
    o = ((1 * steps + 6) * 64 + 3) * 16  # K-step 6 is padding
    assert (fc[o : o + 16] == 0).all()
    uc, us = sops.mxfp4_unshuffle(sc, ss, K)
    assert torch.equal(uc, c) and torch.equal(us, s)


CPU_KW = dict(device="cpu", max_model_len=256, max_batch=4, num_pages=16)


def _with_dequantized_projections(engine, quant):
    """Replace the four projections of an unquantized engine by dequant(quant(w)) in its own dtype."""
    for L in engine.model.layers:
        for k in engine.model.FP8_KEYS:
            w = L[k]
            L[k] = ref.dequant_mxfp4(*quant(w)).to(w.dtype)
    return engine


def test_engine_size_types_generation_and_logits():
    base = LLMEngine.from_model("llama-tiny", **CPU_KW)
    mx = LLMEngine.from_model("llama-tiny", quantization="mxfp4", **CPU_KW)
    # 4.25 bits per projection weight, embedding and head unquantized
    assert mx.model.weight_bytes() < 0.45 * base.model.weight_bytes()
    assert all(isinstance(L[k], Mxfp4Weight) for L in mx.model.layers for k in ("wqkv", "wo", "wgu", "wdown"))
    w = mx.model.layers[0]["wgu"]
    assert tuple(w.shape) == (2048, 512) and w.nbytes() == 2048 * 512 // 2 + 2048 * 512 // 32
    assert not isinstance(mx.model.lm_head, Mxfp4Weight) and mx.model.embed.dtype == base.model.embed.dtype
    out = mx.generate([[1, 2, 3, 4, 5]], SamplingParams(max_tokens=8, temperature=0, ignore_eos=True))
    assert len(out[0].output_ids) == 8
    # logits against the model holding the same (dequantized) weights: only the e4m3 activations and
    # the bf16 rounding of each product differ -- the fp8 engine test's bound
    _with_dequantized_projections(base, ref.quant_mxfp4)
    prompt = torch.tensor(list(range(1, 129)))
    pos = torch.arange(128, dtype=torch.int32)
    slots = torch.arange(128, dtype=torch.int32)
    a = base.model.prefill(prompt, pos, slots, [0], [128])
    b = mx.model.prefill(prompt, pos, slots, [0], [128])
    cos = torch.nn.functional.cosine_similarity(a.float(), b.float(), dim=-1).item()
    assert cos > 0.99, cos


def test_refusals():
    mods = {"a": "/nonexistent/adapter"}
    with pytest.raises(ValueError, match="quantization=\"mxfp4\""):
        LLMEngine.from_model("llama-tiny", device="cpu", quantization="mxfp4", lora_modules=mods)
    m = ServingLlama(load_spec("llama-tiny"), "cpu", quantization="mxfp4")
    with pytest.raises(ValueError, match="quantization=\"mxfp4\""):
        m.enable_lora(1, 8)
    with pytest.raises(ValueError, match="mxfp4.*tensor parallel"):
        LLMEngine.from_model("llama-tiny", device="cpu", quantization="mxfp4", tp_group=object())
    with pytest.raises(ValueError, match="mxfp4.*tensor parallel"):
        ServingLlama(load_spec("llama-tiny"), "cpu", quantization="mxfp4", tp_group=object())
    with pytest.raises(ValueError, match="quantization.*fp8, mxfp4"):
        ServingLlama(load_spec("llama-tiny"), "cpu", quantization="int3")
    # a projection whose K is no multiple of 32 has no MX blocks
    m.init_random(0)
    m.layers[0]["wo"] = torch.zeros(512, 48)
    with pytest.raises(ValueError, match="quantization=\"mxfp4\".*K % 32"):
        m.quantize_mxfp4()


# ------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("N,K", [(256, 512), (16, 4096)])
def test_gpu_quantizer_equals_the_reference(gpu, N, K):
    from dstack_amd.ops import _ext

    C = _ext.require()
    g = torch.Generator(device=gpu).manual_seed(N + K)
    w = (torch.randn(N, K, device=gpu, generator=g) * torch.rand(N, 1, device=gpu, generator=g) * 10).bfloat16()
    hand = torch.cat([_block(v) for v, _, _ in HAND_BLOCKS], dim=1).bfloat16()  # one row of hand-made blocks
    w[0, : hand.shape[1]] = hand[0].to(gpu)
    c, s = C.quant_mxfp4(w)
    cr, sr = ref.quant_mxfp4(w)
    assert torch.equal(s, sr)
    assert torch.equal(c, cr)


@pytest.mark.gpu
def test_gpu_quantizer_hand_made_blocks(gpu):
    from dstack_amd.ops import _ext

    C = _ext.require()
    # the blocks whose values are bf16 (7.9, 0.2, 3e-39 and 1e-40 are not: those blocks go through the
    # reference comparison above after rounding to bf16)
    rows = [(v, sc, cd) for v, sc, cd in HAND_BLOCKS if all(float(torch.tensor(x).bfloat16()) == x for x in v)]
    assert len(rows) >= 5
    w = torch.cat([_block(v) for v, _, _ in rows], dim=0).bfloat16().to(gpu)
    c, s = C.quant_mxfp4(w)
    for i, (_, sc, cd) in enumerate(rows):
        assert int(s[i, 0]) == sc and c[i, : len(cd)].tolist() == cd and (c[i, len(cd):] == 0).all(), i


@pytest.mark.gpu
def test_gpu_dequant_is_exact(gpu):
    from dstack_amd.ops import _ext

    C = _ext.require()
    N, K = 256, 512
    g = torch.Generator(device=gpu).manual_seed(3)
    c = torch.randint(0, 256, (N, K // 2), dtype=torch.uint8, device=gpu, generator=g)
    s = torch.randint(100, 141, (N, K // 32), dtype=torch.uint8, device=gpu, generator=g)
    sc, ss = sops.mxfp4_shuffle(c, s)
    out = torch.full((N, K), float("nan"), dtype=torch.bfloat16, device=gpu)
    C.mxfp4_dequant(sc, ss, N, K, out)
    want = ref.dequant_mxfp4(c, s)
    assert torch.equal(out.float(), want)
    assert torch.equal(torch.signbit(out), torch.signbit(want))  # -0.0 too


def _exact_case(gpu, M, N, K, seed, long_k):
    """Asymmetric integer data whose every partial sum is exact in fp32 in any order.  K <= 1024: scale
    bytes 125..130, activations -8..8 -> |sum| <= 48 * 8 * 1024 < 2^19 at granularity 2^-3 (22 bits).
    Longer K: scale bytes 126..128, activations -2..2 -> |sum| <= 12 * 2 * 8192 < 2^18 at 2^-2."""
    g = torch.Generator(device=gpu).manual_seed(seed)
    c = torch.randint(0, 256, (N, K // 2), dtype=torch.uint8, device=gpu, generator=g)
    lo, hi, amax = (126, 129, 2) if long_k else (125, 131, 8)
    s = torch.randint(lo, hi, (N, K // 32), dtype=torch.uint8, device=gpu, generator=g)
    x = torch.randint(-amax, amax + 1, (M, K), device=gpu, generator=g).float()
    xs = torch.ldexp(torch.ones(M, device=gpu), torch.randint(-3, 4, (M,), device=gpu, generator=g)).float()
    want = ((x.double() @ ref.dequant_mxfp4(c, s).double().t()) * xs.double()[:, None]).to(torch.bfloat16)
    return c, s, x, xs, want


# which instantiation (16-row token blocks) runs M rows: 1 (M <= 16), 4 (<= 64), 8 (<= 128), 16 (<= 256)
FORMS = {1: 1, 3: 1, 5: 1, 16: 1, 17: 4, 100: 8, 256: 16}


@pytest.mark.gpu
@pytest.mark.parametrize("stride_pad", [0, 64])
@pytest.mark.parametrize("N,K", [(256, 512), (1024, 1024)])
@pytest.mark.parametrize("M", [1, 5, 16, 17, 100, 256])
def test_gpu_gemm_exact(gpu, M, N, K, stride_pad):
    """bf16(fp64 product) exactly, in every instantiation (M 1, 5, 16: 1 token block; 17: 4; 100: 8;
    256: 16), unsplit (these shapes are one K slice), with an activation row stride of K and of K + 64."""
    from dstack_amd.ops import _ext

    C = _ext.require()
    assert C.mxfp4_gemm_supported(M, N, K) and C.mxfp4_gemm_form(M) == FORMS[M] and C.mxfp4_gemm_split(M, N, K) >= 1
    c, s, x, xs, want = _exact_case(gpu, M, N, K, seed=M * 7 + N, long_k=False)
    sc, ss = sops.mxfp4_shuffle(c, s)
    buf = torch.zeros(M, K + stride_pad, dtype=torch.uint8, device=gpu)
    xq = buf[:, :K]
    xq.copy_(x.to(torch.float8_e4m3fn).view(torch.uint8))
    y = C.mxfp4_gemm(xq, xs, sc, ss, N, K)
    assert y.shape == (M, N) and y.dtype == torch.bfloat16
    assert torch.equal(y, want), (y.float() - want.float()).abs().max().item()


@pytest.mark.gpu
@pytest.mark.parametrize("M", [3, 256])
def test_gpu_gemm_exact_split_k(gpu, M):
    """(N, K) = (256, 8192) runs as 16 K slices at 3 rows (1 token block) and 2 at 256 rows (16 token
    blocks): fp32 partials and the reduce kernel, still exact."""
    from dstack_amd.ops import _ext

    C = _ext.require()
    N, K = 256, 8192
    assert C.mxfp4_gemm_split(M, N, K) == {3: 16, 256: 2}[M] and C.mxfp4_gemm_form(M) == FORMS[M]
    c, s, x, xs, want = _exact_case(gpu, M, N, K, seed=M, long_k=True)
    y = C.mxfp4_gemm(x.to(torch.float8_e4m3fn).view(torch.uint8), xs, *sops.mxfp4_shuffle(c, s), N, K)
    assert torch.equal(y, want), (y.float() - want.float()).abs().max().item()
    y2 = C.mxfp4_gemm(x.to(torch.float8_e4m3fn).view(torch.uint8), xs, *sops.mxfp4_shuffle(c, s), N, K)
    assert torch.equal(y, y2)  # no atomics: bit-identical from run to run


@pytest.mark.gpu
def test_gpu_unsupported_shape_takes_the_models_fallback(gpu):
    """K = 640 is no multiple of 512: ``mxfp4_gemm_supported`` rejects it, and the model dequantizes the
    weight exactly and runs the bf16 GEMM -- integer activations, so the same exact result."""
    from dstack_amd.ops import _ext

    C = _ext.require()
    M, N, K = 5, 256, 640
    assert not C.mxfp4_gemm_supported(M, N, K) and not C.mxfp4_gemm_supported(257, 256, 512)
    assert all(C.mxfp4_gemm_supported(m, 256, 512) for m in range(1, 257))
    for n, k in [(1024, 512), (512, 512), (2048, 512), (512, 1024),          # llama-tiny
                 (3072, 2048), (2048, 2048), (16384, 2048), (2048, 8192),    # 1B
                 (6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336),   # 8B
                 (10240, 8192), (8192, 8192), (57344, 8192), (8192, 28672)]:  # 70B
        assert C.mxfp4_gemm_supported(1, n, k) and C.mxfp4_gemm_supported(256, n, k), (n, k)
    c, s, x, _, _ = _exact_case(gpu, M, N, K, seed=11, long_k=False)
    want = (x.double() @ ref.dequant_mxfp4(c, s).double().t()).to(torch.bfloat16)
    m = ServingLlama(load_spec("llama-tiny"), "cuda", quantization="mxfp4")
    m._mx_scratch = torch.empty(N * K, dtype=torch.bfloat16, device=gpu)
    y = m._mm(x.bfloat16(), Mxfp4Weight(*sops.mxfp4_shuffle(c, s), N, K))
    assert torch.equal(y, want)


@pytest.mark.gpu
def test_gpu_gemm_random_matches_the_reference(gpu):
    from dstack_amd.ops import _ext

    C = _ext.require()
    M, N, K = 7, 1024, 4096
    g = torch.Generator(device=gpu).manual_seed(5)
    x = torch.randn(M, K, device=gpu, generator=g).bfloat16()
    w = (torch.randn(N, K, device=gpu, generator=g) * 0.02).bfloat16()
    c, s = C.quant_mxfp4(w)
    xq, xs = C.quant_fp8_rows(x)
    y = C.mxfp4_gemm(xq.view(torch.uint8), xs, *sops.mxfp4_shuffle(c, s), N, K)
    want = ref.mxfp4_linear(x, c, s).float()
    err = ((y.float() - want).norm() / want.norm()).item()
    assert y.shape == (M, N) and err < 5e-3, err


GPU_KW = dict(device="cuda", max_model_len=512, max_batch=8, num_pages=128)


@pytest.mark.gpu
def test_gpu_engine_prefill_through_the_dequant_path(gpu):
    """Two 256-token prompts in one prefill step are 512 rows: past the decode GEMM's 256, so every
    projection is dequantized into the scratch and multiplied by the bf16 GEMM.  Against the bf16
    engine holding the dequantized weights only the bf16 summation order can differ."""
    from dstack_amd.ops import _ext

    C = _ext.require()
    base = _with_dequantized_projections(LLMEngine.from_model("llama-tiny", **GPU_KW), C.quant_mxfp4)
    mx = LLMEngine.from_model("llama-tiny", quantization="mxfp4", **GPU_KW)
    assert all(isinstance(L[k], Mxfp4Weight) for L in mx.model.layers for k in mx.model.FP8_KEYS)
    tokens = torch.arange(1, 513, device=gpu) % 1000
    pos = torch.arange(256, dtype=torch.int32, device=gpu).repeat(2)
    slots = torch.arange(512, dtype=torch.int32, device=gpu)
    a = base.model.prefill(tokens, pos, slots, [0, 256], [256, 256])
    b = mx.model.prefill(tokens, pos, slots, [0, 256], [256, 256])
    cos = torch.nn.functional.cosine_similarity(a.float(), b.float(), dim=-1)
    assert cos.shape == (2,) and cos.min().item() > 0.999, cos


@pytest.mark.gpu
@pytest.mark.parametrize("kv_cache_dtype", ["auto", "fp8"])
def test_gpu_engine_decode_in_graphs_equals_eager(gpu, kv_cache_dtype):
    """The decode path (1-token-block GEMM form, split-K workspaces) inside captured graphs gives the
    token ids of the same engine without graphs: the kernels are deterministic."""
    sp = SamplingParams(max_tokens=16, temperature=0, ignore_eos=True)
    prompts = [[1, 2, 3, 4, 5], list(range(7, 90))]
    eager = LLMEngine.from_model("llama-tiny", quantization="mxfp4", kv_cache_dtype=kv_cache_dtype, **GPU_KW)
    want = [o.output_ids for o in eager.generate(prompts, sp)]
    graphs = LLMEngine.from_model("llama-tiny", quantization="mxfp4", kv_cache_dtype=kv_cache_dtype, **GPU_KW)
    graphs.capture_graphs()
    got = [o.output_ids for o in graphs.generate(prompts, sp)]
    assert all(len(ids) == 16 for ids in got) and got == want
