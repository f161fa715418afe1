"""Plain-PyTorch fp32 reference implementations of every fused op.

These are (a) the numerics oracle the HIP kernels are tested against and (b) the CPU path used by
the CPU-only unit tests. They are never used silently on a GPU: ``dstack_amd.ops`` raises if the
HIP extension is missing on a ROCm device (see ``_ext.require``), unless the user explicitly asks
for ``DSTACK_AMD_OPS=torch`` (A/B benchmarking).
"""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F


def rms_norm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    xf = x.float()
    r = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (xf * r * w.float()).to(x.dtype)


def add_rms_norm(x: torch.Tensor, delta: torch.Tensor, w: torch.Tensor, eps: float):
    h = (x.float() + delta.float()).to(x.dtype)
    return h, rms_norm(h, w, eps)


def swiglu(gu: torch.Tensor) -> torch.Tensor:
    f = gu.shape[-1] // 2
    g, u = gu[..., :f].float(), gu[..., f:].float()
    return (F.silu(g) * u).to(gu.dtype)


def rope_cos_sin(seq_len: int, head_dim: int, theta: float, device=None):
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float64) / head_dim))
    t = torch.arange(seq_len, dtype=torch.float64)
    ang = torch.outer(t, inv)
    return ang.cos().float().to(device), ang.sin().float().to(device)


def apply_rope(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """x: [B, S, H, D] (rotate-half convention, as Llama-3 / HF)."""
    d2 = x.shape[-1] // 2
    xf = x.float()
    x1, x2 = xf[..., :d2], xf[..., d2:]
    c = cos[: x.shape[1]].view(1, x.shape[1], 1, d2)
    s = sin[: x.shape[1]].view(1, x.shape[1], 1, d2)
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).to(x.dtype)


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal: bool = True) -> torch.Tensor:
    """q: [B, S, H, D], k/v: [B, S, KV, D] → [B, S, H, D] (GQA by head repetition)."""
    b, s, h, d = q.shape
    kvh = k.shape[2]
    rep = h // kvh
    qf = q.float().transpose(1, 2)
    kf = k.float().transpose(1, 2).repeat_interleave(rep, dim=1)
    vf = v.float().transpose(1, 2).repeat_interleave(rep, dim=1)
    scores = qf @ kf.transpose(-1, -2) / math.sqrt(d)
    if causal:
        mask = torch.ones(s, kf.shape[2], dtype=torch.bool, device=q.device).triu(1)
        scores = scores.masked_fill(mask, float("-inf"))
    p = scores.softmax(-1)
    return (p @ vf).transpose(1, 2).to(q.dtype)


E4M3_MAX = 448.0


def quant_fp8_rows(x: torch.Tensor):
    """Per-row e4m3 quantization (csrc/fp8.hip ``quant_rows``): q [M, K] float8_e4m3fn, s [M] fp32
    with s = max|x_row| / 448, x ~= q * s."""
    xf = x.float()
    s = xf.abs().amax(dim=1).clamp_min(1e-12) / E4M3_MAX
    q = (xf / s[:, None]).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)
    return q, s


def fp8_linear(x: torch.Tensor, q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """x @ (q * s)^T with x quantized per row first: the math of the fp8 serving GEMMs, in fp32."""
    xq, xs = quant_fp8_rows(x)
    return ((xq.float() * xs[:, None]) @ (q.float() * s[:, None]).t()).to(x.dtype)


# ----------------------------------------------------------------------------------------------
# MXFP4 (OCP Microscaling v1.0): e2m1 elements, one E8M0 scale per block of 32 along K
# ----------------------------------------------------------------------------------------------
MXFP4_BLOCK = 32
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)  # magnitude of code 0..7


def quant_mxfp4(w: torch.Tensor):
    """The canonical MXFP4 form of ``w`` [N, K] (bf16 or fp32, finite, K % 32 == 0): ``codes``
    [N, K/2] uint8 (element 2j in the low nibble, 2j+1 in the high one; a nibble is the sign bit and
    the e2m1 magnitude code) and ``scales`` [N, K/32] uint8 E8M0 (2^(byte - 127)).

    Per block of 32: e = floor(log2(amax)) - 2 clamped to [-127, 127] (-127 for an all-zero block),
    each element x / 2^e rounded to nearest even on the e2m1 grid and saturated at 6, with the
    input's sign bit (zeros and values that round to zero keep it).  Byte 255 is never produced."""
    N, K = w.shape
    if K % MXFP4_BLOCK:
        raise ValueError(f"quant_mxfp4: K = {K} is not a multiple of {MXFP4_BLOCK}")
    x = w.float().reshape(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
    amax = x.abs().amax(dim=-1)
    _, ex = torch.frexp(amax)  # amax = m * 2^ex with m in [0.5, 1): floor(log2(amax)) = ex - 1
    e = torch.where(amax > 0, ex.to(torch.int32) - 3, torch.full_like(ex, -127, dtype=torch.int32)).clamp(-127, 127)
    a = torch.ldexp(x.abs().double(), -e[..., None]).float()  # exact: a power-of-two scaling
    code = torch.where(a < 2, torch.round(2 * a),
                       torch.where(a < 4, 2 + torch.round(a), (4 + torch.round(a / 2)).clamp(max=7)))
    nib = code.to(torch.uint8) | (torch.signbit(x).to(torch.uint8) << 3)
    nib = nib.reshape(N, K // 2, 2)
    codes = nib[..., 0] | (nib[..., 1] << 4)
    return codes.contiguous(), (e + 127).to(torch.uint8).contiguous()


def dequant_mxfp4(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """fp32 [N, K] values of a canonical MXFP4 weight (``quant_mxfp4``)."""
    N, K2 = codes.shape
    nib = torch.stack([codes & 15, codes >> 4], dim=-1).reshape(N, 2 * K2).long()
    lut = torch.tensor(E2M1_VALUES, dtype=torch.float64, device=codes.device)
    mag = lut[nib & 7]
    val = torch.where((nib & 8) != 0, -mag, mag).reshape(N, -1, MXFP4_BLOCK)
    return torch.ldexp(val, (scales.to(torch.int32) - 127)[..., None]).float().reshape(N, 2 * K2)


def mxfp4_linear(x: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """x @ W^T for a canonical MXFP4 weight with x quantized per token to e4m3 first (``quant_fp8_rows``):
    the fp32 product of the two dequantized operands, rounded to bf16 once -- what the decode kernel
    (``csrc/mxfp4.hip``) computes.  Returned in x's dtype."""
    xq, xs = quant_fp8_rows(x)
    y = (xq.float() * xs[:, None]) @ dequant_mxfp4(codes, scales).t()
    return y.to(torch.bfloat16).to(x.dtype)


# ----------------------------------------------------------------------------------------------
# W4A16 (AWQ checkpoints): unsigned 4-bit codes, one fp16 scale and one 4-bit zero point per group
# of ``g`` elements along K and output row; activations stay bf16
# ----------------------------------------------------------------------------------------------
AWQ_ORDER = (0, 2, 4, 6, 1, 3, 5, 7)  # nibble i of an AutoAWQ "GEMM" dword holds column 8 c + AWQ_ORDER[i]
W4_GROUPS = (32, 64, 128)


def _unpack_awq_dwords(packed: torch.Tensor) -> torch.Tensor:
    """int32 [R, C] of 8 nibbles each -> uint8 [R, 8 C] in column order."""
    shifts = torch.arange(0, 32, 4, dtype=torch.int32, device=packed.device)
    nib = (packed.to(torch.int32)[..., None] >> shifts) & 15  # arithmetic shift: the mask drops the sign fill
    inv = sorted(range(8), key=AWQ_ORDER.__getitem__)  # column j of a dword sits in nibble inv[j]
    return nib[..., inv].to(torch.uint8).reshape(packed.shape[0], -1)


def unpack_awq(qweight: torch.Tensor, qzeros: torch.Tensor, scales: torch.Tensor):
    """An AutoAWQ "GEMM" 4-bit linear layer (in = K, out = N, group size g = K / rows of ``qzeros``):
    ``qweight`` int32 [K, N/8], ``qzeros`` int32 [K/g, N/8], ``scales`` fp16 [K/g, N]; nibble i of
    dword c of a row holds column ``8 c + (0, 2, 4, 6, 1, 3, 5, 7)[i]``.  Returns the canonical form of
    W [N, K] = (q - z) * s: ``codes`` uint8 [N, K/2] (element 2j in the low nibble), ``zeros`` uint8
    [N, K/g] (0..15) and ``scales`` fp16 [N, K/g]."""
    K, N8 = qweight.shape
    G = qzeros.shape[0]
    if qweight.dtype != torch.int32 or qzeros.dtype != torch.int32 or tuple(qzeros.shape) != (G, N8) \
            or tuple(scales.shape) != (G, 8 * N8) or G == 0 or K % G or K % 2:
        raise ValueError(f"unpack_awq: qweight {tuple(qweight.shape)} {qweight.dtype}, qzeros {tuple(qzeros.shape)} "
                         f"{qzeros.dtype}, scales {tuple(scales.shape)} are not one AWQ GEMM layer")
    q = _unpack_awq_dwords(qweight).t()  # [N, K]
    codes = (q[:, 0::2] | (q[:, 1::2] << 4)).contiguous()
    zeros = _unpack_awq_dwords(qzeros).t().contiguous()
    return codes, zeros, scales.to(torch.float16).t().contiguous()


def _w4_nibbles(codes: torch.Tensor) -> torch.Tensor:
    return torch.stack([codes & 15, codes >> 4], dim=-1).reshape(codes.shape[0], -1)


def dequant_w4(codes: torch.Tensor, zeros: torch.Tensor, scales: torch.Tensor, g: int) -> torch.Tensor:
    """fp32 [N, K] values ``(q - z) * s`` of a canonical W4 weight (``unpack_awq``, ``quant_w4``); exact:
    an integer of at most 5 bits times an fp16 value."""
    N, K = codes.shape[0], 2 * codes.shape[1]
    if K % g or tuple(zeros.shape) != (N, K // g) or tuple(scales.shape) != (N, K // g):
        raise ValueError(f"dequant_w4: zeros {tuple(zeros.shape)} / scales {tuple(scales.shape)} for [{N}, {K}], g = {g}")
    q = _w4_nibbles(codes).reshape(N, K // g, g).float()
    return ((q - zeros.float()[..., None]) * scales.float()[..., None]).reshape(N, K)


def w4_linear(x: torch.Tensor, codes: torch.Tensor, zeros: torch.Tensor, scales: torch.Tensor, g: int) -> torch.Tensor:
    """x @ W^T for a canonical W4 weight: x times the fp32 dequantized weight, the products accumulated
    in fp64 and rounded once to x's dtype -- the CPU path of the serving engine, whose unquantized
    GEMMs are accumulated the same way, so that a row's result does not depend on how many rows are
    multiplied with it."""
    return (x.double() @ dequant_w4(codes, zeros, scales, g).double().t()).to(x.dtype)


def quant_w4(w: torch.Tensor, g: int = 128):
    """Canonical W4 form (``codes``, ``zeros``, ``scales``: see ``unpack_awq``) of ``w`` [N, K] by plain
    asymmetric min/max round-to-nearest per group of ``g`` along K: s = fp16((max - min) / 15),
    z = clamp(round(-min / s), 0, 15), q = clamp(round(w / s) + z, 0, 15); a group whose range is zero
    (or underflows fp16) gets s = 1, z = 0, q = clamp(round(w), 0, 15).

    This is NOT AWQ: there is no calibration data, no activation-aware channel scaling and no
    clipping search.  It exists to give the built-in random-weight models and the tests a 4-bit
    weight to run on; a served model should come as a calibrated AWQ checkpoint."""
    N, K = w.shape
    if g not in W4_GROUPS or K % g or K % 2:
        raise ValueError(f"quant_w4: K = {K} is not a multiple of the group size {g} (one of {W4_GROUPS})")
    x = w.float().reshape(N, K // g, g)
    mn, mx = x.amin(dim=-1), x.amax(dim=-1)
    s = ((mx - mn) / 15).to(torch.float16)
    flat = s == 0
    s = torch.where(flat, torch.ones_like(s), s)
    sf = s.float()
    z = torch.where(flat, torch.zeros_like(sf), torch.round(-mn / sf).clamp(0, 15))
    q = (torch.round(x / sf[..., None]) + z[..., None]).clamp(0, 15).to(torch.uint8).reshape(N, K // 2, 2)
    codes = q[..., 0] | (q[..., 1] << 4)
    return codes.contiguous(), z.to(torch.uint8).contiguous(), s.contiguous()


def cross_entropy(logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    return F.cross_entropy(logits.float(), target, reduction="mean")


def adamw_(
    param: torch.Tensor,
    grad: torch.Tensor,
    master: torch.Tensor,
    m: torch.Tensor,
    v: torch.Tensor,
    lr: float,
    beta1: float,
    beta2: float,
    eps: float,
    weight_decay: float,
    step: int,
    grad_scale: float = 1.0,
) -> None:
    """Decoupled-weight-decay Adam on an fp32 master copy; writes the bf16 param back."""
    g = grad.float() * grad_scale
    m.mul_(beta1).add_(g, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    bc1 = 1 - beta1**step
    bc2 = 1 - beta2**step
    master.mul_(1 - lr * weight_decay)
    denom = (v / bc2).sqrt_().add_(eps)
    master.addcdiv_(m, denom, value=-lr / bc1)
    param.copy_(master.to(param.dtype))
