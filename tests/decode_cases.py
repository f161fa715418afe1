"""Operands for which the decode kernels are exact, their fp64 references, a comparison that says
where a mismatch sits, and models of the defects these kernels get.

Used by ``tests/test_decode_exact.py`` for ``csrc/gemv.hip`` (gemv), ``csrc/fp8.hip`` (gemv_fp8, the
e4m3 row quantizers, scale_rows_cols_), ``csrc/fp8_gemm.hip`` (fp8_rows_gemm, fp8_stream_gemm) and
``csrc/lora.hip`` (lora_shrink, lora_expand).  Nothing here needs a GPU; every builder takes the
device on which the float work (and the fp64 product) runs.

**GEMV and GEMM operands** (as ``tests/gemm_cases.py``).  Activations in {-1, 0, +1}, non-zero with
probability ``min(1, 4096 / K)``, weights in {-1, +1}, seeded from the shape; both are exact in bf16 and
in e4m3.  Every scale (``sw``, ``xs``, ``ws``, ``rs``, ``cs``) is a power of two in 2^-3 .. 2^3 whose
exponent differs from its neighbour's (``pow2_scales``), so a neighbour's scale is another number.
Every partial sum, in any order, is an integer below 2^24 and a power-of-two scale only moves the
exponent: the one ``f2bf`` is the only rounding, and an integer up to 256 times a power of two is
exact in bf16.  ``check_cap`` (at most 1e-3 of the integer products above 256) is a condition on the
inputs.  The expected output is ``to_bf16(fp64 product x scales)`` and the comparison ``torch.equal``.

**Quantizer rows** are built from the bytes they must give: a row is ``decode(codes) * 2^e`` with one
element of magnitude 448 * 2^e, so the scale is exactly 2^e, ``1 / scale`` and every product are
exact and the expected byte is the code itself.  Tie elements sit exactly between two neighbouring
e4m3 values (bf16 holds them); the expected byte is the even one.  The SwiGLU form takes gate values
0, 2^p or 2^(p+1) with p >= 5: ``1 + exp(-g)`` is 1 in fp32, so ``silu(g) = g`` exactly and the
product with an up value from the set above is exact in bf16.

**LoRA.**  shrink: x in {-1, 0, +1}, A in {-1, +1}, the fp32 output is the integer product.  expand:
t and B in {-1, 0, +1}, y0 integers in [-32, 32], so |y| <= 96 and bf16 holds the result.
"""

from __future__ import annotations

import functools
from types import SimpleNamespace

import torch

from tests import gemm_cases as gc
from tests.gemm_cases import BF16, E4M3, F32, F64, check_cap, e4m3_bytes, to_bf16

from dstack_amd.ops import reference as ref
from dstack_amd.ops.serving import fp8_stream_shuffle

U8, I8, I32 = torch.uint8, torch.int8, torch.int32
OLD_GEMV_BOUND, OLD_GEMM_BOUND = 5e-3, 1e-2  # the older tests' bounds on ||y - ref|| / ||ref||
NAN = float("nan")


def _gen(*dims: int) -> torch.Generator:
    return torch.Generator().manual_seed(gc._seed(0xDEC0DE, *dims))


def pow2_scales(n: int, *tag: int) -> torch.Tensor:
    """fp64 [n], 2^e with e in -3 .. 3 and e[i] != e[i + 1] (steps of 1 .. 6 modulo 7)."""
    d = torch.randint(1, 7, (n,), generator=_gen(n, *tag))
    return torch.ldexp(torch.ones(n, dtype=F64), torch.cumsum(d, 0) % 7 - 3)


def check_scales(s: torch.Tensor):
    e = torch.log2(s.to(F64))
    assert torch.equal(e, e.round()) and e.min().item() >= -3 and e.max().item() <= 3
    assert s.numel() == 1 or bool((s[1:] != s[:-1]).all()), "a neighbour's scale must be another number"
    assert s.numel() < 64 or len(e.unique()) == 7


def signs(rows: int, K: int, g: torch.Generator) -> torch.Tensor:
    return torch.randint(0, 2, (rows, K), generator=g, dtype=I8) * 2 - 1


def activations(rows: int, K: int, g: torch.Generator) -> torch.Tensor:
    """int8 [rows, K] in {-1, 0, +1}, non-zero with probability min(1, 4096 / K)."""
    x = signs(rows, K, g)
    if K > 4096:
        x = x * (torch.rand(rows, K, generator=g) < 4096 / K).to(I8)
    return x


def product_i8(x: torch.Tensor, W: torch.Tensor, chunk: int = 2048) -> torch.Tensor:
    """x [M, K] W [N, K]^T in fp64 on the operands' device, W converted ``chunk`` rows at a time."""
    xd = x.to(F64)
    return torch.cat([xd @ W[i:i + chunk].to(F64).t() for i in range(0, W.shape[0], chunk)], 1)


def padded(x: torch.Tensor, left: int, right: int, fill) -> tuple[torch.Tensor, torch.Tensor]:
    """(buffer, view): ``x`` as a column slice of a wider buffer whose other columns hold ``fill``."""
    big = torch.full((x.shape[0], left + x.shape[1] + right), fill, dtype=x.dtype, device=x.device)
    v = big[:, left:left + x.shape[1]]
    v.copy_(x)
    return big, v


def rows_distinct(W: torch.Tensor) -> bool:
    """Sufficient: the rows' first 64 signs, packed into one word each, are all different."""
    k = min(W.shape[1], 62)
    key = ((W[:, :k] > 0).to(torch.int64) << torch.arange(k)).sum(1)
    return key.unique().numel() == W.shape[0]


# ==================================================================================================
# gemv and gemv_fp8
# ==================================================================================================
GEMV_N = [3, 32, 37, 1027]            # grid 1 (nwg < 8) | grid 8, rem 0 | grid 10, rem 2, one live row | 257 workgroups
GEMV_K = [512, 2048, 2560, 3584, 14336]  # tail only | one unrolled step | + 1 tail step | + 3 | 7 steps
GEMV8_N = [1027, 8197, 16391]         # 1, 2 and 4 rows per wave (dsa_gemv_fp8), each with a part-filled last wave
GEMV8_K = [1024, 2048, 3072]          # the second unrolled load absent | both | a second trip with one


def gemv_fp8_rows(N: int) -> int:
    """Rows per wave, the rule of ``dsa_gemv_fp8``."""
    return 4 if N // 16 >= 1024 else 2 if N // 8 >= 1024 else 1


def gemv_plan(N: int, R: int = 1):
    """Grid and tail of a launch with R rows per wave (4 waves per workgroup, XCD-banded)."""
    grid = -(-N // (4 * R))
    waves = -(-N // R)
    return SimpleNamespace(grid=grid, rem=grid & 7, banded=grid >= 8, last_wg_waves=waves - 4 * (grid - 1),
                           last_nr=N - R * (waves - 1))


def gemv_steps(K: int) -> tuple[int, int]:
    """(unrolled 2048-column steps, 512-column tail steps) of ``gemv_kernel<M, 4>``."""
    full = 0 if K < 2048 else (K - 1536 - 1) // 2048 + 1
    return full, (K - 2048 * full) // 512


@functools.lru_cache(maxsize=2)
def gemv_operands(N: int, K: int, fp8: bool = False):
    """(x int8 [4, K], W int8 [N, K], sw fp64 [N]) on the CPU."""
    g = _gen(N, K, int(fp8))
    return activations(4, K, g), signs(N, K, g), pow2_scales(N, K)


@functools.lru_cache(maxsize=2)
def gemv_case(N: int, K: int, fp8: bool = False, device: str = "cpu"):
    """x bf16 [4, K] (a test takes the first M rows); W bf16 [N, K], or e4m3 bytes with ``sw`` fp32 [N];
    ``exact`` fp64 [4, N] and ``want`` its bf16 rounding.  Never modified by a test."""
    x8, W8, sw = gemv_operands(N, K, fp8)
    x8, W8, sw = x8.to(device), W8.to(device), sw.to(device)
    ints = product_i8(x8, W8)
    share = check_cap(ints)
    exact = ints * sw if fp8 else ints
    W = e4m3_bytes(W8) if fp8 else W8.to(BF16)
    return SimpleNamespace(N=N, K=K, fp8=fp8, x=x8.to(BF16), W=W, sw=sw.to(F32), x8=x8, W8=W8, ints=ints, exact=exact,
                           want=to_bf16(exact), share=share)


def gemv_where(N: int, R: int = 1):
    last = (N - 1) // R
    return lambda m, n: {"workgroup (of the row order)": n // (4 * R), "wave": n // R % 4, "row of its wave": n % R,
                         "in the part-filled last wave": ((n // R == last) & (N % R != 0)).int()}


# ==================================================================================================
# fp8_rows_gemm and fp8_stream_gemm
# ==================================================================================================
ROWS_M = [1, 37, 64, 65, 200, 256]  # partial 64-row blocks
ROWS_N = [128, 384]
ROWS_K = [128, 256, 384, 512, 2048]  # one step (under the two-ahead prologue) | 2 | the ring's 3 slots | 4 | 16
STREAM_M = [1, 129, 200, 256]
STREAM_KS = [(512, 1), (1024, 2), (2048, 1), (3584, 7)]  # (K, split): 4 steps, the minimum, per K slice but at 2048
STREAM_FORMS = [(rw, sh) for rw in (64, 32, 28) for sh in (0, 1, 2)]


def stream_wg_rows(rw: int) -> int:
    return 224 if rw == 28 else 256


def stream_depths(rw: int):
    return (2, 3) if rw == 32 else (2,)


def stream_supported(M: int, N: int, K: int, rw: int, S: int) -> bool:
    """What ``dsa_fp8_stream_gemm_supported`` offers (rw 64 without split only)."""
    return (0 < M <= 256 and (rw in (32, 28) or (rw == 64 and S == 1)) and N > 0 and N % stream_wg_rows(rw) == 0
            and S >= 1 and K > 0 and K % (512 * S) == 0)


@functools.lru_cache(maxsize=2)
def gemm_case(M: int, N: int, K: int, device: str = "cpu"):
    """e4m3 bytes ``xq`` [M, K], ``wq`` [N, K], fp32 ``xs`` [M], ``ws`` [N]; ``ints`` the fp64 product,
    ``exact`` = ints x xs x ws, ``want`` its bf16 rounding.  A test with fewer rows or columns takes the
    leading ones (``sub``).  Never modified by a test."""
    a64, b64, _ = gc.operands(M, N, K, 0xF8)
    xs, ws = pow2_scales(M, K, 1).to(device), pow2_scales(N, K, 2).to(device)
    a, b = a64.to(device), b64.to(device)
    ints = gc.product(a, b)
    share = check_cap(ints)
    exact = ints * xs[:, None] * ws[None, :]
    return SimpleNamespace(M=M, N=N, K=K, a=a, b=b, xq=e4m3_bytes(a), wq=e4m3_bytes(b), xs=xs.to(F32), ws=ws.to(F32),
                           xs64=xs, ws64=ws, ints=ints, exact=exact, want=to_bf16(exact), share=share)


def sub(c, M: int, N: int):
    """The leading M token rows and N weight rows of a case (contiguous operands)."""
    return SimpleNamespace(M=M, N=N, K=c.K, xq=c.xq[:M], wq=c.wq[:N], xs=c.xs[:M].contiguous(), ws=c.ws[:N].contiguous(),
                           exact=c.exact[:M, :N], want=c.want[:M, :N].contiguous())


def stream_weight(wq: torch.Tensor, rw: int, shuffled: int) -> torch.Tensor:
    if not shuffled:
        return wq.contiguous()
    return fp8_stream_shuffle(wq.contiguous(), 16 if shuffled == 1 else stream_wg_rows(rw))


def rows_gemm_where(m, n):
    return {"64-row block": m // 64, "128-column block": n // 128, "wave row (32 rows)": m % 64 // 32,
            "wave column (32 columns)": n % 128 // 32, "16-column block of the wave": n % 32 // 16,
            "register of the lane (n % 4)": n % 4}


def stream_where(rw: int):
    wgr, wave = stream_wg_rows(rw), 64 if rw == 64 else 32
    return lambda m, n: {"workgroup": n // wgr, "wave": n % wgr // wave, "fragment of the wave": n % wgr % wave // 16,
                         "token block (16 rows)": m // 16, "register of the lane (n % 4)": n % 4}


# ==================================================================================================
# The e4m3 row quantizers
# ==================================================================================================
QUANT_K = [8, 2048, 2056, 4096, 4104, 8200, 16392, 32768, 32776]  # NIT 2 | 2 | 2 | 2 | 4 | 8 | 16 | 16 | two passes
SWIGLU_F = [4096, 4104, 8192, 8200, 16384, 16392, 32768, 32776]   # 2048 x {2, 4, 8, 16} and 8192 x {2, 4}, + 8; > 32768
SWIGLU_M = [3, 513]                                                 # 1024 threads per row (M <= 512) | 256
SCALE_N = [8, 2048, 2056]
CODE_MAX = 0x7E          # 448
ZERO_ROW_SCALE = (torch.tensor(1e-12, dtype=F32) / 448.0).item()


def quant_nit(K: int) -> int:
    """The register-resident form ``dsa_quant_fp8_rows`` picks (0: two passes)."""
    nit = (K + 2047) // 2048
    return 2 if nit <= 2 else 4 if nit <= 4 else 8 if nit <= 8 else 16 if nit <= 16 else 0


def swiglu_form(M: int, F: int) -> tuple[int, int]:
    """(NIT, threads per row) of ``dsa_swiglu_quant_fp8_rows``."""
    nit4 = (F + 8191) // 8192
    if M <= 512 and nit4 <= 4:
        return (2 if nit4 <= 2 else 4), 1024
    return quant_nit(F), 256


def pow2(e: torch.Tensor) -> torch.Tensor:
    """fp32 2^e for integer -126 <= e <= 127, from the exponent bits: exact on any device (an ``ldexp``
    or ``pow`` on the GPU is not, from 2^16 on)."""
    return ((e.to(torch.int32) + 127) << 23).view(F32)


def decode(codes: torch.Tensor) -> torch.Tensor:
    """e4m3 bytes -> fp32 values (exact)."""
    return codes.view(E4M3).to(F32)


def _max_column(i: int, K: int) -> int:
    """Where row i holds its largest element: first, middle, in the last 8-column chunk (twice), just
    past the first 2048 columns (a first-pass-only absmax misses it) -- in turn."""
    return [0, K // 2, K - 3, K - 8, min(K - 1, 2048 + 5)][i % 5]


QUANT_E = [0, -5, 7, 0, 3, -8, 2, 6]  # the exponent of row i's scale; row 3 is all zeros


def quant_rows_case(K: int, device: str = "cpu"):
    """x bf16 [8, K]; the bytes ``q`` and scales ``s`` it must give.  Rows 0, 1, 2: the maximum first,
    in the middle, in the last chunk; row 3 zeros; rows 4 ..: one element in 8 is a tie (exactly between
    codes c and c + 1, expected the even one), the maximum at the places of ``_max_column``."""
    g = _gen(K, 5)
    R = len(QUANT_E)
    mag = torch.randint(0, CODE_MAX, (R, K), generator=g, dtype=U8)      # 0 .. 0x7D: below 448
    neg = torch.randint(0, 2, (R, K), generator=g, dtype=U8) * (mag > 0)  # (no negative zero)
    tie = (torch.rand(R, K, generator=g) < 0.125) & (torch.arange(R)[:, None] >= 4) & (mag < CODE_MAX - 1)
    for i in range(R):
        mag[i, _max_column(i, K)], tie[i, _max_column(i, K)] = CODE_MAX, False
    mag[3], neg[3], tie[3] = 0, 0, False
    sign = 1.0 - 2.0 * neg.to(F32)
    val = torch.where(tie, (decode(mag) + decode(mag + 1)) / 2, decode(mag)) * sign
    want = torch.where(tie, (mag + 1) & 0xFE, mag) | (neg << 7)
    e = torch.tensor(QUANT_E)
    x = torch.ldexp(val, e[:, None])
    s = torch.ldexp(torch.ones(R), e).to(F32)
    s[3] = ZERO_ROW_SCALE
    assert torch.equal(x.to(BF16).to(F32), x), "the rows must be exact in bf16"
    return SimpleNamespace(K=K, x=x.to(BF16).to(device), q=want.to(device), s=s.to(device), ties=int(tie.sum()))


def quant_where(r, c):
    return {"row": r, "2048-column step": c // 2048, "thread (8-column chunk % 256)": c // 8 % 256}


@functools.lru_cache(maxsize=2)
def _swiglu_codes(M: int, F: int):
    g = _gen(M, F, 6)
    code = torch.randint(0x10, CODE_MAX, (M, F), generator=g, dtype=U8)  # exponent field >= 2: half of it is normal
    neg = torch.randint(0, 2, (M, F), generator=g, dtype=U8)
    sel = torch.randint(0, 3, (M, F), generator=g, dtype=U8)             # gate 0 | 2^p | 2^(p + 1)
    rows = torch.arange(M)
    cols = torch.tensor([_max_column(i, F) for i in range(M)])
    code[rows, cols], sel[rows, cols] = CODE_MAX, 2
    neg = neg * (sel > 0)                                                # (0 x a negative up value is -0)
    want = torch.where(sel == 0, torch.zeros_like(code), torch.where(sel == 1, code - 8, code) | (neg << 7))
    return code | (neg << 7), sel, want


def swiglu_case(M: int, F: int, scaled: bool, device: str = "cpu"):
    """gu bf16 [M, 2F] (gate | up) and the bytes and scales ``swiglu_quant_fp8_rows`` must give; with
    ``scaled`` the raw gu, ``rs`` [M] and ``cs`` [2F] of the deferred-scale form (gu x rs x cs is the
    gu of the plain form, exactly).  Row i: up = decode(code) x 2^e_i, gate in {0, 2^p_i, 2^(p_i + 1)},
    p_i >= 5; the largest product, 448 x 2^(e_i + p_i + 1), once per row."""
    code, sel, want = (t.to(device) for t in _swiglu_codes(M, F))
    rows = torch.arange(M, device=device)
    e, p = rows * 5 % 17 - 8, 5 + rows % 4
    up = decode(code) * pow2(e)[:, None]
    gate = torch.where(sel == 0, torch.zeros((), device=device), pow2(p[:, None] + sel - 1))
    s = pow2(e + p + 1)
    gu = torch.cat([gate, up], 1)
    rs = cs = None
    if scaled:
        rs, cs = pow2_scales(M, F, 3).to(device, F32), pow2_scales(2 * F, M, 4).to(device, F32)
        gu = gu / rs[:, None] / cs[None, :]
    return SimpleNamespace(M=M, F=F, gu=gu.to(BF16), gu32=gu, rs=rs, cs=cs, q=want, s=s, e=e, p=p)


def swiglu_product(c) -> torch.Tensor:
    """bf16 [M, F]: what the kernel quantizes, by plain arithmetic (silu(g) = g on these gates)."""
    gu = c.gu.to(F32)
    if c.rs is not None:
        gu = (gu * c.rs[:, None] * c.cs[None, :]).to(BF16).to(F32)
    return (gu[:, :c.F] * gu[:, c.F:]).to(BF16)


def scale_case(N: int, device: str = "cpu"):
    """y bf16 [5, N] integers in [-256, 256], rs [5], cs [N]; ``want`` = bf16(y x rs x cs), exact."""
    g = _gen(N, 7)
    y = torch.randint(-256, 257, (5, N), generator=g).to(F64)
    rs, cs = pow2_scales(5, N, 8), pow2_scales(N, 9)
    return SimpleNamespace(N=N, y=y.to(BF16).to(device), rs=rs.to(device, F32), cs=cs.to(device, F32),
                           want=to_bf16(y * rs[:, None] * cs[None, :]).to(device))


# ==================================================================================================
# LoRA
# ==================================================================================================
SHRINK_K = [8, 256, 512, 520, 2048, 2056, 4104, 28672]  # one chunk | half a wave step | one | + 1 chunk | every wave once | ...
SHRINK_L = [8, 24, 192]
LORA_S = 3
LORA_IDX = [0, -1, 2, 2, 1, LORA_S, 0]   # no adapter, a slot past the end, repeated slots
EXPAND_R = [8, 16, 32, 64]
CANARY = 123.0


def expand_cols(R: int) -> int:
    """Columns per lora_expand workgroup."""
    return 256 // (R // 8) * 4


def expand_shapes(R: int):
    """(N, slice ends): N one short of, at and one past a workgroup's span, each with a one-column
    middle slice; N = 1000 with (333, 334, 1000), one slice, and a one-column last slice."""
    c = expand_cols(R)
    out = [(N, (N // 3, N // 3 + 1, N)) for N in (c - 1, c, c + 1)]
    return out + [(1000, (333, 334, 1000)), (1000, (1000,)), (1000, (999, 1000))]


def lora_live(idx=LORA_IDX, S: int = LORA_S):
    return [r for r, s in enumerate(idx) if 0 <= s < S]


@functools.lru_cache(maxsize=2)
def shrink_case(K: int, device: str = "cpu"):
    """x bf16 [T, K], A bf16 [S, 192, K] (a test takes the leading L rows), idx int32 [T]; ``want``
    fp32 [T, 192]: the integer product on the rows with an adapter, CANARY elsewhere."""
    g = _gen(K, 10)
    T, L = len(LORA_IDX), max(SHRINK_L)
    x8 = activations(T, K, g).to(device)
    A8 = signs(LORA_S * L, K, g).view(LORA_S, L, K).to(device)
    want = torch.full((T, L), CANARY, dtype=F64, device=device)
    for r in lora_live():
        want[r] = A8[LORA_IDX[r]].to(F64) @ x8[r].to(F64)
    assert want.abs().max().item() < 2 ** 24
    return SimpleNamespace(K=K, x=x8.to(BF16), A=A8.to(BF16), idx=torch.tensor(LORA_IDX, dtype=I32, device=device),
                           want=want.to(F32))


def expand_case(R: int, N: int, ends: tuple, device: str = "cpu"):
    """t fp32 [T, nsl R] and B bf16 [S, N, R] in {-1, 0, +1}, y0 bf16 [T, N] integers in [-32, 32];
    ``want`` bf16 [T, N] (rows without an adapter: y0)."""
    g = _gen(R, N, *ends)
    T, nsl = len(LORA_IDX), len(ends)
    t = torch.randint(-1, 2, (T, nsl * R), generator=g).to(F64)
    B = torch.randint(-1, 2, (LORA_S, N, R), generator=g).to(F64)
    y0 = torch.randint(-32, 33, (T, N), generator=g).to(F64)
    want = expand_ref(t, B, y0, ends, R)
    assert want.abs().max().item() <= 96
    return SimpleNamespace(R=R, N=N, ends=ends, t=t.to(device, F32), B=B.to(device, BF16), y0=y0.to(device, BF16),
                           idx=torch.tensor(LORA_IDX, dtype=I32, device=device), want=to_bf16(want).to(device),
                           t64=t, B64=B, y64=y0)


def expand_ref(t, B, y0, ends, R: int) -> torch.Tensor:
    out = y0.clone()
    for r in lora_live():
        lo = 0
        for j, hi in enumerate(ends):
            out[r, lo:hi] += B[LORA_IDX[r], lo:hi] @ t[r, j * R:(j + 1) * R]
            lo = hi
    return out


def expand_where(R: int, ends: tuple):
    c, N = expand_cols(R), ends[-1]
    e0, e1 = (ends[0] if len(ends) > 1 else N), (ends[1] if len(ends) > 2 else N)
    return lambda m, n: {"slice": (n >= e0).int() + (n >= e1).int(), "workgroup": n // c,
                         "column group of the workgroup": n % c // (c // 4)}


# ==================================================================================================
# The comparison
# ==================================================================================================
def _fmt(v: torch.Tensor, limit: int = 24) -> str:
    s = v.unique().tolist()
    return str(s) if len(s) <= limit else f"{s[:limit]} ... ({len(s)} in all)"


def mismatch_report(out: torch.Tensor, want: torch.Tensor, where=None) -> str | None:
    """None when ``out`` equals ``want`` element for element, else where it does not: the count, the
    first bad (row, column), the rows and columns hit, what ``where(rows, columns)`` says about them
    (the row block, wave, tail or slice: a dict of names to integer tensors) and the first eight
    elements.  Never a whole tensor."""
    assert out.shape == want.shape, (tuple(out.shape), tuple(want.shape))
    assert out.dtype == want.dtype, (out.dtype, want.dtype)
    want = want.to(out.device)
    if torch.equal(out, want):
        return None
    if out.dim() == 1:
        out, want = out[None, :], want[None, :]
    idx = (out != want).nonzero()  # (a NaN differs from everything)
    r, c = idx[:, 0], idx[:, 1]
    lines = [f"{idx.shape[0]} of {out.numel()} elements differ, the first at (row {int(r[0])}, column {int(c[0])})",
             f"rows {_fmt(r)}, columns {int(c.min())}..{int(c.max())} ({c.unique().numel()} of them)"]
    if where is not None:
        lines += [f"{name} in {_fmt(v)}" for name, v in where(r, c).items()]
    lines.append("first (row, column, got, want): " + ", ".join(
        f"({i}, {j}, {out[i, j].item()!r}, {want[i, j].item()!r})" for i, j in idx[:8].tolist()))
    return "\n  ".join(lines)


def assert_exact(out: torch.Tensor, want: torch.Tensor, where=None, what: str = ""):
    rep = mismatch_report(out, want, where)
    assert rep is None, f"{what + ': ' if what else ''}{rep}"


def old_metric(out: torch.Tensor, exact: torch.Tensor) -> float:
    """What the older tests bound: the relative Frobenius norm of the error."""
    return ((out.to(F64) - exact.to(F64)).norm() / exact.to(F64).norm()).item()


# ==================================================================================================
# Defect models: what a kernel with the defect would store, from a case on the CPU
# ==================================================================================================
def _k_part(c, n0: int, n1: int, k0: int, k1: int) -> torch.Tensor:
    """[4, n1 - n0] fp64: the k0 .. k1 terms of a GEMV case's outputs n0 .. n1 (scaled like them)."""
    part = c.x8[:, k0:k1].to(F64) @ c.W8[n0:n1, k0:k1].to(F64).t()
    return part * c.sw[n0:n1].to(F64) if c.fp8 else part


def gemv_defect(c, kind: str) -> torch.Tensor:
    """bf16 [4, N]: a gemv / gemv_fp8 case's output with one defect.
    ``lost_chunk``: lane 37 of the wave of row N / 2 drops its chunk (8 columns; 16 for fp8) of the first step;
    ``tail_step``: the last 512 (fp8: 1024) columns are never added (a skipped K-tail step), in every row;
    ``tail_unwritten`` / ``tail_copied``: the part-filled last wave's rows keep 0 / repeat the row before them;
    ``neighbour_scale``: row n is scaled by sw[n + 1] (fp8)."""
    N, K, R = c.N, c.K, gemv_fp8_rows(c.N) if c.fp8 else 1
    p = c.exact.clone()
    if kind == "lost_chunk":
        w, n = (16 if c.fp8 else 8), N // 2
        p[:, n:n + 1] -= _k_part(c, n, n + 1, 37 * w, 38 * w)
    elif kind == "tail_step":
        p -= _k_part(c, 0, N, K - (1024 if c.fp8 else 512), K)
    elif kind in ("tail_unwritten", "tail_copied"):
        n0 = (N - 1) // R * R if c.fp8 else (N - 1) // 4 * 4  # the last wave's (gemv: the last workgroup's) first row
        assert 0 < n0 < N
        p[:, n0:] = 0.0 if kind == "tail_unwritten" else p[:, n0 - 1:n0]
    elif kind == "neighbour_scale":
        assert c.fp8
        p[:, :-1] = c.ints[:, :-1] * c.sw[1:].to(F64)
    else:
        raise ValueError(kind)
    return to_bf16(p)


def gemm_defect(c, kind: str, M: int | None = None, every_tile: bool = True) -> torch.Tensor:
    """bf16: an fp8_rows_gemm case's output (64 x 128 tiles) with one defect, in every tile or tile (0, 0).
    ``wrong_register``: one lane stores its other 16-column block's 4-column register in place of its own;
    ``stale_slot``: wave (1, 2)'s 32 x 32 quadrant reads the last K-step's activations from the slot's previous
    occupant (the step before);
    ``neighbour_scale``: row m is scaled by xs[m + 1];
    ``padded_row``: with M rows of a 256-row buffer live, the first padded row is stored too (returns the
    buffer: [256, N], the rest NaN)."""
    p = c.exact.clone()
    K, steps = c.K, c.K // 128
    tiles = [(i, j) for i in range(c.M // 64) for j in range(c.N // 128)] if every_tile else [(0, 0)]
    if kind == "wrong_register":
        for i, j in tiles:
            m, n = 64 * i + 32 + 5, 128 * j + 64 + 8
            p[m, n:n + 4] = c.exact[m, n + 16:n + 20]
    elif kind == "stale_slot":
        assert steps >= 2
        ka, kb = (steps - 2) * 128, (steps - 1) * 128
        for i, j in tiles:
            rows, cols = slice(64 * i + 32, 64 * i + 64), slice(128 * j + 64, 128 * j + 96)
            w = c.b[cols, kb:kb + 128]
            d = gc.product(c.a[rows, ka:ka + 128], w) - gc.product(c.a[rows, kb:kb + 128], w)
            p[rows, cols] += d * c.xs64[rows, None] * c.ws64[None, cols]
    elif kind == "neighbour_scale":
        p[:-1] = c.ints[:-1] * c.xs64[1:, None] * c.ws64[None, :]
    elif kind == "padded_row":
        buf = torch.full_like(p, NAN)
        buf[:M + 1] = p[:M + 1]
        return to_bf16(buf)
    else:
        raise ValueError(kind)
    return to_bf16(p)


def padded_want(c, M: int) -> torch.Tensor:
    buf = torch.full_like(c.exact, NAN)
    buf[:M] = c.exact[:M]
    return to_bf16(buf)


def expand_defect(c, shift: int = 1) -> torch.Tensor:
    """bf16 [T, N]: lora_expand with its first slice end off by ``shift``."""
    ends = (c.ends[0] + shift,) + tuple(c.ends[1:])
    return to_bf16(expand_ref(c.t64, c.B64, c.y64, ends, c.R))


def quant_first_pass_only(x: torch.Tensor):
    """(q bytes, s): ``reference.quant_fp8_rows`` with the absmax taken over the first 2048 columns only."""
    xf = x.float()
    s = xf[:, :2048].abs().amax(dim=1).clamp_min(1e-12) / 448.0
    q = (xf / s[:, None]).clamp(-448.0, 448.0).to(E4M3)
    return q.view(U8), s


def quant_reference(x: torch.Tensor):
    q, s = ref.quant_fp8_rows(x)
    return q.view(U8), s
