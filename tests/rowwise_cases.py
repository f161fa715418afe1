"""Inputs, fp64 references, the per-element judge and the defect models for the row-wise kernels of
``csrc/elementwise.hip``.  Used by ``tests/test_rowwise_exact.py``; nothing here needs a GPU.

**The judge.**  Every stored element is compared with fp64 arithmetic on the exact bf16 / fp32 input
values, reproducing the roundings the kernels document (``h = bf16(x + delta)``, ``bf16(delta*dr*dc)``,
``bf16(y)`` before e4m3).  With u = 2^-24 (the relative error of one fp32 operation) an element passes when

    |got - ref| <= [ulp_bf16(ref)] + c * u * T + 2^-126

where the first term is there for a bf16 output only, T is the sum of the magnitudes of the terms the
element is made of (given per kernel below), c counts the fp32 roundings on the element's path, and
2^-126 lets a subnormal result be flushed.  ``C_CAP`` = 64 is the most any kernel may claim.  Nothing
here is taken from what the HIP kernels return; ``Fp32Impl`` (``ops.reference`` on fp32 CPU tensors)
goes through the same judge in the non-GPU tests, which print how much of each bound it uses.

**c, per kernel** (n = 8 * ceil(chunks / threads per row): the per-thread serial chain of a row
reduction; +6 for the wave shuffle levels, +3 for the 4-entry LDS combine of a 256-thread workgroup;
rsqrtf, __expf's v_exp_f32 and __logf's v_log_f32 are taken as 1 ulp = 2 u, the figure of the public
HIP math API tables for the native instructions -- no copy of that table ships with the toolchain, so
no file is cited; fp32 division and sqrtf are correctly rounded by hipcc's default):

* RMSNorm forward.  ss = sum h^2 passes n + 6 (+3) roundings (the squares are fused into the adds),
  / D and + eps add 2; r = rsqrt(.) halves a relative error and adds 2:
  c_rstd = (n + 6 [+3] + 2) / 2 + 2, T = |rstd|.  y = h r w adds two products: c_y = c_rstd + 2,
  T = |h r w|.  Block-per-row (256 threads, D <= 8192): n <= 32, c_y <= 25.5.  Wave-per-row (64 lanes):
  D = 4104 n = 72, c_y = 44; D = 6144 n = 96, c_y = 56; D = 8192 n = 128, c_y = 72 in the worst case --
  held to the cap of 64, which only makes that case stricter.  h = bf16(x + delta) is one IEEE fp32 add
  and one rounding on both sides: compared bit for bit.
* RMSNorm backward.  g = dy w (1), dot = sum g h (n + 9, n <= 32), k = dot r r r / D (4), r g (1),
  h k (1), the subtraction (1), + dres (1): c_dx = n + 18 <= 50,
  T = |dres| + |r g| + |h| r^3 / D * sum_j |g_j h_j| (the projection is made of every term of the dot).
  dw: dy h r (2), the rows one workgroup takes (ceil(rows / grid) <= 3), colsum pass 1
  (ceil(rpb / 4) <= 16 per wave, +3 LDS), pass 2 (min(16, P)), the bf16 accumulate (1): c_dw <= 41,
  T = sum_rows |dy h r| (+ |old|).
* SwiGLU.  s = 1 / (1 + exp(-g)): the argument scaling of __expf weighs |g| (1 - s) =: q, v_exp 2,
  the add 1, the division 1; a = g s u adds 2: <= 6 + q roundings, so c = 8 with
  T_a = |a| (1 + q).  du = d g s the same.  dg = A B, A = d u s, B = 1 + g (1 - s): the error of B is
  at most u (|g| (q + 6) + |B|), so c = 8 with T_dg = |A| (|B| + |g|) (1 + q).
* Cross-entropy forward.  A logit's exp (3), the 8 adds of its chunk, ceil(V / 2048) per-thread merges,
  6 wave and 3 LDS merges (one multiply-add each once the running maximum stands), __logf (2) and the
  add of the maximum (1): c_lse = ceil(V / 2048) + 24 (25, 25, 26, 40 for V <= 32000; 87 at
  V = 128256, held to 64), T_lse = |max| + |log s| + 1 (a relative error of s is an absolute one of
  log s).  loss = lse - logit[target]: c + 1, T + |logit[target]|.
* Cross-entropy backward (lse supplied by the test).  x = logit - lse (1), the argument scaling (|x|),
  v_exp (2), the one-hot (1), the scale (1): c = 6, T = |scale| (p (1 + |x|) + onehot).
* AdamW (hyper-parameters as the fp32 values the kernel receives).  The kernel forms 1 - b from the
  fp32 b, the plain reference from the double: the two differ by b / (1 - b) u of the term, 9 u for
  b1 = 0.9 and 19 u for b2 = 0.95, and either is right.  m: g gscale (1), two products and an add, the
  9: c = 13, T = |b1 m| + |(1 - b1) g|.  v: one product more and the 19: c = 24,
  T = |b2 v| + |(1 - b2) g^2|.  master: decay (2) and its product (1); the update step_size m / denom
  with denom = sqrt(v) rsqrt(bc2) + eps (24 / 2 + 1 + 3 + 1), step_size (1), the product, division and
  subtraction (3), m's own 13: c = 34, T = |p decay| + step_size / denom * T_m.

**Fractions of the bound used by the fp32 reference on the CPU** (largest err / bound over every case
of ``test_fp32_reference_is_inside_every_bound``): rms_norm y 0.500, rstd 0.241; add_rms_norm y 0.500,
rstd 0.271; rms_norm_bwd dx 0.500, dw fp32 0.389, dw bf16 0.500; swiglu a 0.500, dgu 0.500;
cross-entropy lse 0.030, loss 0.021, gradient 0.499; AdamW m 0.338, v 0.205, master 0.105.  (A bf16
output uses half of its bound: the rounding itself.)  The e4m3 norm is held to the bounds the format
sets (scale within 2^-7, bytes within one e4m3 step); the fp32 reference uses 0.500 of the step and
none of the scale's.  h, the exact RMSNorm backward, the embedding backward, RoPE, the transposes and
AdamW's param are compared bit for bit.  (Embedding backward: a row whose id does not occur keeps its
bits in the accumulating form; the storing form clears the table first, so there it must be zero.)

**Shapes** (chunk = 8 columns; ``NCH_DISPATCH`` wave-per-row: NCH = ceil(chunks / 64) rounded up to
1, 2, 4, 8, 16; ``NCH_DISPATCH_BLK`` block-per-row: ceil(chunks / 256) rounded up to 1, 2, 4):

    D      chunks  wave-per-row NCH (last pass)   block-per-row NCH (last pass)
    8      1       1  (1 lane of 64)              1  (1 thread of 256)
    256    32      1  (32)                        1  (32)
    520    65      2  (1)                         1  (65)
    1032   129     4  (3 passes, last 1)          1  (129)
    2048   256     4  (4 passes, full)            1  (256, full)
    2056   257     8  (5 passes, last 1)          2  (1)
    3584   448     8  (7 passes, full)            2  (192)
    4104   513     16 (9 passes, last 1)          4  (3 passes, last 1)
    6144   768     16 (12 passes, full)           4  (3 passes, full)
    8192   1024    16 (16 passes, full)           4  (4 passes, full)

Forward rows 1, 3, 1024: block-per-row (rows <= 1024); 1025, 1027: wave-per-row, 4 rows per workgroup
with 1 and 3 rows in the last one.  Backward rows (grid = min(rows, 1024), P = grid partial rows for
``colsum``, rpb = ceil(P / 16)): 1, 3, 17 -> P 1, 3, 17 (rpb 1, 1, 2: ``blockIdx.y`` ranges past P are
empty); 1024 one row per workgroup; 1025 one workgroup takes two rows; 1500 some take two (an even trip
count of ``red[parity]`` beside an odd one); 2049 one workgroup takes three.  SwiGLU F 8, 1800 x rows
1, 129: one thread; 225 chunks a row, 29025 work items = 113 workgroups + 97 threads.  Cross-entropy V
8 (one chunk), 2048 (exactly one pass of 256 threads), 2056 (one thread starts a second pass), 32000,
128256 (the training vocabularies).  AdamW n 1, 7 (tail only), 8 (one vector), 9, 6149 (768 vectors
+ 5) with grids capped at 1 and 3 workgroups (3 sweeps; exactly one) and uncapped.
"""

from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from dstack_amd.ops import reference as ref
from tests.gemm_cases import BF16, F32, F64, _fmt, _seed, bf16_ulp

U = 2.0 ** -24
TINY = 2.0 ** -126
C_CAP = 64
EPS = 1e-5
EPS32 = float(np.float32(EPS))  # the value the kernels receive

NORM_D = [8, 256, 520, 1032, 2048, 2056, 3584, 4104, 6144, 8192]
NORM_ROWS = [1, 3, 1024, 1025, 1027]
FP8_D = [8, 520, 3584, 4104, 8192]
FP8_ROWS = [1, 37]
FP8_FORMS = ["plain", "delta", "scaled"]
BWD_D = [8, 520, 4104, 8192]
BWD_ROWS = [1, 3, 17, 1024, 1025, 1500, 2049]
BWD_CASES = sorted({(r, D) for D in BWD_D for r in (3, 1500)} | {(r, 520) for r in BWD_ROWS})
BWD_FORMS = [(False, "f32"), (True, "store"), (True, "accumulate"), (False, "accumulate")]  # (dres, dw form)
BWD_EXACT = [(3, 8), (3, 256), (1500, 256), (17, 4096), (1025, 512)]  # rows, D (a power of two)
SWIGLU_CASES = [(r, f) for f in (8, 1800) for r in (1, 129)]
SWIGLU_GATES = [0.0, 88.0, -88.0, 20.0, -20.0]
CE_CASES = [(3, 8), (3, 2048), (3, 2056), (3, 32000), (2, 128256)]  # rows, V
CE_VARIANTS = [0, 1, 2]
ADAMW_N = [1, 7, 8, 9, 6149]
ADAMW_BLOCKS = [0, 1, 3]
ADAMW_WD = [0.0, 0.1]
ADAMW_HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.95, eps=1e-8, grad_scale=0.5)
EMBED_CASES = [(512, 8), (512, 2056)]  # V, D (2056: a second pass of the 256 x 8 column loop)
ROPE_D = [16, 64, 128]
ROPE_B, ROPE_S, ROPE_TABLE, ROPE_ROT, ROPE_NH = 3, 7, 10, 3, 4  # 21 rows; heads 0-2 rotate, head 3 is v
TRANSPOSE_CASES = [(128, 64), (384, 192)]
SWIGLU_T_CASES = [(128, 64), (256, 192), (384, 64)]
BWD_EXACT_LIMIT = 4  # |dy|, |h|, |w|, |dres|, |old| <= 4, rstd = 2^-2


def _gen(*dims):
    return torch.Generator().manual_seed(_seed(*dims))


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F32)


def row_scales(rows: int) -> torch.Tensor:
    """2^-6 .. 2^6, a different one for neighbouring rows."""
    return 2.0 ** ((torch.arange(rows) * 5 % 13) - 6).to(F32)


def ceil_div(a: int, b: int) -> int:
    return -(-a // b)


# ==================================================================================================
# The judge
# ==================================================================================================
def judge(got: torch.Tensor, want: torch.Tensor, T: torch.Tensor, c: float, bf16: bool):
    """(err, bound) per element; a NaN or inf in ``got`` is an infinite error."""
    assert 0 <= c <= C_CAP, c
    assert got.shape == want.shape == T.shape, (got.shape, want.shape, T.shape)
    g = got.to(F64)
    err = torch.where(torch.isfinite(g), (g - want).abs(), torch.full_like(want, float("inf")))
    bound = c * U * T.abs() + TINY
    if bf16:
        assert got.dtype == BF16, got.dtype
        bound = bound + bf16_ulp(want)
    else:
        assert got.dtype == F32, got.dtype
    return err, bound


def layout(kind: str, **kw):
    """Which workgroup stores element (row, chunk) of an output of kernel ``kind``."""
    if kind == "block_row":      # one 256-thread workgroup per row
        return lambda r, ch: r
    if kind == "wave_row":       # one wave per row, 4 rows per workgroup
        return lambda r, ch: r // 4
    if kind == "grid_rows":      # workgroup row % grid (rms_norm_bwd's dx)
        return lambda r, ch: r % kw["grid"]
    if kind == "colsum":         # 64 lanes x 4 columns per workgroup of pass 2
        return lambda r, ch: ch // 32
    if kind == "flat":           # grid-stride over (row, chunk) work items, 256 per workgroup
        return lambda r, ch: (r * kw["nch"] + ch) // 256 % kw.get("grid", 1 << 62)
    raise ValueError(kind)


def where_report(bad: torch.Tensor, got, want, frac, wg, what: str) -> str:
    """Where the elements of the 2-D mask ``bad`` sit: rows, columns, 8-column chunks, the lane and the
    pass of the chunk (64-lane and 256-thread kernels) and the workgroups.  Under 2000 characters."""
    idx = bad.nonzero()
    r, col = idx[:, 0], idx[:, 1]
    ch = col // 8
    s = lambda t: _fmt(set(t.tolist()), 10)  # noqa: E731
    lines = [f"{what}: {idx.shape[0]} of {bad.numel()} elements over the bound",
             f"rows {s(r)}", f"columns {int(col.min())}..{int(col.max())}, chunks (col // 8) {s(ch)}",
             f"lane (chunk % 64) {s(ch % 64)}, wave pass (chunk // 64) {s(ch // 64)}, "
             f"thread (chunk % 256) {s(ch % 256)}, block pass (chunk // 256) {s(ch // 256)}",
             f"workgroups {s(wg(r, ch))}",
             "first (row, col, chunk, got, want, err / bound): " + ", ".join(
                 f"({i}, {j}, {j // 8}, {float(got[i, j]):.6g}, {float(want[i, j]):.6g}, {float(frac[i, j]):.3g})"
                 for i, j in idx[:6].tolist())]
    return "\n  ".join(lines)[:1990]


def _2d(t):
    return t.reshape(1, -1) if t.dim() == 1 else t.reshape(-1, t.shape[-1])


def assert_judged(got, want, T, c, *, bf16: bool, wg, what: str) -> float:
    """Every element of ``got`` inside its bound, or an AssertionError that says where; returns the
    largest used fraction of the bound.  A 1-D output is one row (``per_row``: one column)."""
    got, want, T = _2d(got), _2d(want), _2d(T)
    err, bound = judge(got, want, T, c, bf16)
    frac = err / bound
    bad = err > bound
    if bad.any():
        raise AssertionError(where_report(bad, got, want, frac, wg, what))
    return frac.max().item()


def assert_same(got, want, *, wg, what: str):
    """Bit for bit (NaNs differ from everything)."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if torch.equal(got, want):
        return
    g, w = _2d(got), _2d(want)
    bad = g != w
    frac = torch.full(g.shape, float("inf"), dtype=F64, device=g.device)
    raise AssertionError(where_report(bad, g.to(F64), w.to(F64), frac, wg, what))


def per_row(t):
    return t.reshape(-1, 1)


def old_close(a, b, atol, rtol=0.0) -> bool:
    """``_close`` of tests/test_ops_gpu.py: one bound per tensor."""
    a, b = a.to(F64), b.to(F64)
    return (a - b).abs().max().item() <= atol + rtol * b.abs().max().item()


def rb(x64: torch.Tensor) -> torch.Tensor:
    """fp64 -> bf16 -> fp64 (through fp32: a double rounding only where fp64 sits within 2^-29 of a tie)."""
    return x64.to(F32).to(BF16).to(F64)


# ==================================================================================================
# RMSNorm forward
# ==================================================================================================
def norm_c(D: int, tpr: int):
    """(c_rstd, c_y) for ``tpr`` threads per row (64: wave-per-row, 256: block-per-row)."""
    n = 8 * ceil_div(D // 8, tpr)
    red = n + 6 + (3 if tpr == 256 else 0)
    c_r = (red + 2) / 2 + 2
    return min(C_CAP, c_r), min(C_CAP, c_r + 2)


@functools.lru_cache(maxsize=2)
def norm_inputs(rows: int, D: int, device: str = "cpu", scaled_rows: bool = True, peak_last: bool = False):
    """x, delta [rows, D] bf16 with a scale of their own per row, w [D] bf16 (signs mixed), dr [rows],
    dc [D] fp32; row 1 (of 3 or more) is all zeros; ``peak_last``: row 0's largest |y| sits in its last
    chunk."""
    g = _gen(rows, D, 11)
    sc = row_scales(rows)[:, None] if scaled_rows else torch.ones(rows, 1)
    x, delta = _randn(g, rows, D) * sc, _randn(g, rows, D) * sc * 0.5
    w = 1 + (0.25 if scaled_rows else 0.1) * _randn(g, D)
    if scaled_rows:  # (not scaled: inputs like the older tests', for test_old_bound_misses_these)
        w[1::5] *= -1
    if rows >= 3 and scaled_rows:
        x[1], delta[1] = 0.0, 0.0
    if peak_last:
        x[0, D - 3], delta[0, D - 3], w[D - 3] = 16.0 * sc[0, 0], 0.0, 1.5
    dr, dc = torch.rand(rows, generator=g) * 1e-2 + 1e-3, torch.rand(D, generator=g) * 1e-2 + 1e-3
    raw = (delta / dr[:, None] / dc[None, :])  # the raw fp8 GEMM product whose scaled value is about delta
    t = lambda a, dt=BF16: a.to(dt).to(device)  # noqa: E731
    return SimpleNamespace(rows=rows, D=D, x=t(x), delta=t(delta), raw=t(raw), w=t(w), dr=t(dr, F32), dc=t(dc, F32))


def norm_ref(x, w, delta=None, dr=None, dc=None):
    """h (bf16, bit-exact: IEEE fp32 products and sum, one rounding each as the kernel documents),
    rstd, y in fp64."""
    h = x
    if delta is not None:
        d = delta.to(F32)
        if dr is not None:
            d = (d * dr[:, None] * dc[None, :]).to(BF16).to(F32)
        h = (x.to(F32) + d).to(BF16)
    h64 = h.to(F64)
    rstd = 1.0 / torch.sqrt((h64 * h64).sum(-1) / h.shape[1] + EPS32)
    y = h64 * rstd[:, None] * w.to(F64)[None, :]
    return SimpleNamespace(h=h, rstd=rstd, y=y)


def check_norm_fwd(impl, rows: int, D: int, add: bool, device: str = "cpu") -> dict:
    i = norm_inputs(rows, D, device)
    r = norm_ref(i.x, i.w, i.delta if add else None)
    h, y, rstd = impl.norm_fwd(i.x, i.delta if add else None, i.w, EPS)
    tpr = 256 if rows <= 1024 else 64
    wg = layout("block_row" if tpr == 256 else "wave_row")
    c_r, c_y = norm_c(D, tpr)
    what = f"rms_norm{'+add' if add else ''} {rows}x{D}"
    if add:
        assert_same(h, r.h, wg=wg, what=f"{what} h")
    return {"y": assert_judged(y, r.y, r.y, c_y, bf16=True, wg=wg, what=f"{what} y"),
            "rstd": assert_judged(per_row(rstd), per_row(r.rstd), per_row(r.rstd), c_r, bf16=False, wg=wg,
                                  what=f"{what} rstd")}


# --- the e4m3 output -------------------------------------------------------------------------------
def e4m3_value(q: torch.Tensor) -> torch.Tensor:
    return q.view(torch.float8_e4m3fn).to(F32).to(F64)


def e4m3_step(v: torch.Tensor) -> torch.Tensor:
    """Spacing of e4m3 at |v| <= 448 (3 mantissa bits; 2^-9 below the smallest normal 2^-6)."""
    p2 = (v.abs().clamp_min(2.0 ** -6).view(torch.int64) & 0x7FF0000000000000).view(F64)
    return p2 * 2.0 ** -3


def fp8_expect(r):
    yb = rb(r.y)
    return yb, yb.abs().amax(-1).clamp_min(1e-12) / 448.0


def fp8_verdict(h, q, qs, r, add: bool, wg, what: str) -> dict:
    """The issue's bounds: h bit for bit; the row scale within 2^-7 (relative) of max|bf16(y)| / 448;
    every dequantised byte within one e4m3 step at its own magnitude (times the row scale) of bf16(y);
    the byte of an exact zero is a zero.  Returns the used fractions."""
    yb, scale = fp8_expect(r)
    if add:
        assert_same(h, r.h, wg=wg, what=f"{what} h")
    assert q.dtype == torch.uint8 and qs.dtype == F32
    assert not (q == 0x7F).any() and not (q == 0xFF).any(), f"{what}: NaN bytes"
    s64 = qs.to(F64)
    sfrac = (s64 - scale).abs() / (2.0 ** -7 * scale)
    assert torch.isfinite(s64).all() and (sfrac <= 1).all(), \
        f"{what}: row scales off in rows {_fmt(set((~(sfrac <= 1)).nonzero()[:, 0].tolist()), 10)}: got " \
        f"{qs[~(sfrac <= 1)][:4].tolist()}, want {scale[~(sfrac <= 1)][:4].tolist()}"
    v = e4m3_value(q)
    err = (v * s64[:, None] - yb).abs()
    bound = e4m3_step(v) * s64[:, None]
    bad = err > bound
    frac = err / bound
    if bad.any():
        raise AssertionError(where_report(bad, v * s64[:, None], yb, frac, wg, f"{what} bytes"))
    zero = (yb == 0) & ((q & 0x7F) != 0)
    assert not zero.any(), f"{what}: non-zero bytes for exact zeros at {zero.nonzero()[:6].tolist()}"
    return {"fp8 step": frac.max().item(), "fp8 scale": sfrac.max().item()}


def check_norm_fp8(impl, rows: int, D: int, form: str, device: str = "cpu") -> dict:
    i = norm_inputs(rows, D, device, True, True)
    delta = {"plain": None, "delta": i.delta, "scaled": i.raw}[form]
    dr, dc = (i.dr, i.dc) if form == "scaled" else (None, None)
    r = norm_ref(i.x, i.w, delta, dr, dc)
    yb, _ = fp8_expect(r)
    assert int(yb[0].abs().argmax()) // 8 == D // 8 - 1, "row 0's largest |y| must sit in the last chunk"
    h, q, qs = impl.norm_fp8(i.x, delta, i.w, EPS, dr, dc)
    return fp8_verdict(h, q, qs, r, delta is not None, layout("block_row"), f"rms_norm_fp8 {form} {rows}x{D}")


# ==================================================================================================
# RMSNorm backward
# ==================================================================================================
def bwd_grid(rows: int) -> int:
    return max(1, min(rows, 1024))


def bwd_c(rows: int, D: int):
    n = 8 * ceil_div(D // 8, 256)
    P = bwd_grid(rows)
    rpb = ceil_div(P, 16)
    c_dw = 2 + ceil_div(rows, P) + ceil_div(rpb, 4) + 3 + min(16, P) + 1
    return min(C_CAP, n + 18), min(C_CAP, c_dw)


@functools.lru_cache(maxsize=2)
def bwd_inputs(rows: int, D: int, device: str = "cpu", scaled_rows: bool = True):
    g = _gen(rows, D, 12)
    sc = row_scales(rows)[:, None] if scaled_rows else torch.ones(rows, 1)
    h, dy, dres = _randn(g, rows, D) * sc, _randn(g, rows, D), _randn(g, rows, D)
    w = 1 + (0.25 if scaled_rows else 0.1) * _randn(g, D)
    if scaled_rows:  # (not scaled: inputs like the older tests')
        w[1::5] *= -1
    old = _randn(g, D) * 4
    if rows >= 3 and scaled_rows:
        h[1] = 0.0
    t = lambda a: a.to(BF16).to(device)  # noqa: E731
    i = SimpleNamespace(rows=rows, D=D, h=t(h), dy=t(dy), dres=t(dres), w=t(w), old=t(old))
    i.rstd = norm_ref(i.h, i.w).rstd.to(F32)  # what a forward hands over: the test supplies it
    return i


def bwd_ref(dy, h, w, rstd, dres=None, old=None):
    """fp64 dx, dw and their T from the bf16 inputs and the fp32 rstd."""
    dy, h, w, r = dy.to(F64), h.to(F64), w.to(F64), rstd.to(F64)[:, None]
    D = h.shape[1]
    g = dy * w
    k = (g * h).sum(-1, keepdim=True) * r ** 3 / D
    kabs = (g * h).abs().sum(-1, keepdim=True) * r ** 3 / D
    dx, T_dx = r * g - h * k, (r * g).abs() + h.abs() * kabs
    if dres is not None:
        dx, T_dx = dx + dres.to(F64), T_dx + dres.to(F64).abs()
    term = dy * h * r
    dw, T_dw = term.sum(0), term.abs().sum(0)
    if old is not None:
        dw, T_dw = dw + old.to(F64), T_dw + old.to(F64).abs()
    return SimpleNamespace(dx=dx, T_dx=T_dx, dw=dw, T_dw=T_dw, term=term)


def check_norm_bwd(impl, rows: int, D: int, with_dres: bool, form: str, device: str = "cpu") -> dict:
    i = bwd_inputs(rows, D, device)
    dres = i.dres if with_dres else None
    r = bwd_ref(i.dy, i.h, i.w, i.rstd, dres, i.old if form == "accumulate" else None)
    dw_out = None if form == "f32" else i.old.clone()
    dx, dw = impl.norm_bwd(i.dy, i.h, i.w, i.rstd, dres, dw_out, form == "accumulate", EPS)
    c_dx, c_dw = bwd_c(rows, D)
    what = f"rms_norm_bwd {rows}x{D} dres={with_dres} dw {form}"
    return {"dx": assert_judged(dx, r.dx, r.T_dx, c_dx, bf16=True, wg=layout("grid_rows", grid=bwd_grid(rows)),
                                what=f"{what} dx"),
            f"dw {'f32' if form == 'f32' else 'bf16'}":
                assert_judged(dw, r.dw, r.T_dw, c_dw, bf16=form != "f32", wg=layout("colsum"), what=f"{what} dw")}


# --- exact: small integers, rstd a power of two ----------------------------------------------------
@functools.lru_cache(maxsize=2)
def bwd_exact_inputs(rows: int, D: int, device: str = "cpu"):
    g = _gen(rows, D, 13)
    L = BWD_EXACT_LIMIT
    ri = lambda *s: torch.randint(-L, L + 1, s, generator=g).to(F32)  # noqa: E731
    t = lambda a: a.to(BF16).to(device)  # noqa: E731
    return SimpleNamespace(rows=rows, D=D, dy=t(ri(rows, D)), h=t(ri(rows, D)), w=t(ri(D)), dres=t(ri(rows, D)),
                           old=t(ri(D)), rstd=torch.full((rows,), 0.25, dtype=F32).to(device))


def check_bwd_exact_limits(i):
    """Every intermediate of dx and dw, in any order and with or without fused multiply-adds, is an
    integer multiple of r^3 / D = 2^-6 / D below 2^24 of them: fp32 holds it exactly."""
    L, D, rows = BWD_EXACT_LIMIT, i.D, i.rows
    assert D & (D - 1) == 0 and D <= 4096, "D must be a power of two"
    for x in (i.dy, i.h, i.w, i.dres, i.old):
        assert x.abs().max().item() <= L and torch.equal(x.to(F64), x.to(F64).round())
    assert (i.rstd == 0.25).all()
    unit = 2.0 ** -6 / D
    dot = D * L ** 3                                  # |sum dy w h|
    dx = (0.25 * L * L + L * dot * unit + L) / unit   # |r g| + |h k| + |dres| in units
    dw = (rows * L * L * 0.25 + L) / 0.25             # |sum dy h r| + |old| in units of r
    assert dot < 2 ** 24 and dx < 2 ** 24 and dw < 2 ** 24, (dot, dx, dw)


def check_norm_bwd_exact(impl, rows: int, D: int, device: str = "cpu"):
    i = bwd_exact_inputs(rows, D, device)
    check_bwd_exact_limits(i)
    for with_dres in (False, True):
        dres = i.dres if with_dres else None
        what = f"rms_norm_bwd exact {rows}x{D} dres={with_dres}"
        wg_dx, wg_dw = layout("grid_rows", grid=bwd_grid(rows)), layout("colsum")
        r = bwd_ref(i.dy, i.h, i.w, i.rstd, dres)
        dx, dw = impl.norm_bwd(i.dy, i.h, i.w, i.rstd, dres, None, False, None)
        assert_same(dx, r.dx.to(F32).to(BF16), wg=wg_dx, what=f"{what} dx")
        assert_same(dw, r.dw.to(F32), wg=wg_dw, what=f"{what} dw fp32")
        for acc in (False, True):
            out = i.old.clone()
            dx, dwb = impl.norm_bwd(i.dy, i.h, i.w, i.rstd, dres, out, acc, None)
            want = r.dw + (i.old.to(F64) if acc else 0)
            assert_same(dx, r.dx.to(F32).to(BF16), wg=wg_dx, what=f"{what} dx (dw_out)")
            assert_same(dwb, want.to(F32).to(BF16), wg=wg_dw, what=f"{what} dw_out accumulate={acc}")


# ==================================================================================================
# SwiGLU
# ==================================================================================================
SWIGLU_C = 8


@functools.lru_cache(maxsize=4)
def swiglu_inputs(rows: int, Fh: int, device: str = "cpu"):
    g = _gen(rows, Fh, 14)
    gu, da = _randn(g, rows, 2 * Fh) * 3, _randn(g, rows, Fh)
    n = min(Fh, len(SWIGLU_GATES))
    gu[:, :n] = torch.tensor(SWIGLU_GATES[:n])
    gu[:, Fh:Fh + n] = torch.tensor([1.5, -0.75, 1.25, -2.0, 0.5][:n])
    if Fh > 16:
        gu[:, Fh - 5:Fh] = torch.tensor(SWIGLU_GATES[::-1])  # and in the row's last chunk
    return SimpleNamespace(rows=rows, F=Fh, gu=gu.to(BF16).to(device), da=da.to(BF16).to(device))


def swiglu_ref(gu, da):
    Fh = gu.shape[-1] // 2
    g, u, d = gu[:, :Fh].to(F64), gu[:, Fh:].to(F64), da.to(F64)
    s = 1.0 / (1.0 + torch.exp(-g))
    oms = 1.0 / (1.0 + torch.exp(g))  # 1 - s without cancellation
    q = g.abs() * oms
    a = g * s * u
    A, B = d * u * s, 1.0 + g * oms
    du = d * g * s
    return SimpleNamespace(a=a, T_a=a.abs() * (1 + q), dgu=torch.cat([A * B, du], 1),
                           T_dgu=torch.cat([A.abs() * (B.abs() + g.abs()) * (1 + q), du.abs() * (1 + q)], 1))


def check_swiglu(impl, rows: int, Fh: int, device: str = "cpu") -> dict:
    i = swiglu_inputs(rows, Fh, device)
    gates = set(i.gu[0, :Fh].to(F64).tolist())
    assert gates >= set(SWIGLU_GATES), gates
    r = swiglu_ref(i.gu, i.da)
    assert torch.isfinite(r.a).all() and torch.isfinite(r.dgu).all()
    a, dgu = impl.swiglu_fwd(i.gu), impl.swiglu_bwd(i.da, i.gu)
    what = f"swiglu {rows}x{Fh}"
    return {"a": assert_judged(a, r.a, r.T_a, SWIGLU_C, bf16=True, wg=layout("flat", nch=Fh // 8), what=f"{what} a"),
            "dgu": assert_judged(dgu, r.dgu, r.T_dgu, SWIGLU_C, bf16=True, wg=layout("flat", nch=Fh // 8),
                                 what=f"{what} dgu (columns >= F: du)")}


# ==================================================================================================
# Cross-entropy
# ==================================================================================================
CE_KINDS = ["random", "equal", "spike"]
CE_BWD_C = 6


def ce_fwd_c(V: int) -> float:
    return min(C_CAP, ceil_div(V, 2048) + 24)


def ce_edges(V: int):
    return [t for t in (0, 7, 8, V - 8, V - 1) if 0 <= t < V]


@functools.lru_cache(maxsize=2)
def ce_inputs(rows: int, V: int, variant: int, device: str = "cpu"):
    """Row kinds rotate with ``variant``: random (its maximum in the last chunk), all logits equal, and
    a spike (the target's logit 100 above the rest); targets walk over 0, 7, 8, V - 8, V - 1."""
    g = _gen(rows, V, 15)
    logits = _randn(g, rows, V) * 3
    edges = ce_edges(V)
    target, kinds = [], []
    for i in range(rows):
        kind = CE_KINDS[(i + variant) % 3]
        t = edges[(2 * variant + i) % len(edges)]
        if kind == "random":
            logits[i, V - 2] = 20.0
        elif kind == "equal":
            logits[i] = 1.5
        else:
            logits[i] = logits[i].clamp(-4, 4)
            logits[i, t] = 104.0
        target.append(t)
        kinds.append(kind)
    return SimpleNamespace(rows=rows, V=V, kinds=kinds, logits=logits.to(BF16).to(device),
                           target=torch.tensor(target, dtype=torch.int64).to(device))


def ce_ref(logits, target, lse_given=None, scale: float = 1.0):
    """fp64 lse, per-row loss and the gradient (of ``lse_given``, fp32, when supplied) with their T.
    A target outside [0, V): loss 0 and a zero gradient row."""
    l = logits.to(F64)
    V = l.shape[1]
    live = (target >= 0) & (target < V)
    tc = target.clamp(0, V - 1)
    m = l.amax(-1)
    logs = torch.log(torch.exp(l - m[:, None]).sum(-1))
    lse = m + logs
    lt = l.gather(1, tc[:, None])[:, 0]
    T_lse = m.abs() + logs.abs() + 1
    loss = torch.where(live, lse - lt, torch.zeros_like(lse))
    x = l - (lse if lse_given is None else lse_given.to(F64))[:, None]
    p = torch.exp(x)
    onehot = F.one_hot(tc, V).to(F64) * live[:, None]
    grad = torch.where(live[:, None], (p - onehot) * scale, torch.zeros_like(p))
    T_grad = abs(scale) * (p * (1 + x.abs()) + onehot)
    return SimpleNamespace(lse=lse, T_lse=T_lse, loss=loss, T_loss=T_lse + lt.abs(), grad=grad, T_grad=T_grad, live=live)


def check_ce(impl, rows: int, V: int, variant: int, device: str = "cpu") -> dict:
    assert V % 8 == 0
    i = ce_inputs(rows, V, variant, device)
    r = ce_ref(i.logits, i.target)
    loss, lse = impl.ce_fwd(i.logits, i.target)
    c, wg = ce_fwd_c(V), layout("block_row")
    what = f"cross_entropy {rows}x{V} variant {variant} ({', '.join(i.kinds)}; targets {i.target.tolist()})"
    out = {"lse": assert_judged(per_row(lse), per_row(r.lse), per_row(r.T_lse), c, bf16=False, wg=wg, what=f"{what} lse"),
           "loss": assert_judged(per_row(loss), per_row(r.loss), per_row(r.T_loss), min(C_CAP, c + 1), bf16=False, wg=wg,
                                 what=f"{what} loss")}
    lse32 = r.lse.to(F32)
    fr = []
    for scale, inplace in ((1.0, False), (0.37, True)):
        rg = ce_ref(i.logits, i.target, lse32, float(np.float32(scale)))
        src = i.logits.clone()
        grad = impl.ce_bwd(src, i.target, lse32, scale, inplace)
        if inplace:
            assert grad.data_ptr() == src.data_ptr(), "in place: the gradient must overwrite the logits"
        else:
            assert torch.equal(src, i.logits), "out of place: the logits must stay"
        fr.append(assert_judged(grad, rg.grad, rg.T_grad, CE_BWD_C, bf16=True, wg=wg,
                                what=f"{what} gradient scale={scale} inplace={inplace}"))
        for row, kind in enumerate(i.kinds):
            if kind == "spike":
                assert grad[row, i.target[row]].item() == 0.0, f"{what}: the spike's own gradient must be exactly 0"
    out["gradient"] = max(fr)
    return out


# ==================================================================================================
# AdamW
# ==================================================================================================
ADAMW_C = dict(m=13, v=24, master=34)
ADAMW_PAD = 8  # elements either side of the updated slice (keeps its 16- and 32-byte alignment)


def adamw_inputs(n: int, device: str = "cpu"):
    """Flat buffers of n + 2 * ADAMW_PAD elements; the update runs on the middle n.  Element 0 of the
    slice has g = 0 and v = 0 in every step."""
    g = _gen(n, 16)
    N = n + 2 * ADAMW_PAD
    master = _randn(g, N)
    grad = _randn(g, N) * 0.01
    grad[ADAMW_PAD] = 0.0
    return SimpleNamespace(n=n, master=master.to(device), param=master.to(BF16).to(device), grad=grad.to(BF16).to(device),
                           m=torch.zeros(N, device=device), v=torch.zeros(N, device=device))


def adamw_ref(master, m, v, grad, *, lr, beta1, beta2, eps, weight_decay, step, grad_scale):
    """One step in fp64 from the fp32 state and the fp32 values of the hyper-parameters."""
    f = lambda x: float(np.float32(x))  # noqa: E731
    lr, b1, b2, eps, wd, gs = f(lr), f(beta1), f(beta2), f(eps), f(weight_decay), f(grad_scale)
    bc1, bc2 = f(1.0 - beta1 ** step), f(1.0 - beta2 ** step)
    p0, m0, v0, g = master.to(F64), m.to(F64), v.to(F64), grad.to(F64) * gs
    m1, T_m = b1 * m0 + (1 - b1) * g, (b1 * m0).abs() + ((1 - b1) * g).abs()
    v1, T_v = b2 * v0 + (1 - b2) * g * g, (b2 * v0).abs() + (1 - b2) * g * g
    denom = torch.sqrt(v1) / math.sqrt(bc2) + eps
    step_size, decay = lr / bc1, 1.0 - lr * wd
    p1 = p0 * decay - step_size * m1 / denom
    return SimpleNamespace(master=p1, T_master=(p0 * decay).abs() + step_size / denom * T_m, m=m1, T_m=T_m, v=v1, T_v=T_v)


def check_adamw(impl, n: int, max_blocks: int, weight_decay: float, device: str = "cpu") -> dict:
    i = adamw_inputs(n, device)
    sl = slice(ADAMW_PAD, ADAMW_PAD + n)
    wg = layout("flat", nch=1 << 40, grid=max_blocks if max_blocks > 0 else 1 << 62)
    fr = {"master": 0.0, "m": 0.0, "v": 0.0}
    for step in (1, 2, 3):
        before = {k: getattr(i, k).clone() for k in ("param", "master", "m", "v")}
        kw = dict(ADAMW_HYPER, weight_decay=weight_decay, step=step)
        r = adamw_ref(i.master[sl], i.m[sl], i.v[sl], i.grad[sl], **kw)
        if step == 1:
            assert i.grad[ADAMW_PAD] == 0 and i.v[ADAMW_PAD] == 0
        impl.adamw(i.param[sl], i.grad[sl], i.master[sl], i.m[sl], i.v[sl], max_blocks=max_blocks, **kw)
        what = f"adamw n={n} max_blocks={max_blocks} wd={weight_decay} step {step}"
        for k in fr:
            fr[k] = max(fr[k], assert_judged(getattr(i, k)[sl], getattr(r, k), getattr(r, "T_" + k), ADAMW_C[k],
                                             bf16=False, wg=wg, what=f"{what} {k}"))
        assert_same(i.param[sl], i.master[sl].to(BF16), wg=wg, what=f"{what} param against bf16(master)")
        for k, old in before.items():
            cur = getattr(i, k)
            assert torch.equal(cur[:ADAMW_PAD], old[:ADAMW_PAD]) and torch.equal(cur[ADAMW_PAD + n:], old[ADAMW_PAD + n:]), \
                f"{what}: {k} changed outside the updated slice"
    assert (i.v[ADAMW_PAD] == 0).all() and torch.isfinite(i.master).all()
    return fr


# ==================================================================================================
# Embedding backward (exact)
# ==================================================================================================
@functools.lru_cache(maxsize=2)
def embed_inputs(V: int, D: int, device: str = "cpu"):
    """Runs of 1, 2 and 300 equal ids, at id 0 (300), V - 1 (2) and inside, in shuffled positions;
    integer dy in [-3, 3] and an integer table: every sum is an integer below 2^24."""
    g = _gen(V, D, 17)
    ids = torch.tensor([0] * 300 + [V - 1] * 2 + [5] + [17] * 2 + [V - 2] + [200] * 300 + [201])
    ids = ids[torch.randperm(ids.numel(), generator=g)]
    dy = torch.randint(-3, 4, (ids.numel(), D), generator=g).to(F32)
    table = torch.randint(-8, 9, (V, D), generator=g).to(F32)
    runs = sorted(torch.unique(ids, return_counts=True)[1].tolist())
    assert runs == [1, 1, 1, 2, 2, 300, 300] and V > 201
    return SimpleNamespace(V=V, D=D, ids=ids.to(device), dy=dy.to(BF16).to(device), table=table.to(BF16).to(device))


def check_embedding(impl, V: int, D: int, device: str = "cpu"):
    """Bit for bit in both forms.  Rows whose id does not occur keep their bits in the accumulating form.
    The storing form is documented to clear the whole table first (the binding zeroes ``grad`` before
    the kernel), so there such rows must be zero, whatever they held: only the accumulating form can
    show a row that the kernel touched without cause."""
    i = embed_inputs(V, D, device)
    sums = torch.zeros(V, D, dtype=F64, device=i.dy.device).index_add_(0, i.ids, i.dy.to(F64))
    absent = torch.ones(V, dtype=torch.bool, device=i.dy.device)
    absent[i.ids] = False
    assert absent.sum() == V - 7
    for acc in (True, False):
        want = (sums + (i.table.to(F64) if acc else 0)).to(F32).to(BF16)
        grad = i.table.clone()
        impl.embedding_bwd(i.dy, i.ids, grad, acc)
        assert_same(grad, want, wg=lambda r, ch: r, what=f"embedding_bwd V={V} D={D} accumulate={acc}")
        if acc:
            assert torch.equal(grad[absent], i.table[absent]), "rows whose id does not occur must keep their bits"
        else:
            assert (grad[absent].view(torch.int16) == 0).all(), "a storing call clears the rows whose id does not occur"


# ==================================================================================================
# RoPE with hand-made tables (exact)
# ==================================================================================================
@functools.lru_cache(maxsize=3)
def rope_inputs(D: int, device: str = "cpu"):
    """qkv [B, S, NH * D] with a different bf16 value in every element (consecutive bit patterns from
    2^-31 up, signs alternating with the row), cos / sin [ROPE_TABLE, D / 2] with (cos, sin) per
    position and pair one of (+-1, 0), (0, +-1), (+-0.5, 0), (0, +-0.5): every output is +-x or +-x / 2."""
    B, S, NH = ROPE_B, ROPE_S, ROPE_NH
    n = B * S * NH * D
    assert (B * S) % 256 and ROPE_TABLE > S and 0x3000 + n < 0x7F00
    bits = (0x3000 + torch.arange(n, dtype=torch.int32)).to(torch.int16)
    qkv = bits.view(BF16).reshape(B * S, NH * D).clone()
    qkv[1::2] = -qkv[1::2]
    g = _gen(D, 18)
    pick = torch.randint(0, 8, (ROPE_TABLE, D // 2), generator=g)
    mag = torch.where(pick >= 4, 0.5, 1.0) * torch.where(pick % 2 == 1, -1.0, 1.0)
    on_cos = pick % 4 < 2
    cos, sin = torch.where(on_cos, mag, 0.0).to(F32), torch.where(on_cos, 0.0, mag).to(F32)
    assert len(set(qkv.flatten().tolist())) == n and all((pick == k).any() for k in range(8))
    return SimpleNamespace(D=D, qkv=qkv.reshape(B, S, NH * D).to(device), cos=cos.to(device), sin=sin.to(device))


def rope_ref(qkv, cos, sin, n_rot: int, D: int, inverse: bool, pair_next: bool = False, pos_is_row: bool = False):
    """fp64 rotate-half on heads < n_rot, position = row % S, pairs (i, i + D / 2); rounded to bf16.
    ``pair_next`` / ``pos_is_row``: the two defect models (pairs (i, i + 1); position = row)."""
    B, S, W = qkv.shape
    NH, h = W // D, D // 2
    x = qkv.to(F64).reshape(B * S, NH, D)
    rows = torch.arange(B * S, device=qkv.device)
    pos = rows % cos.shape[0] if pos_is_row else rows % S
    c, s = cos.to(F64)[pos][:, None, :], sin.to(F64)[pos][:, None, :] * (-1.0 if inverse else 1.0)
    if pair_next:
        x1, x2 = x[..., 0::2], x[..., 1::2]
    else:
        x1, x2 = x[..., :h], x[..., h:]
    o1, o2 = x1 * c - x2 * s, x2 * c + x1 * s
    out = torch.stack([o1, o2], -1).flatten(-2) if pair_next else torch.cat([o1, o2], -1)
    out = torch.where((torch.arange(NH, device=qkv.device) < n_rot)[None, :, None], out, x)
    return out.reshape(B, S, W).to(F32).to(BF16)


# ==================================================================================================
# The plain fp32 implementation (ops.reference on fp32 CPU tensors), rounded where the kernels round
# ==================================================================================================
class Fp32Impl:
    def norm_fwd(self, x, delta, w, eps):
        h = None
        if delta is not None:
            h = (x.float() + delta.float()).to(BF16)
        hf = (x if h is None else h).float()
        rstd = torch.rsqrt(hf.pow(2).mean(-1) + eps)
        return h, ref.rms_norm(hf, w.float(), eps).to(BF16), rstd

    def norm_fp8(self, x, delta, w, eps, dr, dc):
        if dr is not None:
            delta = (delta.float() * dr[:, None] * dc[None, :]).to(BF16)
        h, y, _ = self.norm_fwd(x, delta, w, eps)
        q, s = ref.quant_fp8_rows(y)
        return h, q.view(torch.uint8), s

    def norm_bwd(self, dy, h, w, rstd, dres, dw_out, accumulate, eps):
        if eps is None:  # the exact cases supply an rstd that is not the rows' own: the formula in fp32
            r = rstd[:, None]
            g = dy.float() * w.float()
            dx = r * g - h.float() * ((g * h.float()).sum(-1, keepdim=True) * r * r * r / h.shape[1])
            dw = (dy.float() * h.float() * r).sum(0)
        else:
            hf, wf = h.float().requires_grad_(), w.float().requires_grad_()
            ref.rms_norm(hf, wf, eps).backward(dy.float())
            dx, dw = hf.grad, wf.grad
        if dres is not None:
            dx = dx + dres.float()
        if dw_out is None:
            return dx.to(BF16), dw
        return dx.to(BF16), dw_out.copy_((dw + (dw_out.float() if accumulate else 0)).to(BF16))

    def swiglu_fwd(self, gu):
        return ref.swiglu(gu.float()).to(BF16)

    def swiglu_bwd(self, da, gu):
        x = gu.float().requires_grad_()
        ref.swiglu(x).backward(da.float())
        return x.grad.to(BF16)

    def ce_fwd(self, logits, target):
        lf = logits.float()
        return F.cross_entropy(lf, target, reduction="none"), torch.logsumexp(lf, -1)

    def ce_bwd(self, logits, target, lse, scale, inplace):
        lf = logits.float().requires_grad_()
        (F.cross_entropy(lf, target, reduction="sum") * scale).backward()
        g = lf.grad.to(BF16)
        return logits.copy_(g) if inplace else g

    def adamw(self, param, grad, master, m, v, *, lr, beta1, beta2, eps, weight_decay, step, grad_scale, max_blocks):
        ref.adamw_(param, grad, master, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale)

    def embedding_bwd(self, dy, ids, grad, accumulate):
        base = grad.float() if accumulate else torch.zeros_like(grad, dtype=F32)
        grad.copy_(base.index_add_(0, ids, dy.float()).to(BF16))


# ==================================================================================================
# Defect models: what a wrong kernel would store, made from the reference of a case on the CPU
# ==================================================================================================
def norm_defect(kind: str, i, r, row: int = 2):
    """y (bf16) of the forward with ``kind`` (in ``row``)."""
    h, w, rstd = r.h.to(F64), i.w.to(F64), r.rstd.clone()
    y = r.y.clone()
    if kind == "neighbour_rstd":     # a row normalised with the next row's rstd
        y[row] = h[row] * rstd[row + 1] * w
    elif kind == "stale_weight":     # the last chunk multiplied by the previous chunk's weight
        y[:, -8:] = h[:, -8:] * rstd[:, None] * w[-16:-8]
    else:
        raise ValueError(kind)
    return y.to(F32).to(BF16)


def bwd_defect(kind: str, i, r):
    """(dx bf16, dw fp32) of the backward with ``kind``."""
    dx, dw = r.dx.clone(), r.dw.clone()
    D, grid = i.D, bwd_grid(i.rows)
    row, ch = i.rows // 2, D // 8 - 1
    if kind == "dw_chunk_missing":       # one (row, chunk) left out of the weight gradient
        dw[ch * 8:ch * 8 + 8] -= r.term[row, ch * 8:ch * 8 + 8]
    elif kind in ("partial_missing", "partial_twice"):  # one workgroup's partial row lost / counted twice in colsum
        part = r.term[grid // 2::grid].sum(0)
        dw = dw - part if kind == "partial_missing" else dw + part
    elif kind == "projection_scaled":    # h k scaled by D / roundup(D, 2048): the mean taken over the padded row
        rr = i.rstd.to(F64)[:, None]
        g = i.dy.to(F64) * i.w.to(F64)
        hk = i.h.to(F64) * ((g * i.h.to(F64)).sum(-1, keepdim=True) * rr ** 3 / D)
        dx = dx + hk * (1 - D / (ceil_div(D, 2048) * 2048))
    else:
        raise ValueError(kind)
    return dx.to(F32).to(BF16), dw.to(F32)


def fp8_defect_first_pass_scale(i, r):
    """(q, qs): the row scale taken over the first 256-thread pass (2048 columns) only."""
    yb, _ = fp8_expect(r)
    s = (yb[:, :2048].abs().amax(-1).clamp_min(1e-12) / 448.0).to(F32)
    q = (yb / s.to(F64)[:, None]).clamp(-448, 448).to(F32).to(torch.float8_e4m3fn).view(torch.uint8)
    return q, s
