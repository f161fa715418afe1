"""The decode hot path -- ``gemv`` (``csrc/gemv.hip``), ``gemv_fp8``, the e4m3 row quantizers and
``scale_rows_cols_`` (``csrc/fp8.hip``), ``fp8_rows_gemm`` and ``fp8_stream_gemm``
(``csrc/fp8_gemm.hip``), ``lora_shrink`` and ``lora_expand`` (``csrc/lora.hip``) -- on operands for
which every summation order is exact, compared element for element with the rounding of the fp64
result (``tests/decode_cases.py`` has the construction, the comparison and the defect models).

The older tests of these kernels bound one number per call, ``||y - ref|| / ||ref|| < 5e-3`` or
``< 1e-2``, or let 1e-3 of a quantizer's bytes differ: one lane's lost chunk or one wrong register in
a tile stays under that (``test_old_bound_misses_these`` keeps it on record).  Here any of them changes
stored values, and the report says which workgroup, wave, tail or slice.  There is no tolerance
anywhere in this file.

Without a GPU: the builders' invariants and ``check_cap`` for every case the GPU tests use, the
quantizer reference on hand-written bytes (ties included) and on every built row, each defect model
caught by ``assert_exact``.  With one: every K path of ``gemv`` (tail only, one unrolled step, steps
plus tails) at grids under and over 8 workgroups; the 1-, 2- and 4-row forms of ``gemv_fp8`` with a
part-filled last wave; ``fp8_rows_gemm`` at partial 64-row blocks, K under the prologue and strided
operands; every form ``fp8_stream_gemm`` offers (and a refusal where it offers none); the quantizers
bitwise at each register-resident form's edge; the LoRA kernels at slice ends that are not round.

What the binding does not let a test see: ``fp8_rows_gemm`` and ``fp8_stream_gemm`` allocate their
output themselves, [M, N], so a stored padded token row would land outside it; the ``padded_row``
defect model is judged on a 256-row buffer on the CPU only.
"""

import os

import pytest
import torch

from tests import decode_cases as dc
from tests import gemm_cases as gc
from tests.decode_cases import BF16, F32, F64, NAN, U8, assert_exact
from dstack_amd.ops import _ext
from dstack_amd.ops import serving as sops

GEMV = [(N, K) for N in dc.GEMV_N for K in dc.GEMV_K]
GEMV8 = [(N, K) for N in dc.GEMV8_N for K in dc.GEMV8_K]
ROWS = [(N, K) for N in dc.ROWS_N for K in dc.ROWS_K]
ROWS_STRIDED = (200, 384, 384)
STREAM = [(rw, sh, K, S) for rw, sh in dc.STREAM_FORMS for K, S in dc.STREAM_KS]
STREAM_SHAPES = sorted({(2 * dc.stream_wg_rows(rw), K) for rw, _, K, _ in STREAM})
SWIGLU = [(M, F, scaled) for M in dc.SWIGLU_M for F in dc.SWIGLU_F for scaled in (False, True)]


# ==================================================================================================
# Without a GPU: the builders
# ==================================================================================================
def test_pow2_scales():
    for n in (1, 3, 37, 1027, 16391):
        dc.check_scales(dc.pow2_scales(n, 5))
    assert not torch.equal(dc.pow2_scales(64, 1), dc.pow2_scales(64, 2))


@pytest.mark.parametrize("N,K,fp8", [(N, K, False) for N, K in GEMV] + [(N, K, True) for N, K in GEMV8])
def test_gemv_case_invariants(N, K, fp8):
    """Value sets, density, distinct weight rows, ``check_cap`` on the integer products, and that the
    shape reaches the grid, tail and K path it is in the table for."""
    c = dc.gemv_case(N, K, fp8)  # (check_cap runs inside)
    print(f"gemv{'_fp8' if fp8 else ''} N={N} K={K}: share of |product| > 256 {c.share:.2e}, max {c.ints.abs().max().item():g}")
    assert set(c.x8.unique().tolist()) <= {-1, 0, 1} and set(c.W8.unique().tolist()) == {-1, 1}
    assert abs((c.x8 != 0).double().mean().item() - min(1.0, 4096 / K)) <= 0.02
    assert dc.rows_distinct(c.W8), "every row of W must differ"
    assert torch.equal(c.x.to(F64), c.x8.to(F64)) and c.ints.abs().max().item() < 2 ** 24
    assert torch.equal(c.ints, c.ints.round()) and torch.equal(c.want.to(F64)[c.ints.abs() <= 256], c.exact[c.ints.abs() <= 256])
    if fp8:
        dc.check_scales(c.sw)
        assert set(c.W.unique().tolist()) == {0x38, 0xB8}
        R = dc.gemv_fp8_rows(N)
        p = dc.gemv_plan(N, R)
        assert (R, p.last_nr, p.grid, p.rem) == {1027: (1, 1, 257, 1), 8197: (2, 1, 1025, 1), 16391: (4, 3, 1025, 1)}[N]
        assert p.banded
    else:
        p = dc.gemv_plan(N)
        assert (p.grid, p.rem, p.last_wg_waves) == {3: (1, 1, 3), 32: (8, 0, 4), 37: (10, 2, 1), 1027: (257, 1, 3)}[N]
        assert p.banded == (N != 3)
        assert dc.gemv_steps(K) == {512: (0, 1), 2048: (1, 0), 2560: (1, 1), 3584: (1, 3), 14336: (7, 0)}[K]


@pytest.mark.parametrize("N,K", sorted(set(ROWS) | {ROWS_STRIDED[1:]} | set(STREAM_SHAPES)))
def test_gemm_case_invariants(N, K):
    c = dc.gemm_case(256, N, K)  # (check_cap runs inside)
    print(f"fp8 gemm 256x{N}x{K}: share of |product| > 256 {c.share:.2e}, max {c.ints.abs().max().item():g}")
    gc.check_operands(c.a, c.b, torch.zeros(1, dtype=F64), K)
    dc.check_scales(c.xs)
    dc.check_scales(c.ws)
    assert c.ints.abs().max().item() < 2 ** 24 and torch.equal(c.ints, c.ints.round())
    ok = c.ints.abs() <= 256
    assert torch.equal(c.want.to(F64)[ok], c.exact[ok])  # an integer <= 256 times a power of two is a bf16 value
    s = dc.sub(c, 37, 128)
    assert s.xq.is_contiguous() and s.wq.is_contiguous() and torch.equal(s.want, c.want[:37, :128])


def test_densest_case_share_is_within_the_cap():
    """The densest reductions (every activation non-zero, K = 3584 and 4096-of-14336): the measured share
    of integer products above 256 that the summary of this change quotes."""
    shares = {"gemv 1027x3584": dc.gemv_case(1027, 3584).share, "gemv 1027x14336": dc.gemv_case(1027, 14336).share,
              "stream 256x512x3584": dc.gemm_case(256, 512, 3584).share}
    print(shares)
    assert max(shares.values()) <= gc.CAP_SHARE


def test_quant_reference_on_hand_written_bytes():
    """``reference.quant_fp8_rows`` itself, so that kernel and reference cannot agree on a wrong answer:
    448 -> 0x7E; 17 and 19 (between 16, 18 and 20) -> the even 0x58 and 0x5A; 1 -> 0x38; 0.5 -> 0x30;
    -3.25 -> 0xC5; 0 -> 0; 2^-10 (between 0 and the smallest subnormal) -> 0; 3 x 2^-10 (between 0x01 and
    0x02) -> 0x02; 7.5 x 2^-9 (between the largest subnormal and the smallest normal) -> 0x08; -232 (between
    224 and 240) -> 0xF6.  The same row times 2^-4 and 2^7 gives the same bytes; a zero row gives zeros."""
    row = torch.tensor([448.0, 17.0, 19.0, 1.0, 0.5, -3.25, 0.0, 2.0 ** -10, 3 * 2.0 ** -10, 7.5 * 2.0 ** -9, -232.0])
    want = torch.tensor([0x7E, 0x58, 0x5A, 0x38, 0x30, 0xC5, 0x00, 0x00, 0x02, 0x08, 0xF6], dtype=U8)
    x = torch.stack([row, row * 2.0 ** -4, row * 2.0 ** 7, torch.zeros_like(row)]).to(BF16)
    q, s = dc.quant_reference(x)
    assert s.tolist() == [1.0, 2.0 ** -4, 2.0 ** 7, dc.ZERO_ROW_SCALE]
    for i in range(3):
        assert q[i].tolist() == want.tolist(), i
    assert q[3].tolist() == [0] * row.numel()


@pytest.mark.parametrize("K", dc.QUANT_K)
def test_quant_rows_builder(K):
    """Every built row is exact in bf16, holds ties, and ``reference.quant_fp8_rows`` gives the bytes
    and scales it was built from."""
    c = dc.quant_rows_case(K)
    assert c.ties > 0 and (c.x[3] == 0).all() and len(set(c.s.tolist())) >= 6
    q, s = dc.quant_reference(c.x)
    assert_exact(q, c.q, dc.quant_where, "reference bytes")
    assert_exact(s, c.s, what="reference scales")
    cols = [int(c.q[i].to(torch.int16).bitwise_and(0x7F).argmax()) for i in (0, 1, 2)]
    assert cols == [0, K // 2, K - 3]
    assert dc.quant_nit(K) == {8: 2, 2048: 2, 2056: 2, 4096: 2, 4104: 4, 8200: 8, 16392: 16, 32768: 16, 32776: 0}[K]


@pytest.mark.parametrize("M,F,scaled", [(3, F, sc) for F in dc.SWIGLU_F for sc in (False, True)] + [(513, 4104, True)])
def test_swiglu_builder(M, F, scaled):
    """gu is exact in bf16, gates are 0 or a power of two >= 32 after the scales, cs differs between
    the gate and up halves, and quantizing the plain product gives the built bytes and scales."""
    c = dc.swiglu_case(M, F, scaled)
    assert torch.equal(c.gu.to(F32), c.gu32)
    gu = c.gu32 if not scaled else c.gu32 * c.rs[:, None] * c.cs[None, :]
    gate = gu[:, :F]
    assert bool(((gate == 0) | (gate >= 32)).all()) and torch.equal(torch.log2(gate[gate > 0]), torch.log2(gate[gate > 0]).round())
    assert torch.equal(1.0 + torch.exp(-gate[gate > 0]), torch.ones_like(gate[gate > 0]))  # silu(g) = g in fp32
    if scaled:
        dc.check_scales(c.rs) if M > 1 else None
        dc.check_scales(c.cs)
        assert (c.cs[:F] != c.cs[F:]).double().mean().item() > 0.5
    q, s = dc.quant_reference(dc.swiglu_product(c))
    assert_exact(q, c.q, dc.quant_where, "reference bytes")
    assert_exact(s, c.s, what="reference scales")


def test_swiglu_forms():
    assert [dc.swiglu_form(3, F) for F in dc.SWIGLU_F] == [(2, 1024)] * 5 + [(4, 1024)] * 2 + [(0, 256)]
    assert [dc.swiglu_form(513, F)[0] for F in dc.SWIGLU_F] == [2, 4, 4, 8, 8, 16, 16, 0]


def test_lora_builders():
    for K in (8, 520):
        c = dc.shrink_case(K)
        assert torch.equal(c.want[1], torch.full_like(c.want[1], dc.CANARY)) and torch.equal(c.want[5], c.want[1])
        assert torch.equal(c.want[0], (c.A[0].float() @ c.x[0].float())) and not torch.equal(c.want[2], c.want[3])
    for R in dc.EXPAND_R:
        cols = dc.expand_cols(R)
        assert cols == {8: 1024, 16: 512, 32: 256, 64: 128}[R]
        shapes = dc.expand_shapes(R)
        assert [N for N, _ in shapes[:3]] == [cols - 1, cols, cols + 1] and (1000, (333, 334, 1000)) in shapes
        N, ends = shapes[3]
        c = dc.expand_case(R, N, ends)
        assert torch.equal(c.want.to(F64), dc.expand_ref(c.t64, c.B64, c.y64, ends, R))  # bf16 holds it
        assert torch.equal(c.want[1], c.y0[1]) and torch.equal(c.want[5], c.y0[5]) and not torch.equal(c.want[0], c.y0[0])
        idx = torch.where(c.idx < dc.LORA_S, c.idx, -1)  # (the library reference knows -1 only)
        assert torch.equal(c.want, sops.lora_expand_ref(c.t, c.B, idx, ends, c.y0))


# ==================================================================================================
# Without a GPU: the judge
# ==================================================================================================
def test_assert_exact_accepts_equal_and_reports_where():
    c = dc.gemv_case(8197, 1024, True)
    assert_exact(c.want.clone(), c.want)
    out = c.want.clone()
    out[2, 8196] = NAN
    with pytest.raises(AssertionError) as e:
        assert_exact(out, c.want, dc.gemv_where(8197, 2), "poke")
    msg = str(e.value)
    print(msg)
    assert "poke: 1 of 32788 elements differ, the first at (row 2, column 8196)" in msg
    assert "workgroup (of the row order) in [1024]" in msg and "in the part-filled last wave in [1]" in msg and len(msg) < 2000
    with pytest.raises(AssertionError):
        assert_exact(out.float(), c.want)  # another dtype is not "equal"


GEMV_DEFECTS = [("lost_chunk", False, 1027, 2560), ("lost_chunk", True, 8197, 2048), ("tail_step", False, 1027, 2560),
                ("tail_step", True, 8197, 3072), ("tail_unwritten", True, 8197, 2048), ("tail_copied", True, 8197, 2048),
                ("tail_copied", False, 37, 2560), ("neighbour_scale", True, 8197, 2048)]


@pytest.mark.parametrize("kind,fp8,N,K", GEMV_DEFECTS)
def test_gemv_defect_is_caught(kind, fp8, N, K):
    """A lane's lost 8- or 16-column chunk, a skipped K-tail step, a tail wave's rows unwritten or copied
    from the neighbour, a neighbour row's scale: each changes stored values."""
    c = dc.gemv_case(N, K, fp8)
    out = dc.gemv_defect(c, kind)
    rep = dc.mismatch_report(out, c.want, dc.gemv_where(N, dc.gemv_fp8_rows(N) if fp8 else 1))
    print(f"{kind} (fp8 {fp8}) at N={N} K={K}: old metric {dc.old_metric(out, c.exact):.3e}\n  {rep}")
    assert rep is not None
    if kind.startswith("tail_") and kind != "tail_step":
        assert f"workgroup (of the row order) in [{(N - 1) // (8 if fp8 else 4)}]" in rep
    if kind == "lost_chunk":
        assert f"column {N // 2})" in rep


@pytest.mark.parametrize("kind", ["wrong_register", "stale_slot", "neighbour_scale", "padded_row"])
def test_gemm_defect_is_caught(kind):
    """One wrong 4-column register per tile, a stale ring slot (one K-step's activations taken from
    the step before), a neighbour row's scale, a stored padded row."""
    c = dc.gemm_case(256, 384, 512)
    if kind == "padded_row":
        out, want = dc.gemm_defect(c, kind, M=200), dc.padded_want(c, 200)
        assert_exact(want.clone().view(torch.int16), want.view(torch.int16))  # (NaN canary rows: compared as bits)
    else:
        out, want = dc.gemm_defect(c, kind), c.want
    rep = dc.mismatch_report(out.view(torch.int16), want.view(torch.int16), dc.rows_gemm_where)
    print(f"{kind}: {rep}")
    assert rep is not None
    if kind == "wrong_register":
        assert "wave row (32 rows) in [1]" in rep and "wave column (32 columns) in [2]" in rep
    if kind == "padded_row":
        assert "the first at (row 200, column 0)" in rep and "64-row block in [3]" in rep


def test_slice_boundary_off_by_one_is_caught():
    for R in dc.EXPAND_R:
        N, ends = 1000, (333, 334, 1000)
        c = dc.expand_case(R, N, ends)
        for shift in (1, -1):
            rep = dc.mismatch_report(dc.expand_defect(c, shift), c.want, dc.expand_where(R, ends))
            print(f"R={R} shift {shift}: {rep}")
            assert rep is not None and f"columns {333 if shift > 0 else 332}.." in rep


@pytest.mark.parametrize("K", [4104, 32776])
def test_first_pass_only_absmax_is_caught(K):
    c = dc.quant_rows_case(K)
    q, s = dc.quant_first_pass_only(c.x)
    assert dc.mismatch_report(s, c.s) is not None and dc.mismatch_report(q, c.q, dc.quant_where) is not None
    q, s = dc.quant_first_pass_only(dc.quant_rows_case(2048).x)
    assert_exact(q, dc.quant_rows_case(2048).q)


OLD_MISSES = ["gemv_lost_chunk", "gemv_fp8_lost_chunk", "rows_gemm_wrong_register"]


@pytest.mark.parametrize("which", OLD_MISSES)
def test_old_bound_misses_these(which):
    """At the older tests' shapes the relative Frobenius norm of these stays under their bound (5e-3 for the
    GEMVs, 1e-2 for the fp8 GEMMs) while stored values differ: a lane's lost chunk in gemv (4100 x 14336)
    and gemv_fp8 (4101 x 14336); one wrong 4-column register in one tile of fp8_rows_gemm (256 x 1024 x 512).
    (A skipped K-tail step, a neighbour's scale over the whole output, a tail wave's row, a slice end off by
    one and a stale ring slot -- 1.3e-2 for one wave's quadrant of one tile at 256 x 512 x 8192 -- are over
    the old bounds: ``test_*_defect_is_caught`` print their figures.)"""
    if which.startswith("gemv"):
        fp8 = which == "gemv_fp8_lost_chunk"
        c = dc.gemv_case(4101 if fp8 else 4100, 14336, fp8)
        out, want, exact, bound = dc.gemv_defect(c, "lost_chunk"), c.want, c.exact, dc.OLD_GEMV_BOUND
    else:
        c = dc.gemm_case(256, 1024, 512)
        out, want, exact, bound = dc.gemm_defect(c, "wrong_register", every_tile=False), c.want, c.exact, dc.OLD_GEMM_BOUND
    old = dc.old_metric(out, exact)
    print(f"{which}: old metric {old:.3e} < {bound:g}; wrong elements {(out != want).sum().item()}")
    assert old < bound
    assert dc.mismatch_report(out, want) is not None


# ==================================================================================================
# With a GPU
# ==================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("N,K", GEMV)
def test_gemv_exact(gpu, N, K):
    """M = 1 .. 4, x with a padded row stride (NaN past K)."""
    C = _ext.require()
    c = dc.gemv_case(N, K, False, str(gpu))
    _, x = dc.padded(c.x, 0, 64, NAN)
    for M in (1, 2, 3, 4):
        assert C.gemv_supported(M, K)
        y = C.gemv(x[:M], c.W)
        assert_exact(y, c.want[:M].contiguous(), dc.gemv_where(N), f"gemv M={M} N={N} K={K} (steps, tails) {dc.gemv_steps(K)}")


@pytest.mark.gpu
@pytest.mark.parametrize("N,K", GEMV8)
def test_gemv_fp8_exact(gpu, N, K):
    """One, two and four rows per wave by the rule of ``dsa_gemv_fp8``, each with a part-filled last
    wave; a neighbour's ``sw`` is another number."""
    if "DSTACK_AMD_GEMV_FP8_R" in os.environ:
        pytest.skip("DSTACK_AMD_GEMV_FP8_R is set: it forces one form for the whole process")
    C = _ext.require()
    c = dc.gemv_case(N, K, True, str(gpu))
    _, x = dc.padded(c.x, 0, 64, NAN)
    R = dc.gemv_fp8_rows(N)
    for M in (1, 2, 3, 4):
        assert C.gemv_fp8_supported(M, K)
        y = C.gemv_fp8(x[:M], c.W, c.sw)
        assert_exact(y, c.want[:M].contiguous(), dc.gemv_where(N, R), f"gemv_fp8 M={M} N={N} K={K}, {R} rows per wave")


@pytest.mark.gpu
@pytest.mark.parametrize("N,K", ROWS)
def test_fp8_rows_gemm_exact(gpu, N, K):
    C = _ext.require()
    c = dc.gemm_case(256, N, K, str(gpu))
    for M in dc.ROWS_M:
        assert C.fp8_rows_gemm_supported(M, N, K)
        s = dc.sub(c, M, N)
        y = C.fp8_rows_gemm(s.xq, s.xs, s.wq, s.ws)
        assert_exact(y, s.want, dc.rows_gemm_where, f"fp8_rows_gemm {M}x{N}x{K}")


@pytest.mark.gpu
def test_fp8_rows_gemm_strided_exact(gpu):
    """xq and wq as column slices of wider buffers (row strides K + 48 and K + 80, NaN bytes around)."""
    C = _ext.require()
    M, N, K = ROWS_STRIDED
    s = dc.sub(dc.gemm_case(256, N, K, str(gpu)), M, N)
    (_, xq), (_, wq) = dc.padded(s.xq, 16, 32, 0x7F), dc.padded(s.wq, 32, 48, 0x7F)
    assert xq.stride(0) % 16 == 0 and xq.stride(0) > K and wq.stride(0) % 16 == 0 and wq.stride(0) > K
    y = C.fp8_rows_gemm(xq, s.xs, wq, s.ws)
    assert_exact(y, s.want, dc.rows_gemm_where, f"fp8_rows_gemm strided {M}x{N}x{K}")


@pytest.mark.gpu
@pytest.mark.parametrize("rw,shuffled,K,split", STREAM)
def test_fp8_stream_gemm_exact(gpu, rw, shuffled, K, split):
    """Every form on offer: rw 64 (split 1), 32 (depth 2 and 3) and 28; row-major, 16-row-shuffled and
    workgroup-shuffled weights; M = 1, 129, 200, 256 and N one and two workgroups wide.  Split cases run
    twice and repeat bit for bit.  Where ``fp8_stream_gemm_supported`` says no, the call is refused."""
    C = _ext.require()
    wgr = dc.stream_wg_rows(rw)
    c = dc.gemm_case(256, 2 * wgr, K, str(gpu))
    for N in (wgr, 2 * wgr):
        wk = dc.stream_weight(c.wq[:N], rw, shuffled)
        for M in dc.STREAM_M:
            ok = C.fp8_stream_gemm_supported(M, N, K, rw, split)
            assert ok == dc.stream_supported(M, N, K, rw, split) == (rw != 64 or split == 1)
            s = dc.sub(c, M, N)
            if not ok:
                with pytest.raises(RuntimeError):
                    C.fp8_stream_gemm(s.xq, s.xs, wk, s.ws, rw, split, shuffled, 2)
                continue
            for depth in dc.stream_depths(rw):
                what = f"fp8_stream_gemm {M}x{N}x{K} rw {rw} split {split} shuffled {shuffled} depth {depth}"
                y = C.fp8_stream_gemm(s.xq, s.xs, wk, s.ws, rw, split, shuffled, depth)
                assert_exact(y, s.want, dc.stream_where(rw), what)
                if split > 1:
                    assert_exact(C.fp8_stream_gemm(s.xq, s.xs, wk, s.ws, rw, split, shuffled, depth), y, dc.stream_where(rw),
                                 what + ", second run against the first")


@pytest.mark.gpu
@pytest.mark.parametrize("K", dc.QUANT_K)
def test_quant_fp8_rows_bitwise(gpu, K):
    """x strided (NaN around it); bytes and scales equal the built ones and ``reference.quant_fp8_rows``."""
    C = _ext.require()
    c = dc.quant_rows_case(K, str(gpu))
    _, x = dc.padded(c.x, 8, 8, NAN)
    q, s = C.quant_fp8_rows(x)
    what = f"quant_fp8_rows K={K} (NIT {dc.quant_nit(K)})"
    assert_exact(q, c.q, dc.quant_where, what + " bytes")
    assert_exact(s, c.s, what=what + " scales")
    qr, sr = dc.quant_reference(c.x.cpu())
    assert_exact(q.cpu(), qr, dc.quant_where, what + " bytes against the reference")
    assert_exact(s.cpu(), sr, what=what + " scales against the reference")


@pytest.mark.gpu
@pytest.mark.parametrize("M,F,scaled", SWIGLU)
def test_swiglu_quant_fp8_rows_bitwise(gpu, M, F, scaled):
    """Indexing, scale handling and every form (1024 and 256 threads per row, NIT 2 .. 16 and two passes)
    of ``swiglu_quant_fp8_rows``, plain and with ``rs`` / ``cs``, on gates for which silu(g) = g exactly.
    The accuracy of silu itself stays with the judged tests of ``tests/test_rowwise_exact.py`` and
    ``tests/test_serving.py``."""
    C = _ext.require()
    c = dc.swiglu_case(M, F, scaled, str(gpu))
    _, gu = dc.padded(c.gu, 0, 16, NAN)
    q, s = C.swiglu_quant_fp8_rows(gu, c.rs, c.cs) if scaled else C.swiglu_quant_fp8_rows(gu)
    what = f"swiglu_quant_fp8_rows M={M} F={F} scaled={scaled} (NIT, threads) {dc.swiglu_form(M, F)}"
    assert_exact(q, c.q, dc.quant_where, what + " bytes")
    assert_exact(s, c.s, what=what + " scales")
    if M <= 8:
        qr, sr = dc.quant_reference(dc.swiglu_product(c).cpu())
        assert_exact(q.cpu(), qr, dc.quant_where, what + " bytes against the reference")
        assert_exact(s.cpu(), sr, what=what + " scales against the reference")


def quant_where_cols(r, c):
    return {"row": r, "thread (8-column chunk % 256)": c // 8 % 256}


@pytest.mark.gpu
@pytest.mark.parametrize("N", dc.SCALE_N)
def test_scale_rows_cols_exact(gpu, N):
    C = _ext.require()
    c = dc.scale_case(N, str(gpu))
    big, y = dc.padded(c.y, 8, 24, 7.0)
    assert C.scale_rows_cols_(y, c.rs, c.cs) is not None
    assert_exact(y, c.want, quant_where_cols, f"scale_rows_cols_ N={N}")
    assert bool((big[:, :8] == 7).all()) and bool((big[:, 8 + N:] == 7).all()), "columns outside y were written"


@pytest.mark.gpu
@pytest.mark.parametrize("K", dc.SHRINK_K)
def test_lora_shrink_exact(gpu, K):
    """L = 8, 24, 192; idx with -1, a slot past the end and repeated slots; x with a padded row stride."""
    c = dc.shrink_case(K, str(gpu))
    _, x = dc.padded(c.x, 0, 64, NAN)
    for L in dc.SHRINK_L:
        A = c.A[:, :L].contiguous()
        t = torch.full((len(dc.LORA_IDX), L), dc.CANARY, device=gpu, dtype=F32)
        assert sops.lora_shrink(x, A, c.idx, out=t) is t
        assert_exact(t, c.want[:, :L].contiguous(), lambda r, j: {"workgroup (8 outputs)": j // 8}, f"lora_shrink K={K} L={L}")


@pytest.mark.gpu
@pytest.mark.parametrize("R", dc.EXPAND_R)
def test_lora_expand_exact(gpu, R):
    """N one short of, at and one past a workgroup's column span; one-column slices; y a slice of a
    wider buffer; rows without an adapter bitwise unchanged."""
    for N, ends in dc.expand_shapes(R):
        c = dc.expand_case(R, N, ends, str(gpu))
        big, y = dc.padded(c.y0, 0, 24, 7.0)
        assert sops.lora_expand(c.t, c.B, c.idx, ends, y) is y
        assert_exact(y, c.want, dc.expand_where(R, ends), f"lora_expand R={R} N={N} ends {ends}")
        assert bool((big[:, N:] == 7).all()), "columns beyond N were written"
        for r in set(range(len(dc.LORA_IDX))) - set(dc.lora_live()):
            assert torch.equal(y[r], c.y0[r])
