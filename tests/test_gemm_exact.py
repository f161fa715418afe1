"""The training GEMMs (``csrc/gemm_nt.hip``: NT, KM, e4m3, the SwiGLU and RoPE epilogues;
``csrc/gemm.hip``: TN) on operands for which every summation order is exact, compared element for
element with the bf16 rounding of the fp64 product (``tests/gemm_cases.py`` has the construction, the
comparison, the defect models and the launch-plan model).

The older GEMM tests feed i.i.d. normal operands and bound one number per call,
``||out - ref|| / ||ref|| < 5e-3``: a stale ring slot in one wave's quadrant, two rows exchanged in a
fragment or one lost k-term stay under it (``test_old_bound_misses_these`` keeps that on record).
Here any of them changes stored values, and the report says which tiles, waves and fragments.

Without a GPU: the builders' invariants for every case the GPU tests use, each defect model caught by
``assert_exact``, and the launch-plan model confirming for 256 CUs that every multi-round shape reaches
the path it is there for.  With one: every launch form that ships -- the persistent grid with its
split remainder (three launches back to back: the workspace ring has two entries), the per-tile grid
on shapes with more tiles than CUs, other tile-order groups, the claimed tile order and the unsplit
and non-persistent forms (switches read once per process: child processes), strided operands, the
fp32-accumulator forms, the fused epilogues, e4m3 and TN.  The GPU tests evaluate the plan model with
the device's CU count and fail, with a message, when a case no longer reaches its path.
"""

import os
import subprocess
import sys

import pytest
import torch

from tests import gemm_cases as gc
from tests.gemm_cases import BF16, F32, F64, assert_exact
from dstack_amd import ops
from dstack_amd.ops import _ext
from dstack_amd.ops import reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NT_KM = [(M, N, K) for M, N in gc.BASIC_SHAPES for K in gc.KS]
MULTI = [(M, N, K, grid) for M, N in gc.MULTI_ROUND for K in gc.KS for grid in (1, 0)]
F8_CASES = [(M, N, K) for M, N in ((256, 256), (512, 768), (4352, 4096)) for K in (256, 512, 768)]  # K in bytes
TN_CASES = [(T, P, Q) for T in (64, 192, 1024) for P, Q in ((256, 256), (768, 512), (4352, 4096))]
SWIGLU = [(512, 384, 128), (1024, 768, 384), (4352, 2048, 128)]       # T, F, K; the last: T/256 * F/128 = 272 tiles
SWIGLU_BWD = [(512, 512, 128), (1024, 768, 384), (4352, 4096, 128)]   # F % 256 == 0; the last: 272 tiles
ROPE = [(2, 256, 256), (1, 1024, 384), (1, 8192, 128)]                # B, S, K; the last reaches the last positions
ROPE_H, ROPE_KV = 2, 1
F32_CASES = [(3072, 8192, 256), (512, 768, 384)]
STRIDED = [(512, 512, 256), (4352, 4096, 256)]
SWITCH_SHAPES = [(4352, 4096, 256), (512, 33024, 256)]
# every (M, N, K) whose operands a GPU test builds through gc.case (K in elements)
ALL_CASES = sorted(set(NT_KM) | {c[:3] for c in MULTI} | set(gc.LONG_K) | set(F8_CASES)
                   | {(P, Q, T) for T, P, Q in TN_CASES} | {(T, 2 * F, K) for T, F, K in SWIGLU}
                   | {(T, F, K) for T, F, K in SWIGLU_BWD} | set(F32_CASES) | set(STRIDED) | set(SWITCH_SHAPES)
                   | {(B * S, (ROPE_H + 2 * ROPE_KV) * 128, K) for B, S, K in ROPE})

# The largest difference, in bf16 ulps of the separate kernel's element, between the dgu of the two
# fused SwiGLU-backward epilogues (transposing and barrier-free), measured on an MI355X on the inputs of
# ``test_swiglu_bwd_epilogue`` with the kernels as they were before this file was added: none, the two
# forms agree in every element (see that test's docstring).
SWIGLU_BWD_FORMS_ULP = 0.0


# ==================================================================================================
# Without a GPU
# ==================================================================================================
@pytest.mark.parametrize("M,N,K", ALL_CASES)
def test_case_invariants(M, N, K):
    a, b, base = gc.operands(M, N, K)
    gc.check_operands(a, b, base, K)
    exact = gc.product(a, b)
    share = gc.check_cap(exact)
    peak = exact.abs().max().item()
    print(f"{M}x{N}x{K}: share of |ref| > 256 {share:.2e}, max |ref| {peak:g}")
    assert peak < 2 ** 24 and torch.equal(exact, exact.round())
    assert torch.equal(exact.to(F32).to(F64), exact)  # what an fp32 accumulator or workspace holds
    if K >= gc.PLANT_K:  # the planted outputs: K-half partials that bf16 cannot hold, a small total
        h = K // 2
        sites = gc.plant_sites(M, N)
        assert len(sites) == (M // 256) * (N // 256)
        for r, c in sites[:: max(1, len(sites) // 8)]:
            p0, p1 = (a[r, :h] * b[c, :h]).sum().item(), (a[r, h:] * b[c, h:]).sum().item()
            assert p0 in (gc.PLANT, gc.PLANT + 1) and -p1 in (gc.PLANT, gc.PLANT + 1) and abs(p0 + p1) <= 1
            assert gc.rb(torch.tensor(p0, dtype=F64)).item() != p0
    else:      # no K-half partial can be rounded by bf16 at all
        assert K // 2 <= 512


def test_assert_exact_accepts_equal_and_reports_where():
    c = gc.case(512, 768, 256)
    assert_exact(c.want.clone(), c.want)
    out = c.want.clone()
    out[256 + 128 + 64 + 16 + 3, 512 + 64 + 16 + 5] += 1
    with pytest.raises(AssertionError) as e:
        assert_exact(out, c.want, exact=c.exact, halves=lambda: gc.halves(c), what="poke")
    msg = str(e.value)
    print(msg)
    assert "poke: 1 of 393216 elements differ" in msg and "[(1, 2)]" in msg
    assert "row % 64 // 16 in [1], row // 128 in [1], col % 32 // 16 in [1], col // 128 in [0]" in msg
    assert "dropping K half 0 explains 0 of 1" in msg and len(msg) < 2000


def _defect_args(c):
    ntm, ntn = c.M // 256, c.N // 256
    return dict(tm=ntm - 1, tn=ntn // 2, tm2=0, tn2=ntn - 1) if ntm * ntn > 1 else {}


@pytest.mark.parametrize("kind", gc.DEFECTS)
@pytest.mark.parametrize("M,N", [(256, 256), (4352, 4096)])
def test_defect_is_caught(M, N, kind):
    """Every defect model, in one tile of a single-tile output and of the 4352x4096 one, changes stored
    values (an exchange of two tiles needs two tiles).  The old metric of each is printed."""
    if kind == "tiles_exchanged" and (M, N) == (256, 256):
        M = 512  # (the smallest output with two tiles)
    K = 8192 if kind == "partial_rounded" else 1024
    c = gc.case(M, N, K)
    out, want = gc.defect(c, kind, **_defect_args(c))
    exact = c.exact_acc if kind == "base_dropped" else c.exact
    rep = gc.mismatch_report(out, want, exact=exact, halves=lambda: gc.halves(c))
    print(f"{kind} at {M}x{N}x{K}: old metric {gc.old_metric(out, exact):.3e} (bound {gc.OLD_BOUND:g})\n  {rep}")
    assert rep is not None
    with pytest.raises(AssertionError):
        assert_exact(out, want)
    if kind == "half_missing":
        assert "dropping K half 1 explains" in rep and "(all: the split path)" in rep


@pytest.mark.parametrize("kind,K", [("k_term", 1024), ("row_swap", 1024), ("stale_slot", 1024), ("stale_slot", 4096)])
def test_old_bound_misses_these(kind, K):
    """On the 4352x4096 output the relative Frobenius norm of a lost k-term or two exchanged rows in one
    fragment, and of a stale ring slot in one quadrant at K >= 1024, is under the older tests' 5e-3."""
    c = gc.case(4352, 4096, K)
    out, want = gc.defect(c, kind, tm=16, tn=8)
    old = gc.old_metric(out, c.exact)
    print(f"{kind} at K = {K}: old metric {old:.3e} < {gc.OLD_BOUND:g}; wrong elements {(out != want).sum().item()}")
    assert old < gc.OLD_BOUND
    assert gc.mismatch_report(out, want) is not None


def test_plan_model_paths_at_256_cus():
    """For 256 CUs every multi-round shape reaches the path it is in the table for, at every K and in
    both grid modes, and the tile order covers every tile once."""
    for (M, N), _ in gc.MULTI_ROUND.items():
        for K in gc.KS:
            p = gc.reach(M, N, K, 256, 1)
            assert p.stride == 32 and p.grid == 256 and sum(p.cnt) == p.tiles
            assert any(p.splits) == (K in (256, 1024) and (M, N) != (3328, 8192)), (M, N, K, p.splits)
            assert not p.workspace or any(p.splits)
            q = gc.reach(M, N, K, 256, 0)
            assert q.grid == q.tiles and not q.workspace
            for g in (0, *gc.GROUPS):
                o = gc.tile_origins(gc.reach(M, N, K, 256, 1, group_env=g))
                assert sorted(o) == [(i, j) for i in range(p.ntm) for j in range(p.ntn)]
    p = gc.plan(512, 33024, 256, 256, 1)
    assert p.splits == [True, True] + [False] * 6 and p.workspace      # XCDs disagree on the last round
    assert gc.plan(4352, 4096, 256, 256, 1, dynamic_env=True).queue
    assert not any(gc.plan(4352, 4096, 256, 256, 1, dynamic_env=True).splits)   # claimed order: no split
    assert not any(gc.plan(4352, 4096, 256, 256, 1, split_env=False).splits)
    assert not gc.plan(4352, 4096, 256, 256, -1, persistent_env=False).persistent
    assert gc.plan(4352, 4096, 256, 256, 1).heights == [8, 8, 1] and gc.plan(17408, 1024, 256, 256, 1).group == 4
    for T, F, K in SWIGLU[-1:]:
        assert gc.plan(T, F, K, 256, -1, ncol=128, split_epi=False).persistent
    for T, F, K in SWIGLU_BWD[-1:]:
        assert gc.plan(T, F, K, 256, -1, split_epi=False).persistent
    with pytest.raises(AssertionError, match="no longer reaches its path"):
        gc.reach(4352, 4096, 256, 240, 1)  # (another CU count: rx is 4, and the test says so)
    with pytest.raises(AssertionError, match="no longer reaches its path"):
        gc.reach(4352, 4096, 256, 304, 1)  # (fewer tiles than CUs)


# ==================================================================================================
# With a GPU
# ==================================================================================================
def _cus(gpu) -> int:
    return torch.cuda.get_device_properties(gpu).multi_processor_count


def _km(x: torch.Tensor) -> torch.Tensor:
    """[M, K] -> the token-major [K, M] operand of the KM and TN forms."""
    return x.t().contiguous()


def _check(out, want, c, what, acc=False):
    assert_exact(out, want, exact=c.exact_acc if acc else c.exact, halves=lambda: gc.halves(c), what=what)


def _run_nt_km(C, c, reps: int, what: str):
    """NT and KM, storing and accumulating, ``reps`` launches of each back to back into separate
    outputs with no synchronisation between them; then every output against the reference."""
    ak, bk = _km(c.a), _km(c.b)
    outs = []
    for name, fn in (("nt", lambda o, acc: C.gemm_nt(c.a, c.b, o, acc)),
                     ("km", lambda o, acc: C.gemm_km(ak, bk, o, 1 if acc else 0))):
        for acc in (False, True):
            os_ = [c.base.clone() if acc else torch.full_like(c.base, float("nan")) for _ in range(reps)]
            for o in os_:
                fn(o, acc)
            outs += [(f"{what} {name} {'accumulate' if acc else 'store'} launch {i}", o, acc) for i, o in enumerate(os_)]
    for name, o, acc in outs:
        _check(o, c.want_acc if acc else c.want, c, name, acc)


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", NT_KM)
def test_nt_km_exact(gpu, M, N, K):
    C = _ext.require()
    assert C.gemm_nt_supported(M, N, K) and C.gemm_km_supported(M, N, K)
    _run_nt_km(C, gc.case(M, N, K, str(gpu)), 1, f"{M}x{N}x{K}")


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,grid", MULTI)
def test_nt_km_multi_round_exact(gpu, M, N, K, grid):
    """More tiles than CUs, persistent (1: static order, split remainder where the plan says so) and
    per tile (0); three launches back to back (two workspace entries; the ticket counters must be
    back at zero for the third)."""
    C = _ext.require()
    p = gc.reach(M, N, K, _cus(gpu), grid)
    c = gc.case(M, N, K, str(gpu))
    C.gemm_nt_set_grid(grid)
    try:
        _run_nt_km(C, c, 3, f"{M}x{N}x{K} grid {grid} (rx {p.rx}, splits {p.splits}, group {p.group})")
    finally:
        C.gemm_nt_set_grid(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [1, 0])
@pytest.mark.parametrize("group", gc.GROUPS)
def test_nt_km_tile_order_groups_exact(gpu, monkeypatch, group, grid):
    C = _ext.require()
    M, N, K = 4352, 4096, 256
    gc.reach(M, N, K, _cus(gpu), grid, group_env=group)
    monkeypatch.setenv("DSTACK_AMD_GEMM_NT_GROUP", str(group))  # read at every launch
    C.gemm_nt_set_grid(grid)
    try:
        _run_nt_km(C, gc.case(M, N, K, str(gpu)), 1, f"{M}x{N}x{K} grid {grid} group {group}")
    finally:
        C.gemm_nt_set_grid(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", gc.LONG_K)
def test_nt_km_long_k_exact(gpu, M, N, K):
    """The ring's steady state at the step's reduction lengths; the planted outputs carry K-half
    partials that a bf16 rounding would change."""
    _run_nt_km(_ext.require(), gc.case(M, N, K, str(gpu)), 1, f"{M}x{N}x{K}")


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", F32_CASES)
def test_km_f32_forms_exact(gpu, M, N, K):
    """gemm_km_f32 on a strided fp32 accumulator view: mode 0 stores the product, mode 1 adds it (both
    exact outright), mode 2 writes bf16(accumulator + product) into a strided bf16 view; neighbouring
    columns stay untouched.  (3072, 8192, 256) runs the split remainder, three stores back to back."""
    C = _ext.require()
    if (M, N) in gc.MULTI_ROUND:
        assert any(gc.reach(M, N, K, _cus(gpu), -1).splits)
    c = gc.case(M, N, K, str(gpu))
    ak, bk = _km(c.a), _km(c.b)
    bigs = [torch.full((M, N + 128), 7.0, device=gpu, dtype=F32) for _ in range(3)]
    accs = [b[:, 64:64 + N] for b in bigs]
    for a in accs:
        C.gemm_km_f32(ak, bk, a, None, 0)
    for i, a in enumerate(accs):
        assert_exact(a, c.exact.to(F32), exact=c.exact, halves=lambda: gc.halves(c), what=f"mode 0 launch {i}")
    acc = accs[0]
    acc.copy_(c.base)
    C.gemm_km_f32(ak, bk, acc, None, 1)
    assert_exact(acc, c.exact_acc.to(F32), exact=c.exact_acc, halves=lambda: gc.halves(c), what="mode 1")
    obig = torch.full((M, N + 256), 7.0, device=gpu, dtype=BF16)
    out = obig[:, 128:128 + N]
    C.gemm_km_f32(ak, bk, acc, out, 2)
    two = c.exact_acc + c.exact
    assert_exact(out, gc.to_bf16(two), exact=two, halves=lambda: gc.halves(c), what="mode 2")
    assert_exact(acc, c.exact_acc.to(F32), what="mode 2 must leave the accumulator")
    for b in bigs:
        assert (b[:, :64] == 7).all() and (b[:, 64 + N:] == 7).all()
    assert (obig[:, :128] == 7).all() and (obig[:, 128 + N:] == 7).all()


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", STRIDED)
def test_nt_km_strided_exact(gpu, M, N, K):
    """Views into wider buffers: lda, ldb, ldc larger than the extent, storing and accumulating;
    (4352, 4096) is multi-round (a strided C under the persistent grid and its split remainder)."""
    C = _ext.require()
    if (M, N) in gc.MULTI_ROUND:
        assert any(gc.reach(M, N, K, _cus(gpu), -1).splits)
    c = gc.case(M, N, K, str(gpu))

    def view(x, left, right):
        big = torch.full((x.shape[0], left + x.shape[1] + right), 3.0, device=gpu, dtype=BF16)
        v = big[:, left:left + x.shape[1]]
        v.copy_(x)
        return big, v

    for form in ("nt", "km"):
        a, b = (c.a, c.b) if form == "nt" else (_km(c.a), _km(c.b))
        (_, av), (_, bv) = view(a, 32, 32), view(b, 0, 128)
        for acc in (False, True):
            cbig, out = view(c.base, 128, 128)
            if form == "nt":
                C.gemm_nt(av, bv, out, acc)
            else:
                C.gemm_km(av, bv, out, 1 if acc else 0)
            _check(out, c.want_acc if acc else c.want, c, f"{form} strided acc={acc}", acc)
            assert (cbig[:, :128] == 3).all() and (cbig[:, 128 + N:] == 3).all()


@pytest.mark.gpu
@pytest.mark.parametrize("T,F,K", SWIGLU)
@pytest.mark.parametrize("transposed", [True, False])
def test_swiglu_epilogue_exact(gpu, T, F, K, transposed):
    """gu is the exact product, a what the separate SwiGLU kernel makes of that gu, a^T its transpose."""
    C = _ext.require()
    assert C.gemm_nt_swiglu_supported(T, F, K)
    if T // 256 * (F // 128) > 256:
        assert gc.plan(T, F, K, _cus(gpu), -1, ncol=128, split_epi=False).persistent, "no longer more tiles than CUs"
    c = gc.case(T, 2 * F, K, str(gpu))
    gu, a, aT = C.gemm_nt_swiglu(c.a, c.b, transposed)
    _check(gu, c.want, c, "gu")
    assert_exact(a, C.swiglu_fwd(c.want), what="a")
    if transposed:
        assert_exact(aT, a.t().contiguous(), what="aT")
    else:
        assert aT.numel() == 0


def _ulps(x, y, r):
    """max |x - y| in bf16 ulps of ``r`` (0 where x == y)."""
    d = (x.to(F64) - y.to(F64)).abs()
    return torch.where(d == 0, torch.zeros_like(d), d / gc.bf16_ulp(r)).max().item()


@pytest.mark.gpu
@pytest.mark.parametrize("T,F,K", SWIGLU_BWD)
def test_swiglu_bwd_epilogue(gpu, T, F, K):
    """The kernel rounds da to bf16 first, exactly, so dgu is judged per element against the separate
    kernel ``swiglu_bwd(bf16(da), gu)``.  The two compute the same fp32 formula and may differ by the
    compiler's contraction of it.  Measured on an MI355X, on these inputs, before this test existed: the
    two fused forms (transposing and barrier-free) differ from each other by
    ``SWIGLU_BWD_FORMS_ULP`` = 0 bf16 ulps of the separate kernel's element (no element differs, at all
    three shapes); fused against separate is allowed that plus one ulp, and measured 1 ulp, on 4 of
    524288, 10 of 1572864 and 172 of 35651584 elements.  dgu^T is the transpose of dgu."""
    C = _ext.require()
    assert C.gemm_nt_swiglu_bwd_supported(T, F, K)
    if T // 256 * (F // 256) > 256:
        assert gc.plan(T, F, K, _cus(gpu), -1, split_epi=False).persistent, "no longer more tiles than CUs"
    c = gc.case(T, F, K, str(gpu))
    g = torch.Generator(device=gpu).manual_seed(T + F + K)
    gu = torch.randn(T, 2 * F, device=gpu, generator=g).to(BF16)
    sep = C.swiglu_bwd(c.want, gu)  # c.want = bf16(da), exact
    dgu_t, dguT = C.gemm_nt_swiglu_bwd(c.a, c.b, gu, True)
    dgu_r, none = C.gemm_nt_swiglu_bwd(c.a, c.b, gu, False)
    forms, ut, ur = _ulps(dgu_t, dgu_r, sep), _ulps(dgu_t, sep, sep), _ulps(dgu_r, sep, sep)
    print(f"swiglu_bwd {T}x{F}x{K}: ulps transposing vs barrier-free {forms:g}, transposing vs separate {ut:g}, "
          f"barrier-free vs separate {ur:g} (allowed {SWIGLU_BWD_FORMS_ULP + 1:g})")
    assert none.numel() == 0
    assert_exact(dguT, dgu_t.t().contiguous(), what="dguT")
    assert torch.isfinite(dgu_t.float()).all() and torch.isfinite(dgu_r.float()).all()
    assert forms <= SWIGLU_BWD_FORMS_ULP, forms
    assert ut <= SWIGLU_BWD_FORMS_ULP + 1 and ur <= SWIGLU_BWD_FORMS_ULP + 1, (ut, ur)


@pytest.mark.gpu
@pytest.mark.parametrize("B,S,K", ROPE)
def test_rope_epilogue(gpu, B, S, K):
    """The v columns are the exact product.  A rotated column is x cos - y sin (or y cos + x sin) of two
    exact integers and fp32 table entries, computed in fp32 and rounded once: per element
    |err| <= ulp_bf16(ref) + 2^-20 (|x| + |y|) -- the output rounding (half an ulp of the stored value,
    within one of the reference's) plus two products and a sum in fp32 (3 roundings of 2^-24 relative to
    at most |x| + |y|, and their carry through the output rounding)."""
    C = _ext.require()
    H, KV = ROPE_H, ROPE_KV
    M, N, rot = B * S, (H + 2 * KV) * 128, (H + KV) * 128
    assert C.gemm_nt_rope_supported(M, N, K, S, rot)
    c = gc.case(M, N, K, str(gpu))
    cos, sin = ref.rope_cos_sin(S, 128, 500000.0, gpu)
    out = C.gemm_nt_rope(c.a, c.b, cos, sin, S, rot)
    assert_exact(out[:, rot:].contiguous(), c.want[:, rot:].contiguous(), what="v columns")
    p = c.exact[:, :rot].reshape(M, H + KV, 2, 64)
    x, y = p[:, :, 0], p[:, :, 1]
    pos = torch.arange(M, device=gpu) % S
    cs, sn = cos.to(F64)[pos].view(M, 1, 64), sin.to(F64)[pos].view(M, 1, 64)
    want = torch.stack([x * cs - y * sn, y * cs + x * sn], 2)
    err = (out[:, :rot].to(F64).reshape(M, H + KV, 2, 64) - want).abs()
    bound = gc.bf16_ulp(want) + 2.0 ** -20 * (x.abs() + y.abs()).unsqueeze(2)
    worst = (err / bound).max().item()
    print(f"rope B={B} S={S} K={K}: worst err / bound {worst:.3f}")
    bad = (err > bound).nonzero()
    assert bad.shape[0] == 0, (f"{bad.shape[0]} rotated elements over the bound, first (row, head, half, dim): "
                               f"{bad[:8].tolist()}, rows % 256 {sorted(set((bad[:, 0] % 256).tolist()))[:16]}")


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", F8_CASES)
def test_nt_f8_exact(gpu, M, N, K):
    """The same values as e4m3 bytes; K counts bytes (K / 2 of the kernel's 2-byte units)."""
    C = _ext.require()
    assert C.gemm_nt_f8_supported(M, N, K)
    if (M, N) in gc.MULTI_ROUND:  # (the plan counts K in the kernel's 2-byte units)
        p = gc.reach(M, N, K // 2, _cus(gpu), -1)
        assert any(p.splits) == (K == 512)
    c = gc.case(M, N, K, str(gpu))
    a8, b8 = gc.e4m3_bytes(c.a), gc.e4m3_bytes(c.b)
    outs = [torch.full_like(c.base, float("nan")) for _ in range(3)]
    for o in outs:
        C.gemm_nt_f8(a8, b8, o)
    for i, o in enumerate(outs):
        _check(o, c.want, c, f"f8 launch {i}")


@pytest.mark.gpu
@pytest.mark.parametrize("T,P,Q", TN_CASES)
@pytest.mark.parametrize("accumulate", [False, True])
def test_tn_exact(gpu, T, P, Q, accumulate):
    """gemm_tn through ops.weight_grad: one slice (T = 64), an odd slice count (192), 1024; up to
    more workgroups than CUs (4352x4096)."""
    C = _ext.require()
    assert C.gemm_tn_supported(P, Q, T)
    c = gc.case(P, Q, T, str(gpu))
    out = c.base.clone() if accumulate else torch.full_like(c.base, float("nan"))
    ops.weight_grad(_km(c.a), _km(c.b), out, accumulate=accumulate)
    _check(out, c.want_acc if accumulate else c.want, c, f"tn {T}x{P}x{Q}", accumulate)


@pytest.mark.gpu
def test_tn_strided_rows_exact(gpu):
    C = _ext.require()
    T, P, Q = 192, 768, 512
    assert C.gemm_tn_supported(P, Q, T)
    c = gc.case(P, Q, T, str(gpu))
    gw = torch.full((T, P + 128), 3.0, device=gpu, dtype=BF16)
    xw = torch.full((T, Q + 64), 3.0, device=gpu, dtype=BF16)
    g, x = gw[:, 64:64 + P], xw[:, :Q]
    g.copy_(c.a.t())
    x.copy_(c.b.t())
    obig = torch.full((P, Q + 256), 3.0, device=gpu, dtype=BF16)
    out = obig[:, 128:128 + Q]
    for acc in (False, True):
        out.copy_(c.base)
        ops.weight_grad(g, x, out, accumulate=acc)
        _check(out, c.want_acc if acc else c.want, c, f"tn strided acc={acc}", acc)
    assert (obig[:, :128] == 3).all() and (obig[:, 128 + Q:] == 3).all()


def switch_child(reps: int):
    """Body of one child of ``test_process_wide_switches_exact``: NT and KM, storing and accumulating,
    at the switch shapes; exit status 1 with the report on a mismatch."""
    C = _ext.require()
    try:
        for M, N, K in SWITCH_SHAPES:
            _run_nt_km(C, gc.case(M, N, K, "cuda:0"), reps, f"{M}x{N}x{K}")
        torch.cuda.synchronize()
    except AssertionError as e:
        print(e, flush=True)
        sys.exit(1)
    print("exact", flush=True)


@pytest.mark.gpu
def test_process_wide_switches_exact(gpu):
    """DSTACK_AMD_GEMM_NT_DYNAMIC, _SPLIT and _PERSISTENT are read once per process: one fresh child
    per variant, whose environment carries no other DSTACK_AMD_GEMM_NT_* variable.  Under the claimed
    order each shape is launched three times (the queue slot's counters are re-zeroed by the last
    workgroup).  The first child that fails, faults or times out ends the test: nothing starts after it."""
    cus = _cus(gpu)
    for M, N, K in SWITCH_SHAPES:
        gc.reach(M, N, K, cus, 1)
        assert gc.plan(M, N, K, cus, -1, dynamic_env=True).queue
        assert gc.plan(M, N, K, cus, -1, split_env=False).persistent
        assert gc.plan(M, N, K, cus, -1, persistent_env=False).grid > cus
    variants = {"default": {}, "dynamic": {"DSTACK_AMD_GEMM_NT_DYNAMIC": "1"}, "no_split": {"DSTACK_AMD_GEMM_NT_SPLIT": "0"},
                "per_tile": {"DSTACK_AMD_GEMM_NT_PERSISTENT": "0"}}
    for name, extra in variants.items():
        env = {k: v for k, v in os.environ.items() if not k.startswith("DSTACK_AMD_GEMM_NT_")}
        env.update(extra)
        script = f"from tests import test_gemm_exact as t; t.switch_child({3 if name == 'dynamic' else 1})"
        r = subprocess.run([sys.executable, "-c", script], env=env, cwd=ROOT, timeout=120, capture_output=True, text=True)
        tail = (r.stdout + r.stderr)[-3000:]
        assert r.returncode == 0 and "exact" in r.stdout, f"variant {name} ({extra}): exit status {r.returncode}\n{tail}"
