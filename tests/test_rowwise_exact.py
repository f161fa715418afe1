"""The row-wise kernels of ``csrc/elementwise.hip`` -- RMSNorm forward (wave-per-row, block-per-row,
with the residual add, with the e4m3 output and its ``dr`` / ``dc`` scaling), RMSNorm backward and its
two-pass ``colsum``, SwiGLU (plain and transposing), ``rope_qkv``, cross-entropy, AdamW,
``embedding_bwd`` and ``transpose2d`` -- judged in every stored element against fp64 arithmetic on
the same bf16 inputs, at the chunk and grid edges of each kernel (``tests/rowwise_cases.py`` has the
inputs, the references, the judge with the derivation of every bound, the table of shapes and the
defect models).

The older tests of these kernels (``tests/test_ops_gpu.py``) bound one number per tensor,
``max|a - b| <= atol + rtol max|b|``, on i.i.d. inputs at sizes that fill every chunk pass: a row
normalised with its neighbour's rstd or a (row, chunk) missing from the weight gradient stays under
it (``test_old_bound_misses_these``).  ``test_rms_norm``,
``test_add_rms_norm``, ``test_swiglu``, ``test_cross_entropy`` and ``test_adamw`` there are subsumed by
the tests here; they stay as they are.

Without a GPU: the builders' invariants, the plain fp32 implementation (``ops.reference``) inside
every bound at every case the GPU tests run, every defect model rejected.  With one: the same cases
through the HIP bindings.  Right before each call a NaN-filled tensor of every output's size and
dtype is allocated and freed (``HipImpl._poison``), so that an element the kernel does not write is
likely to read NaN: a heuristic on the caching allocator, never the only check on a kernel.
"""

import pytest
import torch

from tests import rowwise_cases as rc
from tests.rowwise_cases import BF16, F32, F64
from dstack_amd import ops
from dstack_amd.ops import _ext
from dstack_amd.ops import reference as ref

CPU = rc.Fp32Impl()


def _merge(into: dict, name: str, fr: dict):
    for k, v in fr.items():
        into[f"{name} {k}"] = max(into.get(f"{name} {k}", 0.0), v)


def _show(fr: dict):
    print("largest used fraction of the bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(fr.items())))


def run_family(impl, family: str, device: str) -> dict:
    """Every case of ``family`` through ``impl``; the largest used fraction of each bound."""
    fr = {}
    if family == "norm_fwd":
        for D in rc.NORM_D:
            for rows in rc.NORM_ROWS:
                for add in (False, True):
                    _merge(fr, "add_rms_norm" if add else "rms_norm", rc.check_norm_fwd(impl, rows, D, add, device))
    elif family == "norm_fp8":
        for D in rc.FP8_D:
            for rows in rc.FP8_ROWS:
                for form in rc.FP8_FORMS:
                    _merge(fr, "rms_norm_fp8", rc.check_norm_fp8(impl, rows, D, form, device))
    elif family == "norm_bwd":
        for rows, D in rc.BWD_CASES:
            for with_dres, form in rc.BWD_FORMS:
                _merge(fr, "rms_norm_bwd", rc.check_norm_bwd(impl, rows, D, with_dres, form, device))
    elif family == "norm_bwd_exact":
        for rows, D in rc.BWD_EXACT:
            rc.check_norm_bwd_exact(impl, rows, D, device)
    elif family == "swiglu":
        for rows, Fh in rc.SWIGLU_CASES:
            _merge(fr, "swiglu", rc.check_swiglu(impl, rows, Fh, device))
    elif family == "cross_entropy":
        for rows, V in rc.CE_CASES:
            for variant in rc.CE_VARIANTS:
                _merge(fr, "cross_entropy", rc.check_ce(impl, rows, V, variant, device))
    elif family == "adamw":
        for n in rc.ADAMW_N:
            for mb in rc.ADAMW_BLOCKS:
                for wd in rc.ADAMW_WD:
                    _merge(fr, "adamw", rc.check_adamw(impl, n, mb, wd, device))
    elif family == "embedding":
        for V, D in rc.EMBED_CASES:
            rc.check_embedding(impl, V, D, device)
    else:
        raise ValueError(family)
    return fr


FAMILIES = ["norm_fwd", "norm_fp8", "norm_bwd", "norm_bwd_exact", "swiglu", "cross_entropy", "adamw", "embedding"]


# ==================================================================================================
# Without a GPU
# ==================================================================================================
@pytest.mark.parametrize("family", FAMILIES)
def test_fp32_reference_is_inside_every_bound(family):
    """The bounds are not too tight: ``ops.reference`` on fp32 CPU tensors, rounded to bf16 where the
    kernels round, passes the judge at every case of the GPU tests, no element left out."""
    fr = run_family(CPU, family, "cpu")
    _show(fr)
    assert all(v <= 1.0 for v in fr.values())


def test_bounds_and_shapes_are_what_the_docstring_says():
    assert rc.norm_c(8192, 64) == (rc.C_CAP, rc.C_CAP) and rc.norm_c(6144, 64)[1] == 56 and rc.norm_c(4104, 64)[1] == 44
    assert max(rc.norm_c(D, 256)[1] for D in rc.NORM_D) == 25.5
    assert max(rc.bwd_c(r, D)[0] for r, D in rc.BWD_CASES) == 50 and max(rc.bwd_c(r, D)[1] for r, D in rc.BWD_CASES) <= 41
    assert [rc.ce_fwd_c(V) for _, V in rc.CE_CASES] == [25, 25, 26, 40, 64]
    assert max(rc.ADAMW_C.values()) <= rc.C_CAP and rc.SWIGLU_C <= rc.C_CAP and rc.CE_BWD_C <= rc.C_CAP
    # NCH of both dispatch macros, every arm, filled and part filled
    nch = lambda D, tpr: next(n for n in (1, 2, 4, 8, 16) if n >= rc.ceil_div(D // 8, tpr))  # noqa: E731
    assert {nch(D, 64) for D in rc.NORM_D} == {1, 2, 4, 8, 16} and {nch(D, 256) for D in rc.NORM_D} == {1, 2, 4}
    # each arm with a part-filled last pass, and each arm above 1 chunk per thread with every pass filled
    assert {nch(D, 64) for D in rc.NORM_D if D // 8 % 64} == {1, 2, 4, 8, 16} and {nch(D, 256) for D in rc.NORM_D if D // 8 % 256} == {1, 2, 4}
    assert {nch(D, 64) for D in rc.NORM_D if D // 8 == 64 * nch(D, 64)} >= {4, 16} and nch(8192, 256) == 4 and 8192 // 8 == 4 * 256
    assert [D // 8 % 256 for D in (520, 2056, 3584, 4104)] == [65, 1, 192, 1]  # part-filled last passes
    assert all(D % 8 == 0 and D <= 8192 for D in rc.NORM_D + rc.FP8_D + rc.BWD_D)
    # backward: rows per workgroup (trip counts of red[parity]) and the partial rows of colsum
    trips = lambda rows: {rc.ceil_div(rows - b, rc.bwd_grid(rows)) for b in (0, rc.bwd_grid(rows) - 1)}  # noqa: E731
    assert trips(1024) == {1} and trips(1025) == {2, 1} and trips(1500) == {2, 1} and trips(2049) == {3, 2}
    assert [(rc.bwd_grid(r), rc.ceil_div(rc.bwd_grid(r), 16)) for r in (1, 3, 17)] == [(1, 1), (3, 1), (17, 2)]
    assert max(r * D for r, D in rc.BWD_CASES) <= 2049 * 8192 and max(r * D for r in rc.NORM_ROWS for D in rc.NORM_D) <= 2049 * 8192


def test_builders_invariants():
    for rows, D in rc.BWD_EXACT:
        rc.check_bwd_exact_limits(rc.bwd_exact_inputs(rows, D))
    sc = rc.row_scales(1027)
    assert sc.min() == 2.0 ** -6 and sc.max() == 2.0 ** 6 and (sc[1:] != sc[:-1]).all()
    i = rc.norm_inputs(3, 520)
    assert (i.x[1] == 0).all() and (i.delta[1] == 0).all() and (i.w < 0).any()
    r = rc.norm_ref(i.x, i.w, i.delta)
    assert abs(r.rstd[1].item() * rc.EPS32 ** 0.5 - 1) < 1e-12 and (r.y[1] == 0).all()
    for V, D in rc.EMBED_CASES:
        e = rc.embed_inputs(V, D)
        assert (e.ids == 0).sum() == 300 and (e.ids == V - 1).sum() == 2 and (e.ids == 5).sum() == 1
    for rows, V in rc.CE_CASES:
        seen = set()
        for variant in rc.CE_VARIANTS:
            c = rc.ce_inputs(rows, V, variant)
            seen |= set(c.target.tolist())
            for row, kind in enumerate(c.kinds):
                l, t = c.logits[row].double(), int(c.target[row])
                if kind == "random":
                    assert int(l.argmax()) // 8 == V // 8 - 1
                elif kind == "equal":
                    assert (l == l[0]).all()
                else:
                    assert l[t] - torch.cat([l[:t], l[t + 1:]]).max() >= 100
        assert seen >= set(rc.ce_edges(V)) or rows < 3, (V, seen)
        assert {k for v in rc.CE_VARIANTS for k in rc.ce_inputs(rows, V, v).kinds} == set(rc.CE_KINDS)
    for D in rc.ROPE_D:
        p = rc.rope_inputs(D)
        assert set(p.cos.unique().tolist()) | set(p.sin.unique().tolist()) == {-1.0, -0.5, 0.0, 0.5, 1.0}
        assert ((p.cos == 0) != (p.sin == 0)).all()
        want = rc.rope_ref(p.qkv, p.cos, p.sin, rc.ROPE_ROT, D, False)
        B, S, W = p.qkv.shape
        x = p.qkv.float().view(B, S, rc.ROPE_NH, D)
        plain = torch.cat([ref.apply_rope(x[:, :, :rc.ROPE_ROT], p.cos, p.sin), x[:, :, rc.ROPE_ROT:]], 2).reshape(B, S, W)
        assert torch.equal(plain.to(BF16), want)  # exact in fp32 too: a signed permutation or a halving
        assert sorted(want.abs().flatten().tolist()) != sorted(p.qkv.abs().flatten().tolist())  # (halved somewhere)
        back = rc.rope_ref(want, p.cos * 2, p.sin * 2, rc.ROPE_ROT, D, True)  # the inverse of a halving rotation
        unit = (p.cos.abs() + p.sin.abs() == 1)[torch.arange(B * S) % S]
        full = torch.ones(B * S, rc.ROPE_NH, 2, D // 2, dtype=torch.bool)
        full[:, :rc.ROPE_ROT] = unit[:, None, None, :]
        full = full.reshape(B, S, W)
        assert torch.equal(rc.rope_ref(want, p.cos, p.sin, rc.ROPE_ROT, D, True)[full], p.qkv[full]) and back.shape == want.shape


def test_judge_reports_where():
    i = rc.norm_inputs(1027, 520)
    r = rc.norm_ref(i.x, i.w)
    y = r.y.to(F32).to(BF16)
    c = rc.norm_c(520, 64)[1]
    assert rc.assert_judged(y, r.y, r.y, c, bf16=True, wg=rc.layout("wave_row"), what="y") <= 0.51
    y[1026, 519] = y[1026, 519] * 1.02
    y[7, 64] = float("nan")
    with pytest.raises(AssertionError) as e:
        rc.assert_judged(y, r.y, r.y, c, bf16=True, wg=rc.layout("wave_row"), what="poke")
    msg = str(e.value)
    print(msg)
    assert "poke: 2 of 534040 elements over the bound" in msg and "rows [7, 1026]" in msg and "chunks (col // 8) [8, 64]" in msg
    assert "lane (chunk % 64) [0, 8], wave pass (chunk // 64) [0, 1]" in msg and "block pass (chunk // 256) [0]" in msg
    assert "workgroups [1, 256]" in msg and len(msg) < 2000
    y[:] = float("nan")
    with pytest.raises(AssertionError) as e:
        rc.assert_same(y, r.y.to(F32).to(BF16), wg=rc.layout("wave_row"), what="all")
    assert len(str(e.value)) < 2000


def _norm_case(rows, D, scaled=True):
    i = rc.norm_inputs(rows, D, "cpu", scaled)
    return i, rc.norm_ref(i.x, i.w)


def _bwd_case(rows, D, scaled=True):
    i = rc.bwd_inputs(rows, D, "cpu", scaled)
    return i, rc.bwd_ref(i.dy, i.h, i.w, i.rstd)


def _rejected(fn) -> bool:
    try:
        fn()
    except AssertionError as e:
        print("  judge:", str(e).splitlines()[0])
        return True
    return False


@pytest.mark.parametrize("kind", ["neighbour_rstd", "stale_weight"])
def test_norm_fwd_defects_are_caught(kind):
    i, r = _norm_case(1027, 520)
    y = rc.norm_defect(kind, i, r)
    print(f"{kind}: old _close(y, 2e-2, 1e-2) passes: {rc.old_close(y, r.y, 2e-2, 1e-2)}")
    assert _rejected(lambda: rc.assert_judged(y, r.y, r.y, rc.norm_c(520, 64)[1], bf16=True, wg=rc.layout("wave_row"), what=kind))


@pytest.mark.parametrize("kind", ["dw_chunk_missing", "partial_missing", "partial_twice", "projection_scaled"])
def test_norm_bwd_defects_are_caught(kind):
    rows, D = 1500, 520
    i, r = _bwd_case(rows, D)
    dx, dw = rc.bwd_defect(kind, i, r)
    c_dx, c_dw = rc.bwd_c(rows, D)
    print(f"{kind}: old _close passes: dx {rc.old_close(dx, r.dx, 3e-2, 1e-2)}, dw {rc.old_close(dw, r.dw, 0.5, 2e-2)}")
    on_dx = kind == "projection_scaled"
    assert _rejected(lambda: rc.assert_judged(dx, r.dx, r.T_dx, c_dx, bf16=True, wg=rc.layout("grid_rows", grid=1024), what=kind)) == on_dx
    assert _rejected(lambda: rc.assert_judged(dw, r.dw, r.T_dw, c_dw, bf16=False, wg=rc.layout("colsum"), what=kind)) != on_dx


@pytest.mark.parametrize("kind", ["pair_next", "pos_is_row", "inverse_sign", "v_heads_rotated"])
def test_rope_defects_are_caught(kind):
    """With a different value in every element and tables that move or halve, nothing cancels: each
    wrong pairing, position, sign or head boundary changes stored bits.  The old bound's verdict on the
    same outputs is printed."""
    for D in rc.ROPE_D:
        p = rc.rope_inputs(D)
        want = rc.rope_ref(p.qkv, p.cos, p.sin, rc.ROPE_ROT, D, False)
        kw = dict(pair_next=kind == "pair_next", pos_is_row=kind == "pos_is_row")
        got = rc.rope_ref(p.qkv, p.cos, p.sin, rc.ROPE_ROT + (kind == "v_heads_rotated"), D, kind == "inverse_sign", **kw)
        print(f"{kind} D={D}: old _close(2e-2, 1e-2) passes: {rc.old_close(got, want, 2e-2, 1e-2)}")
        assert _rejected(lambda: rc.assert_same(got, want, wg=rc.layout("flat", nch=rc.ROPE_NH * D // 16), what=kind))


def test_softmax_gradient_without_its_onehot_is_caught():
    rows, V = 3, 2056
    for variant in rc.CE_VARIANTS:
        i = rc.ce_inputs(rows, V, variant)
        lse32 = rc.ce_ref(i.logits, i.target).lse.to(F32)
        r = rc.ce_ref(i.logits, i.target, lse32, 1.0 / 256)
        row = next(k for k, t in enumerate(i.target.tolist()) if t % 8 in (0, 7))  # a target on a chunk boundary
        g = r.grad.clone()
        g[row, i.target[row]] += 1.0 / 256
        g = g.to(F32).to(BF16)
        print(f"variant {variant} row {row} target {int(i.target[row])}: old _close(2e-4, 2e-2) passes: "
              f"{rc.old_close(g, r.grad, 2e-4, 2e-2)}")
        assert _rejected(lambda: rc.assert_judged(g, r.grad, r.T_grad, rc.CE_BWD_C, bf16=True, wg=rc.layout("block_row"), what="onehot"))


def test_adamw_tail_left_out_is_caught():
    n = 6149
    i = rc.adamw_inputs(n)
    sl = slice(rc.ADAMW_PAD, rc.ADAMW_PAD + n)
    r = rc.adamw_ref(i.master[sl], i.m[sl], i.v[sl], i.grad[sl], weight_decay=0.1, step=1, **rc.ADAMW_HYPER)
    got = r.master.to(F32)
    got[n // 8 * 8 + 3] = i.master[sl][n // 8 * 8 + 3]  # a tail element a capped grid did not reach
    print(f"old _close(master, 1e-5, 1e-5) passes: {rc.old_close(got, r.master, 1e-5, 1e-5)}")
    assert _rejected(lambda: rc.assert_judged(got, r.master, r.T_master, rc.ADAMW_C["master"], bf16=False,
                                              wg=rc.layout("flat", nch=1 << 40, grid=1), what="tail"))


def test_fp8_scale_over_the_first_pass_only_is_caught():
    """The row scale taken over the first 2048 columns: row 0's largest element sits in the last chunk.
    (The older tests compare the fused e4m3 norm with the bf16 norm kernel plus the row quantiser: that
    verdict is printed with the fp32 implementation standing in for the unfused pair.)"""
    i = rc.norm_inputs(37, 4104, "cpu", True, True)
    r = rc.norm_ref(i.x, i.w)
    good = CPU.norm_fp8(i.x, None, i.w, rc.EPS, None, None)
    rc.fp8_verdict(*good, r, False, rc.layout("block_row"), "good")
    q, s = rc.fp8_defect_first_pass_scale(i, r)
    # the older check (test_gpu_rms_norm_fp8_matches_unfused): scales equal to 1e-6, under 1e-3 of the bytes differ
    old = bool(((s - good[2]).abs() <= 1e-6 * good[2].abs()).all()) and (q != good[1]).float().mean().item() < 1e-3
    print(f"first-pass scale: the older fused-against-unfused check, given a right unfused kernel, passes: {old}")
    assert _rejected(lambda: rc.fp8_verdict(None, q, s, r, False, rc.layout("block_row"), "first-pass scale"))


@pytest.mark.parametrize("kind", ["neighbour_rstd", "dw_chunk_missing"])
def test_old_bound_misses_these(kind):
    """On inputs like the older tests' (i.i.d. N(0, 1), w = 1 + 0.1 N(0, 1), 4096 x 4096) the
    one-bound-per-tensor ``_close`` of ``test_rms_norm`` accepts these defects; the judge does not.  (A
    whole row missing from dw it catches, through the tail of a product of two normals among 4096
    columns: ``test_norm_bwd_defects_are_caught`` prints that verdict.)"""
    rows, D = 4096, 4096
    if kind == "neighbour_rstd":
        i, r = _norm_case(rows, D, False)
        step = (r.rstd[1:] / r.rstd[:-1] - 1).abs()
        row = int((step - step.median()).abs().argmin())  # a row as far from its neighbour's rstd as rows typically are
        y = rc.norm_defect(kind, i, r, row)
        print(f"row {row}: rstd {r.rstd[row].item():.6f}, the next row's {r.rstd[row + 1].item():.6f}")
        err = (y.double() - r.y).abs().max().item()
        print(f"{kind}: max error {err:.3g}, old tolerance {2e-2 + 1e-2 * r.y.abs().max().item():.3g}")
        assert rc.old_close(y, r.y, 2e-2, 1e-2)
        assert _rejected(lambda: rc.assert_judged(y, r.y, r.y, rc.norm_c(D, 256)[1], bf16=True, wg=rc.layout("block_row"), what=kind))
        return
    i, r = _bwd_case(rows, D, False)
    _, dw = rc.bwd_defect(kind, i, r)
    err = (dw.double() - r.dw).abs().max().item()
    print(f"{kind}: max error {err:.3g}, old tolerance {0.5 + 2e-2 * r.dw.abs().max().item():.3g}")
    assert rc.old_close(dw, r.dw, 0.5, 2e-2)
    assert _rejected(lambda: rc.assert_judged(dw, r.dw, r.T_dw, rc.bwd_c(rows, D)[1], bf16=False, wg=rc.layout("colsum"), what=kind))


# ==================================================================================================
# With a GPU
# ==================================================================================================
class HipImpl:
    """The HIP bindings behind the interface of ``rowwise_cases.Fp32Impl``, each call behind the
    stale-memory guard."""

    def __init__(self, device):
        self.C = _ext.require()
        self.device = device

    def _poison(self, *specs):
        """Allocate and free NaN-filled (bytes: 0x7f, e4m3's NaN) tensors of the outputs' sizes: the caching
        allocator is then likely to hand these blocks to the call's ``torch::empty`` outputs.  A
        heuristic -- every kernel is also judged element by element."""
        held = [torch.full(shape, 0x7F if dt == torch.uint8 else float("nan"), dtype=dt, device=self.device)
                for shape, dt in specs]
        del held

    @staticmethod
    def _clean(*outs):
        for o in outs:
            if o is None:
                continue
            bad = (o == 0x7F) if o.dtype == torch.uint8 else torch.isnan(o)
            assert not bad.any(), f"{int(bad.sum())} output elements were not written (NaN), first {bad.nonzero()[:4].tolist()}"
        return outs

    def norm_fwd(self, x, delta, w, eps):
        self._poison((x.shape, BF16), (x.shape, BF16), ((x.shape[0],), F32))
        if delta is None:
            return (None, *self._clean(*self.C.rms_norm_fwd(x, w, eps)))
        return self._clean(*self.C.add_rms_norm_fwd(x, delta, w, eps))

    def norm_fp8(self, x, delta, w, eps, dr, dc):
        self._poison((x.shape, BF16), (x.shape, torch.uint8), ((x.shape[0],), F32))
        h, q, qs = self.C.rms_norm_fp8(x, delta, w, eps, dr, dc)
        return self._clean(h if delta is not None else None, q, qs)

    def norm_bwd(self, dy, h, w, rstd, dres, dw_out, accumulate, eps):
        rows, D = h.shape
        self._poison((h.shape, BF16), ((rc.bwd_grid(rows), D), F32), ((D,), F32))
        dx, dw = self.C.rms_norm_bwd(dy, h, w, rstd, dres, dw_out, accumulate)
        return self._clean(dx, dw if dw_out is None else dw_out)

    def swiglu_fwd(self, gu):
        self._poison(((gu.shape[0], gu.shape[1] // 2), BF16))
        return self._clean(self.C.swiglu_fwd(gu))[0]

    def swiglu_bwd(self, da, gu):
        self._poison((gu.shape, BF16))
        return self._clean(self.C.swiglu_bwd(da, gu))[0]

    def ce_fwd(self, logits, target):
        self._poison(((logits.shape[0],), F32), ((logits.shape[0],), F32))
        return self._clean(*self.C.cross_entropy_fwd(logits, target))

    def ce_bwd(self, logits, target, lse, scale, inplace):
        self._poison((logits.shape, BF16))
        sc = torch.tensor([scale], dtype=F32, device=self.device)
        return self._clean(self.C.cross_entropy_bwd(logits, target, lse, sc, inplace))[0]

    def adamw(self, param, grad, master, m, v, *, max_blocks, **kw):
        ops.adamw_(param, grad, master, m, v, max_blocks=max_blocks, **kw)

    def embedding_bwd(self, dy, ids, grad, accumulate):
        sorted_ids, order = torch.sort(ids, stable=True)
        self.C.embedding_bwd(dy, sorted_ids, order, grad, accumulate)


@pytest.fixture
def hip(gpu):
    return HipImpl(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("add", [False, True])
@pytest.mark.parametrize("D", rc.NORM_D)
def test_rms_norm_fwd_judged(gpu, hip, D, add):
    """y, rstd (and h, bit for bit) at rows 1, 3, 1024 (block-per-row) and 1025, 1027 (wave-per-row)."""
    fr = {}
    for rows in rc.NORM_ROWS:
        _merge(fr, f"{rows}x{D}", rc.check_norm_fwd(hip, rows, D, add, str(gpu)))
    _show(fr)


@pytest.mark.gpu
def test_rms_norm_rejects_unsupported_widths(gpu):
    """D = 8200 (more than 16 chunks per lane) and D % 8 != 0 raise before any launch: the launchers return
    ``hipErrorInvalidValue`` ahead of their ``<<<>>>``."""
    C = _ext.require()
    for rows in (3, 1025):
        for D in (8200, 12):
            x, w = torch.ones(rows, D, device=gpu, dtype=BF16), torch.ones(D, device=gpu, dtype=BF16)
            with pytest.raises(RuntimeError):
                C.rms_norm_fwd(x, w, rc.EPS)
            with pytest.raises(RuntimeError):
                C.add_rms_norm_fwd(x, x, w, rc.EPS)
            with pytest.raises(RuntimeError):
                C.rms_norm_fp8(x, None, w, rc.EPS, None, None)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("form", rc.FP8_FORMS)
@pytest.mark.parametrize("D", rc.FP8_D)
def test_rms_norm_fp8_judged(gpu, hip, D, form):
    fr = {}
    for rows in rc.FP8_ROWS:
        _merge(fr, f"{rows}x{D}", rc.check_norm_fp8(hip, rows, D, form, str(gpu)))
    _show(fr)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,D", rc.BWD_CASES)
def test_rms_norm_bwd_judged(gpu, hip, rows, D):
    """dx and dw with and without dres; fp32 dw, bf16 dw_out stored and accumulated."""
    fr = {}
    for with_dres, form in rc.BWD_FORMS:
        _merge(fr, f"dres={with_dres} {form}", rc.check_norm_bwd(hip, rows, D, with_dres, form, str(gpu)))
    _show(fr)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,D", rc.BWD_EXACT)
def test_rms_norm_bwd_exact(gpu, hip, rows, D):
    """Small integers and rstd = 2^-2: dx, the fp32 dw and the bf16 dw_out (stored, accumulated) bit for bit."""
    rc.check_norm_bwd_exact(hip, rows, D, str(gpu))


@pytest.mark.gpu
@pytest.mark.parametrize("rows,Fh", rc.SWIGLU_CASES)
def test_swiglu_judged(gpu, hip, rows, Fh):
    _show(rc.check_swiglu(hip, rows, Fh, str(gpu)))


@pytest.mark.gpu
@pytest.mark.parametrize("T,Fh", rc.SWIGLU_T_CASES)
def test_swiglu_transposing_forms_exact(gpu, hip, T, Fh):
    """a and dgu of the transposing kernels equal the plain kernels' (judged above) bit for bit, and the
    transposed outputs are their ``.t()``."""
    C = hip.C
    g = torch.Generator().manual_seed(T * 1000 + Fh)
    gu = (torch.randn(T, 2 * Fh, generator=g) * 3).to(BF16).to(gpu)
    da = torch.randn(T, Fh, generator=g).to(BF16).to(gpu)
    wg = lambda r, ch: (r // 128) * (Fh // 64) + ch // 8  # noqa: E731  (128 x 64 tiles)
    hip._poison(((T, Fh), BF16), ((Fh, T), BF16))
    a, aT = hip._clean(*C.swiglu_fwd_t(gu))
    rc.assert_same(a, C.swiglu_fwd(gu), wg=wg, what="swiglu_fwd_t a")
    rc.assert_same(aT, a.t().contiguous(), wg=wg, what="swiglu_fwd_t aT")
    hip._poison(((T, 2 * Fh), BF16), ((2 * Fh, T), BF16))
    dgu, dguT = hip._clean(*C.swiglu_bwd_t(da, gu))
    rc.assert_same(dgu, C.swiglu_bwd(da, gu), wg=wg, what="swiglu_bwd_t dgu")
    rc.assert_same(dguT, dgu.t().contiguous(), wg=wg, what="swiglu_bwd_t dguT")


@pytest.mark.gpu
@pytest.mark.parametrize("R,Cc", rc.TRANSPOSE_CASES)
def test_transpose2d_exact(gpu, hip, R, Cc):
    # every finite non-zero normal bf16 value in turn (65024 of them: a value comes back 338 rows and 128
    # columns on, never inside a tile, a row or a column)
    k = torch.arange(R * Cc, dtype=torch.int32) % 65024
    bits = 0x0080 + k % 0x7F00 + (k // 0x7F00) * 0x8000
    x = torch.where(bits >= 0x8000, bits - 0x10000, bits).to(torch.int16).view(BF16).reshape(R, Cc).to(gpu)
    assert torch.isfinite(x.float()).all() and len(set(x[:128, :64].flatten().tolist())) == 128 * 64
    hip._poison(((Cc, R), BF16))
    out, = hip._clean(hip.C.transpose2d(x))
    rc.assert_same(out, x.t().contiguous(), wg=lambda r, ch: r // 64 + (ch // 16) * (Cc // 64), what=f"transpose2d {R}x{Cc}")


@pytest.mark.gpu
@pytest.mark.parametrize("D", rc.ROPE_D)
def test_rope_qkv_exact(gpu, hip, D):
    """Signed permutations and halvings of all-different values: pairs (i, i + D/2), position row % S
    (B = 3), the v head untouched, the inverse's sign; a table longer than S."""
    p = rc.rope_inputs(D, str(gpu))
    wg = rc.layout("flat", nch=rc.ROPE_NH * D // 16)
    for inverse in (False, True):
        hip._poison((p.qkv.shape, BF16))
        out, = hip._clean(hip.C.rope_qkv(p.qkv, p.cos, p.sin, rc.ROPE_ROT, D, inverse))
        want = rc.rope_ref(p.qkv, p.cos, p.sin, rc.ROPE_ROT, D, inverse)
        rc.assert_same(out.reshape(-1, out.shape[-1]), want.reshape(-1, out.shape[-1]), wg=wg, what=f"rope_qkv D={D} inverse={inverse}")
        assert torch.equal(out[..., rc.ROPE_ROT * D:], p.qkv[..., rc.ROPE_ROT * D:])


@pytest.mark.gpu
@pytest.mark.parametrize("rows,V", rc.CE_CASES)
def test_cross_entropy_judged(gpu, hip, rows, V):
    """Per-row loss and lse, every gradient element (out of place at scale 1, in place at 0.37)."""
    fr = {}
    for variant in rc.CE_VARIANTS:
        _merge(fr, f"{rows}x{V}", rc.check_ce(hip, rows, V, variant, str(gpu)))
    _show(fr)


@pytest.mark.gpu
@pytest.mark.parametrize("ignored", ["none", "one", "all_but_one", "all"])
def test_cross_entropy_ignore_index(gpu, ignored):
    """A target of -100 as in ``reference.cross_entropy``: the mean runs over the counted rows and an
    ignored row's gradient is zero.  All rows ignored: loss 0 and zero gradients (the reference gives NaN)."""
    rows, V = 5, 2056
    g = torch.Generator().manual_seed(rows * V)
    logits = (torch.randn(rows, V, generator=g) * 3).to(BF16).to(gpu)
    target = torch.tensor([0, 7, 8, V - 8, V - 1], device=gpu)
    keep = {"none": [0, 1, 2, 3, 4], "one": [0, 1, 3, 4], "all_but_one": [2], "all": []}[ignored]
    mask = torch.ones(rows, dtype=torch.bool, device=gpu)
    mask[keep] = False
    target = torch.where(mask, torch.full_like(target, -100), target)
    count = max(1, len(keep))
    x = logits.clone().requires_grad_()
    loss = ops.cross_entropy(x, target)
    loss.backward()
    grad = x.grad
    r = rc.ce_ref(logits, target, None, 1.0 / count)
    assert torch.equal(r.live, ~mask)
    want = r.loss.sum().item() / count
    c = rc.ce_fwd_c(V)
    bound = (c + 3) * rc.U * (r.T_loss * r.live).sum().item() / count  # + the sum over rows and the division
    print(f"{ignored}: loss {loss.item():.8g}, fp64 {want:.8g}, bound {bound:.3g}")
    assert abs(loss.item() - want) <= bound
    assert (grad[mask] == 0).all(), "an ignored row's gradient must be zero"
    T = (r.T_grad + (abs(1.0 / count) * torch.exp(logits.double() - r.lse[:, None])) * r.T_lse[:, None]) * r.live[:, None]
    rc.assert_judged(grad, r.grad, T, min(rc.C_CAP, c + rc.CE_BWD_C + 2), bf16=True, wg=rc.layout("block_row"),
                     what=f"cross_entropy gradient, ignored: {ignored}")
    if keep:
        xr = logits.float().requires_grad_()
        lref = ref.cross_entropy(xr, target)
        lref.backward()
        assert abs(loss.item() - lref.item()) <= 2 * bound + rc.U * abs(want)
        assert (xr.grad[mask] == 0).all()
    else:
        assert loss.item() == 0.0 and (grad == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("max_blocks", rc.ADAMW_BLOCKS)
@pytest.mark.parametrize("n", rc.ADAMW_N)
def test_adamw_judged(gpu, hip, n, max_blocks):
    """Three steps each at weight decay 0 and 0.1, on the middle of a larger flat buffer: master, m and v
    judged, param = bf16(master) bit for bit, nothing outside the slice touched."""
    fr = {}
    for wd in rc.ADAMW_WD:
        _merge(fr, f"wd={wd}", rc.check_adamw(hip, n, max_blocks, wd, str(gpu)))
    _show(fr)


@pytest.mark.gpu
@pytest.mark.parametrize("V,D", rc.EMBED_CASES)
def test_embedding_bwd_exact(gpu, hip, V, D):
    rc.check_embedding(hip, V, D, str(gpu))
