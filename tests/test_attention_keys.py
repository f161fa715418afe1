"""Attention kernels against fp64 references on inputs in which every key is individually
observable, judged per row (``tests/attn_cases.py`` has the construction, the metric and the
rounding model the thresholds come from).

The older attention tests feed i.i.d. normal q/k/v and compare with one global bound: the softmax
is diffuse, one key carries 1/n of a row, and an off-by-one in a mask, a context length or a page
walk stays under the bound (``test_old_bound_misses_one_key`` keeps that visible).  Here a lost or
leaked key moves an O(1) part of some row.

Without a GPU: the builders' invariants for every case the GPU tests use, the sensitivity of the
metric to each simulated defect (>= 0.25 on some row, 5 x the threshold cap), and the CPU paths.
With one: flash attention forward and gradients, paged decode under every split plan, paged
prefill; bf16 and e4m3 caches; GQA groups 1, 2, 5, 7, 8, 16.

Flash attention runs every case twice.  With V random in bf16 the forward is judged.  The
gradients are judged with V on a 1/8 grid, which makes the O of a needle row exact in bf16: the
backward takes delta = dO . O from the bf16 O, and with a rounded O that one rounding is an absolute
error of 1.4e-3 of the largest dQ row on *every* row -- the per-row metric, floored at 1e-3 of the
largest row, reads it as > 1 on the rows whose true dQ happens to be small (the rounding model
itself: 1.38 for dQ, 0.07 for dK at S=512, H=8, KV=1), so no threshold under the cap could hold.
With an exact O what is left is relative to each term (dS, the bf16 partials and outputs); and each
dO row carries the sign that keeps the parallel dK terms of rows with the same two targets from
cancelling (``attn_cases.flash_case``), so that a dK row is not small beside its own terms either.
"""

import pytest
import torch

from tests import attn_cases as ac
from tests.attn_cases import BF16, D, DETECT, E4M3, PAGE
from dstack_amd import ops
from dstack_amd.ops import reference as ref
from dstack_amd.ops import serving as sops

FLASH = [(S, H, KV, causal) for S, H, KV in ac.FLASH_SHAPES for causal in (True, False)]
CACHES = [BF16, E4M3]


def _report(name, errs, thrs):
    print(f"{name}: " + ", ".join(f"{k} {errs[k]:.3g} (<= {thrs[k]:.3g})" for k in errs))
    bad = {k: (errs[k], thrs[k]) for k in errs if not errs[k] <= thrs[k]}
    assert not bad, f"{name}: worst row error over threshold: {bad}"


# ==================================================================================================
# Builder invariants (no GPU)
# ==================================================================================================
def _mass(p, targets):
    """Sum of ``p`` [..., N] over ``targets`` [..., m] (-1 = none)."""
    return (p.gather(-1, targets.clamp_min(0)) * (targets >= 0)).sum(-1)


@pytest.mark.parametrize("S,H,KV,causal", FLASH)
def test_flash_case_invariants(S, H, KV, causal):
    c = ac.flash_case(S, H, KV, causal)  # (asserts the bf16 round trip itself)
    assert torch.equal(ac.flash_case(S, H, KV, causal, vgrid=True).targets, c.targets)  # (p does not depend on V)
    p = ac.flash_f64(c, grads=False, want_p=True)["p"]
    assert _mass(p, c.targets).min().item() >= 1 - 1e-6
    B = c.B
    # every visible (128-query tile, 64-key tile) pair holds a target, in each batch
    hit = torch.zeros(B, S // 128, S // 64, dtype=torch.bool)
    qt = (torch.arange(S) // 128).view(1, 1, S, 1).expand_as(c.targets)
    bb = torch.arange(B).view(B, 1, 1, 1).expand_as(c.targets)
    ok = c.targets >= 0
    hit[bb[ok], qt[ok], c.targets[ok] // 64] = True
    vis = torch.ones(S // 128, S // 64, dtype=torch.bool)
    if causal:
        vis = torch.arange(S // 64).view(1, -1) <= 2 * torch.arange(S // 128).view(-1, 1) + 1
    assert hit[:, vis].all() and not hit[:, ~vis].any()
    if not causal:
        return
    # the trap head: every row but the last few has a trap key, one position or one tile ahead, and
    # with the mask removed the trap takes at least a third of its row
    trap, i = c.trap, torch.arange(S)
    assert ((trap < 0).sum(1) <= 2).all() and (trap[trap >= 0] > i.expand_as(trap)[trap >= 0]).all()
    edge = i[: S - 1][i[: S - 1] % 64 == 63]
    assert ((trap[:, edge] == edge + 1).sum(0) >= 1).all()  # every tile edge: i + 1 in some batch
    first = i[: S - 64][i[: S - 64] % 64 == 0]
    assert ((trap[:, first] == first + 64).sum(0) >= 1).all()  # and the next tile's first key
    full = torch.ones(S, S, dtype=torch.bool)
    pt = ac.flash_f64(c, vis=full, grads=False, want_p=True)["p"][:, c.trap_head]  # [B, S, S]
    leak = pt.gather(-1, trap.clamp_min(0).unsqueeze(-1)).squeeze(-1)
    assert (leak[trap >= 0] >= 1 / 3).all()


@pytest.mark.parametrize("cache_dtype", CACHES, ids=["bf16", "e4m3"])
@pytest.mark.parametrize("H,KVH", ac.DECODE_HEADS)
def test_decode_case_invariants(H, KVH, cache_dtype):
    c = ac.decode_case(H, KVH, cache_dtype)  # (asserts the exact round trip of q and the caches)
    assert set(ac.decode_contexts()) >= {1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512}
    _, ps = ac.decode_f64(c, want_p=True)
    for b in range(c.B):
        ctx, n = int(c.ctx[b]), c.npg[b]
        t = c.targets[b]
        assert _mass(ps[b], t).min().item() >= 1 - 1e-6
        assert set((t[t >= 0] // PAGE).tolist()) == set(range(n))  # every page, so every split of every plan
        assert (t[:, 0] == ctx - 1).all() and (t[0, 1:] == -1).all()
        # the slot after the context, in the last page or the poison page, takes half of head 0 when seen
        if ctx < c.W * PAGE:
            _, pl = ac.decode_f64(c, ctx=c.ctx + 1, want_p=True, seqs=[b])
            assert pl[0][0, ctx].item() >= 1 / 3
    tb = c.tables
    rows = [tb[b, : c.npg[b]].tolist() for b in range(c.B)]
    assert any(r != sorted(r) for r in rows)                          # not monotone
    firsts = [r[0] for r in rows]
    assert len(firsts) - len(set(firsts)) == 1                        # two sequences share a first page
    flat = [p for r in rows for p in r[1:]] + list(set(firsts))
    assert len(flat) == len(set(flat))


@pytest.mark.parametrize("cache_dtype", CACHES, ids=["bf16", "e4m3"])
@pytest.mark.parametrize("H,KVH", ac.PREFILL_HEADS)
def test_prefill_case_invariants(H, KVH, cache_dtype):
    c = ac.prefill_case(H, KVH, cache_dtype)
    _, ps = ac.prefill_f64(c, want_p=True)
    # each row also sees its trap key where that is a real entry (a later token of the segment),
    # the last row of a segment the slot after the segment's end
    extra = torch.full((c.rows,), -1, dtype=torch.long)
    for s, (start, n) in enumerate(c.segs):
        r = int(c.offsets[s]) + torch.arange(n)
        extra[r] = torch.where(c.trap[r] < start + n, c.trap[r], extra[r])
        extra[r[-1]] = start + n
    _, pl = ac.prefill_f64(c, extra=extra, want_p=True)
    for s, (start, n) in enumerate(c.segs):
        off, end = int(c.offsets[s]), start + n
        t = c.targets[off : off + n].transpose(0, 1)  # [H, n, m]
        assert _mass(ps[s], t).min().item() >= 1 - 1e-6
        # every (48-token tile, page it sees) pair holds a target
        pos = start + torch.arange(n)
        for tile in range(0, n, ac.PREFILL_TILE):
            tt = t[:, tile : tile + ac.PREFILL_TILE]
            assert set((tt[tt >= 0] // PAGE).tolist()) == set(range(int(pos[tile : tile + ac.PREFILL_TILE].max()) // PAGE + 1))
        # trap keys that are real cache entries (later tokens of the segment), and for the last
        # row the first slot after the segment: each takes >= 1/3 of the trap head's row when seen
        trap = c.trap[off : off + n]
        real = trap < end
        leak = pl[s][c.trap_head].gather(-1, trap.clamp_max(c.W * PAGE - 1).unsqueeze(-1)).squeeze(-1)
        assert (leak[real] >= 1 / 3).all()
        assert (pl[s][:, n - 1, end] >= 1 / 3 - 1e-9).all()  # (every head of the last row: <= 2 other targets)
    assert c.listed.sum().item() == sum(n for _, n in c.segs) and not c.listed.all()


# ==================================================================================================
# Sensitivity: each simulated defect, applied to the reference, reaches DETECT on some row
# ==================================================================================================
SENS = (512, 8, 1, True)


def _flash_err(c, vis, names=("o",)):
    good, bad = _flash_good(c), ac.flash_f64(c, vis=vis, grads=len(names) > 1)
    return {n: ac.rowerr(bad[n], good[n]) for n in names}


_GOOD = {}


def _flash_good(c):
    if id(c) not in _GOOD:
        _GOOD[id(c)] = ac.flash_f64(c)
    return _GOOD[id(c)]


def test_metric_sees_flash_defects():
    c = ac.flash_case(*SENS)
    S = c.S
    i = torch.arange(S)
    causal = ac.causal_vis(S)
    assert _flash_err(c, causal & ~torch.eye(S, dtype=torch.bool))["o"] >= DETECT      # the diagonal dropped
    leak = causal.clone()
    edge = i[:-1][i[:-1] % 128 == 127]
    leak[edge, edge + 1] = True                                                        # key i + 1 on tile-edge rows
    assert _flash_err(c, leak)["o"] >= DETECT
    nxt = causal.clone()
    nxt[i[:-64], (i[:-64] // 64 + 1) * 64] = True                                      # the next tile's first key
    assert _flash_err(c, nxt)["o"] >= DETECT
    for qt in range(S // 128):                                                         # any one visible tile dropped
        for kt in range(2 * qt + 2):
            vis = causal.clone()
            vis[128 * qt : 128 * qt + 128, 64 * kt : 64 * kt + 64] = False
            assert _flash_err(c, vis)["o"] >= DETECT, (qt, kt)
    for S2, H2, KV2 in ((384, 6, 3),):                                                 # and not causal
        c2 = ac.flash_case(S2, H2, KV2, False)
        for qt in range(S2 // 128):
            for kt in range(S2 // 64):
                vis = torch.ones(S2, S2, dtype=torch.bool)
                vis[128 * qt : 128 * qt + 128, 64 * kt : 64 * kt + 64] = False
                assert _flash_err(c2, vis)["o"] >= DETECT, (qt, kt)


@pytest.mark.parametrize("qt,kt", [(1, 0), (3, 5), (2, 5)])
def test_metric_sees_dropped_tile_in_gradients(qt, kt):
    c = ac.flash_case(*SENS, vgrid=True)
    vis = ac.causal_vis(c.S)
    vis[128 * qt : 128 * qt + 128, 64 * kt : 64 * kt + 64] = False
    errs = _flash_err(c, vis, ("dq", "dk", "dv"))
    assert min(errs.values()) >= DETECT, errs


def _decode_err(c, **kw):
    if ("decode", id(c)) not in _GOOD:
        _GOOD["decode", id(c)] = ac.heads(ac.decode_f64(c), c.H)
    good = _GOOD["decode", id(c)]
    if kw.get("seqs") is not None:  # a defect in these sequences only: the other rows are not computed again
        keep = torch.zeros(c.B, c.H, dtype=torch.bool)
        keep[kw["seqs"]] = True
        good = good * keep.view(-1, 1)
    return ac.rowerr(ac.heads(ac.decode_f64(c, **kw), c.H), good)


@pytest.mark.parametrize("cache_dtype", CACHES, ids=["bf16", "e4m3"])
@pytest.mark.parametrize("H,KVH", [(4, 2), (28, 4)])
def test_metric_sees_decode_defects(H, KVH, cache_dtype):
    c = ac.decode_case(H, KVH, cache_dtype)
    top = c.W * PAGE
    assert _decode_err(c, ctx=c.ctx - 1) >= DETECT
    assert _decode_err(c, ctx=(c.ctx + 1).clamp_max(top)) >= DETECT
    assert _decode_err(c, ctx=(c.ctx + PAGE - 1) // PAGE * PAGE) >= DETECT             # rounded up to the page
    for b in range(c.B):                                                               # each of them alone, too
        one = (torch.arange(c.B) == b).int()
        assert _decode_err(c, ctx=c.ctx - one, seqs=[b]) >= DETECT
        if int(c.ctx[b]) < top:
            assert _decode_err(c, ctx=c.ctx + one, seqs=[b]) >= DETECT
    for nsplit, pps in ac.DECODE_PLANS.values():                                       # a split's last page skipped
        for s in range(nsplit if nsplit > 1 else 0):
            assert _decode_err(c, drop_pages=(s * pps + pps - 1,)) >= DETECT
    for b in range(c.B):
        n = c.npg[b]
        if n >= 2 and int(c.ctx[b]) % PAGE:                                            # two entries swapped
            t = c.tables.clone()
            t[b, 0], t[b, n - 1] = c.tables[b, n - 1], c.tables[b, 0]
            assert _decode_err(c, tables=t, seqs=[b]) >= DETECT
        for p in range(n):                                                             # one wrong page id
            t = c.tables.clone()
            t[b, p] = c.tables[(b + 1) % c.B, min(p, c.npg[(b + 1) % c.B] - 1)]
            if t[b, p] != c.tables[b, p]:
                assert _decode_err(c, tables=t, seqs=[b]) >= DETECT, (b, p)


@pytest.mark.parametrize("cache_dtype", CACHES, ids=["bf16", "e4m3"])
def test_metric_sees_prefill_defects(cache_dtype):
    c = ac.prefill_case(5, 1, cache_dtype)
    good = ac.heads(ac.prefill_f64(c), c.H)
    assert ac.rowerr(ac.heads(ac.prefill_f64(c, shift=-1), c.H), good) >= DETECT       # key < limit
    full, bad = ac.prefill_f64(c), ac.prefill_f64(c, shift=1)                          # key <= limit + 1
    assert ac.rowerr(ac.heads(bad, c.H), good) >= DETECT
    for s, (start, n) in enumerate(c.segs):  # ... in every segment: a later token, or the slot after its end
        r = slice(int(c.offsets[s]), int(c.offsets[s]) + n)
        assert ac.rowerr(ac.heads(bad[r], c.H), ac.heads(full[r], c.H)) >= DETECT, (start, n)
    s = next(i for i, (st, n) in enumerate(c.segs) if c.npg[i] >= 2 and (st + n) % PAGE)
    t = c.tables.clone()
    t[s, 0], t[s, c.npg[s] - 1] = c.tables[s, c.npg[s] - 1], c.tables[s, 0]
    assert ac.rowerr(ac.heads(ac.prefill_f64(c, tables=t), c.H), good) >= DETECT       # two entries swapped
    t = c.tables.clone()
    t[s, 0] = c.tables[s + 1, 0]
    assert ac.rowerr(ac.heads(ac.prefill_f64(c, tables=t), c.H), good) >= DETECT       # one wrong page id


def test_old_bound_misses_one_key():
    """Why this file exists: on the i.i.d. normal inputs of ``test_gpu_paged_decode_kernel`` a
    context one key short or one key long (a stale slot) stays inside ``assert_close(atol=2e-2,
    rtol=2e-2)``, and on those of ``test_flash_attention`` (S=1024, H=4, KV=1) the key after the
    diagonal leaking into every 128th row stays inside ``2e-2 + 2e-2 max|ref|`` on each of four draws
    (0.026 .. 0.047 against 0.074 .. 0.091)."""
    torch.manual_seed(0)
    H, KVH, pages, W = 8, 8, 80, 40
    k_cache, v_cache = sops.alloc_cache(pages, KVH, torch.float32)
    k_cache.normal_()
    v_cache.normal_()
    tables = torch.randint(0, pages, (2, W), dtype=torch.int32)
    ctx = torch.tensor([1000, 2560], dtype=torch.int32)
    q = torch.randn(2, H * D).to(BF16).float()
    want = sops.paged_decode_ref(q, k_cache, v_cache, tables, ctx, H, KVH)
    for d in (-1, 1):
        bad = sops.paged_decode_ref(q, k_cache, v_cache, tables, ctx + d, H, KVH)
        torch.testing.assert_close(bad, want, atol=2e-2, rtol=2e-2)  # the defect passes
        assert ac.rowerr(bad, want) < ac.CAP  # and random data hides it from the per-row metric as well
    S, H, KV, passed = 1024, 4, 1, 0
    i = torch.arange(S - 1)
    vis = ac.causal_vis(S)
    vis[i[i % 128 == 127], i[i % 128 == 127] + 1] = True
    for seed in range(4):
        c = ac.flash_random_case(S, H, KV, seed=seed)
        good, bad = (ac.flash_f64(c, vis=v, grads=False)["o"] for v in (None, vis))
        passed += (bad - good).abs().max().item() <= 2e-2 + 2e-2 * good.abs().max().item()
    assert passed == 4


# ==================================================================================================
# The CPU paths
# ==================================================================================================
CPU_TOL = 1e-4  # fp32 arithmetic on scores of up to 5 x 22.6 nats


@pytest.mark.parametrize("S,H,KV,causal", [(128, 28, 4, True), (384, 6, 3, False), (512, 8, 1, True)])
def test_cpu_reference_attention(S, H, KV, causal):
    c = ac.flash_case(S, H, KV, causal)
    q, k, v = ops.functional.split_qkv(c.qkv.float(), H, KV)
    assert ac.rowerr(ref.attention(q, k, v, causal), _flash_good(c)["o"]) <= CPU_TOL


@pytest.mark.parametrize("cache_dtype", CACHES, ids=["bf16", "e4m3"])
@pytest.mark.parametrize("H,KVH", [(4, 2), (28, 4), (16, 1)])
def test_cpu_paged_paths(H, KVH, cache_dtype):
    ks, vs = ac._scales(cache_dtype)
    c = ac.decode_case(H, KVH, cache_dtype)
    got = sops.paged_decode(c.qkv.float(), c.k_cache, c.v_cache, c.tables, c.ctx, H, KVH, k_scale=ks, v_scale=vs)
    assert ac.rowerr(got, ac.decode_f64(c)) <= CPU_TOL
    c = ac.prefill_case(H, KVH, cache_dtype)
    out = torch.full((c.rows, H * D), 1024.0)
    sops.paged_prefill(c.qkv.float(), c.k_cache, c.v_cache, c.tables, c.offsets, c.starts, c.lens, H, KVH, out=out,
                       k_scale=ks, v_scale=vs)
    assert (out[~c.listed] == 1024.0).all()
    assert ac.rowerr(out[c.listed], ac.prefill_f64(c)[c.listed]) <= CPU_TOL


# ==================================================================================================
# GPU
# ==================================================================================================
def _run_flash(c, dev):
    qkv = c.qkv.to(dev).requires_grad_()
    o = ops.attention(qkv, c.H, c.KV, causal=c.causal)
    o.backward(c.do.to(dev))
    g = qkv.grad.view(c.B, c.S, c.H + 2 * c.KV, D)
    return {"o": o.detach().view(c.B, c.S, c.H, D), "dq": g[:, :, : c.H], "dk": g[:, :, c.H : c.H + c.KV],
            "dv": g[:, :, c.H + c.KV :]}


def _flash_check(name, c, dev, names):
    want, model = ac.flash_f64(c, device=dev), ac.flash_f64(c, model=True, device=dev)
    got = _run_flash(c, dev)
    _report(name, {n: ac.rowerr(got[n], want[n]) for n in names},
            {n: ac.threshold(ac.rowerr(model[n], want[n])) for n in names})


@pytest.mark.gpu
@pytest.mark.parametrize("S,H,KV,causal", FLASH)
def test_gpu_flash_attention_needles(gpu, S, H, KV, causal):
    """Forward (V random in bf16) and dQ, dK, dV (V on the 1/8 grid; see the module docstring) of
    ``ops.attention`` in the default environment.  S = 128, 384, 1152: the 4-wave forward and dQ
    forms; 512: two 8-wave workgroups.  H % 8 != 0: the plain delta kernel."""
    name = f"flash S={S} H={H} KV={KV} causal={causal}"
    _flash_check(name, ac.flash_case(S, H, KV, causal), gpu, ("o",))
    _flash_check(name + " grid-V", ac.flash_case(S, H, KV, causal, vgrid=True), gpu, ("dq", "dk", "dv"))


@pytest.mark.gpu
def test_gpu_flash_attention_unsaturated(gpu):
    _flash_check("flash random S=1024 H=8 KV=2", ac.flash_random_case(), gpu, ("o", "dq", "dk", "dv"))


def _decode_plans(c, dev):
    """(name, workspace) of every split plan: unsplit, 2 splits, 8 single-page splits, the default."""
    for name, (nsplit, pps) in ac.DECODE_PLANS.items():
        ws = sops.DecodeWorkspace(c.B, c.H, c.KVH, c.W, dev)
        assert ws.nsplit >= nsplit  # the preallocated partials cover the plan
        ws.nsplit, ws.pps = nsplit, pps
        yield name, ws
    yield "default", sops.DecodeWorkspace(c.B, c.H, c.KVH, c.W, dev)


def _run_decode(c, dev, ws):
    ks, vs = c.scales
    ws.o_part.fill_(float("nan"))  # an empty split's partial row must never be read
    return sops.paged_decode(c.qkv.to(dev), c.k_cache.to(dev), c.v_cache.to(dev), c.tables.to(dev), c.ctx.to(dev),
                             c.H, c.KVH, ws=ws, k_scale=ks, v_scale=vs)


@pytest.mark.gpu
@pytest.mark.parametrize("cache_dtype", CACHES, ids=["bf16", "e4m3"])
@pytest.mark.parametrize("H,KVH", ac.DECODE_HEADS)
def test_gpu_paged_decode_needles(gpu, H, KVH, cache_dtype):
    """Every context length at a page or split edge, under every split plan, over a NaN-filled
    workspace; and a one-token prefill segment at ctx - 1 equals the unsplit decode bit for bit."""
    c = ac.decode_case(H, KVH, cache_dtype)
    want = ac.heads(ac.decode_f64(c), H)
    thr = ac.threshold(ac.rowerr(ac.heads(ac.decode_f64(c, model=True), H), want))
    errs, unsplit = {}, None
    for name, ws in _decode_plans(c, gpu):
        got = _run_decode(c, gpu, ws)
        assert torch.isfinite(got).all(), name
        errs[name] = ac.rowerr(ac.heads(got.cpu(), H), want)
        if name == "unsplit":
            unsplit = got
    ks, vs = c.scales
    i32 = dict(dtype=torch.int32, device=gpu)
    pre = sops.paged_prefill(c.qkv.to(gpu), c.k_cache.to(gpu), c.v_cache.to(gpu), c.tables.to(gpu),
                             torch.arange(c.B, **i32), c.ctx.to(gpu) - 1, torch.ones(c.B, **i32), H, KVH,
                             k_scale=ks, v_scale=vs)
    _report(f"paged decode H={H} KVH={KVH} {cache_dtype}", errs, dict.fromkeys(errs, thr))
    assert torch.equal(pre, unsplit)


@pytest.mark.gpu
@pytest.mark.parametrize("cache_dtype", CACHES, ids=["bf16", "e4m3"])
def test_gpu_paged_decode_unsaturated(gpu, cache_dtype):
    c = ac.decode_random_case(cache_dtype)
    want = ac.heads(ac.decode_f64(c), c.H)
    thr = ac.threshold(ac.rowerr(ac.heads(ac.decode_f64(c, model=True), c.H), want))
    one = sops.DecodeWorkspace(1, c.H, c.KVH, c.W, gpu)
    one.nsplit, one.pps = 1, c.W
    plans = {"unsplit": one, "default": sops.DecodeWorkspace(1, c.H, c.KVH, c.W, gpu)}
    errs = {n: ac.rowerr(ac.heads(_run_decode(c, gpu, ws).cpu(), c.H), want) for n, ws in plans.items()}
    _report(f"paged decode random ctx=1000 {cache_dtype}", errs, dict.fromkeys(errs, thr))


def _prefill_check(name, c, dev, max_lens):
    ks, vs = c.scales
    want = ac.prefill_f64(c)[c.listed]
    thr = ac.threshold(ac.rowerr(ac.heads(ac.prefill_f64(c, model=True)[c.listed], c.H), ac.heads(want, c.H)))
    errs = {}
    for max_len in max_lens:  # read back and validated by the binding / given by the caller
        out = torch.full((c.rows, c.H * D), 1024.0, dtype=BF16, device=dev)
        sops.paged_prefill(c.qkv.to(dev), c.k_cache.to(dev), c.v_cache.to(dev), c.tables.to(dev), c.offsets.to(dev),
                           c.starts.to(dev), c.lens.to(dev), c.H, c.KVH, out=out, k_scale=ks, v_scale=vs,
                           max_len=max_len)
        out = out.cpu()
        assert (out[~c.listed] == 1024.0).all()  # rows outside the segments keep the sentinel
        errs[f"max_len={max_len}"] = ac.rowerr(ac.heads(out[c.listed], c.H), ac.heads(want, c.H))
    _report(name, errs, dict.fromkeys(errs, thr))


@pytest.mark.gpu
@pytest.mark.parametrize("cache_dtype", CACHES, ids=["bf16", "e4m3"])
@pytest.mark.parametrize("H,KVH", ac.PREFILL_HEADS)
def test_gpu_paged_prefill_needles(gpu, H, KVH, cache_dtype):
    """40 segments (start x len over the 16-column and 48-token tile edges and the page edges),
    packed with gaps, the last query head a trap head."""
    c = ac.prefill_case(H, KVH, cache_dtype)
    _prefill_check(f"paged prefill H={H} KVH={KVH} {cache_dtype}", c, gpu, (None, max(n for _, n in c.segs)))


@pytest.mark.gpu
@pytest.mark.parametrize("cache_dtype", CACHES, ids=["bf16", "e4m3"])
def test_gpu_paged_prefill_unsaturated(gpu, cache_dtype):
    c = ac.prefill_random_case(cache_dtype)
    _prefill_check(f"paged prefill random 100 over 200 {cache_dtype}", c, gpu, (None, 100))
