"""N-gram speculative decoding: the proposer and the scheduler's lookahead grants (native), the
verify attention (``ops.serving.paged_verify``: reference on the CPU, the HIP kernel against fp64 on
inputs in which every key is individually observable, ``tests/attn_cases.py``), and the engine --
whose outputs with ``speculative_ngram`` on must be the plain engine's, token for token.
"""

import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import attn_cases as ac
from tests.attn_cases import BF16, D, DETECT, E4M3, F64, PAGE
from tests.test_serving import _hf_tiny
from dstack_amd.ops import serving as sops
from dstack_amd.serving._native import Scheduler, ngram_propose
from dstack_amd.serving.engine import LLMEngine, SamplingParams

CACHES = [BF16, E4M3]


# ==================================================================================================
# 1. Proposer
# ==================================================================================================
def _propose(ids, k, n_max=3, n_min=1):
    out = ngram_propose(np.asarray(ids, dtype=np.int32), k, n_max, n_min)
    assert out.dtype == np.int32
    return out.tolist()


def test_ngram_propose():
    assert _propose([1, 2, 3, 4, 5], 4) == []                                   # no match
    # the suffix [2, 3] matches at 1 (-> 9); the shorter [3] alone also matches at 5 (-> 8): longest wins
    assert _propose([1, 2, 3, 9, 7, 3, 8, 2, 3], 2) == [9, 7]
    assert _propose([1, 2, 3, 9, 7, 3, 8, 2, 3], 2, n_max=1) == [8, 2]
    # [5, 6] occurs at 0 (-> 1) and at 3 (-> 2): the most recent one wins
    assert _propose([5, 6, 1, 5, 6, 2, 9, 5, 6], 3, n_max=2) == [2, 9, 5]
    # the copy runs over the end of the history into the drafts it has produced
    assert _propose([5, 6, 7, 5, 6, 7, 5, 6], 4) == [7, 5, 6, 7]
    assert _propose([9, 9, 9], 3) == [9, 9, 9]
    # a history shorter than n_min + 1 tokens
    assert _propose([4], 3) == [] and _propose([], 3) == [] and _propose([4, 4], 3, n_max=3, n_min=2) == []
    assert _propose([4, 4, 4], 3, n_max=3, n_min=2) == [4, 4, 4]
    assert _propose([1, 2, 1, 2], 0) == []
    with pytest.raises(ValueError):
        _propose([1, 2, 1], 2, n_max=1, n_min=2)


# ==================================================================================================
# 2. Scheduler lookahead
# ==================================================================================================
def _sched(num_pages=8, max_model_len=512, caching=False, max_batch=4):
    return Scheduler(num_pages=num_pages, page_size=PAGE, max_batch=max_batch, max_prefill_tokens=4096,
                     max_model_len=max_model_len, pad_to=128, enable_prefix_caching=caching)


def _advance(s, sid, tokens):
    """What the engine does for every token a step emits."""
    for t in tokens:
        s.mark_computed(sid)
        s.append(sid, t)


def test_scheduler_lookahead_slots_cross_a_page_edge():
    s = _sched()
    s.add(1, 62, 200)
    assert s.schedule(False, 4)["kind"] == "prefill"  # (a prefill plan has no lookahead)
    _advance(s, 1, [7])
    plan = s.schedule(False, 4)
    assert plan["kind"] == "decode" and plan["lookahead"].tolist() == [4]
    assert plan["positions"].shape == plan["slots"].shape == (1, 5) and plan["positions"].dtype == np.int32
    assert plan["positions"].tolist() == [[62, 63, 64, 65, 66]] and plan["ctx_lens"].tolist() == [63]
    pages = s.pages(1)
    assert len(pages) == 2 and plan["block_tables"][0, :2].tolist() == pages
    assert plan["slots"].tolist() == [[pages[p // PAGE] * PAGE + p % PAGE for p in range(62, 67)]]
    # all drafts rejected: the second page is not needed by 64 tokens and goes back
    _advance(s, 1, [8])
    assert s.num_tokens(1) == 64
    plan = s.schedule(False, 0)
    assert "lookahead" not in plan and plan["positions"].tolist() == [63] and len(s.pages(1)) == 1
    assert s.free_pages == 7


def test_scheduler_lookahead_grant_shrinks():
    s = _sched()                      # the request's own cap: 10 + 3 tokens
    s.add(1, 10, 13)
    s.schedule(False, 4)
    _advance(s, 1, [7])
    plan = s.schedule(False, 4)       # 11 tokens: the step may emit 2, so 1 draft
    assert plan["lookahead"].tolist() == [1]
    assert plan["positions"].tolist() == [[10, 11, 0, 0, 0]] and plan["slots"][0, 2:].tolist() == [-1, -1, -1]
    _advance(s, 1, [7])
    assert s.schedule(False, 4)["lookahead"].tolist() == [0]  # one token left: a plain row
    s = _sched(max_model_len=14)      # max_model_len caps max_tokens
    s.add(1, 10, 1000)
    s.schedule(False, 4)
    _advance(s, 1, [7])
    assert s.schedule(False, 4)["lookahead"].tolist() == [2]
    s = _sched(num_pages=1)           # no free page for positions >= 64
    s.add(1, 62, 200)
    s.schedule(False, 4)
    _advance(s, 1, [7])
    plan = s.schedule(False, 4)
    assert plan["lookahead"].tolist() == [1] and plan["positions"][0, :2].tolist() == [62, 63]
    s = _sched(num_pages=3)           # the free page goes to the first sequence that asks
    for i in (1, 2):
        s.add(i, 62, 200)
    s.schedule(False, 4)
    for i in (1, 2):
        _advance(s, i, [7])
    assert s.schedule(False, 4)["lookahead"].tolist() == [4, 1]


def _plan_bytes(plan):
    return {k: (v.dtype.str, v.shape, v.tobytes()) if isinstance(v, np.ndarray) else v for k, v in plan.items()}


@pytest.mark.parametrize("caching", [False, True])
def test_scheduler_lookahead_never_preempts_and_zero_is_todays_plan(caching):
    """Three schedulers in lockstep over a pool that just holds the mandatory pages, every draft
    rejected: the one that grants lookahead preempts exactly when the plain ones do, and
    ``lookahead=0`` plans are the plain plans byte for byte."""
    plain, zero, look = (_sched(num_pages=6, caching=caching) for _ in range(3))
    prompts = {i: [(7 * i + t) % 50 for t in range(100 + 9 * i)] for i in range(4)}
    for s in (plain, zero, look):
        for i, p in prompts.items():
            s.add(i, len(p), len(p) + 80, np.asarray(p, dtype=np.int32))
    preemptions = grants = 0
    for step in range(400):
        pp, pz, pl = plain.schedule(False), zero.schedule(False, 0), look.schedule(False, 4)
        assert _plan_bytes(pp) == _plan_bytes(pz)
        assert pl["kind"] == pp["kind"] and list(pl["seq_ids"]) == list(pp["seq_ids"])
        assert list(pl["preempted"]) == list(pp["preempted"])
        preemptions += len(pp["preempted"])
        if pp["kind"] == "idle":
            break
        if pp["kind"] == "decode":
            assert pl["ctx_lens"].tolist() == pp["ctx_lens"].tolist()
            assert pl["positions"][:, 0].tolist() == pp["positions"].tolist()
            grants += int(pl["lookahead"].sum())
        for sid in list(pp["seq_ids"]):
            for s in (plain, zero, look):
                _advance(s, sid, [step % 50])
                if s.is_done(sid):
                    s.finish(sid)
        assert look.free_pages <= plain.free_pages  # (it may hold lookahead pages until its next plan)
    else:
        raise AssertionError("did not finish")
    assert preemptions > 0 and grants > 0
    assert look.free_pages == plain.free_pages == 6


def test_scheduler_rejected_drafts_do_not_register_a_page():
    s = _sched(caching=True)
    ids = list(range(100, 160))
    s.add(1, 60, 200, np.asarray(ids, dtype=np.int32))
    s.schedule(False, 4)
    _advance(s, 1, [11])
    plan = s.schedule(False, 4)       # rows at 60 (the last token) and 61 .. 64: the drafts' K/V fill page 0
    assert plan["lookahead"].tolist() == [4] and plan["positions"][0].tolist() == [60, 61, 62, 63, 64]
    _advance(s, 1, [12])              # all four rejected: 62 tokens, 61 of them cached
    assert s.cached_pages == 0
    s.schedule(False, 4)
    _advance(s, 1, [13, 14])          # one accepted: 64 tokens, 63 cached
    assert s.num_tokens(1) == 64 and s.cached_pages == 0
    s.schedule(False, 4)
    _advance(s, 1, [15])              # position 63 holds an accepted token's K/V now
    assert s.cached_pages == 1
    # and the page serves the accepted tokens, not the drafts: a prompt of those 64 tokens hits it
    s.add(2, 70, 200, np.asarray(ids + [11, 12, 13, 14] + [0] * 6, dtype=np.int32))
    before = s.prefix_hit_tokens
    assert s.schedule(False, 4)["kind"] == "prefill" and s.prefix_hit_tokens - before == 64
    s.add(3, 70, 200, np.asarray(ids + [11, 12, 13, 99] + [0] * 6, dtype=np.int32))
    before = s.prefix_hit_tokens
    assert s.schedule(False, 4)["kind"] == "prefill" and s.prefix_hit_tokens == before


# ==================================================================================================
# 3. paged_verify: the reference
# ==================================================================================================
def _random_verify_inputs(T, H=8, KVH=2, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    pages, W = 24, 5
    k_cache, v_cache = sops.alloc_cache(pages, KVH, dtype)
    k_cache.copy_(torch.randn(k_cache.shape, generator=g))
    v_cache.copy_(torch.randn(v_cache.shape, generator=g))
    ctx = torch.tensor([1, 64, 65, 130, 200, 0, 7], dtype=torch.int32)
    q_lens = torch.tensor([min(i % (T + 1), int(c)) for i, c in enumerate(ctx)], dtype=torch.int32)
    B = ctx.numel()
    tables = torch.stack([torch.randperm(pages, generator=g)[:W] for _ in range(B)]).int()
    q = torch.randn(B * T + 3, (H + 2 * KVH) * D, generator=g).to(dtype)
    return SimpleNamespace(T=T, H=H, KVH=KVH, B=B, q=q, k=k_cache, v=v_cache, tables=tables, ctx=ctx, q_lens=q_lens)


@pytest.mark.parametrize("T", [1, 3, 8])
def test_paged_verify_ref_is_prefill_and_decode(T):
    c = _random_verify_inputs(T)
    got = sops.paged_verify_ref(c.q, c.k, c.v, c.tables, c.ctx, c.q_lens, T, c.H, c.KVH)
    i32 = dict(dtype=torch.int32)
    want = sops.paged_prefill_ref(c.q, c.k, c.v, c.tables, torch.arange(c.B, **i32) * T, c.ctx - c.q_lens, c.q_lens,
                                  c.H, c.KVH)
    torch.testing.assert_close(got, want, atol=1e-6, rtol=1e-6)
    used = torch.zeros(c.q.shape[0], dtype=torch.bool)
    for b in range(c.B):
        used[b * T : b * T + int(c.q_lens[b])] = True
    assert used.any() and (got[~used] == 0).all() and (got[used].abs().sum(1) > 0).all()
    # the op's CPU path is the reference, written into `out`
    out = torch.full((c.q.shape[0], c.H * D), 7.0)
    assert sops.paged_verify(c.q, c.k, c.v, c.tables, c.ctx, c.q_lens, T, c.H, c.KVH, out=out) is out
    assert torch.equal(out, got)
    if T == 1:
        rows = c.q_lens == 1
        dec = sops.paged_decode_ref(c.q[: c.B][rows], c.k, c.v, c.tables[rows], c.ctx[rows], c.H, c.KVH)
        torch.testing.assert_close(got[: c.B][rows], dec, atol=1e-6, rtol=1e-6)


def test_verify_workspace_and_plan():
    assert [sops.verify_plan(T, G) for T, G in ((1, 1), (2, 1), (8, 2), (5, 7), (4, 8), (5, 8), (8, 8), (8, 16))] == \
        [(1, 1), (1, 1), (1, 1), (3, 1), (2, 1), (3, 1), (2, 2), (3, 3)]
    for T, G in ((t, g) for t in range(1, 9) for g in range(1, 17)):
        nt, groups = sops.verify_plan(T, G)
        assert 1 <= nt <= 3 and nt * groups * 16 >= T * G > (groups - 1) * nt * 16
    ws = sops.VerifyWorkspace(40, 5, 32, 8, 16, "cpu")
    assert ws.nsplit * ws.pps >= 16 and ws.o_part.numel() == 40 * 32 * ws.nsplit * D
    with pytest.raises(ValueError):
        sops.VerifyWorkspace(40, 9, 32, 8, 16, "cpu")


# ==================================================================================================
# 7. paged_verify needles
# ==================================================================================================
VERIFY_HEADS = [(8, 8, 2), (4, 2, 8), (28, 4, 5), (32, 4, 4), (16, 1, 8)]  # T*G = 2, 16, 35, 32, 128 columns
VERIFY_W = ac.DECODE_W


@functools.lru_cache(maxsize=None)
def verify_case(H, KVH, T, cache_dtype, seed=0):
    """One sequence per context length of ``ac.decode_contexts()`` (the context ends there, drafts
    included), ``q_len`` cycling over 0 .. T, clipped to the context; sequence b owns rows
    ``b*T .. b*T + T - 1`` and three more rows follow (a row bucket's padding).  The query at position
    ``pos``: heads 0 .. H - 2 target the diagonal and, in every lower page, the key with the same low
    code; head H - 1 is the trap head: the diagonal and the key at ``pos + 1`` -- a later draft's
    real cache entry, and for the last query the slot after the context (``ac._build_tables`` puts
    the last key there again, with the sentinel v: a stale rejected draft that scores like the
    diagonal).  In the shape ``ac.prefill_f64`` takes."""
    g = torch.Generator().manual_seed(seed)
    ends, W = ac.decode_contexts(), VERIFY_W
    B = len(ends)
    q_lens = [min(b % (T + 1), ends[b]) for b in range(B)]
    tables, kc, vc, npg = ac._build_tables(ends, W, KVH, cache_dtype, g)
    rows = B * T + 3
    qkv = ac.rb(torch.randn(rows, (H + 2 * KVH) * D, generator=g, dtype=F64))
    targets = torch.full((rows, H, W), -1, dtype=torch.long)
    trap = torch.full((rows,), -1, dtype=torch.long)
    listed = torch.zeros(rows, dtype=torch.bool)
    for b in range(B):
        n = q_lens[b]
        pos = ends[b] - n + torch.arange(n)
        r = b * T + torch.arange(n)
        listed[r] = True
        targets[r, :, 0] = pos.view(n, 1)
        for p in range(W - 1):
            sel = p < pos // PAGE
            targets[r[sel], : H - 1, 1 + p] = (p * PAGE + pos[sel] % PAGE).view(-1, 1)
        trap[r] = pos + 1
    q = ac.needle_q(targets)
    q[:, H - 1] += 2.0 * ac.code(trap.clamp_min(0)) * (trap >= 0).to(F64).unsqueeze(-1)
    qkv[listed, : H * D] = q[listed].reshape(-1, H * D)
    assert torch.equal(ac.rb(qkv), qkv)
    i32 = dict(dtype=torch.int32)
    live = [b for b in range(B) if q_lens[b] > 0]  # (the reference walks the sequences that hold a query)
    return SimpleNamespace(
        H=H, KVH=KVH, T=T, B=B, W=W, cache_dtype=cache_dtype, rows=rows, npg=npg, listed=listed, ends=ends,
        ctx=torch.tensor(ends, **i32), q_lens=torch.tensor(q_lens, **i32), all_tables=tables,
        segs=[(ends[b] - q_lens[b], q_lens[b]) for b in live], offsets=torch.tensor([b * T for b in live], **i32),
        tables=tables[live], live=live, k_cache=kc, v_cache=vc, targets=targets, trap=trap, trap_head=H - 1,
        qkv=qkv.to(BF16), scales=ac._scales(cache_dtype))


@pytest.mark.parametrize("cache_dtype", CACHES, ids=["bf16", "e4m3"])
@pytest.mark.parametrize("H,KVH,T", VERIFY_HEADS)
def test_verify_case_invariants(H, KVH, T, cache_dtype):
    c = verify_case(H, KVH, T, cache_dtype)
    assert set(c.q_lens.tolist()) == set(range(T + 1)) and (c.q_lens <= c.ctx).all()
    assert c.listed.sum().item() == int(c.q_lens.sum()) and not c.listed[c.B * T :].any()
    _, ps = ac.prefill_f64(c, want_p=True)
    seen_pages = set()
    for s, (start, n) in enumerate(c.segs):
        off = int(c.offsets[s])
        t = c.targets[off : off + n].transpose(0, 1)  # [H, n, m]
        mass = (ps[s].gather(-1, t.clamp_min(0)) * (t >= 0)).sum(-1)
        assert mass.min().item() >= 1 - 1e-6
        assert set((t[t >= 0] // PAGE).tolist()) == set(range((start + n - 1) // PAGE + 1))  # every page it sees
        seen_pages |= {(start + n - 1) // PAGE}
    assert {0, 1, c.W - 1} <= seen_pages
    # the trap key, once visible, takes at least a third of the trap head's row: on every row
    _, pl = ac.prefill_f64(c, shift=1, want_p=True)
    for s, (start, n) in enumerate(c.segs):
        pos = start + torch.arange(n)
        ok = pos + 1 < c.W * PAGE
        leak = pl[s][c.trap_head].gather(-1, (pos + 1).clamp_max(c.W * PAGE - 1).unsqueeze(-1)).squeeze(-1)
        assert (leak[ok] >= 1 / 3 - 1e-9).all()


@pytest.mark.parametrize("cache_dtype", CACHES, ids=["bf16", "e4m3"])
def test_metric_sees_verify_defects(cache_dtype):
    c = verify_case(4, 2, 8, cache_dtype)
    good = ac.heads(ac.prefill_f64(c), c.H)
    assert ac.rowerr(ac.heads(ac.prefill_f64(c, shift=-1), c.H), good) >= DETECT       # key < limit
    full, bad = ac.prefill_f64(c), ac.prefill_f64(c, shift=1)                          # key <= limit + 1
    assert ac.rowerr(ac.heads(bad, c.H), good) >= DETECT
    for s, (start, n) in enumerate(c.segs):  # ... in every sequence: a later draft, or the slot after the context
        if start + n < c.W * PAGE:
            r = slice(int(c.offsets[s]), int(c.offsets[s]) + n)
            assert ac.rowerr(ac.heads(bad[r], c.H), ac.heads(full[r], c.H)) >= DETECT, (start, n)
    swapped = 0
    for s, (start, n) in enumerate(c.segs):                                            # two entries swapped
        npg = (start + n + PAGE - 1) // PAGE
        if npg >= 2 and (start + n) % PAGE:
            t = c.tables.clone()
            t[s, 0], t[s, npg - 1] = c.tables[s, npg - 1], c.tables[s, 0]
            assert ac.rowerr(ac.heads(ac.prefill_f64(c, tables=t), c.H), good) >= DETECT
            swapped += 1
    assert swapped >= 3


@pytest.mark.parametrize("cache_dtype", CACHES, ids=["bf16", "e4m3"])
@pytest.mark.parametrize("H,KVH,T", [(4, 2, 8), (28, 4, 5)])
def test_cpu_paged_verify_needles(H, KVH, T, cache_dtype):
    ks, vs = ac._scales(cache_dtype)
    c = verify_case(H, KVH, T, cache_dtype)
    got = sops.paged_verify(c.qkv.float(), c.k_cache, c.v_cache, c.all_tables, c.ctx, c.q_lens, T, H, KVH,
                            k_scale=ks, v_scale=vs)
    assert (got[~c.listed] == 0).all()
    assert ac.rowerr(ac.heads(got, H), ac.heads(ac.prefill_f64(c), H)) <= 1e-4  # (fp32 on scores of up to 9 x 22.6 nats)


def _verify_plans(c, dev):
    """(name, workspace) of every split plan of ``ac.DECODE_PLANS`` and the default one."""
    for name, (nsplit, pps) in ac.DECODE_PLANS.items():
        ws = sops.VerifyWorkspace(c.rows, c.T, c.H, c.KVH, c.W, dev, target_waves=1 << 20)
        assert ws.nsplit >= nsplit  # the preallocated partials cover the plan
        ws.nsplit, ws.pps = nsplit, pps
        yield name, ws
    yield "default", sops.VerifyWorkspace(c.rows, c.T, c.H, c.KVH, c.W, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("cache_dtype", CACHES, ids=["bf16", "e4m3"])
@pytest.mark.parametrize("H,KVH,T", VERIFY_HEADS)
def test_gpu_paged_verify_needles(gpu, H, KVH, T, cache_dtype):
    """Every context end at a page or split edge with every q_len 0 .. T, under every split plan,
    over a NaN-filled workspace; judged per row against fp64 with the rounding model's threshold."""
    c = verify_case(H, KVH, T, cache_dtype)
    ks, vs = c.scales
    want = ac.heads(ac.prefill_f64(c), H)
    thr = ac.threshold(ac.rowerr(ac.heads(ac.prefill_f64(c, model=True), H), want))
    dev = [t.to(gpu) for t in (c.qkv, c.k_cache, c.v_cache, c.all_tables, c.ctx, c.q_lens)]
    errs = {}
    for name, ws in _verify_plans(c, gpu):
        ws.o_part.fill_(float("nan"))  # an empty split's partial row must never be read
        out = torch.full((c.rows, H * D), 1024.0, dtype=BF16, device=gpu)
        got = sops.paged_verify(*dev, T, H, KVH, out=out, ws=ws, k_scale=ks, v_scale=vs).cpu()
        assert torch.isfinite(got).all(), name
        assert (got[~c.listed] == 0).all(), name  # rows past q_lens, and the bucket's padding rows
        errs[name] = ac.rowerr(ac.heads(got, H), want)
    print(f"paged verify H={H} KVH={KVH} T={T} {cache_dtype}: " +
          ", ".join(f"{k} {v:.3g} (<= {thr:.3g})" for k, v in errs.items()))
    bad = {k: v for k, v in errs.items() if not v <= thr}
    assert not bad, f"worst row error over threshold {thr}: {bad}"


# ==================================================================================================
# 8. Bitwise anchor
# ==================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("cache_dtype", CACHES, ids=["bf16", "e4m3"])
@pytest.mark.parametrize("H,KVH", ac.DECODE_HEADS)
def test_gpu_paged_verify_one_token_is_paged_decode(gpu, H, KVH, cache_dtype):
    """T = 1 is the decode kernel's page walk: bit for bit under the unsplit plan."""
    c = ac.decode_case(H, KVH, cache_dtype)
    ks, vs = c.scales
    dev = [t.to(gpu) for t in (c.qkv, c.k_cache, c.v_cache, c.tables, c.ctx)]
    dws = sops.DecodeWorkspace(c.B, H, KVH, c.W, gpu)
    dws.nsplit, dws.pps = 1, c.W
    vws = sops.VerifyWorkspace(c.B, 1, H, KVH, c.W, gpu)
    vws.nsplit, vws.pps = 1, c.W
    dec = sops.paged_decode(*dev, H, KVH, ws=dws, k_scale=ks, v_scale=vs)
    ver = sops.paged_verify(*dev, torch.ones_like(dev[4]), 1, H, KVH, ws=vws, k_scale=ks, v_scale=vs)
    assert torch.equal(ver, dec)


# ==================================================================================================
# 4. Engine identity (CPU, fp32): with speculation on, the outputs are the plain engine's
# ==================================================================================================
PROMPTS = [[1 + i, 2, 3, 4 + i] * (5 + i) for i in range(4)] + [[1, 5, 9, 33, 7, 100, 2, 45, 61], list(range(3, 140))]
KINDS = {"greedy": dict(temperature=0.0), "sampled": dict(temperature=0.05, seed=3)}
ENGINE = dict(device="cpu", max_model_len=256, max_batch=8, num_pages=64)
# engine options of each variation (speculative_* only go to the speculating engine)
VARIANTS = {
    "base": {},
    "preemption": dict(num_pages=5),
    "prefix_caching": dict(enable_prefix_caching=True),
    "fp8_kv": dict(kv_cache_dtype="fp8"),
    "penalties": {},
    "max_batch_2": dict(max_batch=4, speculative_max_batch=2),
    "top_logprobs": {},
}
PENALISED = 1  # the request that carries a repetition penalty and a logit_bias in "penalties"


def _generate(eng, prompts, params):
    """``eng.generate`` that also records, per request, the step each of its tokens came from."""
    steps = [[] for _ in prompts]
    reqs = [eng.add_request(p, sp, on_event=lambda r, t, f, i=i: steps[i].append(eng.stats["steps"]) if t is not None
                            else None) for i, (p, sp) in enumerate(zip(prompts, params))]
    while any(not r.finished for r in reqs):
        eng.step()
    return reqs, steps


def _params(kind, variant, n=len(PROMPTS)):
    extra = dict(top_logprobs=3) if variant == "top_logprobs" else {}
    ps = [SamplingParams(max_tokens=80, ignore_eos=True, **KINDS[kind], **extra) for _ in range(n)]
    if variant == "penalties":
        ps[PENALISED] = SamplingParams(max_tokens=80, ignore_eos=True, repetition_penalty=1.3,
                                       logit_bias={5: 2.0, 7: -1.0}, **KINDS[kind])
    return ps


@functools.lru_cache(maxsize=None)
def _stop_request():
    """The seventh request: greedy, and it stops on a ``stop_token_ids`` entry.  An accepted draft is
    a copy of an earlier token of its sequence, so the prompt is one of the prompts plus the start
    of the plain engine's greedy output for it, and the stop token is taken from the output that
    follows: one that the speculating engine first emits from an accepted draft, with further
    accepted tokens behind it in the same step (they must be dropped).  Returns (prompt, params, the
    tokens the request must produce)."""
    torch.manual_seed(0)
    plain = LLMEngine.from_model("llama-tiny", **ENGINE).generate(PROMPTS, _params("greedy", "base"))
    prompts = [PROMPTS[i] + plain[i].output_ids[:m] for i in (5, 4, 2, 0) for m in (4, 16)]
    ps = [SamplingParams(max_tokens=80, temperature=0.0, ignore_eos=True)] * len(prompts)
    spec, steps = _generate(LLMEngine.from_model("llama-tiny", speculative_ngram=4, **ENGINE), prompts, ps)
    for prompt, r, st in zip(prompts, spec, steps):
        out = r.output_ids
        for k in range(1, len(out) - 1):
            if out.index(out[k]) == k and st[k - 1] == st[k] == st[k + 1]:
                return prompt, SamplingParams(max_tokens=80, temperature=0.0, stop_token_ids=(out[k],)), out[: k + 1]
    raise AssertionError("no output token is first emitted inside an accepted run")


@functools.lru_cache(maxsize=None)
def _engine_runs(kind, variant):
    """(plain requests, speculating requests, the speculating engine, its per-token step log)."""
    torch.manual_seed(0)
    opts = dict(ENGINE, **VARIANTS[variant])
    spec_opts = dict(opts, speculative_ngram=4)
    opts.pop("speculative_max_batch", None)
    stop_prompt, stop_params, _ = _stop_request()
    prompts, params = PROMPTS + [stop_prompt], _params(kind, variant) + [stop_params]
    plain_eng = LLMEngine.from_model("llama-tiny", **opts)
    eng = LLMEngine.from_model("llama-tiny", **spec_opts)
    plain, out, steps = [], [], []
    for _ in range(2 if variant == "prefix_caching" else 1):  # (twice: the second pass hits the cache)
        plain += plain_eng.generate(prompts, params)
        o, s = _generate(eng, prompts, params)
        out, steps = out + o, steps + s
    return plain, out, eng, steps, plain_eng


CASES = [(k, v) for k in KINDS for v in VARIANTS]


@pytest.mark.parametrize("kind,variant", CASES)
def test_engine_speculative_tokens_are_the_plain_engines(kind, variant):
    plain, out, eng, steps, plain_eng = _engine_runs(kind, variant)
    assert [r.output_ids for r in out] == [r.output_ids for r in plain]
    assert [r.finish_reason for r in out] == [r.finish_reason for r in plain]
    assert all(len(r.logprobs) == len(r.output_ids) for r in out)
    # both branches ran: drafts were accepted and drafts were rejected
    st = eng.stats
    assert st["spec_steps"] > 0 and st["spec_accepted"] > 0 and st["spec_drafted"] > st["spec_accepted"], st
    # decode_tokens counts emitted tokens (every admission's prefill step emits one itself)
    assert st["decode_tokens"] == sum(len(r.output_ids) for r in out) - len(out) - st["preemptions"]
    # the stopped request: cut inside an accepted run, nothing after the stop token
    _, _, want = _stop_request()
    for r in out[len(PROMPTS) :: len(PROMPTS) + 1]:
        assert r.output_ids == want and r.finish_reason == "stop"
    if kind == "sampled":
        greedy = _engine_runs("greedy", variant)[0]
        assert [r.output_ids for r in plain[: len(PROMPTS)]] != [r.output_ids for r in greedy[: len(PROMPTS)]]
    if variant == "preemption":
        assert st["preemptions"] > 0 and plain_eng.stats["preemptions"] > 0
    if variant == "prefix_caching":
        assert st["prefix_hit_tokens"] >= 128 and st["prefix_hit_tokens"] == plain_eng.stats["prefix_hit_tokens"]
        assert eng.sched.free_pages == eng.sched.num_pages
    if variant == "penalties":  # the penalised request rides along without drafts; the others speculate
        assert len(set(steps[PENALISED])) == len(steps[PENALISED]) == 80
        assert any(len(set(s)) < len(s) for i, s in enumerate(steps) if i != PENALISED)
    if variant == "max_batch_2":  # plain steps while more than two sequences run, verify steps after
        assert 0 < st["spec_steps"] and st["steps"] < plain_eng.stats["steps"]
        assert len(set(steps[0])) == len(steps[0])  # (the first four ran in the plain steps)
    if variant == "top_logprobs":
        for a, b in list(zip(out, plain))[: len(PROMPTS)]:
            assert len(a.top_logprobs) == len(a.output_ids)
            assert [[t for t, _ in row] for row in a.top_logprobs] == [[t for t, _ in row] for row in b.top_logprobs]


@pytest.mark.parametrize("kind", KINDS)
def test_engine_speculative_logprobs_are_the_plain_engines(kind):
    """Log-probabilities and top-logprob values against the plain engine's, to 1e-5, in every
    variation.  The CPU path gives a token the same logits at any row count (its products are
    accumulated in fp64, and the verify reference computes a row as the decode reference does), so
    the difference is 0 everywhere but under preemption, where the two engines recompute different
    tokens through a prefill step: 9.5e-7 greedy, 3.8e-6 at ``temperature=0.05``."""
    worst = {}
    for variant in VARIANTS:
        plain, out = _engine_runs(kind, variant)[:2]
        diff = max(abs(p - q) for a, b in zip(out, plain) for p, q in zip(a.logprobs, b.logprobs))
        tops = [abs(p - q) for a, b in zip(out, plain) for ra, rb in zip(a.top_logprobs, b.top_logprobs)
                for (_, p), (_, q) in zip(ra, rb)]
        worst[variant] = max([diff] + tops)
        print(f"{kind} {variant}: largest logprob difference {diff:.3g}, top-logprob difference {max(tops, default=0.0):.3g}")
    assert all(v <= 1e-5 for v in worst.values()), worst


# ==================================================================================================
# 5. Refusals
# ==================================================================================================
def test_speculative_refusals(tmp_path):
    kw = dict(device="cpu", max_model_len=256, max_batch=4, num_pages=16)
    with pytest.raises(ValueError, match="speculative_ngram is not supported with tensor parallel"):
        LLMEngine.from_model("llama-tiny", tp_group=object(), speculative_ngram=4, **kw)

    class TwoRanks:  # what the constructor reads of a tensor-parallel model
        tp, tp_group, tp_rank, device = 2, None, 0, torch.device("cpu")

    with pytest.raises(ValueError, match="speculative_ngram is not supported with tensor parallel"):
        LLMEngine(TwoRanks(), speculative_ngram=4)
    with pytest.raises(ValueError, match="speculative_ngram is not supported with lora_modules"):
        LLMEngine.from_model("llama-tiny", lora_modules={"a": str(tmp_path)}, speculative_ngram=4, **kw)
    for bad in (dict(speculative_ngram=8), dict(speculative_ngram=-1), dict(speculative_ngram=2.0),
                dict(speculative_ngram=True)):
        with pytest.raises(ValueError, match="speculative_ngram must be"):
            LLMEngine.from_model("llama-tiny", **bad, **kw)
    with pytest.raises(ValueError, match="ngram_min must be"):
        LLMEngine.from_model("llama-tiny", speculative_ngram=4, ngram_min=0, **kw)
    with pytest.raises(ValueError, match="ngram_max must be"):
        LLMEngine.from_model("llama-tiny", speculative_ngram=4, ngram_max=0, **kw)
    with pytest.raises(ValueError, match="ngram_min must not exceed ngram_max"):
        LLMEngine.from_model("llama-tiny", speculative_ngram=4, ngram_min=3, ngram_max=2, **kw)
    with pytest.raises(ValueError, match="speculative_max_batch must be"):
        LLMEngine.from_model("llama-tiny", speculative_ngram=4, speculative_max_batch=0, **kw)


def test_speculative_off_allocates_nothing():
    kw = dict(device="cpu", max_model_len=256, max_batch=4, num_pages=16)
    off = LLMEngine.from_model("llama-tiny", **kw)
    assert off.verify_buckets == [] and off.rows_max == 4 and not hasattr(off, "_vws") and not hasattr(off, "s_qlens")
    assert off.s_out_tok.numel() == 4 and "spec_steps" not in off.stats
    on = LLMEngine.from_model("llama-tiny", speculative_ngram=4, speculative_max_batch=3, **kw)
    assert on.verify_buckets == [8, 16] and on.rows_max == 16 and on.s_top_ids.shape[0] == 16 and sorted(on._vws) == [8, 16]
    assert on._verify_rows(1) == 8 and on._verify_rows(3) == 16 and on._verify_rows(4) is None
    # up to 256 rows, whatever the options ask for
    big = LLMEngine.from_model("llama-tiny", speculative_ngram=7, speculative_max_batch=64, device="cpu",
                               max_model_len=128, max_batch=64, num_pages=16)
    assert max(big.verify_buckets) == 256 and big._verify_rows(32) == 256 and big._verify_rows(33) is None


# ==================================================================================================
# 6. Server
# ==================================================================================================
def test_api_speculative_completion_and_metrics():
    from fastapi.testclient import TestClient

    from dstack_amd.serving.server import create_app

    kw = dict(device="cpu", max_model_len=256, max_batch=8, num_pages=32)
    body = {"model": "llama-tiny", "prompt": [1, 2, 3, 4] * 5, "max_tokens": 40, "temperature": 0, "ignore_eos": True,
            "logprobs": 1}
    got = {}
    for name, opts in (("off", {}), ("on", dict(speculative_ngram=4))):
        eng = LLMEngine.from_model("llama-tiny", **kw, **opts)
        with TestClient(create_app(eng, served_model_name="llama-tiny")) as api:
            r = api.post("/v1/completions", json=body)
            assert r.status_code == 200, r.text
            got[name] = (r.json()["choices"][0], r.json()["usage"], api.get("/metrics").text, dict(eng.stats))
    assert got["on"][0]["text"] == got["off"][0]["text"] and got["on"][0]["finish_reason"] == "length"
    assert got["on"][0]["logprobs"]["tokens"] == got["off"][0]["logprobs"]["tokens"]
    assert got["on"][1] == got["off"][1] and got["on"][1]["completion_tokens"] == 40
    st, text = got["on"][3], got["on"][2]
    assert st["spec_accepted"] > 0
    for name, key in (("dstack_serving_spec_steps_total", "spec_steps"),
                      ("dstack_serving_spec_draft_tokens_total", "spec_drafted"),
                      ("dstack_serving_spec_accepted_tokens_total", "spec_accepted")):
        assert f"# TYPE {name} counter" in text and f"\n{name} {st[key]}\n" in text
        assert name not in got["off"][2]


def test_cli_flags_reach_the_engine(monkeypatch):
    import sys
    import types

    from dstack_amd.serving import __main__ as cli
    from dstack_amd.serving import engine as engine_mod

    seen = {}

    class Stop(Exception):
        pass

    def from_model(model, **kw):
        seen.update(kw)
        raise Stop

    monkeypatch.setattr(engine_mod.LLMEngine, "from_model", staticmethod(from_model))
    monkeypatch.setitem(sys.modules, "uvicorn", types.ModuleType("uvicorn"))
    with pytest.raises(Stop):
        cli.main(["--model", "llama-tiny", "--speculative-ngram", "5", "--ngram-max", "4", "--ngram-min", "2",
                  "--speculative-max-batch", "16"])
    assert (seen["speculative_ngram"], seen["ngram_max"], seen["ngram_min"], seen["speculative_max_batch"]) == (5, 4, 2, 16)
    seen.clear()
    with pytest.raises(Stop):
        cli.main(["--model", "llama-tiny"])
    assert (seen["speculative_ngram"], seen["ngram_max"], seen["ngram_min"], seen["speculative_max_batch"]) == (0, 3, 1, 32)


# ==================================================================================================
# 9. Engine on the GPU
# ==================================================================================================
GPU_PROMPTS = [[1, 5, 9, 33, 7, 100, 2, 45, 61], [1, 300, 301, 302], list(range(1, 200)), [7, 8, 9] * 20]


@pytest.mark.gpu
@pytest.mark.parametrize("kv", ["auto", "fp8"])
def test_gpu_engine_speculative(gpu, tmp_path, kv):
    """Tiny HF Llama on the HIP path, greedy, K = 4: captured verify graphs give the eager outputs;
    drafts are accepted and rejected; and (bf16 cache) every emitted token, teacher-forced through
    the fp32 HF model, is within the near-tie bound of ``test_gpu_engine_matches_cpu_and_graphs``
    of that position's best logit -- what a wrongly accepted draft or a leaked stale key breaks."""
    hf, path = _hf_tiny(tmp_path)
    sp = SamplingParams(max_tokens=40, temperature=0, ignore_eos=True)
    kw = dict(device="cuda", max_model_len=512, max_batch=8, num_pages=64, speculative_ngram=4, kv_cache_dtype=kv)
    g = LLMEngine.from_model(path, **kw)
    g.capture_graphs()
    assert sorted(k[1] for k in g._graphs if isinstance(k, tuple) and k[0] == "verify") == g.verify_buckets
    assert g.verify_buckets == [8, 16, 32, 64]  # 1 .. 8 sequences of 5 rows
    out_g = [r.output_ids for r in g.generate(GPU_PROMPTS, sp)]
    ng = LLMEngine.from_model(path, use_graphs=False, **kw)
    out_ng = [r.output_ids for r in ng.generate(GPU_PROMPTS, sp)]
    assert out_g == out_ng and all(len(o) == 40 for o in out_g)
    for eng in (g, ng):
        st = eng.stats
        print(kv, {k: v for k, v in st.items() if k.startswith("spec")})
        assert st["spec_steps"] > 0 and st["spec_accepted"] > 0 and st["spec_drafted"] > st["spec_accepted"], st
    if kv == "fp8":
        return
    with torch.no_grad():
        for p, o in zip(GPU_PROMPTS, out_g):
            ref = hf(torch.tensor([p + o])).logits[0, len(p) - 1 : -1]  # the logits each output token was drawn from
            lo, hi = ref.min(-1).values, ref.max(-1).values
            chosen = ref.gather(1, torch.tensor(o).view(-1, 1)).squeeze(1)
            bad = (chosen < hi - 0.02 * (hi - lo)).nonzero().flatten().tolist()
            assert not bad, (p[:4], bad)
