"""Automatic prefix caching of the serving engine: the native scheduler's page identity, sharing,
reference counts and eviction, the paged-prefix prefill attention (fp32 reference on the CPU, HIP
kernel on the GPU), and the engine / HTTP surface with the feature on (off is the default and is
covered by tests/test_serving.py)."""

import math

import numpy as np
import pytest
import torch

from dstack_amd.ops import serving as sops
from dstack_amd.serving._native import Scheduler
from dstack_amd.serving.engine import LLMEngine, SamplingParams
from dstack_amd.serving.model import ServingLlama, load_spec

PAGE = 64


def _sched(num_pages=16, on=True, **kw):
    args = dict(num_pages=num_pages, page_size=PAGE, max_batch=8, max_prefill_tokens=4096, max_model_len=1024)
    args.update(kw)
    return Scheduler(enable_prefix_caching=on, **args)


def _ids(n, seed):
    return np.random.default_rng(seed).integers(1, 1000, size=n).astype(np.int32)


def _run_prefill(s, sid, ids, max_new=50):
    """add + schedule + mark_computed + one appended token; returns the prefill plan"""
    s.add(sid, len(ids), len(ids) + max_new, ids)
    p = s.schedule()
    assert p["kind"] == "prefill" and list(p["seq_ids"]) == [sid]
    s.mark_computed(sid)
    s.append(sid, 7)
    return p


# ------------------------------------------------------------------------------------------------
# 1. scheduler: hits and sharing
# ------------------------------------------------------------------------------------------------
def test_scheduler_prefix_hit_shares_pages():
    a = _ids(200, 0)
    b = np.concatenate([a[:130], _ids(50, 1)])
    s = _sched()
    pa = _run_prefill(s, 1, a)
    assert list(pa["starts"]) == [0] and list(pa["lens"]) == [200]
    pages_a = s.pages(1)
    assert s.cached_pages == 3  # 200 // 64 full pages
    free = s.free_pages
    s.add(2, len(b), len(b) + 50, b)
    pb = s.schedule()
    assert pb["kind"] == "prefill"
    assert list(pb["starts"]) == [128] and list(pb["lens"]) == [len(b) - 128]
    assert list(pb["block_tables"][0][:2]) == pages_a[:2]
    assert list(pb["ctx_lens"]) == [len(b)]
    # positions and slots cover the computed tokens only, on pages that are not A's
    n = len(b) - 128
    assert list(pb["positions"][:n]) == list(range(128, len(b))) and pb["rows"] == 128
    assert pb["slots"][0] % PAGE == 0 and pb["slots"][0] // PAGE not in pages_a
    assert all(int(x) // PAGE not in pages_a for x in pb["slots"][:n]) and all(pb["slots"][n:] == -1)
    own = (len(b) + 1 + PAGE - 1) // PAGE - 2
    assert s.free_pages == free - own
    assert s.prefix_hit_tokens == 128 and s.prefix_query_tokens == 200 + len(b)
    # the same calls with the flag off: nothing is shared
    s = _sched(on=False)
    _run_prefill(s, 1, a)
    s.add(2, len(b), len(b) + 50, b)
    pb = s.schedule()
    assert list(pb["starts"]) == [0] and list(pb["lens"]) == [len(b)]
    assert "block_tables" not in pb and s.cached_pages == 0


# ------------------------------------------------------------------------------------------------
# 2. scheduler: edges
# ------------------------------------------------------------------------------------------------
def test_scheduler_prefix_one_token_is_always_computed():
    a = _ids(128, 2)
    s = _sched()
    _run_prefill(s, 1, a)
    s.finish(1)
    assert s.free_pages == 16 and s.cached_pages == 2
    p = _run_prefill(s, 2, a)
    assert list(p["starts"]) == [64] and list(p["lens"]) == [64]


def test_scheduler_prefix_same_step_duplicates_register_once():
    a = _ids(200, 3)
    s = _sched()
    s.add(1, 200, 250, a)
    s.add(2, 200, 250, a.copy())
    p = s.schedule()
    assert list(p["seq_ids"]) == [1, 2] and list(p["starts"]) == [0, 0]
    assert not set(s.pages(1)) & set(s.pages(2))
    for sid in (1, 2):
        s.mark_computed(sid)
        s.append(sid, 5)
    assert s.cached_pages == 3  # one copy of each of the 3 full pages
    s.finish(1)
    s.finish(2)
    assert s.free_pages == 16 and s.cached_pages == 3
    p = _run_prefill(s, 3, a)
    assert list(p["starts"]) == [192]


def test_scheduler_prefix_eviction_and_page_ownership():
    a, big = _ids(200, 4), _ids(8 * PAGE - 1, 5)
    s = _sched(num_pages=8)
    _run_prefill(s, 1, a)
    s.finish(1)
    assert s.cached_pages == 3 and s.free_pages == 8
    _run_prefill(s, 2, big)  # needs the whole pool: every cached page is evicted
    assert s.free_pages == 0 and sorted(s.pages(2)) == list(range(8))
    assert s.cached_pages == 7  # its own full pages; A's entries are gone
    s.finish(2)
    assert s.free_pages == 8 and s.cached_pages == 7
    p = _run_prefill(s, 3, a)
    assert list(p["starts"]) == [0]
    assert s.cached_pages <= 8
    # two live sequences share exactly the pages the second took as hits
    c = np.concatenate([a[:64], _ids(30, 6)])
    pc = _run_prefill(s, 4, c)
    assert list(pc["starts"]) == [64]
    assert set(s.pages(3)) & set(s.pages(4)) == {s.pages(3)[0]} and s.pages(4)[0] == s.pages(3)[0]
    assert s.cached_pages <= 8
    s.finish(3)
    s.finish(4)
    assert s.free_pages == 8


def test_scheduler_prefix_hash_collision_is_not_a_hit():
    a, other = _ids(200, 7), _ids(200, 8)
    assert not (a[:64] == other[:64]).all()
    s = _sched()
    s._test_set_hash_mask(0)  # every page hashes to 0
    _run_prefill(s, 1, a)
    p = _run_prefill(s, 2, other)
    assert list(p["starts"]) == [0]  # same hash, other ids: computed, never A's pages
    assert not set(s.pages(1)) & set(s.pages(2))
    assert s.cached_pages == 6
    p = _run_prefill(s, 3, np.concatenate([other[:128], a[128:]]))
    assert list(p["starts"]) == [128] and s.pages(3)[:2] == s.pages(2)[:2]
    p = _run_prefill(s, 4, a)  # colliding entries are told apart by their ids and parents
    assert list(p["starts"]) == [192] and s.pages(4)[:3] == s.pages(1)[:3]


def test_scheduler_prefix_preempted_sequence_hits_its_own_pages():
    s = _sched(num_pages=4)
    s.add(1, 63, 1000, _ids(63, 9))
    s.add(2, 63, 1000, _ids(63, 10))
    s.schedule()
    for sid in (1, 2):
        s.mark_computed(sid)
        s.append(sid, 11)
    for _ in range(200):
        d = s.schedule()
        if d["preempted"]:
            break
        for sid in d["seq_ids"]:
            s.mark_computed(sid)
            s.append(sid, 11)
    assert list(d["preempted"]) == [2] and s.num_tokens(2) > 128
    s.finish(1)
    p = s.schedule()
    assert p["kind"] == "prefill" and list(p["seq_ids"]) == [2]
    assert p["starts"][0] >= 64 and p["starts"][0] + p["lens"][0] == s.num_tokens(2)


# ------------------------------------------------------------------------------------------------
# 3. / 5. paged-prefix prefill attention: one case, shared by the CPU reference test and the kernel
# ------------------------------------------------------------------------------------------------
SEGS = [(64, 1), (192, 17), (64, 130), (100, 64)]  # (start, len)
OFFSETS = [0, 128, 256, 512]                        # (the 130-token segment takes 256 rows)
ROWS = 896                                          # rows 640 .. 767: an unlisted segment; then spare rows


def _prefill_case(dev, cache_dtype, H, KVH, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    pages, W = 40, 8
    k_cache, v_cache = sops.alloc_cache(pages, KVH, cache_dtype, dev)
    if cache_dtype == torch.float8_e4m3fn:
        k_cache.copy_(torch.randn(k_cache.shape, generator=g).clamp(-4, 4).to(dev).to(cache_dtype))
        v_cache.copy_(torch.randn(v_cache.shape, generator=g).clamp(-4, 4).to(dev).to(cache_dtype))
    else:
        k_cache.copy_(torch.randn(k_cache.shape, generator=g).to(dev))
        v_cache.copy_(torch.randn(v_cache.shape, generator=g).to(dev))
    perm = torch.randperm(pages, generator=g).tolist()
    tables = torch.zeros(len(SEGS), W, dtype=torch.int32)
    nxt = 0
    for s, (start, n) in enumerate(SEGS):
        need = (start + n + PAGE - 1) // PAGE
        ids = perm[nxt : nxt + need]
        nxt += need
        if s == 1:
            ids[0] = int(tables[0, 0])  # the first two segments share their first page
        tables[s, :need] = torch.tensor(ids, dtype=torch.int32)
    qkv = torch.randn(ROWS, (H + 2 * KVH) * 128, generator=g).to(dev)
    i32 = dict(dtype=torch.int32, device=dev)
    return dict(qkv=qkv, k_cache=k_cache, v_cache=v_cache, tables=tables.to(dev),
                offsets=torch.tensor(OFFSETS, **i32), starts=torch.tensor([s for s, _ in SEGS], **i32),
                lens=torch.tensor([n for _, n in SEGS], **i32))


@pytest.mark.parametrize("H,KVH", [(8, 2), (8, 1), (4, 4)])
def test_paged_prefill_ref_matches_dense_attention(H, KVH):
    c = _prefill_case("cpu", torch.float32, H, KVH)
    out = torch.full((ROWS, H * 128), 1024.0)
    got = sops.paged_prefill(c["qkv"], c["k_cache"], c["v_cache"], c["tables"], c["offsets"], c["starts"], c["lens"],
                             H, KVH, out=out)
    assert got is out
    listed = torch.zeros(ROWS, dtype=torch.bool)
    for s, (start, n) in enumerate(SEGS):
        off = OFFSETS[s]
        listed[off : off + n] = True
        for i in range(n):
            ctx = start + i + 1
            idx = torch.arange(ctx)
            pages = c["tables"][s][idx // PAGE].long()
            k = c["k_cache"][pages, :, idx % PAGE]  # [ctx, KVH, D]
            v = c["v_cache"][pages, :, :, idx % PAGE]
            q = c["qkv"][off + i, : H * 128].view(H, 128)
            kk = k.repeat_interleave(H // KVH, dim=1).transpose(0, 1)
            vv = v.repeat_interleave(H // KVH, dim=1).transpose(0, 1)
            p = torch.softmax(torch.einsum("hd,hnd->hn", q, kk) / math.sqrt(128), -1)
            torch.testing.assert_close(out[off + i].view(H, 128), torch.einsum("hn,hnd->hd", p, vv),
                                       atol=1e-5, rtol=1e-5)
    assert (out[~listed] == 1024.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("cache_dtype", [torch.bfloat16, torch.float8_e4m3fn])
@pytest.mark.parametrize("H,KVH", [(8, 2), (8, 1), (4, 4)])
def test_gpu_paged_prefill_kernel(gpu, H, KVH, cache_dtype):
    """The HIP kernel against the fp32 reference at the paged-decode tolerance; rows outside the
    listed segments (their padding, a fifth segment, spare rows) keep the sentinel."""
    c = _prefill_case("cuda", cache_dtype, H, KVH)
    qkv = c["qkv"].to(torch.bfloat16)
    ks, vs = (0.5, 2.0) if cache_dtype == torch.float8_e4m3fn else (1.0, 1.0)
    want = sops.paged_prefill_ref(qkv, c["k_cache"], c["v_cache"], c["tables"], c["offsets"], c["starts"], c["lens"],
                                  H, KVH, ks, vs)
    listed = torch.zeros(ROWS, dtype=torch.bool, device="cuda")
    for off, (_, n) in zip(OFFSETS, SEGS):
        listed[off : off + n] = True
    for max_len in (None, 130):  # metadata validated and read back by the binding / given by the caller
        out = torch.full((ROWS, H * 128), 1024.0, dtype=torch.bfloat16, device="cuda")
        sops.paged_prefill(qkv, c["k_cache"], c["v_cache"], c["tables"], c["offsets"], c["starts"], c["lens"], H, KVH,
                           out=out, k_scale=ks, v_scale=vs, max_len=max_len)
        err = (out[listed].float() - want[listed]).abs().max().item()
        print(f"paged_prefill H={H} KVH={KVH} {cache_dtype}: max abs err {err:.4g}")
        assert (out[~listed] == 1024.0).all()
        torch.testing.assert_close(out[listed].float(), want[listed], atol=2e-2, rtol=2e-2)


@pytest.mark.gpu
def test_gpu_paged_prefill_rejects_bad_plans(gpu):
    c = _prefill_case("cuda", torch.bfloat16, 8, 2)
    qkv = c["qkv"].to(torch.bfloat16)
    args = (c["k_cache"], c["v_cache"])
    with pytest.raises(RuntimeError, match="block table"):
        sops.paged_prefill(qkv, *args, c["tables"][:, :3].contiguous(), c["offsets"], c["starts"], c["lens"], 8, 2)
    far = c["offsets"].clone()
    far[3] = ROWS - 10
    with pytest.raises(RuntimeError, match="outside"):
        sops.paged_prefill(qkv, *args, c["tables"], far, c["starts"], c["lens"], 8, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("cache_dtype", [torch.bfloat16, torch.float8_e4m3fn])
def test_gpu_paged_decode_and_prefill_agree_on_single_tokens(gpu, cache_dtype):
    """Decode and prefill share one page walk: a one-token segment at position ctx - 1 is the decode
    of that token, bit for bit when decode runs unsplit (measured: max abs difference 0 for both
    cache types; 0.002 with 4 splits).  Contexts: the first key only, exactly one full page, a
    partial fourth page."""
    g = torch.Generator(device="cpu").manual_seed(0)
    dev, H, KVH, pages = "cuda", 8, 2, 12
    fp8 = cache_dtype == torch.float8_e4m3fn
    ks, vs = (0.5, 2.0) if fp8 else (1.0, 1.0)
    k_cache, v_cache = sops.alloc_cache(pages, KVH, cache_dtype, dev)
    for cache in (k_cache, v_cache):
        x = torch.randn(cache.shape, generator=g)
        cache.copy_((x.clamp(-4, 4) if fp8 else x).to(dev).to(cache_dtype))
    tables = torch.randperm(pages, generator=g).view(3, 4).int().to(dev)
    i32 = dict(dtype=torch.int32, device=dev)
    ctx = torch.tensor([1, 64, 200], **i32)
    qkv = torch.randn(3, (H + 2 * KVH) * 128, generator=g).to(dev).to(torch.bfloat16)
    want = sops.paged_decode_ref(qkv, k_cache, v_cache, tables, ctx, H, KVH, ks, vs)
    tol = dict(atol=2e-2, rtol=2e-2)

    pre = sops.paged_prefill(qkv, k_cache, v_cache, tables, torch.tensor([0, 1, 2], **i32), ctx - 1,
                             torch.tensor([1, 1, 1], **i32), H, KVH, k_scale=ks, v_scale=vs)
    torch.testing.assert_close(pre.float(), want, **tol)
    one = sops.DecodeWorkspace(3, H, KVH, 4, dev)
    one.nsplit, one.pps = 1, 4
    split = sops.DecodeWorkspace(3, H, KVH, 4, dev)
    assert split.nsplit > 1
    for name, ws in (("nsplit=1", one), (f"nsplit={split.nsplit}", split)):
        dec = sops.paged_decode(qkv, k_cache, v_cache, tables, ctx, H, KVH, ws=ws, k_scale=ks, v_scale=vs)
        diff = (dec.float() - pre.float()).abs().max().item()
        print(f"paged decode ({name}) vs prefill, {cache_dtype}: max abs diff {diff:.4g}")
        torch.testing.assert_close(dec.float(), want, **tol)
        torch.testing.assert_close(dec.float(), pre.float(), **tol)
        if ws is one:  # the same instruction sequence per column (the splits' combine reorders the sums)
            assert torch.equal(dec, pre)


# ------------------------------------------------------------------------------------------------
# 4. engine on the CPU
# ------------------------------------------------------------------------------------------------
def _two_wave_prompts():
    rng = np.random.default_rng(11)
    shared = rng.integers(1, 1000, size=128).tolist()
    return [shared + rng.integers(1, 1000, size=n).tolist() for n in (5, 18, 31, 44, 57, 70)]


def _two_waves(eng, prompts, sp):
    first = eng.generate(prompts[:3], sp)
    return first + eng.generate(prompts[3:], sp)


def test_engine_prefix_caching_keeps_greedy_outputs():
    torch.manual_seed(0)
    kw = dict(device="cpu", max_model_len=256, max_batch=8, num_pages=64)
    prompts = _two_wave_prompts()
    sp = SamplingParams(max_tokens=20, temperature=0, ignore_eos=True)
    off = LLMEngine.from_model("llama-tiny", **kw)
    on = LLMEngine.from_model("llama-tiny", enable_prefix_caching=True, **kw)
    assert "prefix_hit_tokens" not in off.stats and "block_tables" not in off.sched.schedule()
    want = [r.output_ids for r in _two_waves(off, prompts, sp)]
    got = _two_waves(on, prompts, sp)
    assert [r.output_ids for r in got] == want and all(len(o) == 20 for o in want)
    assert on.stats["prefix_hit_tokens"] >= 3 * 128
    assert [r.cached_tokens for r in got[3:]] == [128, 128, 128]
    assert on.stats["prefix_cached_pages"] == on.sched.cached_pages > 0
    assert on.metrics()["kv_pages_free"] == 64  # cached pages stay evictable: they count as free
    # a follow-up turn (prompt + its own answer) also hits the pages a decode step filled
    turn = prompts[4] + got[4].output_ids  # 185 + 20 tokens: the third page was completed by decode steps
    before = on.sched.prefix_hit_tokens
    nxt = on.generate([turn + [3, 4, 5]], SamplingParams(max_tokens=4, temperature=0, ignore_eos=True))[0]
    assert on.sched.prefix_hit_tokens - before == 192 > (len(prompts[4]) // PAGE) * PAGE
    assert nxt.cached_tokens == 192
    ref = off.generate([turn + [3, 4, 5]], SamplingParams(max_tokens=4, temperature=0, ignore_eos=True))[0]
    assert nxt.output_ids == ref.output_ids


def test_engine_prefix_caching_with_preemption():
    torch.manual_seed(0)
    kw = dict(device="cpu", max_model_len=256, max_batch=8)
    prompts = [[1 + i, 2, 3, 4 + i] * (5 + i) for i in range(4)]
    sp = SamplingParams(max_tokens=60, temperature=0, ignore_eos=True)
    big = LLMEngine.from_model("llama-tiny", num_pages=64, **kw).generate(prompts, sp)
    small_eng = LLMEngine.from_model("llama-tiny", num_pages=5, enable_prefix_caching=True, **kw)
    small = small_eng.generate(prompts, sp)
    assert small_eng.stats["preemptions"] > 0
    assert [r.output_ids for r in small] == [r.output_ids for r in big]
    assert small_eng.stats["prefix_hit_tokens"] > 0
    assert small_eng.sched.free_pages == 5


def test_engine_prefix_caching_rejects_tensor_parallel():
    with pytest.raises(ValueError, match="prefix caching is not supported with tensor parallel yet"):
        LLMEngine.from_model("llama-tiny", device="cpu", tp_group=object(), enable_prefix_caching=True)

    class TwoRanks:  # what the constructor reads of a tensor-parallel model
        tp, tp_group, tp_rank, device = 2, None, 0, torch.device("cpu")

    with pytest.raises(ValueError, match="prefix caching is not supported with tensor parallel yet"):
        LLMEngine(TwoRanks(), enable_prefix_caching=True)


def test_api_reports_cached_tokens_and_metrics():
    from fastapi.testclient import TestClient

    from dstack_amd.serving.server import create_app

    eng = LLMEngine.from_model("llama-tiny", device="cpu", max_model_len=256, max_batch=8, num_pages=32,
                               enable_prefix_caching=True)
    prompt = _two_wave_prompts()[1]  # 146 tokens
    body = {"model": "llama-tiny", "prompt": prompt, "max_tokens": 3, "temperature": 0, "ignore_eos": True}
    with TestClient(create_app(eng, served_model_name="llama-tiny")) as api:
        first = api.post("/v1/completions", json=body).json()
        assert first["usage"]["prompt_tokens_details"] == {"cached_tokens": 0}
        again = api.post("/v1/completions", json=body).json()
        assert again["usage"]["prompt_tokens"] == len(prompt)
        assert again["usage"]["prompt_tokens_details"] == {"cached_tokens": 128}
        assert again["choices"][0]["text"] == first["choices"][0]["text"]
        chat = api.post("/v1/chat/completions", json={"model": "llama-tiny", "max_tokens": 2, "temperature": 0,
                                                      "messages": [{"role": "user", "content": "hi"}]}).json()
        assert chat["usage"]["prompt_tokens_details"] == {"cached_tokens": 0}
        m = api.get("/metrics").text
    assert "dstack_serving_prefix_cache_hit_tokens_total 128" in m
    assert f"dstack_serving_prefix_cache_query_tokens_total {2 * len(prompt) + chat['usage']['prompt_tokens']}" in m
    assert "dstack_serving_prefix_cached_pages 2" in m


# ------------------------------------------------------------------------------------------------
# 6. / 7. model and engine on the GPU
# ------------------------------------------------------------------------------------------------
def _gpu_model(kv):
    m = ServingLlama(load_spec("llama-tiny"), "cuda", max_model_len=512, kv_cache_dtype=kv)
    m.init_random(0)
    m.allocate_kv(16)
    return m


def _prefill_rows(dev, toks, start, pages):
    """(tokens, positions, slots) of one 128-row-aligned segment holding toks[start:] at its positions"""
    n = len(toks) - start
    rows = (n + 127) // 128 * 128
    t = torch.zeros(rows, dtype=torch.int64, device=dev)
    t[:n] = torch.tensor(toks[start:], device=dev)
    pos = torch.zeros(rows, dtype=torch.int32, device=dev)
    pos[:n] = torch.arange(start, len(toks), dtype=torch.int32, device=dev)
    slots = torch.full((rows,), -1, dtype=torch.int32, device=dev)
    p = torch.arange(start, len(toks))
    slots[:n] = (torch.tensor(pages)[p // PAGE] * PAGE + p % PAGE).int().to(dev)
    return t, pos, slots


@pytest.mark.gpu
def test_gpu_model_prefill_over_cached_prefix(gpu):
    """Logits of a 200-token prompt: full prefill vs prefill of tokens 128.. over the first 128
    tokens' KV left in the same pages by an earlier prefill of that prefix."""
    toks = np.random.default_rng(5).integers(1, 1000, size=200).tolist()
    pages = [9, 3, 12, 6]
    table = torch.tensor([pages + [0] * 4], dtype=torch.int32, device=gpu)
    res = {}
    for kv in ("auto", "fp8"):
        m = _gpu_model(kv)
        full = m.prefill(*_prefill_rows(gpu, toks, 0, pages), [0], [200]).float()
        for kc, vc in zip(m.k_cache, m.v_cache):
            kc.zero_()
            vc.zero_()
        m.prefill(*_prefill_rows(gpu, toks[:128], 0, pages), [0], [128])
        part = m.prefill(*_prefill_rows(gpu, toks, 128, pages), [0], [72], starts=[128], block_tables=table).float()
        res[kv] = (full, part)
    full, part = res["auto"]
    band = 0.02 * (full.max() - full.min()).item()
    diff = (part - full).abs().max().item()
    print(f"bf16 cache: max |logit diff| {diff:.4g}, band {band:.4g}")
    assert diff <= band
    f8 = res["fp8"][1]
    assert torch.isfinite(f8).all()
    assert full[0, f8.argmax()] >= full.max() - band


@pytest.mark.gpu
def test_gpu_engine_prefix_caching_with_graphs(gpu):
    kw = dict(device="cuda", max_model_len=256, max_batch=8, num_pages=64)
    prompts = _two_wave_prompts()
    sp = SamplingParams(max_tokens=20, temperature=0, ignore_eos=True)
    on = LLMEngine.from_model("llama-tiny", enable_prefix_caching=True, **kw)
    on.capture_graphs()
    assert on._graphs
    got = _two_waves(on, prompts, sp)
    assert all(r.finished and len(r.output_ids) == 20 for r in got)
    assert on.stats["prefix_hit_tokens"] >= 3 * 128
    assert on.metrics()["kv_pages_free"] == on.metrics()["kv_pages_total"] == 64
    off = LLMEngine.from_model("llama-tiny", **kw)
    outs = _two_waves(off, prompts, sp)
    assert all(r.finished and len(r.output_ids) == 20 for r in outs)
    assert "prefix_hit_tokens" not in off.stats
