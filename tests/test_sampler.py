"""Truncated sampling (top-k / top-p / min-p) and top-N log-probabilities: the references in
``dstack_amd.ops.serving``, the engine and the HTTP API on the CPU, and the HIP kernels of
``csrc/sampler.hip`` against the references on the GPU."""

import json
import math

import pytest
import torch

from dstack_amd.ops import serving as sops
from dstack_amd.serving.engine import LLMEngine, SamplingParams, _filter_top_k_top_p

NEG = float("-inf")


def _f32(*v):
    return torch.tensor(v, dtype=torch.float32)


def _i32(*v):
    return torch.tensor(v, dtype=torch.int32)


# ------------------------------------------------------------------------------------------------
# references (CPU)
# ------------------------------------------------------------------------------------------------
def _tie_free_rows(rows, V, seed):
    """bf16 rows without repeated values: a random permutation of V distinct bf16 values."""
    g = torch.Generator().manual_seed(seed)
    pool = torch.unique((torch.randn(64 * V + 4096, generator=g) * 4).to(torch.bfloat16).float())
    assert pool.numel() >= V
    out = torch.empty(rows, V)
    for r in range(rows):
        out[r] = pool[torch.randperm(pool.numel(), generator=g)[:V]]
    return out.to(torch.bfloat16)


def _brute_force_tau(row, T, k, p, min_p):
    """The smallest kept logit of a tie-free row by a plain descending sort (fp64)."""
    x = row.double()
    srt = torch.sort(x, descending=True).values
    z = srt / T if T > 0 else srt
    n = k if 0 < k < x.numel() else x.numel()
    tau = [srt[n - 1]] if 0 < k < x.numel() else []
    if p < 1:
        w = torch.exp(z[:n] - z[0])
        before = w.cumsum(0) - w
        tau.append(srt[:n][before <= p * w.sum()][-1])
    if min_p > 0:
        tau.append(srt[z >= z[0] + math.log(min_p)][-1])
    return max(tau).item() if tau else NEG


@pytest.mark.parametrize("V", [8, 1000, 2500])  # (N(0, 16) rounds to ~3000 distinct bf16 values)
def test_threshold_ref_matches_brute_force_on_tie_free_rows(V):
    cases = [(1.0, 0, 1.0, 0.0), (0.7, 5, 1.0, 0.0), (1.3, 0, 0.9, 0.0), (0.8, 50, 0.5, 0.0), (1.0, 0, 1.0, 0.1),
             (0.0, 3, 0.8, 0.02), (1.0, 1, 1.0, 0.0), (1.0, V, 1.0, 0.0), (0.9, 0, 0.0, 0.0)]
    logits = _tie_free_rows(len(cases), V, seed=V)
    T, k, p, mp = (list(c) for c in zip(*cases))
    tau = sops.sample_threshold_ref(logits, _f32(*T), _i32(*k), _f32(*p), _f32(*mp))
    want = [_brute_force_tau(logits[r].float(), *cases[r]) for r in range(len(cases))]
    assert tau.tolist() == want
    assert tau[0] == NEG and tau[7] == NEG  # nothing asked for; k >= V is a no-op
    assert tau[6] == logits[6].float().max() and tau[8] == logits[8].float().max()


def test_threshold_ref_keeps_what_the_python_filter_keeps():
    """On tie-free rows the kept set is the one ``_filter_top_k_top_p`` leaves finite."""
    class R:
        def __init__(self, T, k, p):
            self.params = SamplingParams(top_k=k, top_p=p, temperature=T)

    cases = [(1.0, 4, 1.0), (0.7, 0, 0.9), (1.2, 40, 0.6), (0.0, 7, 0.95)]
    logits = _tie_free_rows(len(cases), 1000, seed=5).float()
    T, k, p = (list(c) for c in zip(*cases))
    tau = sops.sample_threshold_ref(logits, _f32(*T), _i32(*k), _f32(*p), torch.zeros(len(cases)))
    old = _filter_top_k_top_p(logits, [R(*c) for c in cases])
    assert torch.equal(logits >= tau[:, None], torch.isfinite(old))


def test_threshold_ref_ties_and_masked_logits():
    one = torch.ones(4)
    eq = torch.full((1, 16), 1.5)
    # all-equal logits: every rule keeps everything
    for k, p, mp in [(3, 1.0, 0.0), (0, 0.1, 0.0), (0, 1.0, 1.0), (2, 0.5, 0.5)]:
        assert sops.sample_threshold_ref(eq, one[:1], _i32(k), _f32(p), _f32(mp)).tolist() == [1.5]
    # a tie straddling k keeps the whole tie; -inf is never counted or kept; -0 equals +0
    x = torch.tensor([[3.0, 2.0, 2.0, 2.0, 1.0, NEG],
                      [NEG, 5.0, NEG, 4.0, 4.0, 1.0],
                      [0.0, -0.0, -1.0, 0.0, -2.0, -3.0],
                      [NEG, NEG, NEG, NEG, NEG, NEG]])
    tau = sops.sample_threshold_ref(x, one, _i32(2, 3, 1, 2), torch.ones(4), torch.zeros(4))
    assert tau.tolist() == [2.0, 4.0, 0.0, NEG]
    # top-p on the survivors of top-k: k = 3 leaves 0.5 / 0.25 / 0.15 of total 0.9, so p = 0.55 allows
    # 0.495 above a kept value (0.25 has 0.5 above it: dropped; kept without top-k), p = 0.6 allows 0.54
    x = torch.log(torch.tensor([[0.5, 0.25, 0.15, 0.1]])).repeat(3, 1)
    tau = sops.sample_threshold_ref(x, torch.ones(3), _i32(3, 0, 3), _f32(0.55, 0.55, 0.6), torch.zeros(3))
    assert tau.tolist() == [x[0, 0].item(), x[0, 1].item(), x[0, 1].item()]
    # a tie at the top-p boundary stays whole: 0.7 lies above both 0.15s
    x = torch.log(torch.tensor([[0.5, 0.15, 0.2, 0.15]]))
    assert sops.sample_threshold_ref(x, torch.ones(1), _i32(0), _f32(0.8), torch.zeros(1)).tolist() == [x[0, 1].item()]


def test_top_logprobs_ref_orders_by_value_then_id():
    x = torch.tensor([[1.0, 3.0, 2.0, 3.0, NEG, 2.0, 0.5], [1.0, 3.0, 2.0, 3.0, NEG, 2.0, 0.5]])
    tau = _f32(NEG, 2.0)
    ids, lps = sops.top_logprobs_ref(x, _f32(1.0, 0.5), tau, _i32(3, 20))
    assert ids[0].tolist()[:4] == [1, 3, 2, -1]
    assert ids[1].tolist()[:5] == [1, 3, 2, 5, -1]  # only the kept set {x >= 2}; shorter than N
    torch.testing.assert_close(lps[0, :3], torch.log_softmax(x[0], -1)[[1, 3, 2]])
    kept = torch.tensor([3.0, 3.0, 2.0, 2.0]) / 0.5
    torch.testing.assert_close(lps[1, :4], torch.log_softmax(kept, -1))
    assert torch.isinf(lps[1, 4:]).all()


def test_sample_filtered_cpu_without_filters_is_sample():
    torch.manual_seed(0)
    x = torch.randn(5, 300)
    t, seeds, steps = _f32(0.0, 0.7, 1.0, 1.3, 0.0), torch.arange(5), torch.arange(5, dtype=torch.int32)
    tok, lp = sops.sample(x, t, seeds, steps)
    ftok, flp, ids, tlp = sops.sample_filtered(x, t, seeds, steps, torch.zeros(5, dtype=torch.int32), torch.ones(5),
                                               torch.zeros(5))
    assert torch.equal(tok, ftok) and torch.equal(lp, flp) and ids is None and tlp is None


# ------------------------------------------------------------------------------------------------
# engine and API (CPU)
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine():
    return LLMEngine.from_model("llama-tiny", device="cpu", max_model_len=256, max_batch=8, num_pages=32)


PROMPTS = [[1, 5, 9, 33, 7], [1, 300, 301, 302, 17, 4]]


def test_engine_top_k_1_and_min_p_1_are_greedy(engine):
    greedy = [r.output_ids for r in engine.generate(PROMPTS, SamplingParams(max_tokens=8, temperature=0,
                                                                            ignore_eos=True))]
    for kw in (dict(top_k=1), dict(min_p=1.0)):
        got = engine.generate(PROMPTS, SamplingParams(max_tokens=8, temperature=0.9, ignore_eos=True, seed=3, **kw))
        assert [r.output_ids for r in got] == greedy, kw
        assert all(lp == 0.0 for r in got for lp in r.logprobs)  # one kept token: probability 1


def test_engine_top_logprobs(engine):
    sp = SamplingParams(max_tokens=6, temperature=0.8, top_p=0.95, top_logprobs=5, seed=11, ignore_eos=True)
    plain = SamplingParams(max_tokens=6, temperature=0.8, top_p=0.95, seed=11, ignore_eos=True)
    a, b = engine.generate([PROMPTS[0], PROMPTS[0]], [sp, plain])
    assert a.output_ids == b.output_ids and b.top_logprobs == []  # asking for alternatives changes no draw
    assert len(a.top_logprobs) == len(a.output_ids) == 6
    for tok, lp, top in zip(a.output_ids, a.logprobs, a.top_logprobs):
        assert 1 <= len(top) <= 5
        lps = [v for _, v in top]
        assert lps == sorted(lps, reverse=True) and all(math.isfinite(v) and v <= 0 for v in lps)
        alts = dict(top)
        if tok in alts:
            assert alts[tok] == pytest.approx(lp, abs=1e-5)
        else:
            assert lp <= lps[-1] + 1e-6
    # greedy: the chosen token is the first alternative, with the same log-probability
    g = engine.generate([PROMPTS[1]], SamplingParams(max_tokens=4, temperature=0, top_logprobs=3, ignore_eos=True))[0]
    for tok, lp, top in zip(g.output_ids, g.logprobs, g.top_logprobs):
        assert len(top) == 3 and top[0][0] == tok and top[0][1] == pytest.approx(lp, abs=1e-5)


def test_engine_rejects_bad_sampling_params(engine):
    for kw in (dict(min_p=-0.1), dict(min_p=1.5), dict(top_logprobs=-1), dict(top_logprobs=21)):
        with pytest.raises(ValueError):
            engine.add_request([1, 2, 3], SamplingParams(**kw))
    assert not engine.has_work()


@pytest.fixture(scope="module")
def api():
    from fastapi.testclient import TestClient

    from dstack_amd.serving.server import create_app

    eng = LLMEngine.from_model("llama-tiny", device="cpu", max_model_len=256, max_batch=8, num_pages=32)
    with TestClient(create_app(eng, served_model_name="llama-tiny")) as c:
        yield c


def test_api_completions_top_logprobs(api):
    req = {"model": "llama-tiny", "prompt": "The quick brown", "max_tokens": 4, "temperature": 0, "ignore_eos": True}
    r = api.post("/v1/completions", json=dict(req, logprobs=3))
    assert r.status_code == 200, r.text
    lp = r.json()["choices"][0]["logprobs"]
    assert len(lp["tokens"]) == len(lp["token_logprobs"]) == len(lp["top_logprobs"]) == 4
    plain = api.post("/v1/completions", json=req).json()
    text = r.json()["choices"][0]["text"]
    assert text and text == plain["choices"][0]["text"] == "".join(lp["tokens"])  # alternatives change no text
    assert r.json()["usage"] == plain["usage"]
    for tok, v, top in zip(lp["tokens"], lp["token_logprobs"], lp["top_logprobs"]):
        assert 1 <= len(top) <= 3 and all(isinstance(s, str) and x <= 0 for s, x in top.items())
        assert max(top.values()) == pytest.approx(v, abs=1e-5)  # greedy: the chosen token leads
        assert top.get(tok, v) == pytest.approx(v, abs=1e-5)
    # logprobs without a count: the chosen token's only, as before
    r = api.post("/v1/completions", json={"model": "llama-tiny", "prompt": [1, 2, 3], "max_tokens": 2, "logprobs": 0,
                                          "temperature": 0})
    assert "top_logprobs" not in r.json()["choices"][0]["logprobs"]


def _check_chat_entries(entries, n_top):
    for e in entries:
        assert set(e) == {"token", "logprob", "bytes", "top_logprobs"}
        assert e["bytes"] == list(e["token"].encode("utf-8")) and e["logprob"] <= 0
        assert 1 <= len(e["top_logprobs"]) <= n_top
        for t in e["top_logprobs"]:
            assert set(t) == {"token", "logprob", "bytes"}
        lps = [t["logprob"] for t in e["top_logprobs"]]
        assert lps == sorted(lps, reverse=True)


def test_api_chat_logprobs_streamed_and_not(api):
    body = {"model": "llama-tiny", "max_tokens": 5, "temperature": 0.7, "seed": 5, "min_p": 0.01, "logprobs": True,
            "top_logprobs": 2, "ignore_eos": True, "messages": [{"role": "user", "content": "hi"}]}
    r = api.post("/v1/chat/completions", json=body)
    assert r.status_code == 200, r.text
    entries = r.json()["choices"][0]["logprobs"]["content"]
    assert len(entries) == r.json()["usage"]["completion_tokens"] == 5
    _check_chat_entries(entries, 2)
    content = r.json()["choices"][0]["message"]["content"]
    plain = api.post("/v1/chat/completions", json=dict(body, logprobs=False, top_logprobs=None)).json()
    assert content and content == plain["choices"][0]["message"]["content"]  # the same text with and without
    with api.stream("POST", "/v1/chat/completions", json=dict(body, stream=True)) as s:
        assert s.status_code == 200
        lines = [ln for ln in s.iter_lines() if ln.startswith("data: ")]
    chunks = [json.loads(ln[6:]) for ln in lines[:-1]]
    assert "logprobs" not in chunks[0]["choices"][0]  # the role chunk
    streamed = [e for c in chunks[1:] for e in c["choices"][0]["logprobs"]["content"]]
    assert streamed == entries  # same seed: the same tokens, each entry exactly once
    assert "".join(c["choices"][0]["delta"].get("content", "") for c in chunks) == content
    # without logprobs the responses carry none
    r = api.post("/v1/chat/completions", json=dict(body, logprobs=False, top_logprobs=None))
    assert "logprobs" not in r.json()["choices"][0]


def test_api_rejects_bad_sampling_values(api):
    chat = {"model": "llama-tiny", "max_tokens": 2, "messages": [{"role": "user", "content": "hi"}]}
    for extra in (dict(min_p=2), dict(min_p=-0.5), dict(min_p="x"), dict(logprobs=True, top_logprobs=21),
                  dict(logprobs=True, top_logprobs=-1), dict(top_logprobs=2)):
        r = api.post("/v1/chat/completions", json=dict(chat, **extra))
        assert r.status_code == 400, (extra, r.text)
        assert r.json()["error"]["type"] == "invalid_request_error"
    for extra in (dict(min_p=2), dict(logprobs=21), dict(logprobs=-1), dict(logprobs=1.5)):
        r = api.post("/v1/completions", json=dict(model="llama-tiny", prompt="x", max_tokens=2, **extra))
        assert r.status_code == 400, (extra, r.text)
    m = api.get("/metrics").text  # nothing was admitted
    assert "dstack_serving_running 0" in m and "dstack_serving_waiting 0" in m


# ------------------------------------------------------------------------------------------------
# GPU: csrc/sampler.hip against the references
# ------------------------------------------------------------------------------------------------
def _cum_midpoint(row, T, k, lo_frac):
    """A top-p value for ``row`` that no rounding can move across a boundary: the midpoint of two
    adjacent cumulative masses of the fp64 reference (over the row's distinct values, survivors of
    top-k) that lie at least 1e-4 of the total apart -- the first such pair at or after the fraction
    ``lo_frac`` of the distinct values.  The kernel's fp32 exp and fixed-point sums err by ~1e-6."""
    x = row.float()
    v, c = torch.unique(x[x > NEG], return_counts=True)
    v, c = v.flip(0), c.flip(0)
    if 0 < k < row.numel():
        n = int(((c.cumsum(0) - c) < k).sum())
        v, c = v[:n], c[:n]
    inv_t = (1.0 / torch.tensor(T, dtype=torch.float32)) if T > 0 else torch.tensor(1.0)
    z = (v * inv_t).double()
    w = torch.exp(z - z[0]) * c
    cum = torch.cat([torch.zeros(1, dtype=torch.float64), w.cumsum(0)]) / w.sum()  # mass above value i, then 1
    gaps = cum[1:] - cum[:-1]
    start = int(lo_frac * gaps.numel())
    wide = (gaps[start:] >= 1e-4).nonzero()
    i = start + int(wide[0]) if wide.numel() else int((gaps >= 1e-4).nonzero()[-1])
    assert gaps[i] >= 1e-4
    return float((cum[i] + cum[i + 1]) / 2)


def _min_p_midpoint(row, T, target):
    """A min-p value for ``row`` near ``target`` that no rounding can move across a boundary:
    ``ln(min_p)`` is the midpoint of two adjacent distinct values of ``z - zmax`` that lie at least
    1e-3 apart (the first such pair at or below ``ln(target)``, else the last one above it).  The
    kernel's fp32 ``zmax + ln(min_p)`` and the fp32 rounding of min_p itself err by ~1e-6."""
    x = row.float()
    v = torch.unique(x[x > NEG]).flip(0)
    inv_t = (1.0 / torch.tensor(T, dtype=torch.float32)) if T > 0 else torch.tensor(1.0)
    d = (v * inv_t).double()
    d = d - d[0]
    wide = (d[:-1] - d[1:]) >= 1e-3  # pair (i, i + 1)
    below = wide & (d[1:] < math.log(target))
    i = int(below.nonzero()[0]) if below.any() else int(wide.nonzero()[-1])
    return math.exp(float(d[i] + d[i + 1]) / 2)


KINDS = [6, 0, 3, 10, 1, 2, 4, 5, 7, 8, 9]  # (so that R = 1 and R = 3 take the hardest rows)


def _mixed_case(R, V, dev, seed):
    """Rows of a column slice of a wider tensor (odd row stride, unaligned rows) that mix signs, +-0,
    -inf, ties across the k boundary, k = 1, k >= V, a top-p that keeps only the maximum, min-p
    alone, all three rules together and untouched rows."""
    g = torch.Generator().manual_seed(seed)
    wide = (torch.randn(R, V + 5, generator=g) * 3).to(torch.bfloat16)
    x = wide[:, 3 : 3 + V]
    T, k, p, mp = [1.0] * R, [0] * R, [1.0] * R, [0.0] * R
    for r in range(R):
        kind = KINDS[r % len(KINDS)]
        if V >= 8:
            x[r, torch.randperm(V, generator=g)[: max(1, V // 50)]] = NEG
            x[r, 1], x[r, V - 2] = 0.0, -0.0
        T[r] = [1.0, 0.7, 1.5, 0.0][r % 4]
        if kind == 0:    # a tie group across the k boundary: k lands inside five equal maxima
            top = x[r].float().max().item() + 1.0
            x[r, torch.randperm(V, generator=g)[: min(5, V)]] = top
            k[r] = 3
        elif kind == 1:
            k[r] = 1
        elif kind == 2:
            k[r] = V + (r % 2)
        elif kind == 3:  # keeps only the maximum
            p[r] = _cum_midpoint(x[r], T[r], 0, 0.0)
        elif kind == 4:
            mp[r] = _min_p_midpoint(x[r], T[r], 0.05)
        elif kind == 5:  # (ln 1 = 0 in any precision: z >= zmax compares one fp32 product with itself)
            mp[r] = 1.0
        elif kind == 6:  # all three
            k[r] = max(2, V // 3)
            p[r] = _cum_midpoint(x[r], T[r], k[r], 0.02)
            mp[r] = _min_p_midpoint(x[r], T[r], 1e-3)
        elif kind == 7:
            p[r] = _cum_midpoint(x[r], T[r], 0, 0.05)
        elif kind == 8:
            k[r] = min(V - 1, 50) if V > 1 else 0
            p[r] = _cum_midpoint(x[r], T[r], k[r], 0.3)
        elif kind == 9:
            k[r] = max(1, V // 2)
        # kind 10: untouched
    wide_d = wide.to(dev)
    return wide_d[:, 3 : 3 + V], _f32(*T).to(dev), _i32(*k).to(dev), _f32(*p).to(dev), _f32(*mp).to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("R", [1, 3, 33])
@pytest.mark.parametrize("V", [8, 1000, 32000, 128256])
def test_gpu_thresholds_are_exact(gpu, R, V):
    x, T, k, p, mp = _mixed_case(R, V, gpu, seed=V + R)
    assert x.stride(0) % 8 != 0
    ref = sops.sample_threshold_ref(x, T, k, p, mp)
    tau = sops.sample_threshold(x, T, k, p, mp)
    print("tau", tau.tolist()[:12], "ref", ref.tolist()[:12])
    assert torch.equal(tau, ref)
    if R >= 11:
        assert tau[3] == NEG and tau[5] == NEG  # untouched; k >= V
        assert torch.isfinite(tau[[0, 1, 2, 4, 6, 7, 8, 9, 10]]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("V", [1000, 128256])
def test_gpu_masked_sampling_matches_sample_on_masked_logits(gpu, V):
    R = 33
    x, T, k, p, mp = _mixed_case(R, V, gpu, seed=7 * V)
    seeds = torch.arange(100, 100 + R, device=gpu, dtype=torch.int64)
    steps = torch.arange(R, device=gpu, dtype=torch.int32)
    n0 = torch.zeros(R, dtype=torch.int32, device=gpu)
    tau = sops.sample_threshold_ref(x, T, k, p, mp)
    masked = x.float().masked_fill(x.float() < tau[:, None], NEG).to(torch.bfloat16)
    want_tok, want_lp = sops.sample(masked, T, seeds, steps)
    tok, lp, ids, lps = sops.sample_filtered(x, T, seeds, steps, k, p, mp, top_n=n0)
    assert torch.equal(tok, want_tok)
    torch.testing.assert_close(lp, want_lp, atol=1e-3, rtol=1e-3)
    assert (x.float().gather(1, tok.long()[:, None]).squeeze(1) >= tau).all()
    assert (ids == -1).all() and torch.isinf(lps).all()  # top_n = 0 rows are not written
    # rows that ask for nothing: exactly what `sample` returns on the raw logits
    raw_tok, raw_lp = sops.sample(x, T, seeds, steps)
    plain = torch.isinf(tau)
    assert plain.sum() >= 4
    assert torch.equal(tok[plain], raw_tok[plain])
    torch.testing.assert_close(lp[plain], raw_lp[plain], atol=1e-3, rtol=1e-3)
    none_tok, none_lp, _, _ = sops.sample_filtered(x, T, seeds, steps, n0, torch.ones_like(p), torch.zeros_like(mp))
    assert torch.equal(none_tok, raw_tok)
    torch.testing.assert_close(none_lp, raw_lp, atol=1e-3, rtol=1e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("V", [8, 1000, 128256])
def test_gpu_top_logprobs_match_reference(gpu, V):
    R = 33
    x, T, k, p, mp = _mixed_case(R, V, gpu, seed=13 * V)
    if V >= 1000:
        x[4] = 2.5            # (k = 1) one value everywhere: 20 ties by ascending id
        x[5, 7:] = -1.0       # (no rule) a long tie at the boundary value after a few leaders
        x[6, 100:140] = 40.0  # (min-p) 40 equal maxima in the middle of the row
    tau = sops.sample_threshold_ref(x, T, k, p, mp)
    n = torch.tensor([(1, 20, 5, 0, 20, 12, 20, 3)[r % 8] for r in range(R)], dtype=torch.int32, device=gpu)
    want_ids, want_lps = sops.top_logprobs_ref(x, T, tau, n)
    ids, lps = sops.top_logprobs(x, T, tau, n)
    print("ids", ids[:3].tolist(), "lps", lps[:3].tolist())
    assert torch.equal(ids, want_ids)
    fin = want_ids >= 0
    torch.testing.assert_close(lps[fin], want_lps[fin], atol=1e-3, rtol=1e-3)
    assert torch.isinf(lps[~fin]).all() and (lps[~fin] < 0).all()
    assert (ids[n == 0] == -1).all()


@pytest.mark.gpu
def test_gpu_truncated_sampling_distribution(gpu):
    n = 4096
    row = [0.0, 1.0, 2.0, -1.0, 1.5, 0.5] + [-3.0] * 10
    x = torch.tensor([row], device=gpu).to(torch.bfloat16).repeat(n, 1)
    T = torch.full((n,), 0.7, device=gpu)
    k = torch.full((n,), 3, dtype=torch.int32, device=gpu)
    tok, lp, _, _ = sops.sample_filtered(x, T, torch.arange(n, device=gpu, dtype=torch.int64),
                                         torch.zeros(n, dtype=torch.int32, device=gpu), k, torch.ones(n, device=gpu),
                                         torch.zeros(n, device=gpu))
    kept = [2, 4, 1]
    assert set(tok.tolist()) <= set(kept)
    q = torch.softmax(torch.tensor([row[i] for i in kept], dtype=torch.float64) / 0.7, -1)
    freq = torch.bincount(tok.long().cpu(), minlength=16)[kept].double() / n
    bound = 5 * torch.sqrt(q * (1 - q) / n)
    print("freq", freq.tolist(), "q", q.tolist(), "bound", bound.tolist())
    assert ((freq - q).abs() <= bound).all()
    want_lp = torch.log(q).float()[torch.tensor([kept.index(t) for t in tok.tolist()])]
    torch.testing.assert_close(lp.cpu(), want_lp, atol=1e-3, rtol=1e-3)


@pytest.mark.gpu
def test_gpu_sampler_is_reproducible(gpu):
    R, V = 33, 128256
    x, T, k, p, mp = _mixed_case(R, V, gpu, seed=99)
    seeds = torch.arange(R, device=gpu, dtype=torch.int64)
    steps = torch.zeros(R, dtype=torch.int32, device=gpu)
    n = torch.full((R,), 20, dtype=torch.int32, device=gpu)
    runs = []
    for _ in range(2):
        tau = sops.sample_threshold(x, T, k, p, mp)
        tok, lp, ids, lps = sops.sample_filtered(x, T, seeds, steps, k, p, mp, top_n=n)
        runs.append((tau, tok, lp, ids, lps))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_gpu_sample_filtered_in_a_graph(gpu):
    R, V = 11, 1000
    x, T, k, p, mp = _mixed_case(R, V, gpu, seed=3)
    x = x.contiguous()
    seeds = torch.arange(R, device=gpu, dtype=torch.int64)
    steps = torch.zeros(R, dtype=torch.int32, device=gpu)
    n = torch.full((R,), 4, dtype=torch.int32, device=gpu)
    out = dict(tokens=torch.zeros(R, dtype=torch.int32, device=gpu), logprobs=torch.zeros(R, device=gpu),
               top_ids=torch.full((R, 20), -1, dtype=torch.int32, device=gpu),
               top_lps=torch.full((R, 20), NEG, device=gpu), tau=torch.zeros(R, device=gpu))
    sops.sample_filtered(x, T, seeds, steps, k, p, mp, top_n=n, **out)  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sops.sample_filtered(x, T, seeds, steps, k, p, mp, top_n=n, **out)
    # other parameters and logits, in place
    x2, T2, k2, p2, mp2 = _mixed_case(R, V, gpu, seed=4)
    x.copy_(x2)
    k.copy_(k2.roll(1))
    p.copy_(torch.where(k2.roll(1) > 0, torch.ones_like(p2), p2))
    mp.copy_(mp2.roll(2))
    n.copy_(torch.arange(R, dtype=torch.int32, device=gpu) % 5)
    for t in (out["top_ids"], out["top_lps"]):
        t.fill_(-1 if t.dtype == torch.int32 else NEG)
    g.replay()
    torch.cuda.synchronize()
    tok, lp, ids, lps = sops.sample_filtered(x, T, seeds, steps, k, p, mp, top_n=n)
    assert torch.equal(out["tau"], sops.sample_threshold(x, T, k, p, mp))
    assert torch.equal(out["tokens"], tok) and torch.equal(out["logprobs"], lp)
    assert torch.equal(out["top_ids"], ids) and torch.equal(out["top_lps"], lps)
    assert (ids[n == 0] == -1).all() and (ids[n > 0, 0] >= 0).all()


@pytest.mark.gpu
def test_gpu_engine_mixed_batch_in_graphs(gpu):
    """One graph-replayed batch holding a greedy, a top-p, a top-k + min-p and a top_logprobs request:
    the greedy request decodes what it decodes alone, the seeded ones reproduce."""
    prompts = [[1, 5, 9, 33, 7, 100, 2, 45, 61], [1, 300, 301, 302], list(range(1, 60)), [1, 7, 7, 7, 12]]
    sps = [SamplingParams(max_tokens=12, temperature=0, ignore_eos=True),
           SamplingParams(max_tokens=12, temperature=0.9, top_p=0.9, seed=1, ignore_eos=True),
           SamplingParams(max_tokens=12, temperature=1.1, top_k=5, min_p=0.05, seed=2, ignore_eos=True),
           SamplingParams(max_tokens=12, temperature=0.8, top_logprobs=4, seed=3, ignore_eos=True)]

    def run(which):
        eng = LLMEngine.from_model("llama-tiny", device="cuda", max_model_len=512, max_batch=8, num_pages=64)
        eng.capture_graphs()
        assert eng._graphs
        return eng.generate([prompts[i] for i in which], [sps[i] for i in which])

    a, b = run(range(4)), run(range(4))
    alone = run([0])[0]
    assert a[0].output_ids == alone.output_ids
    for ra, rb in zip(a, b):
        assert ra.output_ids == rb.output_ids and ra.logprobs == rb.logprobs and ra.top_logprobs == rb.top_logprobs
    assert all(lp <= 1e-6 for r in a for lp in r.logprobs)
    assert a[0].top_logprobs == [] and len(a[3].top_logprobs) == 12
    for tok, lp, top in zip(a[3].output_ids, a[3].logprobs, a[3].top_logprobs):
        assert len(top) == 4 and [v for _, v in top] == sorted((v for _, v in top), reverse=True)
        if tok in dict(top):
            assert dict(top)[tok] == pytest.approx(lp, abs=1e-3)
    # at most 5 kept tokens, each at least min_p times the likeliest: q >= min_p * pmax / (5 * pmax)
    assert all(lp >= math.log(0.05 / 5) - 1e-3 for lp in a[2].logprobs)
