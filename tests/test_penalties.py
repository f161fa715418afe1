"""Presence / frequency / repetition penalties and logit_bias: the reference in
``dstack_amd.ops.serving`` against a per-element loop, the engine's slot and state bookkeeping and
the HTTP API on the CPU, and the HIP kernels of ``csrc/penalties.hip`` against the reference, bit for
bit, on the GPU."""

import numpy as np
import pytest
import torch

from dstack_amd.ops import serving as sops
from dstack_amd.serving.engine import LLMEngine, SamplingParams

NEG = float("-inf")
NB = sops.LOGIT_BIAS_MAX


def _bits(t):
    return t.contiguous().view(torch.int16)


def _state_row(req, V):
    """2 * count(output_ids) + in_prompt, rebuilt from the request."""
    row = torch.zeros(V, dtype=torch.int32)
    row[sorted(set(req.prompt_ids))] = 1
    for t in req.output_ids:
        row[t] += 2
    return row


def _pen_args(slots, V, rows):
    """(state, bias_ids, bias_vals, bias_n), and inert per-row (slot, rep, inv_rep, freq, pres)."""
    return (sops.alloc_penalty_state(slots, V),
            [torch.full((rows,), -1, dtype=torch.int32), torch.ones(rows), torch.ones(rows), torch.zeros(rows),
             torch.zeros(rows)])


# ------------------------------------------------------------------------------------------------
# reference (CPU)
# ------------------------------------------------------------------------------------------------
def _loop(logits, state, slot, rep, inv_rep, freq, pres, bias_ids, bias_vals, bias_n):
    """The specified steps one element at a time in numpy fp32 scalars."""
    f32 = np.float32
    out = logits.clone()
    with np.errstate(all="ignore"):
        for i, s in enumerate(slot.tolist()):
            if s < 0:
                continue
            r, ir, f, p = (f32(t[i].item()) for t in (rep, inv_rep, freq, pres))
            bias = {int(bias_ids[s, j]): f32(bias_vals[s, j].item()) for j in range(int(bias_n[s]))}
            for v in range(logits.shape[1]):
                x = f32(logits[i, v].float().item())
                st = int(state[s, v])
                c = st >> 1
                if r != f32(1) and st != 0:
                    x = f32(x * ir) if x > 0 else f32(x * r)
                m = f32(f * f32(c))
                x = f32(x - m)
                if c > 0:
                    x = f32(x - p)
                if v in bias:
                    x = f32(x + bias[v])
                out[i, v] = torch.tensor(float(x), dtype=torch.float32).to(out.dtype)
    return out


def test_ref_matches_a_per_element_loop():
    V = 8
    #                 0    1     2     3    4     5     6    7
    x = torch.tensor([[2.5, -1.25, 0.0, NEG, 3.0, -0.0, 0.3, -7.0],
                      [1.0, 2.0, -3.0, 0.5, NEG, 0.0, -0.1, 9.0],
                      [0.7, 0.7, 0.7, -0.7, -0.7, -0.7, NEG, 0.0],
                      [5.0, -5.0, 1.5, 2.5, NEG, 0.0, 0.0, 1.0],
                      [1.1, -1.1, 2.2, -2.2, 3.3, -3.3, 0.0, NEG]]).to(torch.bfloat16)
    (state, bias_ids, bias_vals, bias_n), (slot, rep, inv, freq, pres) = _pen_args(4, V, 5)
    # counts 0, 1 and 5 (state 0 / 2, 3 / 10, 11) and prompt-only tokens (state 1), on +, -, 0 and -inf logits
    state[2] = torch.tensor([2, 10, 1, 3, 0, 11, 1, 2])
    state[0] = torch.tensor([0, 1, 2, 10, 11, 0, 3, 1])
    state[3] = torch.tensor([10, 10, 0, 0, 2, 2, 1, 1])
    state[1] = torch.tensor([3, 0, 0, 1, 1, 2, 10, 11])
    slot[:] = torch.tensor([2, -1, 0, 3, 1])
    rep[:] = torch.tensor([1.3, 1.9, 0.75, 1.0, 1.0])
    freq[:] = torch.tensor([0.7, 1.0, -0.3, 0.0, 1.1])
    pres[:] = torch.tensor([-0.4, 1.0, 0.9, 0.0, 0.6])
    inv = sops.inv_rep_of(rep)
    for s, items in {2: {0: 1.7, 5: -2.3, 4: 100.0}, 3: {7: -100.0, 0: 0.33}, 1: {6: 0.1}}.items():
        sops.penalties_fill(state.clone(), bias_ids, bias_vals, bias_n, s, [], [], items)  # (only the bias list)
    assert bias_n.tolist() == [0, 1, 3, 2] and bias_ids[2, :3].tolist() == [0, 4, 5]
    args = (state, slot, rep, inv, freq, pres, bias_ids, bias_vals, bias_n)
    ref = sops.apply_penalties_ref(x, *args)
    want = _loop(x, *args)
    assert ref.dtype == torch.bfloat16 and torch.equal(_bits(ref), _bits(want))
    assert torch.equal(_bits(ref[1]), _bits(x[1]))  # slot -1
    assert not torch.equal(ref[0], x[0]) and not torch.equal(ref[3], x[3])  # (row 3: bias alone)
    assert (ref[x == NEG] == NEG).all()
    assert ref[0, 4] == 103.0 and ref[3, 7] == -99.0  # an unseen token; a prompt-only one with r = 1: the bias alone
    # the in-place entry point writes only the rows that hold a slot
    y = x.clone()
    assert sops.apply_penalties(y, *args) is y and torch.equal(_bits(y), _bits(ref))


def test_fill_and_update_keep_the_state_definition():
    (state, bias_ids, bias_vals, bias_n), _ = _pen_args(3, 16, 1)
    state.fill_(7)
    sops.penalties_fill(state, bias_ids, bias_vals, bias_n, 1, [3, 3, 5, 9], [5, 5, 2], {9: 1.5, 2: -4})
    want = torch.zeros(16, dtype=torch.int32)
    want[[3, 9]] = 1
    want[5], want[2] = 5, 2
    assert torch.equal(state[1], want) and (state[[0, 2]] == 7).all()
    assert bias_n.tolist() == [0, 2, 0] and bias_ids[1, :2].tolist() == [2, 9] and bias_vals[1, :2].tolist() == [-4, 1.5]
    sops.penalties_update(state, torch.tensor([-1, 1, 2], dtype=torch.int32), torch.tensor([4, 5, 0], dtype=torch.int32))
    want[5] = 7
    assert torch.equal(state[1], want) and (state[0] == 7).all() and state[2, 0] == 9 and (state[2, 1:] == 7).all()
    sops.penalties_fill(state, bias_ids, bias_vals, bias_n, 1, [1], [], None)  # a reused slot starts clean
    assert state[1].sum() == 1 and state[1, 1] == 1 and bias_n[1] == 0


# ------------------------------------------------------------------------------------------------
# engine (CPU)
# ------------------------------------------------------------------------------------------------
KW = dict(device="cpu", max_model_len=256, max_batch=8)
PROMPTS = [[1, 5, 9, 33, 7], [1, 300, 301, 302, 17, 4]]


@pytest.fixture(scope="module")
def engine():
    return LLMEngine.from_model("llama-tiny", num_pages=32, **KW)


def _greedy(**kw):
    return SamplingParams(max_tokens=8, temperature=0, ignore_eos=True, **kw)


def test_engine_logit_bias_forces_and_bans(engine):
    plain = engine.generate(PROMPTS, _greedy())
    forced = engine.generate(PROMPTS, _greedy(logit_bias={777: 100}))
    assert all(r.output_ids == [777] * 8 for r in forced)
    for r, p in zip(engine.generate(PROMPTS, [_greedy(logit_bias={str(p.output_ids[0]): -100}) for p in plain]), plain):
        assert p.output_ids[0] not in r.output_ids and len(r.output_ids) == 8
    assert not engine._pen_slots and len(engine._pen_free) == engine.max_batch  # every slot came back


def test_engine_default_penalties_change_nothing(engine, monkeypatch):
    slots = []
    orig = sops.apply_penalties
    monkeypatch.setattr(sops, "apply_penalties", lambda logits, state, slot, *a: (slots.extend(slot.tolist()),
                                                                                 orig(logits, state, slot, *a))[1])
    sp = dict(max_tokens=8, temperature=0.8, seed=4, ignore_eos=True)
    a = engine.generate(PROMPTS, SamplingParams(**sp))
    b = engine.generate(PROMPTS, SamplingParams(presence_penalty=0.0, frequency_penalty=0.0, repetition_penalty=1.0,
                                                logit_bias={}, **sp))
    assert [r.output_ids for r in a] == [r.output_ids for r in b]
    assert [r.logprobs for r in a] == [r.logprobs for r in b]
    assert slots and all(s == -1 for s in slots)  # a request that asks for nothing never takes a slot


def _watch(eng, monkeypatch):
    """Check at every ``apply_penalties`` call of ``eng`` that each participating request's state row
    is ``2 * count(output_ids) + in_prompt``, that its parameters and bias list are its own, and that
    a row without such a request has slot -1.  Returns the call counters."""
    seen = dict(calls=0, rows=0, readmitted=0)
    cur = {}
    orig_sample, orig_decode, orig_apply = eng._sample, eng._decode, sops.apply_penalties
    V = eng.model.cfg.vocab_size

    def sample(logits, reqs):
        cur["reqs"], cur["prefill"] = reqs, True
        return orig_sample(logits, reqs)

    def decode(plan, reqs):
        cur["reqs"], cur["prefill"] = reqs, False
        return orig_decode(plan, reqs)

    def apply(logits, state, slot, rep, inv_rep, freq, pres, bias_ids, bias_vals, bias_n):
        reqs, sl = cur["reqs"], slot.tolist()
        assert len(sl) >= len(reqs) and all(s == -1 for s in sl[len(reqs):])
        used = [s for s in sl if s >= 0]
        assert len(set(used)) == len(used) and all(s < state.shape[0] for s in used)
        for i, (r, s) in enumerate(zip(reqs, sl)):
            if not r.params.wants_penalties:
                assert s == -1
                continue
            assert s >= 0 and eng._pen_slots[r.id] == s
            assert torch.equal(state[s].cpu(), _state_row(r, V)), (r.id, len(r.output_ids))
            q = r.params
            r32 = np.float32(q.repetition_penalty)
            assert [t[i].item() for t in (rep, inv_rep, freq, pres)] == [float(v) for v in (
                r32, np.float32(1) / r32, np.float32(q.frequency_penalty), np.float32(q.presence_penalty))]
            n = int(bias_n[s])
            assert dict(zip(bias_ids[s, :n].tolist(), bias_vals[s, :n].tolist())) == {
                int(k): float(v) for k, v in (q.logit_bias or {}).items()}
            seen["rows"] += 1
            seen["readmitted"] += bool(cur["prefill"] and r.output_ids)
        seen["calls"] += 1
        return orig_apply(logits, state, slot, rep, inv_rep, freq, pres, bias_ids, bias_vals, bias_n)

    monkeypatch.setattr(eng, "_sample", sample)
    monkeypatch.setattr(eng, "_decode", decode)
    monkeypatch.setattr(sops, "apply_penalties", apply)
    return seen


def _mixed_params(n, max_tokens):
    """Seeded requests; every other one asks for nothing."""
    kinds = [dict(frequency_penalty=0.5, repetition_penalty=1.1), {}, dict(presence_penalty=1.5, logit_bias={7: 3.0}),
             {}, dict(logit_bias={"3": -100, 2: 0.5}), {},
             dict(repetition_penalty=1.5, frequency_penalty=-0.5, logit_bias={9: 100.0}), {}]
    return [SamplingParams(max_tokens=max_tokens, temperature=0.8, seed=10 + i, ignore_eos=True, **kinds[i % len(kinds)])
            for i in range(n)]


def test_engine_state_invariant(monkeypatch):
    eng = LLMEngine.from_model("llama-tiny", num_pages=32, **KW)
    seen = _watch(eng, monkeypatch)
    prompts = [[1 + i, 2, 3, 4 + i] * (2 + i) for i in range(7)]
    out = eng.generate(prompts, _mixed_params(7, 10))
    assert all(len(r.output_ids) == 10 for r in out)
    assert seen["rows"] == 4 * 10 and seen["calls"] >= 10
    assert not eng._pen_slots and sorted(eng._pen_free) == list(range(8))
    # the penalised requests differ from what they decode without, the others do not
    plain = eng.generate(prompts, [SamplingParams(max_tokens=10, temperature=0.8, seed=10 + i, ignore_eos=True)
                                   for i in range(7)])
    assert [r.output_ids for r in out[1::2]] == [r.output_ids for r in plain[1::2]]
    assert [r.logprobs for r in out[1::2]] == [r.logprobs for r in plain[1::2]]
    # (a near-uniform random model: the draws rarely move, the distribution they are reported under does)
    assert all(a.logprobs != b.logprobs for a, b in zip(out[0::2], plain[0::2]))
    assert 3 not in out[4].output_ids and out[6].output_ids == [9] * 10


def test_engine_state_invariant_with_preemption(monkeypatch):
    prompts = [[1 + i, 2, 3, 4 + i] * (5 + i) for i in range(4)]
    sps = _mixed_params(5, 60)[1:]  # (the later arrivals are preempted first: three of them are penalised here)
    sps[2].frequency_penalty = 0.3
    big = LLMEngine.from_model("llama-tiny", num_pages=64, **KW).generate(prompts, sps)
    small_eng = LLMEngine.from_model("llama-tiny", num_pages=5, **KW)
    seen = _watch(small_eng, monkeypatch)
    small = small_eng.generate(prompts, sps)
    assert small_eng.stats["preemptions"] > 0
    assert seen["readmitted"] > 0  # a penalised request came back through prefill with a rebuilt row
    assert [r.output_ids for r in small] == [r.output_ids for r in big]
    assert not small_eng._pen_slots and sorted(small_eng._pen_free) == list(range(8))


def test_engine_reuses_slots(monkeypatch):
    prompts = [[1 + i, 2, 3, 4 + i] * (2 + i % 3) for i in range(7)]
    sps = [SamplingParams(max_tokens=5 + i % 3, temperature=0, ignore_eos=True, frequency_penalty=0.8,
                          repetition_penalty=1.2, logit_bias={i: 2.0}) for i in range(7)]
    want = LLMEngine.from_model("llama-tiny", num_pages=32, **KW).generate(prompts, sps)
    eng = LLMEngine.from_model("llama-tiny", num_pages=32, device="cpu", max_model_len=256, max_batch=2)
    seen = _watch(eng, monkeypatch)
    got = eng.generate(prompts, sps)
    assert all(r.finished and r.finish_reason == "length" for r in got)
    assert [r.output_ids for r in got] == [r.output_ids for r in want]
    assert seen["rows"] == sum(sp.max_tokens for sp in sps)
    assert not eng._pen_slots and sorted(eng._pen_free) == [0, 1]


BAD = [dict(presence_penalty=2.5), dict(presence_penalty=-2.01), dict(frequency_penalty=3), dict(frequency_penalty=-2.5),
       dict(repetition_penalty=0), dict(repetition_penalty=2.5), dict(repetition_penalty=-1),
       dict(logit_bias={str(i): 1 for i in range(NB + 1)}), dict(logit_bias={"1024": 1}), dict(logit_bias={"-1": 1}),
       dict(logit_bias={"5": 101}), dict(logit_bias={"5": -100.5}), dict(logit_bias={"x": 1}), dict(logit_bias=[1, 2])]


def test_engine_rejects_bad_penalties(engine):
    for kw in BAD:
        with pytest.raises(ValueError):
            engine.add_request([1, 2, 3], SamplingParams(**kw))
    assert not engine.has_work()
    for kw in (dict(presence_penalty=2, frequency_penalty=-2, repetition_penalty=2),
               dict(logit_bias={str(i): -100 for i in range(NB)}), dict(logit_bias={1023: 100, "0": -100})):
        assert len(engine.generate([[1, 2, 3]], SamplingParams(max_tokens=2, **kw))[0].output_ids) == 2


# ------------------------------------------------------------------------------------------------
# API (CPU)
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def api():
    from fastapi.testclient import TestClient

    from dstack_amd.serving.server import create_app

    eng = LLMEngine.from_model("llama-tiny", num_pages=32, **KW)
    with TestClient(create_app(eng, served_model_name="llama-tiny")) as c:
        c.engine = eng
        yield c


def test_api_accepts_penalties_on_both_routes(api):
    comp = {"model": "llama-tiny", "prompt": [1, 5, 9], "max_tokens": 6, "temperature": 0, "ignore_eos": True}
    chat = {"model": "llama-tiny", "max_tokens": 6, "temperature": 0, "ignore_eos": True,
            "messages": [{"role": "user", "content": "hi"}]}
    # (the byte tokenizer: token 68 is "A"); string keys, as JSON objects have them
    extra = {"presence_penalty": 0.5, "frequency_penalty": -0.5, "repetition_penalty": 1.2,
             "logit_bias": {"68": 100, "69": -100}}
    for route, body in (("/v1/completions", comp), ("/v1/chat/completions", chat)):
        plain = api.post(route, json=body)
        r = api.post(route, json=dict(body, **extra))
        assert plain.status_code == 200 and r.status_code == 200, r.text
        assert r.json()["usage"]["completion_tokens"] == 6
        text = r.json()["choices"][0]["text"] if "prompt" in body else r.json()["choices"][0]["message"]["content"]
        assert text == "AAAAAA"  # +100 on one token: both routes emit it six times
    r = api.post("/v1/completions", json=dict(comp, logit_bias={"68": 100}, logprobs=0))
    lp = r.json()["choices"][0]["logprobs"]
    assert lp["tokens"] == ["A"] * 6 and all(v > -1e-3 for v in lp["token_logprobs"])  # under the adjusted logits
    assert not api.engine._pen_slots


def test_api_rejects_bad_penalties(api):
    chat = {"model": "llama-tiny", "max_tokens": 2, "messages": [{"role": "user", "content": "hi"}]}
    comp = {"model": "llama-tiny", "prompt": "x", "max_tokens": 2}
    for extra in BAD + [dict(presence_penalty="x"), dict(repetition_penalty=True)]:
        for route, body in (("/v1/chat/completions", chat), ("/v1/completions", comp)):
            r = api.post(route, json=dict(body, **extra))
            assert r.status_code == 400, (route, extra, r.text)
            assert r.json()["error"]["type"] == "invalid_request_error"
    m = api.get("/metrics").text  # nothing was admitted
    assert "dstack_serving_running 0" in m and "dstack_serving_waiting 0" in m


# ------------------------------------------------------------------------------------------------
# GPU: csrc/penalties.hip against the reference
# ------------------------------------------------------------------------------------------------
#        (rep, freq, pres, bias entries); None: slot -1
KINDS = [(1.3, 0.7, -0.4, NB), None, (0.8, 0.0, 0.0, 0), (1.0, -1.5, 0.0, 1), (1.0, 0.0, 0.9, 0), (1.0, 0.0, 0.0, NB),
         (1.7, 0.0, 0.0, 0), (1.0, 0.6, -1.2, 1), None, (0.5, -0.25, 2.0, 7), (2.0, 2.0, 2.0, NB)]


def _kernel_case(R, V, seed):
    """CPU tensors: bf16 logits (a column slice of a wider tensor: odd row stride, unaligned rows)
    with -inf, +-0 and both signs; a state with unseen, prompt-only and generated
    tokens (counts 1 and 5 among them); slots not in row order; rows of every kind in one launch."""
    g = torch.Generator().manual_seed(seed)
    wide = (torch.randn(R, V + 5, generator=g) * 3).to(torch.bfloat16)
    x = wide[:, 3 : 3 + V]
    slots = R + 2
    (state, bias_ids, bias_vals, bias_n), (slot, rep, inv, freq, pres) = _pen_args(slots, V, R)
    u = torch.rand(slots, V, generator=g)
    state[:] = torch.where(u < 0.70, 0, torch.where(u < 0.80, 1, torch.where(u < 0.90, 2, torch.where(u < 0.95, 3, 10))))
    state[:, 0], state[:, V - 1] = 11, 2  # ids 0 and V - 1 carry counts (5 with the prompt, 1 without)
    order = torch.randperm(slots, generator=g).tolist()
    for r in range(R):
        x[r, torch.randperm(V, generator=g)[: max(1, V // 50)]] = NEG
        x[r, 1], x[r, V - 2] = 0.0, -0.0
        kind = KINDS[r % len(KINDS)]
        if kind is None:
            continue
        s = order[r]
        slot[r], rep[r], freq[r], pres[r] = s, kind[0], kind[1], kind[2]
        n = min(kind[3], V)
        if n:
            # ids 0 and V - 1 first (n == 1 alternates), then distinct others, many with nonzero counts
            rest = (torch.randperm(V - 2, generator=g) + 1)[: max(0, n - 2)].tolist()
            ids = ([0, V - 1] + rest)[:n] if n > 1 else [(0, V - 1)[r % 2]]
            vals = ((torch.rand(n, generator=g) * 200 - 100).round(decimals=2)).tolist()
            vals[0] = (100.0, -100.0)[r % 2]
            sops.penalties_fill(state.clone(), bias_ids, bias_vals, bias_n, s, [], [], dict(zip(ids, vals)))
    inv = sops.inv_rep_of(rep)
    return wide, x, (state, slot, rep, inv, freq, pres, bias_ids, bias_vals, bias_n)


@pytest.mark.gpu
@pytest.mark.parametrize("sliced", [False, True], ids=["rows16B", "slice"])
@pytest.mark.parametrize("R", [1, 3, 33])
@pytest.mark.parametrize("V", [8, 1000, 128256])
def test_gpu_apply_penalties_is_bit_exact(gpu, R, V, sliced):
    wide, x, args = _kernel_case(R, V, seed=V + R)
    ref = sops.apply_penalties_ref(x, *args)
    wide_d = wide.clone().to(gpu)
    xd = wide_d[:, 3 : 3 + V] if sliced else torch.empty(R, V, dtype=wide.dtype, device=gpu).copy_(wide_d[:, 3 : 3 + V])
    assert (xd.data_ptr() % 16 == 0 and xd.stride(0) % 8 == 0) != sliced and torch.equal(_bits(xd.cpu()), _bits(x))
    dargs = [a.to(gpu) for a in args]
    keep = [a.clone() for a in dargs]
    assert sops.apply_penalties(xd, *dargs) is xd
    got = xd.cpu()
    bad = (_bits(got) != _bits(ref)).nonzero()
    print("mismatches", bad.shape[0], bad[:8].tolist())
    assert torch.equal(_bits(got), _bits(ref))
    idle = args[1] < 0
    assert torch.equal(_bits(got[idle]), _bits(x[idle]))  # slot -1: bit-identical
    assert (got[x == NEG] == NEG).all()
    if R >= 3:
        assert idle.any() and not torch.equal(_bits(got[~idle]), _bits(x[~idle]))
    if sliced:  # nothing outside the slice was written
        assert torch.equal(_bits(wide_d[:, :3].cpu()), _bits(wide[:, :3]))
        assert torch.equal(_bits(wide_d[:, 3 + V :].cpu()), _bits(wide[:, 3 + V :]))
    for a, b in zip(dargs, keep):  # the state and the parameters are inputs only
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("V", [8, 128256])
def test_gpu_penalties_update(gpu, V):
    R, slots = 33, 40
    g = torch.Generator().manual_seed(V)
    state = torch.randint(0, 12, (slots, V), generator=g, dtype=torch.int32)
    slot = torch.randperm(slots, generator=g)[:R].to(torch.int32)
    slot[[2, 7, 30]] = -1
    tokens = torch.randint(0, V, (R,), generator=g, dtype=torch.int32)
    tokens[0], tokens[1], tokens[2] = 0, V - 1, V - 1
    want = state.clone()
    for s, t in zip(slot.tolist(), tokens.tolist()):
        if s >= 0:
            want[s, t] += 2
    sd = state.clone().to(gpu)
    sops.penalties_update(sd, slot.to(gpu), tokens.to(gpu))
    assert torch.equal(sd.cpu(), want) and (want != state).sum() == R - 3


@pytest.mark.gpu
def test_gpu_penalties_and_sampler_in_a_graph(gpu):
    R, V = 11, 1000
    cases = [_kernel_case(R, V, seed=s) for s in (21, 22, 23)]
    _, x0, a0 = cases[0]
    x = x0.contiguous().to(gpu)
    state, slot, rep, inv, freq, pres, bias_ids, bias_vals, bias_n = (a.to(gpu) for a in a0)
    T = torch.tensor([(0.0, 0.7, 1.0, 1.3)[r % 4] for r in range(R)], device=gpu)
    seeds = torch.arange(R, device=gpu, dtype=torch.int64)
    steps = torch.zeros(R, dtype=torch.int32, device=gpu)
    k = torch.tensor([(0, 5, 0, 50)[r % 4] for r in range(R)], dtype=torch.int32, device=gpu)
    p = torch.tensor([(1.0, 1.0, 0.9, 0.8)[r % 4] for r in range(R)], device=gpu)
    mp = torch.zeros(R, device=gpu)
    tok, lp, tau = torch.zeros(R, dtype=torch.int32, device=gpu), torch.zeros(R, device=gpu), torch.zeros(R, device=gpu)

    def chain():
        sops.apply_penalties(x, state, slot, rep, inv, freq, pres, bias_ids, bias_vals, bias_n)
        sops.sample_filtered(x, T, seeds, steps, k, p, mp, tok, lp, tau=tau)
        sops.penalties_update(state, slot, tok)

    keep = state.clone()
    chain()  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain()
    state.copy_(keep)
    want_state = keep.cpu()
    for step, (_, raw, args) in enumerate(cases):
        # restage: raw logits, slots, parameters and bias lists of this case; the state carries over
        x.copy_(raw)
        for dst, src in zip((slot, rep, inv, freq, pres, bias_ids, bias_vals, bias_n), args[1:]):
            dst.copy_(src)
        steps.fill_(step)
        g.replay()
        torch.cuda.synchronize()
        ref = sops.apply_penalties_ref(raw, want_state, *args[1:])
        assert torch.equal(_bits(x.cpu()), _bits(ref))
        want_tok, want_lp, _, _ = sops.sample_filtered(ref.to(gpu), T, seeds, steps, k, p, mp)
        assert torch.equal(tok, want_tok) and torch.equal(lp, want_lp)
        for s, t in zip(args[1].tolist(), want_tok.tolist()):
            if s >= 0:
                want_state[s, t] += 2
        assert torch.equal(state.cpu(), want_state)
    assert not torch.equal(want_state, keep.cpu())


@pytest.mark.gpu
def test_gpu_engine_penalties_in_graphs(gpu):
    """Seeded requests, half of them with penalties or a bias: graph replay and eager steps give the
    same tokens, and the requests that ask for nothing decode what they decode when nobody asks."""
    prompts = [[1, 5, 9, 33, 7, 100, 2, 45, 61], [1, 300, 301, 302], list(range(1, 60)), [1, 7, 7, 7, 12],
               [2, 4, 6, 8, 10, 12], [9, 9, 9], [3, 1, 4, 1, 5, 9, 2, 6]]
    sps = _mixed_params(7, 12)
    plain = [SamplingParams(max_tokens=12, temperature=0.8, seed=10 + i, ignore_eos=True) for i in range(7)]

    def run(params, use_graphs):
        eng = LLMEngine.from_model("llama-tiny", device="cuda", max_model_len=512, max_batch=8, num_pages=64,
                                   use_graphs=use_graphs)
        eng.capture_graphs()
        assert bool(eng._graphs) == use_graphs
        out = eng.generate(prompts, params)
        assert not eng._pen_slots
        return out

    a, b, c = run(sps, True), run(sps, False), run(plain, True)
    assert [r.output_ids for r in a] == [r.output_ids for r in b]
    assert [r.logprobs for r in a] == [r.logprobs for r in b]
    assert [r.output_ids for r in a[1::2]] == [r.output_ids for r in c[1::2]]
    assert [r.logprobs for r in a[1::2]] == [r.logprobs for r in c[1::2]]
    assert all(ra.logprobs != rc.logprobs for ra, rc in zip(a[0::2], c[0::2]))
    assert 3 not in a[4].output_ids and a[6].output_ids == [9] * 12 and all(len(r.output_ids) == 12 for r in a)
    assert all(lp <= 1e-6 for r in a for lp in r.logprobs)
