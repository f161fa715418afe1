"""The routed expert MLP of a prefill of more than 256 rows (``csrc/moe_prefill.hip``): the plan and the tiled
grouped GEMM against fp64 on exact integer data, the fused SwiGLU epilogue against its steps, the whole MLP
against the 256-row slices it replaces, and the engine's wiring."""

import pytest
import torch

from dstack_amd.ops import reference as ref
from dstack_amd.ops import serving as sops
from dstack_amd.serving.engine import LLMEngine, SamplingParams
from tests.test_moe import _mlp64, _patterns
from tests.test_qwen3_moe import GPU_KW, _gpu_case


def _check_plan(tile_e, pairs, topk_e, alive):
    """Every live pair exactly once, in a tile of its own expert; everything else is -1; a tile has an expert
    exactly when it has a pair."""
    used = pairs >= 0
    assert sorted(pairs[used].tolist()) == torch.nonzero(alive).flatten().tolist()
    assert int(pairs.min()) >= -1 and int(tile_e.min()) >= -1
    assert torch.equal(tile_e[:, None].expand_as(pairs)[used], topk_e.flatten()[pairs[used].long()])
    assert torch.equal(tile_e >= 0, used.any(1))


def test_cpu_mlp_equals_the_reference():
    """Without the kernels every step falls back to plain torch: the plan holds (ragged tiles, a dead row) and the
    MLP is ``ref.moe_mlp`` but for that one's bf16 rounding of the gate/up products: three roundings of 2^-9
    relative on terms that add up to results of order 1, far inside 2e-2."""
    g = torch.Generator().manual_seed(0)
    R, E, k, D, F = 70, 8, 2, 128, 128
    h, router = torch.randn(R, D, generator=g).bfloat16(), torch.randn(E, D, generator=g).bfloat16()
    wgu = (torch.randn(E, 2 * F, D, generator=g) / D ** 0.5).bfloat16()
    wdown = (torch.randn(E, D, F, generator=g) / F ** 0.5).bfloat16()
    live = (torch.arange(R) != 5).int()
    topk_e = ref.moe_route(h, router, live, k)[0]
    tile_e, pairs = sops.moe_prefill_plan(topk_e, live, E)
    assert pairs.shape == (sops.moe_prefill_tiles(R, k, E, 64), 64)
    _check_plan(tile_e, pairs, topk_e, (live > 0).repeat_interleave(k))
    got = sops.moe_prefill_mlp(h, router, wgu, wdown, k, live, sops.MoePrefillWorkspace(E, k, D, F, "cpu", rows=R))
    torch.testing.assert_close(got, ref.moe_mlp(h, router, wgu, wdown, k, live), rtol=2e-2, atol=2e-2)
    assert got[4].any() and not got[5].any()


@pytest.mark.gpu
@pytest.mark.parametrize("N,K", [(128, 128), (384, 192), (256, 768)])
@pytest.mark.parametrize("E,k", [(128, 8), (8, 2)])
@pytest.mark.parametrize("R,tile", [(257, None), (300, None), (1000, None), (128, 128), (129, 128)])
def test_gpu_gemm_and_plan_exact(gpu, R, tile, E, k, N, K):
    """x in {-1, 0, 1}, W in {-1, +1}: every summation order is exact, so the plain epilogue equals the fp64
    product ``x[p // src_div] @ W[topk_e[p]]^T`` in every element of every live pair, gathered per token and
    per pair, and dead rows come out of ``moe_combine`` as exact zeros from a NaN-filled output.  The tile is
    the shape's own (64 pairs, but 128 at R = 1000 with 8 experts) or forced to 128.  "all to the first k"
    gives an expert R pairs: 4 tiles of 64 and one pair, 4 and 44, 15 and 40 or 7 tiles of 128 and 104, one
    full tile of 128, one and one pair; with 128 experts the other patterns leave every tile nearly empty.
    One, three and two weight tiles; two K-steps, three (the double buffer ends on its other half), twelve."""
    g = torch.Generator().manual_seed(R * 1000 + N + E)
    Wc = (torch.randint(0, 2, (E, N, K), generator=g) * 2 - 1).to(torch.bfloat16)
    W = Wc.to(gpu)
    xs = {k: torch.randint(-1, 2, (R, K), generator=g).to(torch.bfloat16),
          1: torch.randint(-1, 2, (R * k, K), generator=g).to(torch.bfloat16)}
    for name, (topk_e, live) in _patterns(R, E, k, g).items():
        topk_e = topk_e.to(torch.int32).contiguous()
        alive = (live > 0).repeat_interleave(k)
        plan = sops.moe_prefill_plan(topk_e.to(gpu), live.to(gpu), E, tile)
        assert plan[1].shape[1] == (tile or sops.moe_prefill_tile(R, k, E)), name
        _check_plan(plan[0].cpu(), plan[1].cpu(), topk_e, alive)
        for src_div, x in xs.items():
            part = sops.moe_prefill_gemm(x.to(gpu), src_div, W, *plan, k)
            want = torch.zeros(R * k, N, dtype=torch.float64)
            for e in range(E):
                mine = torch.nonzero((topk_e.flatten() == e) & alive).flatten()
                want[mine] = x[mine // src_div].double() @ Wc[e].double().t()
            assert torch.equal(part[0].cpu().double()[alive], want[alive]), (name, src_div)
        y = torch.full((R, N), float("nan"), dtype=torch.bfloat16, device=gpu)
        sops.moe_combine(part, torch.ones(R, k, device=gpu), live.to(gpu), out=y)
        assert torch.equal(y.cpu(), want.view(R, k, N).sum(1).to(torch.bfloat16)), name


def _gaussian(gpu, R, seed):
    g = torch.Generator().manual_seed(seed)
    E, k, D, F = 128, 8, 512, 768
    h = torch.randn(R, D, generator=g).to(gpu, torch.bfloat16)
    router = torch.randn(E, D, generator=g).to(gpu, torch.bfloat16)
    wgu = (torch.randn(E, 2 * F, D, generator=g) / D ** 0.5).to(gpu, torch.bfloat16)
    wdown = (torch.randn(E, D, F, generator=g) / F ** 0.5).to(gpu, torch.bfloat16)
    return E, k, D, F, h, router, wgu, wdown


@pytest.mark.gpu
def test_gpu_fused_swiglu_equals_its_steps(gpu):
    """``a`` from the gate/up epilogue has the bits of ``moe_swiglu`` over the plain epilogue's ``part`` for
    every live pair; the dead row's pairs keep the NaN they were filled with."""
    R = 300
    E, k, D, F, h, router, wgu, _ = _gaussian(gpu, R, 2)
    live = torch.ones(R, dtype=torch.int32, device=gpu)
    live[5] = 0
    topk_e = torch.rand(R, E, generator=torch.Generator().manual_seed(3)).argsort(dim=1)[:, :k].to(gpu, torch.int32).contiguous()
    plan = sops.moe_prefill_plan(topk_e, live, E)
    a = torch.full((R * k, F), float("nan"), dtype=torch.bfloat16, device=gpu)
    sops.moe_prefill_gemm_swiglu(h, k, wgu, *plan, k, out=a)
    want = sops.moe_swiglu(sops.moe_prefill_gemm(h, k, wgu, *plan, k), live)
    alive = (live > 0).repeat_interleave(k)
    assert want[alive].any() and torch.equal(a[alive].view(torch.int16), want[alive].view(torch.int16))
    assert a[~alive].isnan().all()


@pytest.mark.gpu
@pytest.mark.parametrize("R", [300, 1000])
def test_gpu_mlp_no_worse_than_the_slices(gpu, R, capsys):
    """Gaussian data, D 512, F 768, 128 experts, top-8: the RMS error of ``moe_prefill_mlp`` against the fp64
    reference is no larger than that of the path it replaces, ``moe_fine_mlp`` over 256-row slices.  Both
    keep fp32 from the accumulators to the one bf16 rounding of ``a`` and of the result, so no margin."""
    E, k, D, F, h, router, wgu, wdown = _gaussian(gpu, R, R)
    live = torch.ones(R, dtype=torch.int32, device=gpu)
    want = _mlp64(h.cpu(), router.cpu(), wgu.cpu(), wdown.cpu(), k)
    got = sops.moe_prefill_mlp(h, router, wgu, wdown, k, live, sops.MoePrefillWorkspace(E, k, D, F, gpu, rows=R))
    ws = sops.MoeWorkspace(E, k, D, F, gpu, fine=True)
    sliced = torch.cat([sops.moe_fine_mlp(h[i : i + 256], router, wgu, wdown, k, live[i : i + 256], ws) for i in range(0, R, 256)])
    err, err_sliced = ((t.cpu().double() - want).pow(2).mean().sqrt().item() for t in (got, sliced))
    with capsys.disabled():
        print(f"\nmoe_prefill_mlp R={R}: rms error {err:.6e}, 256-row slices {err_sliced:.6e}, rms of the result "
              f"{want.pow(2).mean().sqrt().item():.3e}")
    assert err <= err_sliced


@pytest.mark.gpu
def test_gpu_engine_prefills_on_the_tiled_gemm(gpu, tmp_path_factory, monkeypatch):
    """A 300-token prompt (384 rows in 128-row segments) runs ``moe_prefill_mlp`` once per layer; the decode
    kernels' MLP never sees a slice of it."""
    path, _ = _gpu_case(str(tmp_path_factory.getbasetemp() / "qwen3_moe_gpu"))
    prefill, fine, calls = sops.moe_prefill_mlp, sops.moe_fine_mlp, {"prefill": [], "fine": []}
    monkeypatch.setattr(sops, "moe_prefill_mlp", lambda h, *a: calls["prefill"].append(h.shape[0]) or prefill(h, *a))
    monkeypatch.setattr(sops, "moe_fine_mlp", lambda h, *a: calls["fine"].append(h.shape[0]) or fine(h, *a))
    eng = LLMEngine.from_model(path, use_graphs=False, **GPU_KW)
    out = eng.generate([[5 + i % 100 for i in range(300)]], SamplingParams(max_tokens=2, temperature=0, ignore_eos=True))
    assert len(out[0].output_ids) == 2 and calls["prefill"] == [384, 384] and max(calls["fine"], default=0) < 128
