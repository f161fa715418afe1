"""Attention inputs in which every key is individually observable, fp64 references with editable
masks and metadata, a rounding model of the kernels, and a metric that looks at every row.

Used by ``tests/test_attention_keys.py`` for flash attention (``csrc/flash_attn.hip``), paged decode
(``csrc/paged_attn.hip``) and paged-prefix prefill (``csrc/paged_prefill.hip``).

**Needles.**  ``code(j)`` is a 128-vector of +-1 built from two rows of the 64x64 Sylvester
Hadamard matrix: the low half is row ``j % 64``, the high half row ``((j + 32) // 64) % 64``
(unique for j < 4096).  Keys are ``k_j = 2 code(j)`` and a query is ``2 * sum(code(t) for t in
targets)`` with all targets sharing the low code.  Two codes agree in 128, 64 or 0 places (both,
one or no half equal), so in units of ``64 * 4 / sqrt(128) = 22.6`` nats a target scores
``m + 1`` (m targets) and every other key at most ``m``: the reference softmax puts
``>= 1 - 1e-6`` of a row on its targets, ``1 / m`` each, and losing one key, or seeing one key too
many, moves an O(1) part of the row.  Everything is a small integer: exact in bf16, in e4m3 (keys
+-2, stored as +-4 with ``k_scale = 0.5``) and in the fp32 MFMA accumulators.

The high half changes at ``j % 64 == 32`` rather than at 0 so that keys ``i`` and ``i + 1`` share
it across every 64-key tile edge: a *trap* query ``2 (code(i) + code(t))`` with ``t = i + 1`` (or
``t = i + 64``, which shares the low half) then has exactly one best visible key, ``i``, and gives
half of its row to ``t`` the moment ``t`` leaks through the causal mask.  (With the boundary at 0,
key ``64 * (i // 64)`` would tie with ``i`` on the rows ``i % 64 == 63``, the ones that matter.)

**Metric.**  ``rowerr``: per 128-vector (token, head) the L2 error over the reference's L2 norm,
floored at 1e-3 of the largest row norm; the maximum over rows.

**Threshold.**  ``threshold(model_err)`` = min(FACTOR x the error of the rounding model, CAP).  The
model is the fp64 reference with only the roundings the kernels make: the unnormalised P to bf16
before P V (the normaliser sums the unrounded values), O to bf16; backward: delta from the bf16 O,
dS to bf16, P to bf16 for dV, bf16 outputs, and per-query-head dK/dV partials rounded to bf16
before the GQA group sum.  FACTOR covers summation order, the fp32 ``exp2`` and the deferred-max
rescale.  It never comes from a kernel's output.
"""

from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import torch

PAGE, D = 64, 128
SCALE = 1.0 / math.sqrt(D)
BF16, E4M3, F64 = torch.bfloat16, torch.float8_e4m3fn, torch.float64
FACTOR, CAP = 4.0, 0.05
DETECT = 0.25  # what a simulated defect must reach on some row: 5 x CAP


def _hadamard(n: int) -> torch.Tensor:
    h = torch.ones(1, 1, dtype=F64)
    while h.shape[0] < n:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return h


HAD64 = _hadamard(64)


def code(j) -> torch.Tensor:
    """[..., 128] fp64 of +-1 for integer positions ``j`` (any shape)."""
    j = torch.as_tensor(j, dtype=torch.long)
    return torch.cat([HAD64[j % 64], HAD64[((j + 32) // 64) % 64]], -1)


def needle_q(targets: torch.Tensor) -> torch.Tensor:
    """``2 * sum code(t)`` over the last axis of ``targets`` (long; -1 = no target)."""
    keep = (targets >= 0).to(F64).unsqueeze(-1)
    return 2.0 * (code(targets.clamp_min(0)) * keep).sum(-2)


def rb(x: torch.Tensor) -> torch.Tensor:
    """Round to bf16 (through fp32), back in fp64."""
    return x.to(torch.float32).to(BF16).to(F64)


def r8(x: torch.Tensor) -> torch.Tensor:
    """Round to e4m3, back in fp64."""
    return x.to(torch.float32).to(E4M3).to(F64)


def rowerr(got: torch.Tensor, ref: torch.Tensor) -> float:
    g, r = got.to(F64).reshape(-1, D), ref.to(F64).reshape(-1, D)
    rn = r.norm(dim=1)
    return ((g - r).norm(dim=1) / torch.maximum(rn, 1e-3 * rn.max())).max().item()


def threshold(model_err: float) -> float:
    return min(FACTOR * model_err, CAP)


def _softmax_parts(s: torch.Tensor):
    """(e, l, p) of masked scores ``s`` (-inf = masked); a row with no visible key gives zeros."""
    if s.shape[-1] == 0:
        z = s.new_zeros(*s.shape[:-1], 1)
        return s, z, s
    mx = s.amax(-1, keepdim=True)
    mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)
    e = torch.exp(s - mx)
    l = e.sum(-1, keepdim=True)
    return e, l, e / torch.where(l == 0, torch.ones_like(l), l)


# ==================================================================================================
# Flash attention
# ==================================================================================================
# (S, H, KV): G = 8, 7, 2, 1 each at a 4-wave length (S % 256 != 0) and at the 8-wave length 512;
# every case runs causal (its last query head is then the trap head) and not
FLASH_SHAPES = [(128, 28, 4), (128, 8, 8), (384, 8, 1), (384, 6, 3), (512, 8, 1), (512, 28, 4), (512, 6, 3),
                (512, 8, 8), (1152, 8, 1), (1152, 6, 3)]
FLASH_B = 2


def causal_vis(S: int) -> torch.Tensor:
    return torch.ones(S, S, dtype=torch.bool).tril()


def flash_trap_keys(S: int, b: int) -> torch.Tensor:
    """Trap key of every row of the trap head of batch ``b`` (-1: none fits below S): ``i + 1`` on
    half of the rows -- every row before a 64-key tile edge among them in one of the two batches --
    and ``i + 64``, the next tile, on the others and wherever ``i`` and ``i + 1`` share no half."""
    i = torch.arange(S)
    near = ((i + b) % 2 == 1) & (i % 64 != 31)
    t = torch.where(near, i + 1, i + 64)
    t = torch.where((t >= S) & (i % 64 != 31), i + 1, t)
    return torch.where(t < S, t, torch.full_like(t, -1))


@functools.lru_cache(maxsize=None)
def flash_case(S: int, H: int, KV: int, causal: bool, vgrid: bool = False, seed: int = 0):
    """Needle inputs for ``ops.attention``: ``qkv`` [B, S, (H + 2 KV) 128] and ``do`` [B, S, H 128]
    in bf16, ``targets`` [B, H, S, 2] (long, -1 = none), ``trap`` [B, S] (causal: the trap key of
    the last query head's rows, -1 = none; else None).  V is random normal, rounded to bf16 or
    (``vgrid``, for judging gradients) to multiples of 1/8 below 4: the mean of two such values is
    exact in bf16, so the O of a needle row carries no rounding into the backward's delta."""
    B = FLASH_B
    g = torch.Generator().manual_seed(seed)
    i = torch.arange(S).view(1, 1, S)
    h = torch.arange(H).view(1, H, 1)
    b = torch.arange(B).view(B, 1, 1)
    low = i % 64
    mix = i + 5 * h + 3 * b
    if causal:  # the diagonal and a key of an earlier 64-block, the block sweeping with the row
        t0 = i.expand(B, H, S)
        t1 = (mix % (i // 64 + 1)) * 64 + low
    else:       # two different 64-blocks, both sweeping
        nblk = S // 64
        ablk = mix % nblk
        t0 = ablk * 64 + low
        t1 = ((ablk + 1 + (i // 64 + h) % (nblk - 1)) % nblk) * 64 + low
    t1 = torch.where(t1 == t0, torch.full_like(t1, -1), t1)
    targets = torch.stack([t0, t1], -1).contiguous()
    trap = None
    if causal:
        trap = torch.stack([flash_trap_keys(S, bb) for bb in range(B)])
        targets[:, H - 1, :, 1] = -1
    q = needle_q(targets)  # [B, H, S, D]
    if causal:
        q[:, H - 1] += 2.0 * code(trap.clamp_min(0)) * (trap >= 0).to(F64).unsqueeze(-1)
    k = (2.0 * code(torch.arange(S))).view(1, S, 1, D).expand(B, S, KV, D)
    v = torch.randn(B, S, KV, D, generator=g, dtype=F64)
    v = ((v * 8).round() / 8).clamp(-3.875, 3.875) if vgrid else rb(v)
    do = rb(torch.randn(B, S, H, D, generator=g, dtype=F64))
    # Rows that share both targets have the same query, so their dK terms dS q are parallel and can
    # cancel: a dK row would then be small beside its own bf16-rounded terms and per-head partials, and
    # a per-row relative metric reads that rounding as an O(1) error (the rounding model itself gave up
    # to 1.2).  dS of a two-key row is +-1/4 dO.(v_a - v_b): each dO row takes the sign that makes its
    # term of the lower target's dK positive, so parallel terms add.
    kvh = (torch.arange(H) // (H // KV)).view(1, H, 1).expand(B, H, S)
    bi = torch.arange(B).view(B, 1, 1).expand(B, H, S)
    dv = v[bi, t0, kvh] - v[bi, t1.clamp_min(0), kvh]  # [B, H, S, D]
    sgn = torch.sign((do.transpose(1, 2) * dv).sum(-1)) * torch.sign(t1 - t0)
    do = do * torch.where((t1 < 0) | (sgn == 0), torch.ones_like(sgn), sgn).transpose(1, 2).unsqueeze(-1)
    x = torch.cat([q.transpose(1, 2), k, v], 2)  # [B, S, H + 2 KV, D]
    assert torch.equal(rb(x), x) and torch.equal(rb(do), do)
    return SimpleNamespace(B=B, S=S, H=H, KV=KV, causal=causal, targets=targets, trap=trap,
                           trap_head=H - 1 if causal else None,
                           qkv=x.reshape(B, S, -1).to(BF16), do=do.reshape(B, S, -1).to(BF16))


@functools.lru_cache(maxsize=None)
def flash_random_case(S: int = 1024, H: int = 8, KV: int = 2, seed: int = 0):
    """Unsaturated softmax: i.i.d. normal q/k/v (causal), for the values of p the needles never make."""
    g = torch.Generator().manual_seed(seed)
    return SimpleNamespace(B=1, S=S, H=H, KV=KV, causal=True,
                           qkv=torch.randn(1, S, (H + 2 * KV) * D, generator=g).to(BF16),
                           do=torch.randn(1, S, H * D, generator=g).to(BF16))


def flash_f64(c, vis: torch.Tensor | None = None, model: bool = False, grads: bool = True, device="cpu",
              want_p: bool = False):
    """fp64 attention over the case's bf16 inputs.  ``vis`` [S, S] or [B, H, S, S] bool: which keys
    each row sees (default: the case's own mask) -- simulated defects edit it.  ``model``: with the
    kernels' roundings.  Returns o, dq [B, S, H, D] and dk, dv [B, S, KV, D] (and p [B, H, S, S])."""
    B, S, H, KV = c.B, c.S, c.H, c.KV
    G = H // KV
    if vis is None:
        vis = causal_vis(S) if c.causal else torch.ones(S, S, dtype=torch.bool)
    vis = vis.to(device)
    x = c.qkv.to(device).to(F64).view(B, S, H + 2 * KV, D)
    dox = c.do.to(device).to(F64).view(B, S, H, D)
    out = {n: [] for n in ("o", "dq", "dk", "dv", "p")}
    for b in range(B):
        q = x[b, :, :H].transpose(0, 1)
        k = x[b, :, H : H + KV].transpose(0, 1).repeat_interleave(G, 0)
        v = x[b, :, H + KV :].transpose(0, 1).repeat_interleave(G, 0)
        s = (q @ k.transpose(1, 2) * SCALE).masked_fill(~(vis if vis.dim() == 2 else vis[b]), float("-inf"))
        e, l, p = _softmax_parts(s)
        o = rb(rb(e) @ v / torch.where(l == 0, torch.ones_like(l), l)) if model else p @ v
        out["o"].append(o.transpose(0, 1))
        if want_p:
            out["p"].append(p)
        if not grads:
            continue
        do = dox[b].transpose(0, 1)
        ds = p * (do @ v.transpose(1, 2) - (do * o).sum(-1, keepdim=True))
        if model:
            ds = rb(ds)
        dq = ds @ k * SCALE
        dkh = ds.transpose(1, 2) @ q * SCALE
        dvh = (rb(p) if model else p).transpose(1, 2) @ do
        if model:
            dq, dkh, dvh = rb(dq), rb(dkh), rb(dvh)
        dk, dv = dkh.view(KV, G, S, D).sum(1), dvh.view(KV, G, S, D).sum(1)
        if model:
            dk, dv = rb(dk), rb(dv)
        for n, t in (("dq", dq), ("dk", dk), ("dv", dv)):
            out[n].append(t.transpose(0, 1))
    return {n: torch.stack(t) for n, t in out.items() if t}


# ==================================================================================================
# Paged caches
# ==================================================================================================
def _scales(cache_dtype):
    return (0.5, 2.0) if cache_dtype == E4M3 else (1.0, 1.0)


def sentinel_v(cache_dtype) -> float:
    """The value of every trap slot's v: finite (a masked key still enters P V as 0 x v), exact in
    the cache type and far outside the data.  e4m3 ends at 448, so at v_scale = 2 the trap is 896."""
    return 448.0 * 2.0 if cache_dtype == E4M3 else 1000.0


class _Pages:
    """Physical pages handed out in a random, non-monotone order; real values in fp64."""

    def __init__(self, total: int, KVH: int, cache_dtype, g):
        self.order = torch.randperm(total, generator=g).tolist()
        self.KVH, self.dtype, self.g, self.used = KVH, cache_dtype, g, 0
        self.k = torch.zeros(total, KVH, PAGE, D, dtype=F64)
        self.v = torch.zeros(total, KVH, D, PAGE, dtype=F64)

    def rand_v(self, *shape):
        x = torch.randn(*shape, generator=self.g, dtype=F64)
        return r8(x) * 2.0 if self.dtype == E4M3 else rb(x)

    def take(self) -> int:
        self.used += 1
        return self.order[self.used - 1]

    def fill(self, page: int, first_pos: int, end: int, trap_key: int):
        """Slots of positions ``first_pos .. first_pos + 63``: below ``end`` key 2 code(pos) and a
        random v; from ``end`` on the trap: key 2 code(trap_key) and the sentinel v."""
        pos = first_pos + torch.arange(PAGE)
        real = pos < end
        kk = torch.where(real.unsqueeze(-1), 2.0 * code(pos), 2.0 * code(torch.full_like(pos, trap_key)))
        self.k[page] = kk.unsqueeze(0)
        vv = self.rand_v(self.KVH, D, PAGE)
        self.v[page] = torch.where(real.view(1, 1, PAGE), vv, torch.full_like(vv, sentinel_v(self.dtype)))

    def caches(self):
        assert self.used == len(self.order)
        ks, vs = _scales(self.dtype)
        kc, vc = (self.k / ks).to(torch.float32).to(self.dtype), (self.v / vs).to(torch.float32).to(self.dtype)
        assert torch.equal(kc.to(F64) * ks, self.k) and torch.equal(vc.to(F64) * vs, self.v)  # exact round trip
        return kc, vc


def _build_tables(ends, W, KVH, cache_dtype, g):
    """One block-table row per sequence of ``ends[s]`` cached tokens: its pages, then its poison
    page (all trap slots) in every further entry.  The first two sequences of >= 64 tokens share
    their first physical page.  Trap slots hold the key of position ``ends[s] - 1``."""
    n = len(ends)
    npg = [(e + PAGE - 1) // PAGE for e in ends]
    assert max(npg) <= W
    full = [s for s in range(n) if ends[s] >= PAGE][:2]
    pages = _Pages(sum(npg) + n - (len(full) == 2), KVH, cache_dtype, g)
    tables = torch.zeros(n, W, dtype=torch.int32)
    for s in range(n):
        for p in range(npg[s]):
            if len(full) == 2 and s == full[1] and p == 0:
                tables[s, 0] = tables[full[0], 0]
                continue
            page = pages.take()
            pages.fill(page, p * PAGE, ends[s], ends[s] - 1)
            tables[s, p] = page
        poison = pages.take()
        pages.fill(poison, 0, 0, ends[s] - 1)
        tables[s, npg[s] :] = poison
    kc, vc = pages.caches()
    return tables, kc, vc, npg


def gather_f64(c, table_row: torch.Tensor, npages: int):
    """Keys and values [KVH, npages * 64, D] fp64 (dequantised) of a block-table row's first pages."""
    ks, vs = _scales(c.cache_dtype)
    pg = table_row[:npages].long()
    k = c.k_cache[pg].to(torch.float32).to(F64).permute(1, 0, 2, 3).reshape(c.KVH, -1, D) * ks
    v = c.v_cache[pg].to(torch.float32).to(F64).permute(1, 0, 3, 2).reshape(c.KVH, -1, D) * vs
    return k, v


def _attend(q, k, v, vis, model):
    """q [KVH, G, n, D] over k, v [KVH, N, D] with ``vis`` broadcastable to [KVH, G, n, N]."""
    s = (torch.einsum("hgid,hkd->hgik", q, k) * SCALE).masked_fill(~vis, float("-inf"))
    e, l, p = _softmax_parts(s)
    if not model:
        return torch.einsum("hgik,hkd->hgid", p, v), p
    return rb(torch.einsum("hgik,hkd->hgid", rb(e), v) / torch.where(l == 0, torch.ones_like(l), l)), p


# --------------------------------------------------------------------------------------------------
# Paged decode
# --------------------------------------------------------------------------------------------------
DECODE_W = 8
DECODE_HEADS = [(8, 8), (4, 2), (28, 4), (32, 4), (16, 1)]  # G = 1, 2, 7, 8, 16
DECODE_PLANS = {"unsplit": (1, 8), "two": (2, 4), "pages": (8, 1)}  # (nsplit, pages per split)


def decode_contexts(W: int = DECODE_W):
    ctx = {1, 2, 63, 64, 65, 127, 128, 129, 511, 512}
    for _, pps in DECODE_PLANS.values():
        ctx |= {pps * PAGE - 1, pps * PAGE, pps * PAGE + 1}
    return sorted(c for c in ctx if c <= W * PAGE)


@functools.lru_cache(maxsize=None)
def decode_case(H: int, KVH: int, cache_dtype, seed: int = 0):
    """One sequence per context length.  Every head targets ``ctx - 1``; head 0 nothing else (a
    leaked trap slot takes half of it), and pages 0 .. last - 1 are dealt round-robin to heads
    1 .. H - 1, each adding that page's key with the same low code: every page of every sequence,
    hence every split of every plan, holds a key that some row needs."""
    g = torch.Generator().manual_seed(seed)
    ctxs = decode_contexts()
    B, W = len(ctxs), DECODE_W
    tables, kc, vc, npg = _build_tables(ctxs, W, KVH, cache_dtype, g)
    targets = torch.full((B, H, W), -1, dtype=torch.long)
    for b, ctx in enumerate(ctxs):
        targets[b, :, 0] = ctx - 1
        for p in range(npg[b] - 1):
            targets[b, 1 + p % (H - 1), 1 + p // (H - 1)] = p * PAGE + (ctx - 1) % PAGE
    q = needle_q(targets)  # [B, H, D]
    qkv = torch.cat([q.reshape(B, -1), rb(torch.randn(B, 2 * KVH * D, generator=g, dtype=F64))], 1)
    assert torch.equal(rb(qkv), qkv)
    return SimpleNamespace(B=B, H=H, KVH=KVH, W=W, cache_dtype=cache_dtype, ctx=torch.tensor(ctxs, dtype=torch.int32),
                           tables=tables, k_cache=kc, v_cache=vc, npg=npg, targets=targets, qkv=qkv.to(BF16),
                           scales=_scales(cache_dtype))


@functools.lru_cache(maxsize=None)
def decode_random_case(cache_dtype, H: int = 8, KVH: int = 2, ctx: int = 1000, seed: int = 0):
    g = torch.Generator().manual_seed(seed)
    W = (ctx + PAGE - 1) // PAGE
    kc, vc = (torch.randn(W + 3, KVH, PAGE, D, generator=g), torch.randn(W + 3, KVH, D, PAGE, generator=g))
    if cache_dtype == E4M3:
        kc, vc = kc.clamp(-4, 4), vc.clamp(-4, 4)
    tables = torch.randperm(W + 3, generator=g)[:W].view(1, W).int()
    return SimpleNamespace(B=1, H=H, KVH=KVH, W=W, cache_dtype=cache_dtype, ctx=torch.tensor([ctx], dtype=torch.int32),
                           tables=tables, k_cache=kc.to(cache_dtype), v_cache=vc.to(cache_dtype),
                           qkv=torch.randn(1, (H + 2 * KVH) * D, generator=g).to(BF16), scales=_scales(cache_dtype))


def decode_f64(c, ctx=None, tables=None, drop_pages=(), model: bool = False, want_p: bool = False, seqs=None):
    """fp64 decode attention [B, H * D].  Simulated defects: other ``ctx`` / ``tables``, and
    ``drop_pages``: table columns whose keys no row sees.  ``seqs``: only these sequences (the
    other rows stay zero)."""
    ctx = c.ctx if ctx is None else ctx
    tables = c.tables if tables is None else tables
    G = c.H // c.KVH
    out, ps = torch.zeros(c.B, c.H * D, dtype=F64), []
    for b in range(c.B) if seqs is None else seqs:
        n = int(ctx[b])
        npages = (n + PAGE - 1) // PAGE
        k, v = gather_f64(c, tables[b], npages)
        key = torch.arange(npages * PAGE)
        vis = key < n
        for p in drop_pages:
            vis &= key // PAGE != p
        q = c.qkv[b, : c.H * D].to(F64).view(c.KVH, G, 1, D)
        o, p = _attend(q, k, v, vis.view(1, 1, 1, -1), model)
        out[b] = o.reshape(-1)
        ps.append(p.reshape(c.H, -1))
    return (out, ps) if want_p else out


# --------------------------------------------------------------------------------------------------
# Paged-prefix prefill
# --------------------------------------------------------------------------------------------------
PREFILL_W = 8
PREFILL_HEADS = [(4, 2), (28, 4), (16, 1), (5, 1)]  # G = 2, 7 (4 + 3 waves), 16 (4 x 4), 5 (4 + 1)
PREFILL_SEGS = [(start, n) for start in (0, 1, 63, 64, 100) for n in (1, 15, 16, 17, 47, 48, 49, 130)]
PREFILL_TILE = 48  # query tokens per wave (NT = 3 column tiles of 16)


def prefill_trap_key(pos: torch.Tensor) -> torch.Tensor:
    return torch.where((pos % 2 == 1) & (pos % 64 != 31), pos + 1, pos + 64)


@functools.lru_cache(maxsize=None)
def prefill_case(H: int, KVH: int, cache_dtype, seed: int = 0):
    """Every (start, len) segment, packed with gaps.  The cache holds each sequence up to the
    segment's end, so a row's later tokens are real entries.  Query heads 0 .. H - 2: the diagonal
    plus, for the pages below the row's own, that page's key with the same low code, the pages dealt
    over the heads and shifting with the row.  Head H - 1 is the trap head: the diagonal and a key
    one or 64 positions later.  Slots past a segment's end are traps for its last row."""
    g = torch.Generator().manual_seed(seed)
    segs, W = PREFILL_SEGS, PREFILL_W
    ends = [s + n for s, n in segs]
    tables, kc, vc, npg = _build_tables(ends, W, KVH, cache_dtype, g)
    offsets, rows = [], 5
    for i, (_, n) in enumerate(segs):
        offsets.append(rows)
        rows += n + (3, 0, 17, 1)[i % 4]
    rows += 9
    qkv = rb(torch.randn(rows, (H + 2 * KVH) * D, generator=g, dtype=F64))
    nh = min(H - 1, 4)
    targets, listed, posl = torch.full((rows, H, 5), -1, dtype=torch.long), torch.zeros(rows, dtype=torch.bool), []
    trap = torch.full((rows,), -1, dtype=torch.long)
    for s, (start, n) in enumerate(segs):
        pos = start + torch.arange(n)
        r = offsets[s] + torch.arange(n)
        listed[r] = True
        targets[r, :, 0] = pos.view(n, 1)
        for p in range(npg[s]):
            for h in range(H - 1):
                sel = (p < pos // PAGE) & ((p + pos) % nh == h % nh)
                targets[r[sel], h, 1 + p] = p * PAGE + pos[sel] % PAGE
        trap[r] = prefill_trap_key(pos)
        posl.append(pos)
    q = needle_q(targets)
    q[:, H - 1] += 2.0 * code(trap.clamp_min(0)) * (trap >= 0).to(F64).unsqueeze(-1)
    qkv[listed, : H * D] = q[listed].reshape(-1, H * D)
    assert torch.equal(rb(qkv), qkv)
    i32 = dict(dtype=torch.int32)
    return SimpleNamespace(H=H, KVH=KVH, W=W, cache_dtype=cache_dtype, rows=rows, segs=segs, npg=npg, listed=listed,
                           offsets=torch.tensor(offsets, **i32), starts=torch.tensor([s for s, _ in segs], **i32),
                           lens=torch.tensor([n for _, n in segs], **i32), tables=tables, k_cache=kc, v_cache=vc,
                           targets=targets, trap=trap, trap_head=H - 1, qkv=qkv.to(BF16), scales=_scales(cache_dtype))


@functools.lru_cache(maxsize=None)
def prefill_random_case(cache_dtype, H: int = 8, KVH: int = 2, start: int = 200, n: int = 100, seed: int = 0):
    g = torch.Generator().manual_seed(seed)
    W = (start + n + PAGE - 1) // PAGE
    kc, vc = (torch.randn(W + 3, KVH, PAGE, D, generator=g), torch.randn(W + 3, KVH, D, PAGE, generator=g))
    if cache_dtype == E4M3:
        kc, vc = kc.clamp(-4, 4), vc.clamp(-4, 4)
    i32 = dict(dtype=torch.int32)
    listed = torch.zeros(n + 8, dtype=torch.bool)
    listed[4 : 4 + n] = True
    return SimpleNamespace(H=H, KVH=KVH, W=W, cache_dtype=cache_dtype, rows=n + 8, segs=[(start, n)], listed=listed,
                           offsets=torch.tensor([4], **i32), starts=torch.tensor([start], **i32),
                           lens=torch.tensor([n], **i32), tables=torch.randperm(W + 3, generator=g)[:W].view(1, W).int(),
                           k_cache=kc.to(cache_dtype), v_cache=vc.to(cache_dtype),
                           qkv=torch.randn(n + 8, (H + 2 * KVH) * D, generator=g).to(BF16), scales=_scales(cache_dtype))


def prefill_f64(c, shift: int = 0, tables=None, extra=None, model: bool = False, want_p: bool = False):
    """fp64 prefill attention [rows, H * D], zero outside the segments; row at position ``pos``
    sees keys ``<= pos + shift`` of all W table entries (``shift`` != 0 and other ``tables``
    simulate defects) and the key ``extra[row]`` (long [rows], -1 = none)."""
    tables = c.tables if tables is None else tables
    G = c.H // c.KVH
    out, ps = torch.zeros(c.rows, c.H * D, dtype=F64), []
    for s, (start, n) in enumerate(c.segs):
        off = int(c.offsets[s])
        k, v = gather_f64(c, tables[s], c.W)
        pos = start + torch.arange(n)
        key = torch.arange(c.W * PAGE).view(1, -1)
        vis = key <= (pos + shift).view(-1, 1)
        if extra is not None:
            vis = vis | (key == extra[off : off + n].view(-1, 1))
        q = c.qkv[off : off + n, : c.H * D].to(F64).view(n, c.KVH, G, D).permute(1, 2, 0, 3)
        o, p = _attend(q, k, v, vis.view(1, 1, n, -1), model)
        out[off : off + n] = o.permute(2, 0, 1, 3).reshape(n, -1)
        ps.append(p.reshape(c.H, n, -1))
    return (out, ps) if want_p else out


def heads(x: torch.Tensor, H: int) -> torch.Tensor:
    """[rows, >= H * D] -> the [rows * H, D] rows the metric looks at."""
    return x[:, : H * D].reshape(-1, D)
