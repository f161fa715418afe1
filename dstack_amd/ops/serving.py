"""Serving ops: paged KV cache writes, paged decode attention, paged-prefix prefill attention and
sampling.

HIP kernels in ``csrc/paged_attn.hip``, ``csrc/paged_prefill.hip``, ``csrc/sampler.hip`` (top-k /
top-p / min-p truncation, top-N log-probabilities) and ``csrc/penalties.hip`` (presence / frequency /
repetition penalties, logit_bias) and ``csrc/lora.hip`` (batched multi-LoRA shrink / expand) for ROCm
tensors; the PyTorch
functions here are the CPU path of the engine and the fp32 references the GPU tests compare against.

Cache layout (per layer): ``k_cache [pages, KVH, PAGE, 128]`` token-major and
``v_cache [pages, KVH, 128, PAGE]`` dim-major (see the kernel file for why), ``PAGE = 64``.
A token's cache slot is ``page * PAGE + offset``.
"""

from __future__ import annotations

import math

import torch

from dstack_amd.ops import _ext

PAGE = 64
HEAD_DIM = 128


def alloc_cache(num_pages: int, n_kv_heads: int, dtype=torch.bfloat16, device=None):
    """``dtype`` bf16 (or fp32 on the CPU) or ``torch.float8_e4m3fn`` (an fp8 cache holds
    k / k_scale and v / v_scale: half the bytes a decode step streams, twice the tokens)."""
    k = torch.zeros(num_pages, n_kv_heads, PAGE, HEAD_DIM, dtype=dtype, device=device)
    v = torch.zeros(num_pages, n_kv_heads, HEAD_DIM, PAGE, dtype=dtype, device=device)
    return k, v


def _is_fp8(cache: torch.Tensor) -> bool:
    return cache.dtype == torch.float8_e4m3fn


# ----------------------------------------------------------------------------------------------
# RoPE + cache write
# ----------------------------------------------------------------------------------------------
def rope_cache_write(qkv: torch.Tensor, positions: torch.Tensor, slots: torch.Tensor, cos: torch.Tensor,
                     sin: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, n_heads: int,
                     n_kv_heads: int, k_scale: float = 1.0, v_scale: float = 1.0, rs=None, cs=None) -> torch.Tensor:
    """Rotate q and k of ``qkv`` [T, (H + 2*KVH) * 128] in place (token t at ``positions[t]``) and
    store k/v of every token with ``slots[t] >= 0`` in the cache.  Returns ``qkv``.

    ``rs`` [T] / ``cs`` [(H + 2*KVH) * 128]: ``qkv`` is the raw product of a tensor-wise-scaled fp8
    GEMM; its row-wise scales are applied first, in place for every head."""
    if _ext.use_hip(qkv):
        _ext.require().rope_cache_write(qkv, positions, slots, cos, sin, k_cache, v_cache, n_heads, n_kv_heads,
                                        k_scale, v_scale, rs, cs)
        return qkv
    if rs is not None:
        qkv.copy_((qkv.float() * rs[:, None] * cs[None, :]).to(qkv.dtype))
    return rope_cache_write_ref(qkv, positions, slots, cos, sin, k_cache, v_cache, n_heads, n_kv_heads,
                                k_scale, v_scale)


def rope_cache_write_ref(qkv, positions, slots, cos, sin, k_cache, v_cache, n_heads, n_kv_heads,
                         k_scale: float = 1.0, v_scale: float = 1.0):
    T = positions.numel()
    x = qkv.view(T, n_heads + 2 * n_kv_heads, HEAD_DIM)
    rot = x[:, : n_heads + n_kv_heads].float()
    c = cos[positions.long()].unsqueeze(1)
    s = sin[positions.long()].unsqueeze(1)
    x1, x2 = rot[..., : HEAD_DIM // 2], rot[..., HEAD_DIM // 2 :]
    x[:, : n_heads + n_kv_heads] = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).to(qkv.dtype)
    keep = slots >= 0
    if keep.any():
        sl = slots[keep].long()
        page, off = sl // PAGE, sl % PAGE
        k = x[keep][:, n_heads : n_heads + n_kv_heads]  # [n, KVH, D]
        v = x[keep][:, n_heads + n_kv_heads :]
        if _is_fp8(k_cache):
            k = (k.float() / k_scale).clamp(-448, 448)
            v = (v.float() / v_scale).clamp(-448, 448)
        k_cache[page, :, off, :] = k.to(k_cache.dtype)
        v_cache[page, :, :, off] = v.to(v_cache.dtype)
    return qkv


# ----------------------------------------------------------------------------------------------
# Paged decode attention
# ----------------------------------------------------------------------------------------------
def split_plan(batch: int, n_kv_heads: int, table_width: int, target_waves: int = 2048):
    """(nsplit, pages_per_split): enough one-wave workgroups to fill 256 CUs at any context, a
    function of the batch bucket and the block-table width only (graph-capturable)."""
    want = max(1, math.ceil(target_waves / max(1, batch * n_kv_heads)))
    nsplit = max(1, min(want, table_width))
    pps = math.ceil(table_width / nsplit)
    return math.ceil(table_width / pps), pps


class DecodeWorkspace:
    """Preallocated split-KV partials for a batch bucket (hipGraph-safe: no allocation per step)."""

    def __init__(self, batch: int, n_heads: int, n_kv_heads: int, table_width: int, device,
                 target_waves: int = 2048):
        self.nsplit, self.pps = split_plan(batch, n_kv_heads, table_width, target_waves)
        n = batch * n_heads * self.nsplit if self.nsplit > 1 else 1
        self.o_part = torch.empty(n * HEAD_DIM, dtype=torch.float32, device=device)
        self.lse_part = torch.empty(n, dtype=torch.float32, device=device)


def paged_decode(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, block_tables: torch.Tensor,
                 ctx_lens: torch.Tensor, n_heads: int, n_kv_heads: int, out: torch.Tensor | None = None,
                 ws: DecodeWorkspace | None = None, k_scale: float = 1.0, v_scale: float = 1.0) -> torch.Tensor:
    """Attention of one new query token per sequence over its cached keys/values.

    ``q`` [B, >= H*128] (rows may be the fused qkv output: only the first H*128 columns are read),
    ``block_tables`` [B, W] int32 page ids, ``ctx_lens`` [B] int32.  Returns [B, H*128]."""
    B = q.shape[0]
    if out is None:
        out = torch.empty(B, n_heads * HEAD_DIM, dtype=q.dtype, device=q.device)
    if _ext.use_hip(q):
        if ws is None:
            ws = DecodeWorkspace(B, n_heads, n_kv_heads, block_tables.shape[1], q.device)
        _ext.require().paged_decode(q, k_cache, v_cache, block_tables, ctx_lens, out, ws.o_part, ws.lse_part,
                                    n_heads, n_kv_heads, ws.nsplit, ws.pps, 1.0 / math.sqrt(HEAD_DIM), k_scale,
                                    v_scale)
        return out
    out.copy_(paged_decode_ref(q, k_cache, v_cache, block_tables, ctx_lens, n_heads, n_kv_heads, k_scale,
                               v_scale).to(out.dtype))
    return out


def _gather_kv(k_cache, v_cache, table_row, n: int, n_kv_heads: int, k_scale: float, v_scale: float):
    """The first ``n`` cached keys and values of one block-table row as fp32 [KVH, n, D] (an fp8
    cache dequantised with its scales; any other cache holds the values themselves)."""
    pages = table_row[: (n + PAGE - 1) // PAGE].long()
    ks, vs = (k_scale, v_scale) if _is_fp8(k_cache) else (1.0, 1.0)
    k = k_cache[pages].float().permute(1, 0, 2, 3).reshape(n_kv_heads, -1, HEAD_DIM)[:, :n] * ks
    v = v_cache[pages].float().permute(1, 0, 3, 2).reshape(n_kv_heads, -1, HEAD_DIM)[:, :n] * vs
    return k, v


def paged_decode_ref(q, k_cache, v_cache, block_tables, ctx_lens, n_heads, n_kv_heads, k_scale: float = 1.0,
                     v_scale: float = 1.0):
    """fp32 reference: gathers each sequence's pages and runs plain softmax attention."""
    B = q.shape[0]
    G = n_heads // n_kv_heads
    out = torch.empty(B, n_heads * HEAD_DIM, dtype=torch.float32, device=q.device)
    for b in range(B):
        n = int(ctx_lens[b])
        k, v = _gather_kv(k_cache, v_cache, block_tables[b], n, n_kv_heads, k_scale, v_scale)
        qb = q[b, : n_heads * HEAD_DIM].float().view(n_kv_heads, G, HEAD_DIM)
        s = torch.einsum("hgd,hnd->hgn", qb, k) / math.sqrt(HEAD_DIM)
        p = torch.softmax(s, dim=-1)
        out[b] = torch.einsum("hgn,hnd->hgd", p, v).reshape(-1)
    return out


# ----------------------------------------------------------------------------------------------
# Paged verify attention (speculative decoding: a few new query tokens per sequence)
# ----------------------------------------------------------------------------------------------
VERIFY_MAX_T = 8


def verify_plan(T: int, group: int):
    """(column tiles per wave, waves per (sequence, KV head)) of the verify kernel: the ``T * group``
    (token, query head) columns of a KV head in tiles of 16, at most 3 tiles on a wave."""
    tiles = (T * group + 15) // 16
    groups = (tiles + 2) // 3
    return (tiles + groups - 1) // groups, groups


class VerifyWorkspace:
    """Preallocated split-KV partials of :func:`paged_verify` for ``rows`` query rows (a batch bucket
    of the engine) of ``T`` rows per sequence -- the :class:`DecodeWorkspace` of the verify step."""

    def __init__(self, rows: int, T: int, n_heads: int, n_kv_heads: int, table_width: int, device,
                 target_waves: int = 2048):
        if not 1 <= T <= VERIFY_MAX_T:
            raise ValueError(f"paged_verify takes 1..{VERIFY_MAX_T} query tokens per sequence, got {T}")
        self.rows, self.T = rows, T
        seqs = (rows + T - 1) // T
        self.nsplit, self.pps = split_plan(seqs * verify_plan(T, n_heads // n_kv_heads)[1], n_kv_heads, table_width,
                                           target_waves)
        n = rows * n_heads * self.nsplit if self.nsplit > 1 else 1
        self.o_part = torch.empty(n * HEAD_DIM, dtype=torch.float32, device=device)
        self.lse_part = torch.empty(n, dtype=torch.float32, device=device)


def paged_verify(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, block_tables: torch.Tensor,
                 ctx_lens: torch.Tensor, q_lens: torch.Tensor, T: int, n_heads: int, n_kv_heads: int,
                 out: torch.Tensor | None = None, ws: VerifyWorkspace | None = None, k_scale: float = 1.0,
                 v_scale: float = 1.0) -> torch.Tensor:
    """Attention of up to ``T`` (1..8) new query tokens per sequence over its cached keys/values.

    ``q`` [R, >= H*128] with ``R >= B*T`` (rows may be the fused qkv output); row ``b*T + j`` is query
    j of sequence b.  ``block_tables`` [B, W], ``ctx_lens`` [B], ``q_lens`` [B] int32 with
    ``0 <= q_lens[b] <= min(T, ctx_lens[b])``: query ``j < q_lens[b]`` sits at position
    ``ctx_lens[b] - q_lens[b] + j`` and attends to cache keys 0 .. that position -- its own K/V and
    the earlier queries' are in the cache already (``rope_cache_write``).  Returns [R, H*128]; the rows
    ``j >= q_lens[b]`` and the rows from ``B*T`` on are zeros."""
    R = q.shape[0]
    if out is None:
        out = torch.empty(R, n_heads * HEAD_DIM, dtype=q.dtype, device=q.device)
    if _ext.use_hip(q):
        if ws is None:
            ws = VerifyWorkspace(R, T, n_heads, n_kv_heads, block_tables.shape[1], q.device)
        _ext.require().paged_verify(q, k_cache, v_cache, block_tables, ctx_lens, q_lens, out, ws.o_part, ws.lse_part,
                                    T, n_heads, n_kv_heads, ws.nsplit, ws.pps, 1.0 / math.sqrt(HEAD_DIM), k_scale,
                                    v_scale)
        return out
    out.copy_(paged_verify_ref(q, k_cache, v_cache, block_tables, ctx_lens, q_lens, T, n_heads, n_kv_heads, k_scale,
                               v_scale).to(out.dtype))
    return out


def paged_verify_ref(q, k_cache, v_cache, block_tables, ctx_lens, q_lens, T, n_heads, n_kv_heads,
                     k_scale: float = 1.0, v_scale: float = 1.0):
    """fp32 reference of :func:`paged_verify`: [R, H*128] with zeros in the rows that hold no query.
    Every query row is computed with the operations of :func:`paged_decode_ref` over its own keys, so
    it has the bits the decode reference gives that token."""
    G = n_heads // n_kv_heads
    out = torch.zeros(q.shape[0], n_heads * HEAD_DIM, dtype=torch.float32, device=q.device)
    for b in range(block_tables.shape[0]):
        ctx, n = int(ctx_lens[b]), int(q_lens[b])
        if n <= 0:
            continue
        for j in range(n):
            m = ctx - n + j + 1  # keys 0 .. its own position
            k, v = _gather_kv(k_cache, v_cache, block_tables[b], m, n_kv_heads, k_scale, v_scale)
            qb = q[b * T + j, : n_heads * HEAD_DIM].float().view(n_kv_heads, G, HEAD_DIM)
            s = torch.einsum("hgd,hnd->hgn", qb, k) / math.sqrt(HEAD_DIM)
            p = torch.softmax(s, dim=-1)
            out[b * T + j] = torch.einsum("hgn,hnd->hgd", p, v).reshape(-1)
    return out


# ----------------------------------------------------------------------------------------------
# Paged-prefix prefill attention (prefix caching: new tokens over a cached prefix)
# ----------------------------------------------------------------------------------------------
def paged_prefill(qkv: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, block_tables: torch.Tensor,
                  seg_offsets: torch.Tensor, seg_starts: torch.Tensor, seg_lens: torch.Tensor, n_heads: int,
                  n_kv_heads: int, out: torch.Tensor | None = None, k_scale: float = 1.0, v_scale: float = 1.0,
                  max_len: int | None = None) -> torch.Tensor:
    """Causal attention of ``n`` segments of new tokens, packed in ``qkv`` [rows, >= H*128], over the
    paged cache.  Segment s holds ``seg_lens[s]`` tokens from row ``seg_offsets[s]``; ``seg_starts[s]``
    tokens of its sequence are cached already (any value >= 0).  The query at row
    ``seg_offsets[s] + i`` sits at position ``seg_starts[s] + i`` and attends to cache keys
    ``0 .. seg_starts[s] + i`` of ``block_tables[s]`` -- the segment's own K/V are read from the cache
    too, where ``rope_cache_write`` has stored them.  Metadata: int32, ``block_tables`` [n, W].

    Returns ``out`` [rows, H*128]; only the segments' rows are written.  ``max_len``: the longest
    segment when the caller has it on the host (and has checked the plan); otherwise the HIP path
    reads the metadata back to validate it and size its grid."""
    rows = qkv.shape[0]
    if out is None:
        out = torch.zeros(rows, n_heads * HEAD_DIM, dtype=qkv.dtype, device=qkv.device)
    if _ext.use_hip(qkv):
        _ext.require().paged_prefill(qkv, k_cache, v_cache, block_tables, seg_offsets, seg_starts, seg_lens, out,
                                     n_heads, n_kv_heads, 1.0 / math.sqrt(HEAD_DIM), k_scale, v_scale,
                                     -1 if max_len is None else int(max_len))
        return out
    ref = paged_prefill_ref(qkv, k_cache, v_cache, block_tables, seg_offsets, seg_starts, seg_lens, n_heads,
                            n_kv_heads, k_scale, v_scale)
    for off, n in zip(seg_offsets.tolist(), seg_lens.tolist()):
        out[off : off + n] = ref[off : off + n].to(out.dtype)
    return out


def paged_prefill_ref(qkv, k_cache, v_cache, block_tables, seg_offsets, seg_starts, seg_lens, n_heads, n_kv_heads,
                      k_scale: float = 1.0, v_scale: float = 1.0):
    """fp32 reference: gathers each segment's pages and runs masked softmax attention per row.
    Returns [rows, H*128] fp32 with zeros outside the segments."""
    G = n_heads // n_kv_heads
    out = torch.zeros(qkv.shape[0], n_heads * HEAD_DIM, dtype=torch.float32, device=qkv.device)
    for s in range(seg_lens.numel()):
        off, start, n = int(seg_offsets[s]), int(seg_starts[s]), int(seg_lens[s])
        if n <= 0:
            continue
        ctx = start + n
        k, v = _gather_kv(k_cache, v_cache, block_tables[s], ctx, n_kv_heads, k_scale, v_scale)
        q = qkv[off : off + n, : n_heads * HEAD_DIM].float().view(n, n_kv_heads, G, HEAD_DIM)
        sc = torch.einsum("ihgd,hkd->hgik", q, k) / math.sqrt(HEAD_DIM)
        key = torch.arange(ctx, device=qkv.device)[None, :]
        pos = start + torch.arange(n, device=qkv.device)[:, None]
        sc = sc.masked_fill(key > pos, float("-inf"))
        p = torch.softmax(sc, dim=-1)
        out[off : off + n] = torch.einsum("hgik,hkd->ihgd", p, v).reshape(n, -1)
    return out


# ----------------------------------------------------------------------------------------------
# Sampling
# ----------------------------------------------------------------------------------------------
def sample(logits: torch.Tensor, temps: torch.Tensor, seeds: torch.Tensor, steps: torch.Tensor,
           tokens: torch.Tensor | None = None, logprobs: torch.Tensor | None = None):
    """Per row: greedy argmax when ``temps[r] <= 0``, else an exact draw from softmax(logits/T)
    (Gumbel-max with a counter-based hash of (seed, step, token)).  Returns (tokens int32,
    logprobs fp32: log-probability of the chosen token under softmax(logits / T))."""
    R = logits.shape[0]
    if tokens is None:
        tokens = torch.empty(R, dtype=torch.int32, device=logits.device)
    if logprobs is None:
        logprobs = torch.empty(R, dtype=torch.float32, device=logits.device)
    if _ext.use_hip(logits):
        _ext.require().sample(logits, temps, seeds, steps, tokens, logprobs)
        return tokens, logprobs
    t, lp = sample_ref(logits, temps, seeds, steps)
    tokens.copy_(t)
    logprobs.copy_(lp)
    return tokens, logprobs


def sample_ref(logits, temps, seeds, steps):
    x = logits.float()
    t = temps.float().clamp_min(0)
    scale = torch.where(t > 0, 1.0 / torch.where(t > 0, t, torch.ones_like(t)), torch.ones_like(t))
    z = x * scale[:, None]
    lse = torch.logsumexp(z, dim=-1)
    score = z.clone()
    for r in range(x.shape[0]):
        if t[r] > 0:
            g = torch.Generator(device="cpu").manual_seed(int(seeds[r]) * 1000003 + int(steps[r]))
            u = torch.rand(x.shape[1], generator=g).clamp(1e-7, 1 - 1e-7).to(x.device)
            score[r] = z[r] - torch.log(-torch.log(u))
    tok = score.argmax(dim=-1)
    lp = z.gather(1, tok[:, None]).squeeze(1) - lse
    return tok.to(torch.int32), lp


# ----------------------------------------------------------------------------------------------
# Truncated sampling (top-k / top-p / min-p) and top-N log-probabilities: csrc/sampler.hip
# ----------------------------------------------------------------------------------------------
TOP_LOGPROBS_MAX = 20


def sample_threshold(logits: torch.Tensor, temps: torch.Tensor, top_k: torch.Tensor, top_p: torch.Tensor,
                     min_p: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """``tau`` fp32 [R]: row r keeps exactly the logits ``x >= tau[r]``.  Every truncation is a
    threshold on the logit value, so equal logits are kept or dropped together.  With
    ``z = x / T`` (``T <= 0``: greedy, z = x) and -inf logits never counted:

    - top-k (``0 < top_k[r] < V``; int32): keep v iff fewer than k tokens are strictly greater than v;
    - top-p (``top_p[r] < 1``), on the survivors of top-k, with ``w = exp(z - zmax)``: keep v iff the
      mass of the survivors strictly greater than v is at most p times the survivors' total mass;
    - min-p (``min_p[r] > 0``): keep v iff ``z >= zmax + ln(min_p)``.

    Each active rule gives the smallest logit of the row that it keeps; ``tau`` is the largest of
    them, and -inf for a row that asks for nothing (or has no finite logit)."""
    if out is None:
        out = torch.empty(logits.shape[0], dtype=torch.float32, device=logits.device)
    if _ext.use_hip(logits):
        _ext.require().sample_threshold(logits, temps, top_k, top_p, min_p, out)
        return out
    out.copy_(sample_threshold_ref(logits, temps, top_k, top_p, min_p))
    return out


def _inv_temp(temps: torch.Tensor) -> torch.Tensor:
    """fp32 1/T (1 for greedy rows), as the kernels compute it."""
    t = temps.float()
    return torch.where(t > 0, 1.0 / torch.where(t > 0, t, torch.ones_like(t)), torch.ones_like(t))


def sample_threshold_ref(logits, temps, top_k, top_p, min_p) -> torch.Tensor:
    """fp64 reference of :func:`sample_threshold` over each row's distinct values."""
    R, V = logits.shape
    x = logits.float().cpu()
    inv_t = _inv_temp(temps.cpu())
    ks, ps, ms = top_k.cpu().tolist(), top_p.float().cpu().tolist(), min_p.float().cpu()
    tau = torch.full((R,), float("-inf"))
    for r in range(R):
        k, p, mp = int(ks[r]), max(float(ps[r]), 0.0), float(ms[r])
        want_k, want_p, want_m = 0 < k < V, p < 1.0, mp > 0.0
        row = x[r][x[r] > float("-inf")]
        if not (want_k or want_p or want_m) or row.numel() == 0:
            continue
        v, c = torch.unique(row, return_counts=True)
        v, c = v.flip(0), c.flip(0)  # descending
        z = (v * inv_t[r]).double()  # (the fp32 product, as the kernel forms it)
        w = torch.exp(z - z[0]) * c
        n, cands = v.numel(), []
        if want_k:
            n = int(((c.cumsum(0) - c) < k).sum())
            cands.append(v[n - 1])
        if want_p:
            m = w[:n]
            keep = (m.cumsum(0) - m) <= p * m.sum()
            cands.append(v[:n][keep][-1])
        if want_m:
            cands.append(v[z >= z[0] + math.log(ms[r].double().item())][-1] if mp <= 1.0 else v[0])
        tau[r] = torch.stack(cands).max()
    return tau.to(logits.device)


def top_logprobs(logits: torch.Tensor, temps: torch.Tensor, tau: torch.Tensor, top_n: torch.Tensor,
                 top_ids: torch.Tensor | None = None, top_lps: torch.Tensor | None = None):
    """For rows with ``top_n[r] > 0`` (int32, at most ``TOP_LOGPROBS_MAX``): the kept tokens
    (``x >= tau[r]``) with the ``top_n`` largest logits, by value descending then token id ascending,
    as ``top_ids`` int32 / ``top_lps`` fp32 [R, TOP_LOGPROBS_MAX]; ``lp = z - logsumexp(z over the kept
    set)``, unused entries -1 / -inf.  Rows with ``top_n == 0`` are left as they are."""
    R = logits.shape[0]
    if top_ids is None:
        top_ids = torch.full((R, TOP_LOGPROBS_MAX), -1, dtype=torch.int32, device=logits.device)
    if top_lps is None:
        top_lps = torch.full((R, TOP_LOGPROBS_MAX), float("-inf"), dtype=torch.float32, device=logits.device)
    if _ext.use_hip(logits):
        _ext.require().top_logprobs(logits, temps, tau, top_n, top_ids, top_lps)
        return top_ids, top_lps
    ids, lps = top_logprobs_ref(logits, temps, tau, top_n)
    rows = top_n > 0
    top_ids[rows] = ids[rows]
    top_lps[rows] = lps[rows]
    return top_ids, top_lps


def top_logprobs_ref(logits, temps, tau, top_n):
    """Reference of :func:`top_logprobs` (fp64 log-sum-exp; a stable sort of -x, so ties go by
    ascending id).  Rows with ``top_n == 0`` come back as -1 / -inf."""
    R = logits.shape[0]
    x = logits.float().cpu()
    inv_t = _inv_temp(temps.cpu())
    ids = torch.full((R, TOP_LOGPROBS_MAX), -1, dtype=torch.int32)
    lps = torch.full((R, TOP_LOGPROBS_MAX), float("-inf"), dtype=torch.float32)
    for r, n in enumerate(top_n.cpu().tolist()):
        n = min(int(n), TOP_LOGPROBS_MAX)
        kept = (x[r] >= tau[r].item()) & (x[r] > float("-inf"))
        if n <= 0 or not kept.any():
            continue
        z = (x[r] * inv_t[r]).double()
        lse = torch.logsumexp(z[kept], dim=0)
        order = torch.sort(-x[r], stable=True).indices
        order = order[kept[order]][:n]
        ids[r, : order.numel()] = order.to(torch.int32)
        lps[r, : order.numel()] = (z[order] - lse).float()
    return ids.to(logits.device), lps.to(logits.device)


def sample_filtered(logits: torch.Tensor, temps: torch.Tensor, seeds: torch.Tensor, steps: torch.Tensor,
                    top_k: torch.Tensor, top_p: torch.Tensor, min_p: torch.Tensor,
                    tokens: torch.Tensor | None = None, logprobs: torch.Tensor | None = None,
                    top_n: torch.Tensor | None = None, top_ids: torch.Tensor | None = None,
                    top_lps: torch.Tensor | None = None, tau: torch.Tensor | None = None):
    """:func:`sample` over each row's kept set (:func:`sample_threshold`): the same draw per
    (seed, step, token), restricted to ``x >= tau[r]``, with the chosen token's log-probability under
    the kept set -- a row that asks for nothing gets what :func:`sample` returns.  With ``top_n``
    also :func:`top_logprobs` under the same kept set.  On ROCm tensors nothing is allocated when
    every output (and the ``tau`` workspace) is passed in, so the call can be captured in a hipGraph.

    Returns ``(tokens, logprobs, top_ids, top_lps)``; the last two are None without ``top_n``."""
    R = logits.shape[0]
    if tokens is None:
        tokens = torch.empty(R, dtype=torch.int32, device=logits.device)
    if logprobs is None:
        logprobs = torch.empty(R, dtype=torch.float32, device=logits.device)
    tau = sample_threshold(logits, temps, top_k, top_p, min_p, out=tau)
    if _ext.use_hip(logits):
        _ext.require().sample_masked(logits, temps, seeds, steps, tau, tokens, logprobs)
    else:
        t, lp = sample_ref(logits.float().masked_fill(logits.float() < tau[:, None], float("-inf")), temps, seeds,
                           steps)
        tokens.copy_(t)
        logprobs.copy_(lp)
    if top_n is None:
        return tokens, logprobs, None, None
    top_ids, top_lps = top_logprobs(logits, temps, tau, top_n, top_ids, top_lps)
    return tokens, logprobs, top_ids, top_lps


# ----------------------------------------------------------------------------------------------
# Sampling penalties (presence / frequency / repetition) and logit_bias: csrc/penalties.hip
# ----------------------------------------------------------------------------------------------
LOGIT_BIAS_MAX = 300


def alloc_penalty_state(slots: int, vocab: int, device=None):
    """``(state, bias_ids, bias_vals, bias_n)`` for ``slots`` sequences: ``state`` int32 [slots, V]
    holds ``2 * c[v] + in_prompt[v]`` (``c``: how often the sequence generated token v), the bias
    list of a slot is ``bias_ids`` int32 / ``bias_vals`` fp32 [slots, LOGIT_BIAS_MAX] with ``bias_n``
    int32 [slots] entries in use."""
    return (torch.zeros(slots, vocab, dtype=torch.int32, device=device),
            torch.zeros(slots, LOGIT_BIAS_MAX, dtype=torch.int32, device=device),
            torch.zeros(slots, LOGIT_BIAS_MAX, dtype=torch.float32, device=device),
            torch.zeros(slots, dtype=torch.int32, device=device))


def check_logit_bias(logit_bias, vocab: int) -> dict:
    """``logit_bias`` as ``{token id (int): bias (float)}``: at most LOGIT_BIAS_MAX entries, keys ints
    or strings of ints in ``[0, vocab)``, values numbers in [-100, 100].  Raises ValueError otherwise."""
    if not logit_bias:
        return {}
    if not isinstance(logit_bias, dict):
        raise ValueError("logit_bias must be an object mapping token ids to numbers")
    if len(logit_bias) > LOGIT_BIAS_MAX:
        raise ValueError(f"logit_bias may hold at most {LOGIT_BIAS_MAX} entries, got {len(logit_bias)}")
    out = {}
    for k, v in logit_bias.items():
        try:
            if isinstance(k, (bool, float)):
                raise ValueError
            t = int(k)
        except (TypeError, ValueError):
            raise ValueError(f"logit_bias key {k!r} is not a token id") from None
        if not 0 <= t < vocab:
            raise ValueError(f"logit_bias token id {t} is outside [0, {vocab})")
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not -100.0 <= v <= 100.0:
            raise ValueError(f"logit_bias value for token {t} must be a number in [-100, 100], got {v!r}")
        if t in out:
            raise ValueError(f"logit_bias names token {t} twice")
        out[t] = float(v)
    return out


def penalties_fill(state: torch.Tensor, bias_ids: torch.Tensor, bias_vals: torch.Tensor, bias_n: torch.Tensor,
                   slot: int, prompt_ids, output_ids, logit_bias: dict | None = None) -> None:
    """Rebuild slot ``slot`` from a request: its state row from the prompt and the generated tokens,
    its bias list from ``logit_bias`` ({int id: number}, validated by :func:`check_logit_bias`).
    Ordinary torch ops -- this runs once per admission, not per step."""
    dev = state.device
    row = state[slot]
    row.zero_()
    if len(prompt_ids):
        row[torch.unique(torch.as_tensor(list(prompt_ids), dtype=torch.int64)).to(dev)] = 1
    if len(output_ids):
        ids, cnt = torch.unique(torch.as_tensor(list(output_ids), dtype=torch.int64), return_counts=True)
        row.index_add_(0, ids.to(dev), (2 * cnt).to(torch.int32).to(dev))
    items = sorted((logit_bias or {}).items())
    n = len(items)
    assert n <= LOGIT_BIAS_MAX, n
    bias_n[slot] = n
    if n:
        bias_ids[slot, :n] = torch.tensor([k for k, _ in items], dtype=torch.int32).to(dev)
        bias_vals[slot, :n] = torch.tensor([v for _, v in items], dtype=torch.float32).to(dev)


def inv_rep_of(rep: torch.Tensor) -> torch.Tensor:
    """fp32 ``1 / r``, the one division of the repetition penalty (done on the host, not in the kernel)."""
    return 1.0 / rep.to(torch.float32)


def apply_penalties(logits: torch.Tensor, state: torch.Tensor, slot: torch.Tensor, rep: torch.Tensor,
                    inv_rep: torch.Tensor, freq: torch.Tensor, pres: torch.Tensor, bias_ids: torch.Tensor,
                    bias_vals: torch.Tensor, bias_n: torch.Tensor) -> torch.Tensor:
    """Rewrite, in place, the logits of every row r with ``slot[r] >= 0`` (int32; -1: the row asks for
    nothing and is not written).  With ``s = state[slot[r]]``, ``c = s >> 1``, ``seen = s != 0``, per
    element in fp32, each step one correctly rounded operation:

    1. repetition (``rep[r] != 1`` and seen): ``x = x * inv_rep[r] if x > 0 else x * rep[r]``;
    2. frequency: ``x = x - freq[r] * float(c)``;
    3. presence (``c > 0``): ``x = x - pres[r]``;
    4. bias (the ``bias_n`` ids of the slot's list): ``x = x + bias``;
    5. one rounding to the logits' dtype.  A -inf logit stays -inf.

    ``rep`` / ``inv_rep`` / ``freq`` / ``pres``: fp32 [rows].  On ROCm tensors nothing is allocated or
    read back (hipGraph-capturable).  Returns ``logits``."""
    if _ext.use_hip(logits):
        _ext.require().apply_penalties(logits, state, slot, rep, inv_rep, freq, pres, bias_ids, bias_vals, bias_n)
        return logits
    rows = slot >= 0
    if bool(rows.any()):
        ref = apply_penalties_ref(logits, state, slot, rep, inv_rep, freq, pres, bias_ids, bias_vals, bias_n)
        logits[rows] = ref[rows]
    return logits


def apply_penalties_ref(logits, state, slot, rep, inv_rep, freq, pres, bias_ids, bias_vals, bias_n) -> torch.Tensor:
    """Reference of :func:`apply_penalties`: the fp32 steps as separate torch operations on the CPU.
    Returns a new tensor like ``logits`` (rows with ``slot < 0`` are copies)."""
    out = logits.detach().cpu().clone()
    state, bias_ids, bias_vals, bias_n = state.cpu(), bias_ids.cpu(), bias_vals.cpu(), bias_n.cpu()
    rep, inv_rep, freq, pres = (t.detach().float().cpu() for t in (rep, inv_rep, freq, pres))
    for i, s in enumerate(slot.cpu().tolist()):
        if s < 0:
            continue
        x = out[i].float()
        c = state[s] >> 1
        r, ir, f, p = rep[i], inv_rep[i], freq[i], pres[i]  # 0-dim fp32 tensors: every product stays fp32
        if r != 1:
            x = torch.where(state[s] != 0, torch.where(x > 0, x * ir, x * r), x)
        m = f * c.float()
        x = x - m
        x = torch.where(c > 0, x - p, x)
        n = int(bias_n[s])
        if n:
            ids = bias_ids[s, :n].long()
            x[ids] = x[ids] + bias_vals[s, :n]
        out[i] = x.to(out.dtype)
    return out.to(logits.device)


def penalties_update(state: torch.Tensor, slot: torch.Tensor, tokens: torch.Tensor) -> None:
    """Record the sampled ``tokens`` (int32 [rows]): ``state[slot[r]][tokens[r]] += 2`` for the rows
    with ``slot[r] >= 0``.  Slots are unique among the rows of a step."""
    if _ext.use_hip(state):
        _ext.require().penalties_update(state, slot, tokens)
        return
    rows = slot >= 0
    state[slot[rows].long(), tokens[rows].long()] += 2


# ----------------------------------------------------------------------------------------------
# Structured outputs (the token mask of a byte-level DFA): csrc/guide.hip
# ----------------------------------------------------------------------------------------------
GUIDE_MAX_STATES = 4096  # rows of one grammar's transition table
GUIDE_EOS_MAX = 8  # EOS ids the mask looks at


def _guide_keep_ref(trans, accept_s: bool, s: int, off: list, blob: list, V: int, eos) -> torch.Tensor:
    """bool [V]: the tokens the grammar table ``trans`` (numpy uint16 [S, 256]) keeps in state ``s``."""
    keep = [False] * V
    for v in range(min(V, len(off) - 1)):
        b0, b1 = off[v], off[v + 1]
        if b0 < 0 or b1 <= b0 or b1 > len(blob):
            continue
        cur = s
        for i in range(b0, b1):
            cur = int(trans[cur, blob[i]])
            if cur >= GUIDE_MAX_STATES:
                cur = 0
            if cur == 0:
                break
        keep[v] = cur != 0
    if accept_s:
        for e in eos:
            if 0 <= e < V:
                keep[e] = True
    return torch.tensor(keep, dtype=torch.bool)


def apply_guide_ref(logits, guide, state, trans, accept, tok_off, tok_bytes, eos_ids, n_eos) -> torch.Tensor:
    """Reference of :func:`apply_guide`: a plain loop over rows, tokens and bytes on the CPU.  Returns
    a new tensor like ``logits`` (rows with ``guide < 0`` or an out-of-range guide / state are copies)."""
    import numpy as np

    out = logits.detach().cpu().clone()
    t16 = trans.detach().cpu()
    t16 = t16.view(torch.int16) if t16.dtype == torch.uint16 else t16
    acc, off, blob = accept.cpu(), tok_off.cpu().tolist(), tok_bytes.cpu().tolist()
    ne = max(0, min(int(n_eos.reshape(-1)[0]) if torch.is_tensor(n_eos) else int(n_eos), eos_ids.numel(), GUIDE_EOS_MAX))
    eos = eos_ids.cpu().tolist()[:ne]
    V = out.shape[1]
    for r, (g, s) in enumerate(zip(guide.cpu().tolist(), state.cpu().tolist())):
        if not (0 <= g < t16.shape[0] and 0 <= s < GUIDE_MAX_STATES):
            continue
        keep = _guide_keep_ref(t16[g].numpy().view(np.uint16), bool(acc[g, s]), s, off, blob, V, eos)
        out[r, ~keep] = float("-inf")
    return out.to(logits.device)


def apply_guide(logits: torch.Tensor, guide: torch.Tensor, state: torch.Tensor, trans: torch.Tensor,
                accept: torch.Tensor, tok_off: torch.Tensor, tok_bytes: torch.Tensor, eos_ids: torch.Tensor,
                n_eos: torch.Tensor) -> torch.Tensor:
    """Mask, in place, the logits of every row r with ``guide[r] >= 0`` (int32; -1: the row asks for
    nothing and is not written) by the byte-level DFA ``trans[guide[r]]`` (16-bit [G, 4096, 256],
    state 0 dead) / ``accept[guide[r]]`` (uint8 [G, 4096]) in state ``state[r]``.  Token v is kept iff

    * v is one of the first ``n_eos`` (int32 [1], at most 8) ids of ``eos_ids`` and the state accepts, or
    * v has at least one byte (``tok_bytes[tok_off[v] : tok_off[v + 1]]``; ids from ``len(tok_off) - 1``
      on have none) and walking its bytes from the state never reaches state 0.

    Every other logit becomes -inf; kept logits keep their bits.  A guide or state out of range leaves
    the row untouched.  On ROCm tensors nothing is allocated or read back (hipGraph-capturable).
    Returns ``logits``."""
    if _ext.use_hip(logits):
        if trans.dtype == torch.uint16:
            trans = trans.view(torch.int16)
        _ext.require().apply_guide(logits, guide, state, trans, accept, tok_off, tok_bytes, eos_ids, n_eos)
        return logits
    rows = guide >= 0
    if bool(rows.any()):
        ref = apply_guide_ref(logits, guide, state, trans, accept, tok_off, tok_bytes, eos_ids, n_eos)
        logits[rows] = ref[rows]
    return logits


# ----------------------------------------------------------------------------------------------
# Batched multi-LoRA projections: csrc/lora.hip
# ----------------------------------------------------------------------------------------------
LORA_RANKS = (8, 16, 32, 64)  # padded ranks the kernels take


def lora_shrink(x: torch.Tensor, A: torch.Tensor, idx: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """``t[r, j] = sum_k x[r, k] * A[idx[r], j, k]`` in fp32 for the rows with ``idx[r] >= 0`` (int32;
    -1: the row has no adapter and its row of ``t`` is not written).  ``x`` [T, K] (rows contiguous,
    any row stride), ``A`` [S, L, K] the stacked adapter weights, ``L = slices * R``.  Returns ``t``
    [T, L] fp32 (``out`` when given; otherwise zeros outside the written rows).  On ROCm tensors
    nothing is allocated when ``out`` is passed (hipGraph-capturable)."""
    T, L = x.shape[0], A.shape[1]
    if out is None:
        out = torch.zeros(T, L, dtype=torch.float32, device=x.device)
    if _ext.use_hip(x):
        _ext.require().lora_shrink(x, A, idx, out)
        return out
    rows = idx >= 0
    if bool(rows.any()):
        out[rows] = lora_shrink_ref(x, A, idx)[rows]
    return out


def lora_shrink_ref(x, A, idx) -> torch.Tensor:
    """Reference of :func:`lora_shrink`: fp32 [T, L], zeros in the rows with ``idx < 0``."""
    t = torch.zeros(x.shape[0], A.shape[1], dtype=torch.float32, device=x.device)
    for s in torch.unique(idx[idx >= 0]).tolist():
        rows = idx == s
        t[rows] = x[rows].float() @ A[s].float().t()
    return t


def lora_expand(t: torch.Tensor, B: torch.Tensor, idx: torch.Tensor, slice_ends, y: torch.Tensor) -> torch.Tensor:
    """In place, for the rows with ``idx[r] >= 0`` and every column n of slice j (columns
    ``slice_ends[j - 1] .. slice_ends[j]``): ``y[r, n] = dtype(float(y[r, n]) + sum_i t[r, j * R + i] *
    B[idx[r], n, i])`` -- the sum in fp32, one rounding.  ``t`` [T, slices * R] fp32, ``B`` [S, N, R]
    (``alpha / r`` folded in), ``y`` [T, N].  Rows with ``idx < 0`` are not written.  Returns ``y``."""
    if _ext.use_hip(y):
        _ext.require().lora_expand(t, B, idx, [int(e) for e in slice_ends], y)
        return y
    rows = idx >= 0
    if bool(rows.any()):
        y[rows] = lora_expand_ref(t, B, idx, slice_ends, y)[rows]
    return y


def lora_expand_ref(t, B, idx, slice_ends, y) -> torch.Tensor:
    """Reference of :func:`lora_expand`: a new tensor like ``y`` (rows with ``idx < 0`` are copies)."""
    out = y.clone()
    R = B.shape[2]
    for s in torch.unique(idx[idx >= 0]).tolist():
        rows = idx == s
        acc = y[rows].float()
        lo = 0
        for j, hi in enumerate(slice_ends):
            acc[:, lo:hi] += t[rows][:, j * R : (j + 1) * R].float() @ B[s, lo:hi].float().t()
            lo = hi
        out[rows] = acc.to(y.dtype)
    return out


def lora_runs(x: torch.Tensor, A: torch.Tensor, B: torch.Tensor, runs, slice_ends, y: torch.Tensor) -> torch.Tensor:
    """The prefill form: ``runs`` is a list of ``(slot, first row, end row)`` -- a prompt belongs to
    one request and hence one adapter -- and each run is two library GEMMs, ``x[run] @ A[slot]^T`` and
    an ``addmm_`` into each column slice of ``y[run]`` (the per-token kernels would stream ``A`` again
    for every row)."""
    R = B.shape[2]
    for s, a, b in runs:
        t = x[a:b] @ A[s].t()
        lo = 0
        for j, hi in enumerate(slice_ends):
            y[a:b, lo:hi].addmm_(t[:, j * R : (j + 1) * R], B[s, lo:hi].t())
            lo = hi
    return y


# ----------------------------------------------------------------------------------------------
# Decode-GEMM weight layout
# ----------------------------------------------------------------------------------------------
def fp8_stream_shuffle(wq: torch.Tensor, group: int = 16) -> torch.Tensor:
    """The weight layout of ``fp8_stream_gemm(..., shuffled=1 | 2)`` (``csrc/fp8_gemm.hip``): for each
    block of 16 weight rows and each 128-byte K-step, the 2 KiB that one MFMA fragment of a wave
    reads, in lane order -- half h (16 bytes of 32) of lane ``r + 16 g`` (row r, bytes 32 g .. 32 g + 32)
    at ``h * 1024 + lane * 16``.  Every weight load of the kernel is then 1 KiB contiguous.
    ``group`` 16 (shuffled=1): a block's pieces run consecutively over K; the workgroup's rows
    (shuffled=2: 256, or 224 for the 7-wave form): per K-step the blocks of one workgroup sit side
    by side (group x 128 bytes contiguous per workgroup and step).  ``wq`` [N][K] 1-byte, N % group == 0, K % 128 == 0; returns a contiguous
    [N][K] tensor of the same dtype (done once, when the weights are loaded)."""
    N, K = wq.shape
    assert group % 16 == 0 and N % group == 0 and K % 128 == 0 and wq.element_size() == 1, (
        tuple(wq.shape), wq.dtype, group)
    nb = group // 16
    b = wq.view(torch.uint8).reshape(N // group, nb, 16, K // 128, 4, 2, 16)  # (grp, blk, r, t, g, h, byte)
    return b.permute(0, 3, 1, 5, 4, 2, 6).contiguous().view(N, K).view(wq.dtype)


def fp8_stream_unshuffle(ws: torch.Tensor, group: int = 16) -> torch.Tensor:
    """Inverse of :func:`fp8_stream_shuffle` (tests)."""
    N, K = ws.shape
    nb = group // 16
    b = ws.view(torch.uint8).reshape(N // group, K // 128, nb, 2, 4, 16, 16)  # (grp, t, blk, h, g, r, byte)
    return b.permute(0, 2, 5, 1, 4, 3, 6).contiguous().view(N, K).view(ws.dtype)


def mxfp4_shuffle(codes: torch.Tensor, scales: torch.Tensor):
    """The stored form of a canonical MXFP4 weight (``ops.reference.quant_mxfp4``: ``codes`` [N, K/2],
    ``scales`` [N, K/32], uint8) -- the order ``mxfp4_gemm`` (``csrc/mxfp4.hip``) streams it in.  Lane
    ``r + 16 g`` of a wave holds weight row r of a 16-row block and K elements [32 g, 32 g + 32) of a
    128-wide K-step (one MX block):

    * codes: per 16-row block and K-step, the 1 KiB of the 64 lanes' 16 bytes in lane order, the
      steps of a block consecutive over K (the nibble order within a byte is the canonical one);
    * scales: per 16-row block and group of 4 K-steps, the 256 B of the 64 lanes' dwords in lane
      order, byte j of a dword the scale of step 4 G + j.

    N % 16 == 0, K % 32 == 0.  K is padded to a multiple of 512 (Kp) with zero codes, so that every
    K-step and scale dword is whole; returns contiguous (codes [N, Kp/2], scales [N, Kp/32]) (done
    once, when the weights are loaded; the engine keeps only this form)."""
    N, K2 = codes.shape
    K = 2 * K2
    assert N % 16 == 0 and K % 32 == 0 and tuple(scales.shape) == (N, K // 32), (tuple(codes.shape), tuple(scales.shape))
    assert codes.dtype == torch.uint8 and scales.dtype == torch.uint8
    pad = -K % 512
    if pad:
        codes = torch.nn.functional.pad(codes, (0, pad // 2))
        scales = torch.nn.functional.pad(scales, (0, pad // 32), value=127)
        K, K2 = K + pad, K2 + pad // 2
    c = codes.reshape(N // 16, 16, K // 128, 4, 16)  # (blk, r, t, g, byte)
    c = c.permute(0, 2, 3, 1, 4).contiguous().view(N, K2)  # (blk, t, g, r, byte)
    s = scales.reshape(N // 16, 16, K // 512, 4, 4)  # (blk, r, G, j, g)
    s = s.permute(0, 2, 4, 1, 3).contiguous().view(N, K // 32)  # (blk, G, g, r, j)
    return c, s


def mxfp4_unshuffle(codes: torch.Tensor, scales: torch.Tensor, K: int | None = None):
    """Inverse of :func:`mxfp4_shuffle`: the canonical (codes, scales) of a stored weight; ``K``: the
    weight's K where the stored form is padded."""
    N, K2 = codes.shape
    Kp = 2 * K2
    c = codes.reshape(N // 16, Kp // 128, 4, 16, 16).permute(0, 3, 1, 2, 4).contiguous().view(N, K2)
    s = scales.reshape(N // 16, Kp // 512, 4, 16, 4).permute(0, 3, 1, 4, 2).contiguous().view(N, Kp // 32)
    if K is not None and K != Kp:
        c, s = c[:, : K // 2].contiguous(), s[:, : K // 32].contiguous()
    return c, s


W4_NIBBLE_ORDER = (0, 2, 4, 6, 1, 3, 5, 7)  # nibble p of a stored dword holds K element W4_NIBBLE_ORDER[p] of its 8


def w4_shuffle(codes: torch.Tensor, zeros: torch.Tensor, scales: torch.Tensor, g: int):
    """The stored form of a canonical W4 weight (``ops.reference.unpack_awq`` / ``quant_w4``: ``codes``
    uint8 [N, K/2], ``zeros`` uint8 [N, K/g], ``scales`` fp16 [N, K/g]) -- the order ``w4_gemm``
    (``csrc/w4.hip``) streams it in.  A K-step is 128 elements: four 32-wide MFMA steps ``kk``.  Lane
    ``r + 16 gq`` of a wave holds weight row r of a 16-row block and, of MFMA step kk, the K elements
    ``[128 t + 32 kk + 8 gq, + 8)``; its accumulator holds rows ``4 gq + e`` (e = 0..3) of the block:

    * codes: per 16-row block and K-step the 1 KiB of the 64 lanes' 16 bytes in lane order, the steps
      of a block consecutive over K.  A lane's dword kk holds its 8 elements of MFMA step kk, element
      ``(0, 2, 4, 6, 1, 3, 5, 7)[p]`` in nibble p (bits 4p .. 4p+3): ``(dword >> 4 i) & 0x000F000F`` is
      then elements 2i (low half) and 2i + 1 (high half), one MFMA operand register;
    * scales (fp16) and zeros (one byte each, holding ``128 + z``: the kernel multiplies bf16 values
      ``128 + q`` and subtracts that): per 16-row block and K-step, for lane group gq = 0..3, for each
      of the step's 128 / g groups G, the values of rows ``4 gq + e``, e = 0..3 -- the ``8 * 128 / g``
      and ``4 * 128 / g`` bytes a lane loads at once, at ``((b * steps + t) * 4 + gq)`` times that size.

    N % 16 == 0, K % g == 0, g in (32, 64, 128).  K is padded to a multiple of 128 (Kp) with zero
    codes, zeros and scales; returns contiguous (codes [N, Kp/2], zeros [N, Kp/g], scales [N, Kp/g])
    (done once, when the weights are loaded; the engine keeps only this form).  Stored bytes:
    ``N Kp / 2 + N Kp / g * (2 + 1)`` -- a zero point takes a byte, not a nibble."""
    N, K2 = codes.shape
    K = 2 * K2
    assert g in (32, 64, 128) and N % 16 == 0 and K % g == 0, (N, K, g)
    assert tuple(zeros.shape) == (N, K // g) and tuple(scales.shape) == (N, K // g), (zeros.shape, scales.shape)
    assert codes.dtype == torch.uint8 and zeros.dtype == torch.uint8 and scales.dtype == torch.float16
    pad = -K % 128
    if pad:
        codes = torch.nn.functional.pad(codes, (0, pad // 2))
        zeros = torch.nn.functional.pad(zeros, (0, pad // g))
        scales = torch.nn.functional.pad(scales, (0, pad // g))
        K, K2 = K + pad, K2 + pad // 2
    T, GS = K // 128, 128 // g
    q = torch.stack([codes & 15, codes >> 4], dim=-1).reshape(N // 16, 16, T, 4, 4, 8)  # (blk, r, t, kk, gq, j)
    q = q.permute(0, 2, 4, 1, 3, 5)[..., list(W4_NIBBLE_ORDER)]  # (blk, t, gq, r, kk, p)
    c = (q[..., 0::2] | (q[..., 1::2] << 4)).contiguous().view(N, K2)
    z = (zeros + 128).reshape(N // 16, 4, 4, T, GS).permute(0, 3, 1, 4, 2).contiguous().view(N, K // g)  # (blk, t, gq, G, e)
    s = scales.reshape(N // 16, 4, 4, T, GS).permute(0, 3, 1, 4, 2).contiguous().view(N, K // g)
    return c, z, s


def w4_unshuffle(codes: torch.Tensor, zeros: torch.Tensor, scales: torch.Tensor, g: int, K: int | None = None):
    """Inverse of :func:`w4_shuffle`: the canonical (codes, zeros, scales) of a stored weight; ``K``: the
    weight's K where the stored form is padded."""
    N, K2 = codes.shape
    Kp = 2 * K2
    T, GS = Kp // 128, 128 // g
    p = torch.stack([codes & 15, codes >> 4], dim=-1).reshape(N // 16, T, 4, 16, 4, 8)  # (blk, t, gq, r, kk, p)
    inv = sorted(range(8), key=W4_NIBBLE_ORDER.__getitem__)
    q = p[..., inv].permute(0, 3, 1, 4, 2, 5).reshape(N, K2, 2)  # (blk, r, t, kk, gq, j)
    c = (q[..., 0] | (q[..., 1] << 4)).contiguous()
    z = (zeros - 128).reshape(N // 16, T, 4, GS, 4).permute(0, 2, 4, 1, 3).contiguous().view(N, Kp // g)
    s = scales.reshape(N // 16, T, 4, GS, 4).permute(0, 2, 4, 1, 3).contiguous().view(N, Kp // g)
    if K is not None and K != Kp:
        c, z, s = c[:, : K // 2].contiguous(), z[:, : K // g].contiguous(), s[:, : K // g].contiguous()
    return c, z, s
