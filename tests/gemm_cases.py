"""Operands for which the training GEMMs are exact, the exact reference, a comparison that says where
a mismatch sits, models of the defects these kernels get, and a model of the launch plan.

Used by ``tests/test_gemm_exact.py`` for ``csrc/gemm_nt.hip`` (NT, KM, e4m3 and the fused epilogues)
and ``csrc/gemm.hip`` (TN).  Nothing here needs a GPU.

**Operands.**  A [M, K] has entries in {-1, 0, +1} (uniform signs, non-zero with probability
``min(1, 4096 / K)``), B [N, K] entries in {-1, +1}; the generator is seeded from the shape.  Every
product and every partial sum, in any order, is an integer below 2^24: the MFMA accumulation, a K
split and an fp32 workspace are all exact, and the one ``f2bf`` (round to nearest even) of the
epilogue is the only rounding.  Integers up to 256 are exact in bf16, so a lost, extra or mis-paired
k-term changes the stored value; ``check_cap`` asserts per case that at most 1e-3 of the outputs
exceed 256 in magnitude (a condition on the inputs, not a tolerance on the kernel).  The KM and TN
forms take the same values transposed (``a.t()``: [K, M]), the e4m3 form the same values as e4m3.

**Plants.**  With i.i.d. operands a K-half partial is N(0, <= 2048): it never leaves the range in
which bf16 holds every integer, so an extra bf16 rounding of a partial could not be seen.  At
K >= 2048 one output per 256x256 tile is therefore planted: row r of A repeats row c of B (on A's own
non-zero pattern) so that the first K half sums to +601 or +602 (its parity is that of the row's
non-zero count) and the second to -601 or -602.  Neither is a bf16 value (600 and 604 are), the total
is -1, 0 or 1, the value sets and the cap are unchanged.

**Reference.**  ``product(a, b) = a.double() @ b.double().T`` (+ the accumulator's integers in
[-32, 32]), converted once to bf16 (``to_bf16``); the comparison is ``torch.equal``.
"""

from __future__ import annotations

import functools
from types import SimpleNamespace

import torch

BF16, E4M3, F32, F64 = torch.bfloat16, torch.float8_e4m3fn, torch.float32, torch.float64
TILE, BK = 256, 64
CAP_VALUE, CAP_SHARE = 256, 1e-3
OLD_BOUND = 5e-3  # the older tests' bound on ||out - ref|| / ||ref||
PLANT_K, PLANT = 2048, 601


def to_bf16(x: torch.Tensor) -> torch.Tensor:
    """The one rounding: fp64 integers below 2^24 are exact in fp32, fp32 -> bf16 rounds to nearest even."""
    return x.to(F32).to(BF16)


def rb(x: torch.Tensor) -> torch.Tensor:
    return to_bf16(x).to(F64)


def product(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a [M, K] b [N, K]^T in fp64, on the operands' device."""
    return a.to(F64) @ b.to(F64).t()


def check_cap(ref: torch.Tensor) -> float:
    share = (ref.abs() > CAP_VALUE).double().mean().item()
    assert share <= CAP_SHARE, f"{share:.2e} of the outputs exceed {CAP_VALUE}: the operands are too dense"
    return share


def _seed(*dims: int) -> int:
    s = 0x5EED
    for d in dims:
        s = (s * 1000003 + int(d)) % (2 ** 62)
    return s


def plant_sites(M: int, N: int):
    """One (row, column) per 256x256 tile; rows and columns are each used once."""
    ntm, ntn = M // TILE, N // TILE
    return [(TILE * tm + (7 * tn + 3) % TILE, TILE * tn + (11 * tm + 5) % TILE)
            for tm in range(ntm) for tn in range(ntn) if tn < TILE and tm < TILE]


def _plant(a: torch.Tensor, b: torch.Tensor, r: int, c: int):
    K = a.shape[1]
    for h, sign in ((0, 1.0), (1, -1.0)):
        ks = torch.arange(h * K // 2, (h + 1) * K // 2)
        nz = ks[a[r, ks] != 0]
        assert nz.numel() > PLANT + 1
        agree = torch.ones(nz.numel(), dtype=F64)  # PLANT agreeing terms, then + - + - ...: 0 or 1 more
        agree[PLANT + 1::2] = -1.0
        a[r, nz] = sign * agree * b[c, nz]


@functools.lru_cache(maxsize=4)
def operands(M: int, N: int, K: int, tag: int = 0):
    """(a [M, K], b [N, K], base [M, N]) in fp64 on the CPU; ``base``: the accumulator's integers."""
    g = torch.Generator().manual_seed(_seed(M, N, K, tag))
    sign = torch.randint(0, 2, (M, K), generator=g, dtype=torch.int8) * 2 - 1
    if K > 4096:
        sign = sign * (torch.rand(M, K, generator=g) < 4096 / K).to(torch.int8)
    a = sign.to(F64)
    b = (torch.randint(0, 2, (N, K), generator=g, dtype=torch.int8) * 2 - 1).to(F64)
    base = torch.randint(-32, 33, (M, N), generator=g, dtype=torch.int8).to(F64)
    if K >= PLANT_K:
        for r, c in plant_sites(M, N):
            _plant(a, b, r, c)
    return a, b, base


def e4m3_bytes(x: torch.Tensor) -> torch.Tensor:
    return x.to(F32).to(E4M3).view(torch.uint8)


def check_operands(a, b, base, K: int):
    """The builder's invariants: value sets, density, exact bf16 and e4m3 round trips."""
    assert set(a.unique().tolist()) <= {-1.0, 0.0, 1.0} and set(b.unique().tolist()) == {-1.0, 1.0}
    dens = (a != 0).double().mean().item()
    want = min(1.0, 4096 / K)
    assert abs(dens - want) <= 0.01, (dens, want)
    if want == 1.0:
        assert dens == 1.0
    assert abs(a.sum().item()) <= 6 * a.numel() ** 0.5 and abs(b.sum().item()) <= 6 * b.numel() ** 0.5  # uniform signs
    assert base.abs().max().item() <= 32 and torch.equal(base, base.round())
    for x in (a, b, base):
        assert torch.equal(x.to(F32).to(BF16).to(F64), x)
    for x in (a, b):
        assert torch.equal(x.to(F32).to(E4M3).to(F64), x)
    assert set(e4m3_bytes(a).unique().tolist()) <= {0x00, 0x38, 0xB8} and set(e4m3_bytes(b).unique().tolist()) == {0x38, 0xB8}


@functools.lru_cache(maxsize=3)
def case(M: int, N: int, K: int, device: str = "cpu", tag: int = 0):
    """Operands and expected outputs of C (+)= A B^T on ``device`` (the fp64 matmul runs there).
    ``a``, ``b`` bf16 [M, K], [N, K]; ``base`` bf16 [M, N]; ``exact`` / ``exact_acc`` fp64 (product,
    base + product); ``want`` / ``want_acc`` their bf16 roundings.  Never modified by a test."""
    a64, b64, base64 = operands(M, N, K, tag)
    a, b, base = a64.to(device), b64.to(device), base64.to(device)
    exact = product(a, b)
    share = check_cap(exact)
    exact_acc = exact + base
    return SimpleNamespace(M=M, N=N, K=K, a=a.to(BF16), b=b.to(BF16), base=base.to(BF16), exact=exact,
                           exact_acc=exact_acc, want=to_bf16(exact), want_acc=to_bf16(exact_acc), share=share)


def halves(c):
    """fp64 products over the first and the second K half (what a split tile's two units hold)."""
    h = c.K // 2
    return product(c.a[:, :h], c.b[:, :h]), product(c.a[:, h:], c.b[:, h:])


# ==================================================================================================
# The comparison
# ==================================================================================================
def _fmt(s, limit=24):
    s = sorted(s)
    return str(s) if len(s) <= limit else f"{s[:limit]} ... ({len(s)} in all)"


def mismatch_report(out: torch.Tensor, want: torch.Tensor, tile: int = TILE, exact=None, halves=None) -> str | None:
    """None when ``out`` equals ``want`` element for element, else where it does not: the count, the
    tiles hit, the wave / sub-tile coordinates inside the worst tile (gemm_nt.hip's header: wave
    (wr, wc) owns rows 64 wr + [0, 64) of each 128-row half in 16-row fragments and columns
    32 wc + [0, 32) of each 128-column half in 16-column fragments), the first eight elements, and
    (with ``exact``, the fp64 value before rounding, and ``halves``, a callable giving the two K-half
    products) whether leaving out a K half explains it.  Never a whole tensor."""
    assert out.shape == want.shape, (out.shape, want.shape)
    assert out.dtype == want.dtype, (out.dtype, want.dtype)
    if torch.equal(out, want):
        return None
    bad = out != want  # (a NaN differs from everything)
    idx = bad.nonzero()
    m, n = idx[:, 0], idx[:, 1]
    tm, tn = m // tile, n // tile
    ntn = (out.shape[1] + tile - 1) // tile
    tid, per = torch.unique(tm * ntn + tn, return_counts=True)
    tiles = [(int(t) // ntn, int(t) % ntn) for t in tid.tolist()]
    worst = int(tid[per.argmax()])
    sel = (tm * ntn + tn) == worst
    r, c = (m[sel] % tile), (n[sel] % tile)
    lines = [f"{idx.shape[0]} of {out.numel()} elements differ",
             f"tiles hit (tile row, tile column): {_fmt(tiles)}",
             f"worst tile {(worst // ntn, worst % ntn)}: {int(per.max())} elements;"
             f" row % 64 // 16 in {_fmt(set((r % 64 // 16).tolist()))}, row // 128 in {_fmt(set((r // 128).tolist()))},"
             f" col % 32 // 16 in {_fmt(set((c % 32 // 16).tolist()))}, col // 128 in {_fmt(set((c // 128).tolist()))},"
             f" rows {int(r.min())}..{int(r.max())}, columns {int(c.min())}..{int(c.max())}"]
    first = idx[:8].tolist()
    lines.append("first (m, n, got, want): " + ", ".join(
        f"({i}, {j}, {out[i, j].item():g}, {want[i, j].item():g})" for i, j in first))
    if exact is not None and halves is not None:
        got = out[bad]
        for h, part in enumerate(halves()):
            alt = (exact - part.to(exact.device))[bad].to(F32).to(out.dtype)
            k = int((alt == got).sum())
            lines.append(f"dropping K half {h} explains {k} of {idx.shape[0]} wrong elements"
                         + (" (all: the split path)" if k == idx.shape[0] else ""))
    return "\n  ".join(lines)


def assert_exact(out: torch.Tensor, want: torch.Tensor, tile: int = TILE, exact=None, halves=None, what: str = ""):
    rep = mismatch_report(out, want, tile, exact, halves)
    assert rep is None, f"{what + ': ' if what else ''}{rep}"


def old_metric(out: torch.Tensor, exact: torch.Tensor) -> float:
    """What the older GEMM tests bound by 5e-3: the relative Frobenius norm of the error."""
    return ((out.to(F64) - exact).norm() / exact.norm()).item()


def bf16_ulp(x: torch.Tensor) -> torch.Tensor:
    """Spacing of bf16 at ``x`` (8 significant bits; the smallest normal's below it), in fp64: the
    power of two at or below |x|, by clearing the fp64 mantissa (exact on any device, which a ``pow`` or
    ``ldexp`` on the GPU is not), times 2^-7."""
    p2 = (x.to(F64).abs().clamp_min(2.0 ** -126).view(torch.int64) & 0x7FF0000000000000).view(F64)
    return p2 * 2.0 ** -7


# ==================================================================================================
# Defect models: what the kernel would store, from the exact fp64 product of a case on the CPU
# ==================================================================================================
def _blk(r0, nr, c0, nc):
    return slice(r0, r0 + nr), slice(c0, c0 + nc)


def _sub(c, rows, cols, k0, k1):
    return product(c.a[rows, k0:k1], c.b[cols, k0:k1])


def defect(c, kind: str, tm: int = 0, tn: int = 0, tm2: int = 0, tn2: int = 0) -> tuple[torch.Tensor, torch.Tensor]:
    """(stored, wanted) bf16 outputs with defect ``kind`` in tile (tm, tn); ``(tm2, tn2)``: the
    other tile of an exchange.  The site inside the tile is wave (1, 2)'s second m-subtile."""
    r0, c0 = TILE * tm, TILE * tn
    K = c.K
    acc = kind == "base_dropped"
    p = (c.exact_acc if acc else c.exact).clone()
    want = c.want_acc if acc else c.want
    fr, fc = r0 + 128 + 64 + 16, c0 + 64 + 16  # a 16x16 fragment of wave (wr 1, wc 2)
    if kind == "k_term":            # (a) one k-term lost in one fragment
        k = K // 2 + 5
        rows, cols = _blk(fr, 16, fc, 16)
        p[rows, cols] -= _sub(c, rows, cols, k, k + 1)
    elif kind == "stale_slot":      # (b) one K-tile of one 64x32 quadrant read from the slot's previous tile
        kt = K // BK - 1
        rows, cols = _blk(r0 + 128 + 64, 64, c0 + 64, 32)
        p[rows, cols] += _sub(c, rows, cols, (kt - 1) * BK, kt * BK) - _sub(c, rows, cols, kt * BK, (kt + 1) * BK)
    elif kind == "row_swap":        # (c) rows r and r ^ 1 of one fragment exchanged
        p[[fr + 6, fr + 7], fc:fc + 16] = p[[fr + 7, fr + 6], fc:fc + 16]
    elif kind == "half_missing":    # (d) a split tile without its second K half
        rows, cols = _blk(r0, TILE, c0, TILE)
        p[rows, cols] -= _sub(c, rows, cols, K // 2, K)
    elif kind == "tiles_exchanged":  # (e) two tiles written to each other's place
        assert (tm, tn) != (tm2, tn2)
        (ra, ca), (rb_, cb) = _blk(r0, TILE, c0, TILE), _blk(TILE * tm2, TILE, TILE * tn2, TILE)
        x = p[ra, ca].clone()
        p[ra, ca] = p[rb_, cb]
        p[rb_, cb] = x
    elif kind == "base_dropped":    # (f) an accumulating tile that stored instead
        rows, cols = _blk(r0, TILE, c0, TILE)
        p[rows, cols] = c.exact[rows, cols]
    elif kind == "partial_rounded":  # (g) a split tile whose first K-half partial went through bf16
        rows, cols = _blk(r0, TILE, c0, TILE)
        p[rows, cols] = rb(_sub(c, rows, cols, 0, K // 2)) + _sub(c, rows, cols, K // 2, K)
    else:
        raise ValueError(kind)
    return to_bf16(p), want


DEFECTS = ["k_term", "stale_slot", "row_swap", "half_missing", "tiles_exchanged", "base_dropped", "partial_rounded"]


# ==================================================================================================
# The launch plan of nt_launch and the kernel's prologue (csrc/gemm_nt.hip)
# ==================================================================================================
def nt_group(ntm: int, ntn: int) -> int:
    g = 4 if ntm > 2 * ntn else 8
    return g if ntm >= g else ntm


def plan(M: int, N: int, K: int, cus: int, grid_mode: int = -1, *, ncol: int = TILE, split_epi: bool = True,
         persistent_env: bool = True, split_env: bool = True, dynamic_env: bool = False, group_env: int = 0):
    """What a launch does: ``grid_mode`` as ``gemm_nt_set_grid`` (-1: the environment's default,
    ``persistent_env``); ``ncol``: output columns per tile (256; 128 for the SwiGLU forward);
    ``split_epi``: the epilogue is one the split-remainder path runs (plain and fp32-accumulator).
    K in 2-byte units (the e4m3 form: bytes / 2).  Per XCD x: ``cnt`` tiles, ``rounds``, ``rx`` tiles
    in a part-filled last round, ``splits`` (that round runs as K halves)."""
    ntm, ntn = M // TILE, N // ncol
    tiles, cap, nk = ntm * ntn, cus // 8 * 8, K // BK
    want_persistent = grid_mode == 1 if grid_mode >= 0 else persistent_env
    persistent = want_persistent and tiles > cap and cap >= 8
    stride = cap // 8 if persistent else 1 << 30
    per, rem = tiles >> 3, tiles & 7
    cnt = [per + (1 if x < rem else 0) for x in range(8)]
    queue = persistent and dynamic_env
    rx_launch = (tiles + 7) // 8 % stride
    ws = (persistent and split_env and not queue and split_epi and rx_launch > 0 and 2 * rx_launch <= stride
          and nk % 4 == 0)
    rx = [n % stride if persistent else 0 for n in cnt]
    splits = [bool(ws and r > 0 and 2 * r <= stride and nk % 4 == 0) for r in rx]
    group = group_env if group_env > 0 else nt_group(ntm, ntn)
    heights = [min(group, ntm - g) for g in range(0, ntm, group)]  # the last group is clipped
    return SimpleNamespace(ntm=ntm, ntn=ntn, tiles=tiles, cap=cap, grid=cap if persistent else tiles,
                           persistent=persistent, stride=stride if persistent else None, cnt=cnt,
                           rounds=[-(-n // stride) if persistent else min(n, 1) for n in cnt], rx=rx,
                           workspace=ws, splits=splits, queue=queue, group=group, heights=heights, nk=nk)


def tile_origins(p) -> list[tuple[int, int]]:
    """(tile row, tile column) of every logical tile, in order (``nt_tile_origin``)."""
    out = []
    in_group = p.group * p.ntn
    for t in range(p.tiles):
        first_m = t // in_group * p.group
        gm = min(p.ntm - first_m, p.group)
        out.append((first_m + t % in_group % gm, t % in_group // gm))
    return out


# --- the shapes of the tests and the path each is there for ---------------------------------------
# "basic": few tiles; (2304, 9472) has 333 (two rounds on 256 CUs, rx 10 and 9) but sits here as
# the older tests' shape, without a claim
BASIC_SHAPES = [(256, 256), (512, 768), (2304, 9472)]
KS = [128, 256, 384, 1024]  # prologue + one iteration; smallest split K; (K / 64) % 4 != 0; several iterations
LONG_K = [(1024, 4096, 4096), (1024, 4096, 8192), (1024, 4096, 14336)]


def _eligible(p):
    return p.nk % 4 == 0


def _claim_4352x4096(p):
    assert p.tiles == 272 and set(p.rx) == {2}, "rx = 2 on every XCD"
    assert p.group == 8 and p.heights[-1] == 1 and p.ntm == 17, "ragged last tile group (17 tile rows, group 8)"
    assert all(p.splits) == _eligible(p) and any(p.splits) == _eligible(p)


def _claim_3072x8192(p):
    assert p.tiles == 384 and all(2 * r == p.stride for r in p.rx), "rx = stride / 2, the largest split remainder"
    assert all(p.splits) == _eligible(p)


def _claim_3328x8192(p):
    assert p.tiles == 416 and set(p.rx) == {20} and p.stride == 32, "rx = 20"
    assert not any(p.splits) and set(p.rounds) == {2}, "the part-filled last round stays whole"


def _claim_512x33024(p):
    assert p.tiles == 258 and p.rx == [1, 1, 0, 0, 0, 0, 0, 0], "XCDs 0 and 1 hold one tile more"
    assert p.splits == [_eligible(p)] * 2 + [False] * 6, "XCDs 0 and 1 split, 2-7 have nothing to split"
    assert p.group == 2 and p.ntm == 2, "group clipped to the 2 tile rows"


def _claim_4352x4352(p):
    assert p.tiles == 289 and p.cnt == [37] + [36] * 7 and p.rx == [5] + [4] * 7, "unequal XCD slices, rx 5 and 4"
    assert all(p.splits) == _eligible(p)


def _claim_17408x1024(p):
    assert p.tiles == 272 and p.group == 4 and set(p.rx) == {2}, "group 4"
    assert all(p.splits) == _eligible(p)


MULTI_ROUND = {(4352, 4096): _claim_4352x4096, (3072, 8192): _claim_3072x8192, (3328, 8192): _claim_3328x8192,
               (512, 33024): _claim_512x33024, (4352, 4352): _claim_4352x4352, (17408, 1024): _claim_17408x1024}
GROUPS = [1, 3, 16]  # DSTACK_AMD_GEMM_NT_GROUP on (4352, 4096)


def reach(M: int, N: int, K: int, cus: int, grid_mode: int, **kw):
    """The plan of a multi-round case, or an AssertionError that names the path it no longer reaches
    (the table's claims are about the kernel's own tile-order group, whatever ``group_env`` is)."""
    p = plan(M, N, K, cus, grid_mode, **kw)
    d = plan(M, N, K, cus, grid_mode, **{**kw, "group_env": 0})
    what = f"{M}x{N}, K = {K}, {cus} CUs, grid mode {grid_mode}"
    assert p.tiles > p.cap >= 8, (f"{what}: the case no longer reaches its path: {p.tiles} tiles do not outnumber the "
                                 f"{p.cap} workgroups of a persistent grid")
    if grid_mode == 0:
        assert not p.persistent and p.grid == p.tiles and not any(p.splits), what
        return p
    assert p.persistent and p.grid == p.cap, what
    try:
        MULTI_ROUND[(M, N)](d)
        assert (p.cnt, p.rx, p.splits) == (d.cnt, d.rx, d.splits)
    except AssertionError as e:
        raise AssertionError(f"{what}: the case no longer reaches its path ({e}); cnt {p.cnt}, rx {p.rx}, "
                             f"splits {p.splits}, group {p.group}") from None
    return p
