"""The small linears of csrc/small_linear.hip through the C ABI against float64 references on the same rounded inputs: the MoE
router's skinny linear (apertis_skinny_linear_fwd / _bwd) and the SSM's dt_proj_head tiny linear (apertis_tiny_linear_fwd,
apertis_tiny_linear_doc_fwd, apertis_tiny_linear_bwd / _bwd_pad).

Reference: float64 F.linear on the inputs as the kernel reads them (x rounded to its dtype), float64 autograd for dx, dW, db.

Skinny: a template on (dtype, IT = ceil(K / 256), NN = N); every accepted triple has a case, at K whose last 256-column pass
is partial (4, 260, 704) and full (256, 1024), with and without a bias, at T = 1 (three idle waves of the block), 7, 33 (a
ragged last block; no multiple of the backward's 8 rows per wave) and, backward only, T = 0 (the launch leaves zeros); one
case runs past the forward's 4096-block cap, one (N = 8, K = 1024) asks the backward for 96 KiB of dynamic LDS.

Tiny: the forward takes a thread-per-output kernel at T <= 64 and the LDS kernel above, the latter with 16-byte row loads
(VEC) or element loads; VEC is refused for an unaligned base, a row pitch that is no multiple of 16 bytes, or a slice whose
rounded-up chunks pass the row - the mirror below shows that the last never happens alone (a pitch of whole chunks that holds
K elements holds their chunks), so it is met together with the pitch.  x is always a column slice of a wider NaN-filled
buffer: a chunk mask that lets a neighbour column in shows as NaN.  The backward adds the alignment of dx and its pitch, odd N
(the 2 x 4 ownership of dW), K % 4 != 0, T on both sides of a 128-row tile, a walk of two tiles per block past the
1024-block cap with a ragged last tile, and the zero fill of [K, zero_to) in its three forms (vector, vector + tail, scalar).

Tolerances are the project's (tests/test_row_kernels_gpu.py): fp32 outputs rtol 1e-4 with a floor of 1e-5 of the tensor's
largest entry, bf16 dx one bf16 rounding (rtol 8e-3), dW and db _sum_close's 1.6e-4 sqrt(T).  Every output is carved from a
NaN-filled buffer whose guards must still be NaN; the partial-row workspaces start NaN."""
import pytest
import torch
import torch.nn.functional as F

from test_row_kernels_gpu import BF16, F32, NAN, OK, _close, _code, _lib, _sum_close, _tag

gpu = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------------------------------
# mirror of the dispatch in csrc/small_linear.hip and of SKINNY_N / SKINNY_IT in csrc/row_common.h: a change there must be made
# here too, and then test_case_tables_cover_every_dispatch_path says whether the cases still reach every path
SK_NS, SK_MAXK, SK_RPW = (2, 4, 8, 16), 1024, 8
SK_FWD_ROWS_PER_BLOCK, SK_FWD_BLOCK_CAP = 8, 4096      # grid = min(ceil(T / 8), 4096) blocks of four waves, a row per wave and pass
SK_BWD_ROWS_PER_BLOCK = 4 * SK_RPW
TL_MAXK, TL_MAXN, TL_ROWS = 64, 16, 128
TL_SMALL_T, TL_FWD_BLOCK_CAP, TL_BWD_BLOCK_CAP = 64, 4096, 1024


def _sk_ok(K, N):
    return 0 < K <= SK_MAXK and K % 4 == 0 and N in SK_NS and not (N > 8 and K > 256)


def _sk_it(K):
    return -(-K // 256)


def _sk_bwd_lds(K, N):
    """Dynamic LDS of skinny_bwd_k: three waves' [N][K] fp32 sums."""
    return 3 * N * K * 4


def _sk_fwd_passes(T):
    """Most rows a wave of skinny_fwd_k walks."""
    waves = 4 * min(-(-T // SK_FWD_ROWS_PER_BLOCK), SK_FWD_BLOCK_CAP)
    return -(-T // waves)


def _esz(dt):
    return 2 if dt == BF16 else 4


def _tl_novec(dt, K, ldx, offx, lddx=None, offdx=0):
    """The set of reasons the entry points refuse 16-byte row accesses (empty: VEC).  off*: elements between a 16-byte boundary
    and the operand's first element."""
    e = _esz(dt)
    epc = 16 // e
    why = set()
    if (offx * e) % 16:
        why.add("x-base")
    if (ldx * e) % 16:
        why.add("x-pitch")
    if -(-K // epc) * epc > ldx:
        why.add("x-overrun")
    if lddx is not None:
        if (offdx * e) % 16:
            why.add("dx-base")
        if (lddx * e) % 16:
            why.add("dx-pitch")
    return frozenset(why)


def _tl_fwd_path(T, dt, K, ldx, offx):
    if T <= TL_SMALL_T:
        return "small"
    return "lds-vec" if not _tl_novec(dt, K, ldx, offx) else "lds-elem"


def _tl_fwd_passes(T):
    return -(-T // (TL_ROWS * min(-(-T // TL_ROWS), TL_FWD_BLOCK_CAP)))


def _tl_bwd_tiles(T):
    """(blocks, row tiles): a block walks more than one tile when there are more tiles than blocks."""
    tiles = -(-max(T, 1) // TL_ROWS)
    return min(tiles, TL_BWD_BLOCK_CAP), tiles


def _tl_fill(dt, K, ldx, offx, lddx, offdx, zero_to):
    """The form of tiny_linear_bwd_k's zero fill of [K, zero_to): the set of 'vector' / 'scalar' stores it makes."""
    zero_to = max(zero_to, K)
    if zero_to == K:
        return frozenset()
    if _tl_novec(dt, K, ldx, offx, lddx, offdx) or K % 4:
        return frozenset({"scalar"})
    n = zero_to - K
    return frozenset((["vector"] if n >= 4 else []) + (["scalar"] if n % 4 else []))


# ---------------------------------------------------------------------------------------------------------------------------
# case tables
SK_KS = (4, 256, 260, 704, 1024)


def _skinny_cases():
    """(K, N, dtype, T, bias): every accepted (dtype, IT, NN), T and the bias cycling; then the named cases."""
    out, i = [], 0
    for dt in (F32, BF16):
        for K in SK_KS:
            for N in SK_NS:
                if _sk_ok(K, N):
                    out.append((K, N, dt, (1, 7, 33)[i % 3], i % 4 != 1))
                    i += 1
    out += [(4, 2, F32, 32768 + 9, True),                              # past the forward's block cap: a wave walks three rows
            (1024, 8, F32, 33, True), (1024, 8, BF16, 7, False),       # the backward's largest LDS request
            (512, 4, BF16, 13, True), (768, 2, F32, 13, False), (1020, 8, F32, 5, True),   # full IT 2 / 3, ragged IT 4
            (4, 2, F32, 0, True), (260, 4, BF16, 0, False), (256, 16, F32, 0, True)]       # T = 0: the backward only
    return out


SK_CASES = _skinny_cases()

# tiny forward: (T, K, N, dtype, ldx, offx, bias)
TL_BIG_T = 524288 + 130
TL_FWD_CASES = [
    # the T <= 64 kernel
    (1, 22, 11, BF16, 48, 0, True), (64, 44, 16, F32, 44, 0, True), (64, 3, 1, BF16, 3, 1, False), (1, 64, 15, F32, 64, 0, True),
    (64, 63, 2, BF16, 64, 0, True), (7, 8, 11, F32, 9, 1, False),
    # the LDS kernel with 16-byte row loads
    (65, 22, 11, BF16, 48, 0, True), (65, 4, 2, F32, 4, 0, True), (65, 8, 16, BF16, 8, 0, False), (130, 64, 16, F32, 64, 0, True),
    (257, 64, 15, BF16, 72, 0, True), (65, 63, 1, F32, 64, 0, True), (65, 1, 1, BF16, 8, 0, True), (65, 3, 2, F32, 4, 0, False),
    (129, 44, 11, F32, 48, 0, True), (65, 44, 11, BF16, 48, 0, True), (65, 22, 15, F32, 24, 0, True),
    # element loads: the base off a 16-byte boundary
    (65, 22, 11, BF16, 48, 1, True), (65, 8, 2, F32, 8, 1, True),
    # element loads: a row pitch that is no multiple of 16 bytes (the rounded-up slice still inside the row)
    (65, 22, 11, F32, 25, 0, True), (65, 22, 11, BF16, 25, 0, True),
    # element loads: the rounded-up slice passes the row (and then the pitch is no whole number of chunks either)
    (65, 22, 2, F32, 22, 0, True), (65, 63, 15, BF16, 63, 0, True), (65, 1, 1, F32, 1, 0, True), (65, 3, 16, BF16, 3, 0, False),
    (66, 44, 11, BF16, 44, 0, True),
    # past the 4096-block cap: the threads of block 0 and two of block 1 walk a second row
    (TL_BIG_T, 1, 1, F32, 1, 0, True),
]

# the T = 64 kernel against the LDS kernel, bit for bit: (K, N, dtype, ldx, offx, bias)
TL_SAME_BITS_CASES = [(22, 11, BF16, 48, 0, True), (64, 16, F32, 64, 0, True), (63, 15, BF16, 63, 0, True), (3, 2, F32, 4, 0, False),
                      (44, 11, F32, 45, 1, True)]

# tiny backward: (T, K, N, dtype, ldx, offx, lddx, offdx, zero_to); zero_to None = apertis_tiny_linear_bwd (no fill)
TL_BWD_BIG_T = 131072 + 130


def _tiny_bwd_cases():
    out = [
        # 16-byte accesses on both sides
        (129, 22, 11, BF16, 48, 0, 48, 0, None), (127, 4, 2, F32, 4, 0, 4, 0, None), (1, 64, 16, F32, 64, 0, 64, 0, None),
        (129, 64, 15, BF16, 64, 0, 72, 0, None), (127, 44, 1, BF16, 48, 0, 48, 0, None), (129, 63, 3, F32, 64, 0, 64, 0, None),
        (1, 8, 16, BF16, 8, 0, 8, 0, None), (300, 3, 5, F32, 4, 0, 4, 0, None),
        # element accesses, one reason at a time: x base, x pitch, the slice past the row, dx base, dx pitch
        (129, 22, 11, BF16, 48, 1, 48, 0, None), (127, 8, 2, F32, 8, 1, 8, 0, None),
        (129, 22, 11, F32, 25, 0, 24, 0, None), (127, 22, 11, BF16, 25, 0, 24, 0, None),
        (129, 22, 3, F32, 22, 0, 24, 0, None), (127, 63, 15, BF16, 63, 0, 64, 0, None),
        (129, 22, 11, BF16, 48, 0, 48, 1, None), (127, 8, 2, F32, 8, 0, 8, 1, None),
        (129, 22, 11, F32, 24, 0, 25, 0, None), (127, 22, 11, BF16, 24, 0, 25, 0, None), (1, 1, 1, F32, 1, 0, 1, 0, None),
        # nothing to sum: dW and db are zeros, dx is not touched
        (0, 22, 11, BF16, 48, 0, 48, 0, None), (0, 4, 2, F32, 4, 0, 8, 0, 8),
        # past the 1024-block cap: blocks 0 and 1 walk a second tile, the last one of two rows
        (TL_BWD_BIG_T, 4, 2, F32, 4, 0, 4, 0, None),
    ]
    # the zero fill: zero_to below K (clamped), K, K + 1, K + 4, K + 6 and lddx on 16-byte rows with K % 4 == 0, on 16-byte
    # rows with K % 4 != 0 and on element rows
    for i, (K, N, ldx, offx, lddx, offdx) in enumerate([(44, 11, 48, 0, 64, 0), (8, 2, 8, 0, 24, 0),        # vector fill
                                                        (22, 11, 48, 0, 48, 0), (3, 16, 8, 0, 16, 0),       # K % 4 != 0
                                                        (44, 11, 48, 0, 63, 0), (8, 3, 8, 1, 24, 0),        # element rows
                                                        (4, 2, 4, 0, 16, 1)]):
        for j, zt in enumerate((K - 1, K, K + 1, K + 4, K + 6, lddx)):
            out.append(((1, 127, 129)[(i + j) % 3], K, N, (BF16, F32)[(i + j) % 2], ldx, offx, lddx, offdx, zt))
    return out


TL_BWD_CASES = _tiny_bwd_cases()

# the packed-row form: (B, L, K, N, dtype, ldx, offx, bias); K = 0: the overwrite-only form (x == NULL)
TL_DOC_CASES = [(3, 43, 22, 11, BF16, 48, 0, True), (2, 65, 4, 2, F32, 5, 0, True), (1, 130, 64, 16, F32, 64, 0, False),
                (5, 13, 63, 15, BF16, 64, 1, True), (3, 43, 0, 20, F32, 0, 0, False), (1, 7, 0, 1, F32, 0, 0, False),
                (4, 16500, 0, 16, F32, 0, 0, False)]


def test_case_tables_cover_every_dispatch_path():
    """From the mirror: the skinny cases meet every accepted (dtype, IT, NN), full and partial last passes, both bias forms,
    every T of the list, the forward's block cap and the backward's 96 KiB of LDS; the tiny cases meet the three forward
    kernels, every reason to refuse 16-byte accesses, every K and N of the list, both sides of the block caps and every form of
    the zero fill on every kind of row."""
    seen = {}

    def add(ep, *key):
        seen.setdefault(ep, set()).add(key)
    for K, N, dt, T, bias in SK_CASES:
        assert _sk_ok(K, N), (K, N)
        for ep in (("fwd", "bwd") if T else ("bwd",)):
            add(ep, "tmpl", dt, _sk_it(K), N)
            add(ep, "bias", dt, bias)
            add(ep, "T", T)
            add(ep, "last-pass", "full" if K % 256 == 0 else "partial")
        if T:
            add("fwd", "passes", _sk_fwd_passes(T))
        add("bwd", "lds", "96K" if _sk_bwd_lds(K, N) == 96 * 1024 else (">64K" if _sk_bwd_lds(K, N) > 64 * 1024 else "<=64K"), dt)
    tmpl = {("tmpl", dt, it, N) for dt in (F32, BF16) for it in (1, 2, 3, 4) for N in SK_NS if N <= 8 or it == 1}
    assert len(tmpl) == 26
    for ep in ("fwd", "bwd"):
        assert tmpl <= seen[ep], (ep, tmpl - seen[ep])
        assert {("bias", dt, b) for dt in (F32, BF16) for b in (True, False)} <= seen[ep]
        assert {("T", t) for t in (1, 7, 33)} <= seen[ep] and {("last-pass", "full"), ("last-pass", "partial")} <= seen[ep]
    assert ("T", 0) in seen["bwd"] and ("T", 0) not in seen["fwd"]
    assert {K for K, *_ in SK_CASES} >= {4, 256, 260, 704, 1024}
    assert _sk_fwd_passes(32768) == 2 and _sk_fwd_passes(32768 + 9) == 3 and ("passes", 3) in seen["fwd"]
    assert (4, 2, F32, 32768 + 9, True) in SK_CASES
    assert ("lds", "96K", F32) in seen["bwd"] and _sk_bwd_lds(1024, 8) == max(_sk_bwd_lds(K, N) for K in range(4, 1025, 4)
                                                                                for N in SK_NS if _sk_ok(K, N))
    assert all(T % SK_RPW for T in (1, 7, 33)), "no T of the list is a whole number of a wave's eight rows"

    # a pitch of whole 16-byte chunks that holds K elements holds their rounded-up chunks: 'x-overrun' never comes alone
    for dt in (F32, BF16):
        for K in range(1, TL_MAXK + 1):
            for ldx in range(K, 2 * TL_MAXK + 9):
                assert _tl_novec(dt, K, ldx, 0) != {"x-overrun"}
    for T, K, N, dt, ldx, offx, bias in TL_FWD_CASES:
        assert 1 <= K <= TL_MAXK and 1 <= N <= TL_MAXN and ldx >= K
        path = _tl_fwd_path(T, dt, K, ldx, offx)
        add("tfwd", "path", path, dt)
        if path == "lds-elem":
            add("tfwd", "why", _tl_novec(dt, K, ldx, offx))
        add("tfwd", "K", K)
        add("tfwd", "N", N)
        add("tfwd", "T", T)
        add("tfwd", "passes", _tl_fwd_passes(T))
        add("tfwd", "bias", bias)
    assert {("path", p, dt) for p in ("small", "lds-vec", "lds-elem") for dt in (F32, BF16)} <= seen["tfwd"]
    assert {("why", frozenset(w)) for w in (["x-base"], ["x-pitch"], ["x-pitch", "x-overrun"])} <= seen["tfwd"]
    assert {("K", k) for k in (1, 3, 4, 8, 22, 44, 63, 64)} <= seen["tfwd"] and {("N", n) for n in (1, 2, 11, 15, 16)} <= seen["tfwd"]
    assert {("T", t) for t in (1, 64, 65)} <= seen["tfwd"] and {("bias", True), ("bias", False)} <= seen["tfwd"]
    assert _tl_fwd_passes(524288) == 1 and _tl_fwd_passes(TL_BIG_T) == 2 and ("passes", 2) in seen["tfwd"]
    assert (TL_BIG_T, 1, 1, F32, 1, 0, True) in TL_FWD_CASES
    for K, N, dt, ldx, offx, bias in TL_SAME_BITS_CASES:
        add("tsame", "path", _tl_fwd_path(128, dt, K, ldx, offx), dt)
    assert {("path", p, dt) for p in ("lds-vec", "lds-elem") for dt in (F32, BF16)} <= seen["tsame"]

    for T, K, N, dt, ldx, offx, lddx, offdx, zt in TL_BWD_CASES:
        assert 1 <= K <= TL_MAXK and 1 <= N <= TL_MAXN and ldx >= K and lddx >= K and (zt is None or zt <= lddx)
        why = _tl_novec(dt, K, ldx, offx, lddx, offdx)
        add("tbwd", "vec", not why, dt)
        add("tbwd", "why", why)
        add("tbwd", "T", T)
        add("tbwd", "N-odd", N % 2)
        add("tbwd", "K%4", K % 4 != 0, not why)
        blocks, tiles = _tl_bwd_tiles(T)
        add("tbwd", "walk", "many" if tiles > blocks else "one", "ragged" if T % TL_ROWS else "whole")
        if zt is not None:
            rows = "elem" if why else ("vec-k4" if K % 4 == 0 else "vec-odd")
            rel = "below" if zt < K else ("lddx" if zt == lddx else zt - K)
            add("tfill", rows, rel)
            add("tfill", "form", rows, _tl_fill(dt, K, ldx, offx, lddx, offdx, zt))
            add("tfill", "dt", dt, rows)
    assert {("vec", v, dt) for v in (True, False) for dt in (F32, BF16)} <= seen["tbwd"]
    assert {("why", frozenset(w)) for w in ([], ["x-base"], ["x-pitch"], ["x-pitch", "x-overrun"], ["dx-base"], ["dx-pitch"])} \
        <= seen["tbwd"]
    assert {("T", t) for t in (0, 1, 127, 129, TL_BWD_BIG_T)} <= seen["tbwd"]
    assert {("N-odd", 0), ("N-odd", 1)} <= seen["tbwd"]
    assert {("K%4", a, b) for a in (True, False) for b in (True, False)} <= seen["tbwd"]
    assert _tl_bwd_tiles(131072) == (1024, 1024) and _tl_bwd_tiles(TL_BWD_BIG_T) == (1024, 1026) and TL_BWD_BIG_T % TL_ROWS == 2
    assert ("walk", "many", "ragged") in seen["tbwd"] and ("walk", "one", "ragged") in seen["tbwd"]
    assert {N for _, _, N, *_ in TL_BWD_CASES} >= {1, 3, 5, 11, 15, 16}, "odd N on both sides of a thread's pair of dW rows"
    for rows in ("vec-k4", "vec-odd", "elem"):
        assert {(rows, r) for r in ("below", 0, 1, 4, 6, "lddx")} <= seen["tfill"], (rows, seen["tfill"])
        assert {("dt", dt, rows) for dt in (F32, BF16)} <= seen["tfill"]
    vk4 = {k[2] for k in seen["tfill"] if k[0] == "form" and k[1] == "vec-k4"}
    assert {frozenset(), frozenset({"vector"}), frozenset({"scalar"}), frozenset({"vector", "scalar"})} <= vk4, vk4
    for rows in ("vec-odd", "elem"):
        assert {k[2] for k in seen["tfill"] if k[0] == "form" and k[1] == rows} == {frozenset(), frozenset({"scalar"})}

    for B, L, K, N, dt, ldx, offx, bias in TL_DOC_CASES:
        add("tdoc", "form", "overwrite" if K == 0 else _tl_fwd_path(65, dt, K, ldx, offx), dt)
        add("tdoc", "N", N)
        assert K == 0 or B * L > TL_SMALL_T
    assert {("form", "lds-vec", BF16), ("form", "lds-vec", F32), ("form", "lds-elem", F32), ("form", "lds-elem", BF16),
            ("form", "overwrite", F32)} <= seen["tdoc"] and ("N", 20) in seen["tdoc"]
    assert any(K == 0 and B * L * N > 4096 * 256 for B, L, K, N, *_ in TL_DOC_CASES), "the overwrite kernel's grid cap"


# ---------------------------------------------------------------------------------------------------------------------------
# helpers
G16 = 64            # guard elements on each side of an output: whole 16-byte chunks in both dtypes


def _carve(n, dt, dev, off=0):
    """(buffer, flat view of n elements): NaN-filled, the view `off` elements past a 16-byte boundary, G16 guard elements on
    each side of it."""
    buf = torch.full((n + 2 * G16 + off,), NAN, dtype=dt, device=dev)
    return buf, buf[G16 + off:G16 + off + n]


def _guards(*pairs):
    for i, (buf, view) in enumerate(pairs):
        lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
        g = torch.cat([buf[:lo], buf[lo + view.numel():]]).float()
        assert torch.isnan(g).all(), f"output {i}: {int((~torch.isnan(g)).sum())} guard elements written"


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)))


def _linear64(x, W, b, dy):
    """float64 F.linear and its autograd gradients: (y, dx, dW, db)."""
    x, W = x.clone().requires_grad_(True), W.clone().requires_grad_(True)
    b = b.clone().requires_grad_(True) if b is not None else None
    y = F.linear(x, W, b)
    y.backward(dy)
    return y.detach(), x.grad, W.grad, (b.grad if b is not None else dy.sum(0))


def _operands(T, K, N, dt, bias, gen):
    """x [T, K] rounded to dt, W [N, K] and b [N] as fp32 values, dy [T, N] as fp32 values - all float64."""
    x = torch.randn(T, K, generator=gen, dtype=torch.float64).to(dt).double()
    W = (torch.randn(N, K, generator=gen, dtype=torch.float64) / K ** 0.5).float().double()
    b = torch.randn(N, generator=gen, dtype=torch.float64).float().double() if bias else None
    dy = torch.randn(T, N, generator=gen, dtype=torch.float64).float().double()
    return x, W, b, dy


def _dx_rtol(dt):
    return 8e-3 if dt == BF16 else 1e-4


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the skinny linear
@gpu
@pytest.mark.parametrize("K,N,dt,T,bias", SK_CASES, ids=[f"K{c[0]}-N{c[1]}-{_tag(c[2])}-T{c[3]}-{'b' if c[4] else 'nob'}" for c in SK_CASES])
def test_skinny_linear_against_fp64(dev, K, N, dt, T, bias):
    """apertis_skinny_linear_fwd (y) and _bwd (dx, dW, db) against float64; T = 0 runs the backward alone, which must leave dW
    and db exact zeros and dx untouched.  The backward is repeated and must give the same bits."""
    lib, P, S = _lib()
    x, W, b, dy = _operands(T, K, N, dt, bias, _gen(K, N, T, _esz(dt)))
    y_ref, dx_ref, dW_ref, db_ref = _linear64(x, W, b, dy)
    Ta = max(T, 1)                                   # (no null pointers at T = 0)
    X = torch.zeros(Ta, K, dtype=dt, device=dev)
    X[:T] = x.to(dt).to(dev)
    Wd, Bd = W.float().to(dev), (b.float().to(dev) if bias else None)
    DY = torch.zeros(Ta, N, device=dev)
    DY[:T] = dy.float().to(dev)
    if T:
        ybuf, y = _carve(T * N, F32, dev)
        assert lib.apertis_skinny_linear_fwd(P(X), P(Wd), P(Bd), P(y), T, K, N, _code(dt), S()) == OK
        torch.cuda.synchronize()
        _guards((ybuf, y))
        _close(y.view(T, N), y_ref, "y", 1e-4)
    nblk = lib.apertis_skinny_linear_bwd_blocks(T)
    assert nblk == max(1, -(-T // SK_BWD_ROWS_PER_BLOCK))
    cols = N * K + N
    outs = []
    for rep in range(2):
        part = torch.full((nblk, cols), NAN, device=dev)
        dxbuf, dx = _carve(Ta * K, dt, dev)
        gbuf, g = _carve(cols, F32, dev)
        assert lib.apertis_skinny_linear_bwd(P(X), P(Wd), P(DY), P(dx), P(part), P(g), T, K, N, _code(dt), S()) == OK
        torch.cuda.synchronize()
        _guards((dxbuf, dx), (gbuf, g))
        outs.append((dx.clone(), g.clone()))
    dx, g = outs[0]
    assert torch.equal(g, outs[1][1]) and torch.equal(dx[:T * K], outs[1][0][:T * K]), "the backward is not deterministic"
    assert torch.isnan(dx[T * K:].float()).all(), "dx rows past T written"
    if T == 0:
        assert torch.equal(g.cpu(), torch.zeros(cols)), "T = 0 must leave dW and db zeros"
        return
    _close(dx[:T * K].view(T, K), dx_ref, "dx", _dx_rtol(dt))
    _sum_close(g[:N * K].view(N, K), dW_ref, T, "dW")
    _sum_close(g[N * K:], db_ref, T, "db")


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the tiny linear, forward
def _slice_of_wider(x, ldx, off, dt, dev, extra=0):
    """x [T, K] as the first K columns of rows of pitch ldx in a NaN-filled device buffer that starts `off` elements past a
    16-byte boundary: (buffer, [T, ldx] view)."""
    T, K = x.shape
    buf = torch.full((off + T * ldx + extra,), NAN, dtype=dt, device=dev)
    v = buf[off:off + T * ldx].view(T, ldx)
    v[:, :K] = x.to(dt).to(dev)
    return buf, v


def _tiny_fwd(lib, P, S, dev, xv, Wd, Bd, T, K, N, dt, ldx):
    ybuf, y = _carve(T * N, F32, dev)
    assert lib.apertis_tiny_linear_fwd(P(xv), ldx, P(Wd), P(Bd), P(y), T, K, N, _code(dt), S()) == OK
    torch.cuda.synchronize()
    _guards((ybuf, y))
    return y.view(T, N)


@gpu
@pytest.mark.parametrize("T,K,N,dt,ldx,offx,bias", TL_FWD_CASES,
                         ids=[f"T{c[0]}-K{c[1]}-N{c[2]}-{_tag(c[3])}-ld{c[4]}-off{c[5]}-{'b' if c[6] else 'nob'}" for c in TL_FWD_CASES])
def test_tiny_linear_fwd_against_fp64(dev, T, K, N, dt, ldx, offx, bias):
    """apertis_tiny_linear_fwd on x[:, :K] read in place from rows of pitch ldx whose other columns are NaN."""
    lib, P, S = _lib()
    x, W, b, _ = _operands(T, K, N, dt, bias, _gen(T, K, N, ldx, offx, _esz(dt)))
    _, xv = _slice_of_wider(x, ldx, offx, dt, dev)
    assert (xv.data_ptr() % 16 == 0) == (offx * _esz(dt) % 16 == 0)
    y = _tiny_fwd(lib, P, S, dev, xv, W.float().to(dev), b.float().to(dev) if bias else None, T, K, N, dt, ldx)
    _close(y, F.linear(x, W, b), "y", 1e-4)


@gpu
@pytest.mark.parametrize("K,N,dt,ldx,offx,bias", TL_SAME_BITS_CASES,
                         ids=[f"K{c[0]}-N{c[1]}-{_tag(c[2])}-ld{c[3]}-off{c[4]}" for c in TL_SAME_BITS_CASES])
def test_tiny_linear_small_kernel_has_the_lds_kernels_bits(dev, K, N, dt, ldx, offx, bias):
    """Rows 0..63 of a T = 64 call (a thread per output, W from global memory) equal the same rows of a T = 128 call (a
    thread per row, W from LDS) bit for bit: both add the bias first and then the products in column order."""
    lib, P, S = _lib()
    x, W, b, _ = _operands(128, K, N, dt, bias, _gen(K, N, ldx, offx, 5))
    _, xv = _slice_of_wider(x, ldx, offx, dt, dev)
    Wd, Bd = W.float().to(dev), (b.float().to(dev) if bias else None)
    y64 = _tiny_fwd(lib, P, S, dev, xv, Wd, Bd, 64, K, N, dt, ldx)
    y128 = _tiny_fwd(lib, P, S, dev, xv, Wd, Bd, 128, K, N, dt, ldx)
    assert torch.equal(y64, y128[:64]), f"{int((y64 != y128[:64]).sum())} of {64 * N} outputs differ between the two kernels"
    _close(y128, F.linear(x, W, b), "y", 1e-4)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the tiny linear, packed rows
def _doc_layout(B, L, gen):
    """int32 [B, L] start-of-document index of every token (documents of 1..4 tokens; row 0 starts at 0, row 1 is one
    document), and the bool mask of the rows the kernels reset: first tokens at t >= 1."""
    start = torch.zeros(B, L, dtype=torch.int32)
    for b in range(B):
        t = 0
        while t < L and b != 1:
            n = int(torch.randint(1, 5, (1,), generator=gen))
            start[b, t:t + n] = t
            t += n
    tl = torch.arange(L)[None, :].expand(B, L)
    return start, (start == tl) & (tl > 0)


@gpu
@pytest.mark.parametrize("B,L,K,N,dt,ldx,offx,bias", TL_DOC_CASES,
                         ids=[f"B{c[0]}-L{c[1]}-K{c[2]}-N{c[3]}-{_tag(c[4])}-ld{c[5]}-off{c[6]}" for c in TL_DOC_CASES])
def test_tiny_linear_doc_fwd_resets_document_starts(dev, B, L, K, N, dt, ldx, offx, bias):
    """apertis_tiny_linear_doc_fwd: rows with start[t] == t % L at t % L > 0 hold `reset` in every column (their x row, NaN
    here, is not read), rows at t % L == 0 never do, every other row carries apertis_tiny_linear_fwd's bits; with x == NULL
    only the reset rows of a y that already holds logits are overwritten (any N)."""
    lib, P, S = _lib()
    T, reset = B * L, -37.5
    gen = _gen(B, L, K, N, ldx, 3)
    start, rs = _doc_layout(B, L, gen)
    rs = rs.reshape(T)
    assert rs.any() and not rs.reshape(B, L)[:, 0].any() and (B < 2 or not rs.reshape(B, L)[1].any())
    ST = start.to(dev)
    if K == 0:
        y0 = torch.randn(T, N, generator=gen)
        ybuf, y = _carve(T * N, F32, dev)
        y.copy_(y0.reshape(-1).to(dev))
        assert lib.apertis_tiny_linear_doc_fwd(None, 0, None, None, P(ST), reset, P(y), T, L, 0, N, _code(F32), S()) == OK
        torch.cuda.synchronize()
        _guards((ybuf, y))
        want = torch.where(rs[:, None], torch.full_like(y0, reset), y0)
        assert torch.equal(y.view(T, N).cpu(), want)
        return
    x, W, b, _ = _operands(T, K, N, dt, bias, gen)
    _, xv = _slice_of_wider(x, ldx, offx, dt, dev)
    Wd, Bd = W.float().to(dev), (b.float().to(dev) if bias else None)
    plain = _tiny_fwd(lib, P, S, dev, xv, Wd, Bd, T, K, N, dt, ldx)
    xv[rs.to(dev)] = NAN                                  # the reset rows are not loaded
    ybuf, y = _carve(T * N, F32, dev)
    assert lib.apertis_tiny_linear_doc_fwd(P(xv), ldx, P(Wd), P(Bd), P(ST), reset, P(y), T, L, K, N, _code(dt), S()) == OK
    torch.cuda.synchronize()
    _guards((ybuf, y))
    y = y.view(T, N).cpu()
    assert torch.equal(y[rs], torch.full((int(rs.sum()), N), reset)), "a document's first row does not hold `reset`"
    assert torch.equal(y[~rs], plain.cpu()[~rs]), "a row that is no document start differs from apertis_tiny_linear_fwd"
    _close(y[~rs], F.linear(x, W, b)[~rs], "y", 1e-4)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the tiny linear, backward
def _bwd_id(c):
    T, K, N, dt, ldx, offx, lddx, offdx, zt = c
    return f"T{T}-K{K}-N{N}-{_tag(dt)}-ld{ldx}-off{offx}-ldd{lddx}-off{offdx}-z{'no' if zt is None else zt}"


@gpu
@pytest.mark.parametrize("T,K,N,dt,ldx,offx,lddx,offdx,zero_to", TL_BWD_CASES, ids=[_bwd_id(c) for c in TL_BWD_CASES])
def test_tiny_linear_bwd_against_fp64(dev, T, K, N, dt, ldx, offx, lddx, offdx, zero_to):
    """apertis_tiny_linear_bwd (zero_to None) / _bwd_pad: dx rows of pitch lddx written in a NaN-filled buffer - columns [0, K)
    against float64, [K, zero_to) exact zeros, [zero_to, lddx) still NaN -, dW and db against float64 (zeros at T = 0); twice,
    the same bits."""
    lib, P, S = _lib()
    x, W, _, dy = _operands(T, K, N, dt, False, _gen(T, K, N, ldx, lddx, offx, offdx, _esz(dt)))
    _, dx_ref, dW_ref, db_ref = _linear64(x, W, None, dy)
    Ta = max(T, 1)
    xa = torch.zeros(Ta, K, dtype=torch.float64)
    xa[:T] = x
    _, xv = _slice_of_wider(xa, ldx, offx, dt, dev)
    Wd = W.float().to(dev)
    DY = torch.zeros(Ta, N, device=dev)
    DY[:T] = dy.float().to(dev)
    nblk = lib.apertis_tiny_linear_bwd_blocks(T)
    assert nblk == _tl_bwd_tiles(T)[0]
    cols = N * K + N
    zt = K if zero_to is None else max(zero_to, K)
    outs = []
    for rep in range(2):
        part = torch.full((nblk, cols), NAN, device=dev)
        dxbuf, dxf = _carve(Ta * lddx, dt, dev, offdx)
        assert (dxf.data_ptr() % 16 == 0) == (offdx * _esz(dt) % 16 == 0)
        gbuf, g = _carve(cols, F32, dev)
        if zero_to is None:
            rc = lib.apertis_tiny_linear_bwd(P(xv), ldx, P(Wd), P(DY), P(dxf), lddx, P(part), P(g), T, K, N, _code(dt), S())
        else:
            rc = lib.apertis_tiny_linear_bwd_pad(P(xv), ldx, P(Wd), P(DY), P(dxf), lddx, P(part), P(g), T, K, N, zero_to, _code(dt), S())
        assert rc == OK
        torch.cuda.synchronize()
        _guards((dxbuf, dxf), (gbuf, g))
        outs.append((dxf.view(Ta, lddx).cpu(), g.cpu()))
    dx, g = outs[0]
    assert torch.equal(g, outs[1][1]) and torch.equal(dx[:T, :zt], outs[1][0][:T, :zt]), "the backward is not deterministic"
    assert torch.isnan(dx[T:].float()).all(), "dx rows past T written"
    assert torch.isnan(dx[:T, zt:].float()).all(), f"columns [{zt}, {lddx}) behind the zero fill written"
    if T == 0:
        assert torch.equal(g, torch.zeros(cols)), "T = 0 must leave dW and db zeros"
        return
    assert torch.equal(dx[:T, K:zt].float(), torch.zeros(T, zt - K)), f"columns [{K}, {zt}) are not exact zeros"
    _close(dx[:T, :K], dx_ref, "dx", _dx_rtol(dt))
    _sum_close(g[:N * K].view(N, K), dW_ref, T, "dW")
    _sum_close(g[N * K:], db_ref, T, "db")
