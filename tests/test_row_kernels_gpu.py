"""The LayerNorm row-kernel family against float64 references on the same rounded inputs, at every row-width bucket:
apertis_layernorm_fwd / _bwd, the block boundary apertis_dropout_add_layernorm_fwd (dense and combine forms),
apertis_layernorm_combine_bwd, the MoE entrance and exit apertis_moe_gather_ln_fwd / _bwd and apertis_moe_combine_fwd / _bwd,
apertis_dropout_add_fwd / apertis_dropout_bwd, and the router family at its four widths (apertis_router_fwd,
apertis_router_bwd_rows, apertis_dropout_add_layernorm_router_fwd, apertis_boundary_router_bwd).

Every kernel here is a template on IT = ceil(H / 256), rounded up by DISPATCH_IT to 1, 2, 3, 4, 6, 8, 12 or 16 (H <= 4096,
H % 4 == 0); the router family takes IT 1..4 (H <= 1024).  The cases below sit at both ends of every bucket, ragged widths
(H % 256 != 0) included, in every dtype pair the entry points accept; the LayerNorm backward runs on both sides of its
two-level fold (ceil(T / 32) >= 256 partial rows), with a short last fold group, and at widths whose dynamic LDS (24 H bytes)
passes 64 KiB.  test_case_tables_cover_every_dispatch_path checks that from a mirror of the dispatch.

The dropout keep mask is pinned bit for bit against a numpy copy of drop_keep (csrc/common.h) in every kernel that makes or
regenerates it; the references below then use that mask exactly.

Tolerances: fp32 outputs rtol 1e-4 with an absolute floor of 1e-5 of the tensor's largest entry; bf16 outputs one bf16
rounding (rtol 8e-3) against the reference computed on the rounded inputs; parameter gradients (sums over T rows) an absolute
bound growing with sqrt(T).  Where an input of a step is an output the kernel rounded (the LayerNorm of a boundary reads the
y it stored), the reference starts from that stored output, itself checked against fp64.  Expert rows and combine weights
are dyadic (n / 32, m / 64), so the combine sums are exact in fp32 and their rounding to bf16 is the reference's.  Every
output is carved from a larger NaN-filled buffer whose guard must still be NaN after the call."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_error_report

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -2
NAN = float("nan")

# ---------------------------------------------------------------------------------------------------------------------------
# mirror of the dispatch in csrc/layernorm.hip and csrc/row_common.h (check_H, DISPATCH_IT, DISPATCH_2T, ln_part_rows /
# ln_two_level, the backward launches' dynamic LDS) and csrc/ssm_elementwise.hip (apertis_dropout_add_fwd's grid cap): a change
# there must be made here too, and then test_case_tables_cover_every_dispatch_path says whether the cases still reach every path
IT_BUCKETS = (1, 2, 3, 4, 6, 8, 12, 16)
H_MAX = 4096
LN_ROWS_PER_BLOCK = 4 * 8           # four waves x APERTIS_LN_RPW (8) rows
LN_FOLD_GROUPS = 32
DROP_BLOCK_CAP = 8192               # apertis_dropout_add_fwd / _bwd: blocks of 256 threads, 4 elements each
PAIRS_2T = [(F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16)]
PAIRS_DROP_ADD = [(BF16, F32), (F32, F32), (BF16, BF16)]      # (x, res)
PAIRS_DROP_BWD = [(F32, BF16), (F32, F32), (BF16, BF16)]      # (g, dx)


def _bucket(H):
    it = -(-H // 256)
    return next(b for b in IT_BUCKETS if it <= b)


def _h_ok(H):
    return 0 < H <= H_MAX and H % 4 == 0


def _ln_fold(T):
    """'two' when apertis_layernorm_bwd folds its partial rows in two levels (ln_two_level), else 'one'."""
    return "two" if -(-max(T, 1) // LN_ROWS_PER_BLOCK) >= 8 * LN_FOLD_GROUPS else "one"


def _bwd_lds(H):
    """The dynamic LDS of gather_ln_bwd2_k / layernorm_bwd_k: three waves' [2][H] fp32 sums."""
    return 3 * 2 * H * 4


def _lds_class(H):
    return ">64K" if _bwd_lds(H) > 64 * 1024 else (">48K" if _bwd_lds(H) > 48 * 1024 else "<=48K")


def _tag(t):
    return "f32" if t == F32 else "bf16"


# ---------------------------------------------------------------------------------------------------------------------------
# case tables
WIDTHS = [4, 252, 260, 512, 516, 768, 772, 1024, 1028, 1536, 1540, 2048, 2052, 3072, 3076, 4096]
ROUTER_WIDTHS = [4, 252, 260, 512, 516, 772, 1020, 1024]

# LayerNorm fwd + bwd: (H, dtype_x, dtype_y = dtype_g, T, form); form 'plain' = no dres / dblk, 'full' = dres and dblk at p 0.1
LN_CASES = ([(H, tx, ty, 1, "plain") for H in WIDTHS for tx, ty in PAIRS_2T] +
            [(H, tx, ty, 3, "full") for H in WIDTHS for tx, ty in PAIRS_2T] +
            [(4096, F32, F32, 97, "full"), (3076, BF16, BF16, 97, "full"), (2052, F32, BF16, 161, "full"),
             (1540, BF16, F32, 65, "plain"), (772, F32, F32, 300, "full"),
             # the fold threshold (8160 rows: 255 partial rows, one level; 8161: 256, two), a short last fold group (8225:
             # 258 rows in groups of 9 - the last has 6), and 70 000 rows (2188 partial rows) at a narrow width
             (252, F32, F32, 8160, "plain"), (252, BF16, BF16, 8161, "full"), (244, F32, BF16, 8225, "full"),
             (260, BF16, F32, 8225, "plain"), (12, F32, F32, 70_000, "full")])

# boundary forward: (H, dtype_x, dtype_y, T, K): K = 0 the dense form, else the combine form with K slots per token
BOUNDARY_CASES = ([(H, *PAIRS_2T[i % 4], 5, 0) for i, H in enumerate(WIDTHS)] +
                  [(H, *PAIRS_2T[(i + 1) % 4], 6, (1, 2, 3, 8)[i % 4]) for i, H in enumerate(WIDTHS)] +
                  [(H, tx, ty, 9, 0) for H in (260, 3076) for tx, ty in PAIRS_2T] +
                  [(1028, tx, ty, 7, 2) for tx, ty in PAIRS_2T])

# layernorm_combine_bwd: (H, dtype_x, dtype_g, T, K)
COMB_BWD_CASES = ([(H, *PAIRS_2T[i % 4], 7, 1 + i % 2) for i, H in enumerate(WIDTHS)] +
                  [(1024, tx, tg, 40, 2) for tx, tg in PAIRS_2T] +
                  [(252, F32, F32, 8225, 2), (132, BF16, BF16, 8161, 1)])

# gather-LN and combine: (id, H, dtype_x, dtype_out, S, E, K, plan shape)
GATHER_CASES = ([(f"w{H}", H, *PAIRS_2T[i % 4], 70, 8, 2, "mixed") for i, H in enumerate(WIDTHS)] +
                [(f"pair-{_tag(a)}-{_tag(b)}", 772, a, b, 70, 8, 2, "mixed") for a, b in PAIRS_2T] +
                [("e64-k8", 132, F32, F32, 200, 64, 8, "mixed"), ("e64-k8-bf16", 1028, BF16, BF16, 90, 64, 8, "mixed"),
                 ("edge64", 260, F32, F32, 300, 4, 2, "edge"), ("edge64-wide", 4096, BF16, BF16, 300, 4, 1, "edge"),
                 ("e1", 516, F32, BF16, 33, 1, 1, "mixed")])

# router family: (H, N, dtype_x)
ROUTER_CASES = [(H, N, (F32, BF16)[(i + j) % 2]) for i, H in enumerate((260, 772, 1020)) for j, N in enumerate((2, 4, 8))] + \
               [(H, 4, F32) for H in ROUTER_WIDTHS]


def test_case_tables_cover_every_dispatch_path():
    """From the mirror of the dispatch: every entry point of the family meets every IT bucket (the router family its four),
    every dtype pair it accepts, and - where it has them - both fold levels of the LayerNorm backward and a backward launch
    whose dynamic LDS passes 64 KiB; the ragged end of every bucket (H % 256 != 0) is among the widths."""
    seen = {}

    def add(ep, *key):
        seen.setdefault(ep, set()).add(key)
    for H, tx, ty, T, form in LN_CASES:
        assert _h_ok(H)
        for ep in ("layernorm_fwd", "layernorm_bwd"):
            add(ep, "it", _bucket(H))
            add(ep, "pair", tx, ty)
            add(ep, "it-pair", _bucket(H), tx, ty)
        add("layernorm_bwd", "fold", _ln_fold(T))
        add("layernorm_bwd", "lds", _lds_class(H))
        add("layernorm_bwd", "form", form)
    for H, tx, ty, T, K in BOUNDARY_CASES:
        ep = "dropout_add_layernorm_fwd" + ("[combine]" if K else "[dense]")
        add(ep, "it", _bucket(H))
        add(ep, "pair", tx, ty)
    for H, tx, tg, T, K in COMB_BWD_CASES:
        ep = "layernorm_combine_bwd"
        add(ep, "it", _bucket(H))
        add(ep, "pair", tx, tg)
        add(ep, "fold", _ln_fold(T))
        add(ep, "lds", _lds_class(H))
    for _, H, tx, to, S, E, K, shape in GATHER_CASES:
        for ep in ("moe_gather_ln_fwd", "moe_gather_ln_bwd", "moe_combine_fwd", "moe_combine_bwd"):
            add(ep, "it", _bucket(H))
            add(ep, "pair", tx, to)
        add("moe_gather_ln_bwd", "lds", _lds_class(H))
    for H, N, tx in ROUTER_CASES:
        for ep in ("router_fwd", "router_bwd_rows", "dropout_add_layernorm_router_fwd", "boundary_router_bwd"):
            add(ep, "it", _bucket(H))
            add(ep, "N", N)
    all_pairs = {("pair", a, b) for a, b in PAIRS_2T}
    for ep in ("layernorm_fwd", "layernorm_bwd", "dropout_add_layernorm_fwd[dense]", "dropout_add_layernorm_fwd[combine]",
               "layernorm_combine_bwd", "moe_gather_ln_fwd", "moe_gather_ln_bwd", "moe_combine_fwd", "moe_combine_bwd"):
        assert {("it", b) for b in IT_BUCKETS} <= seen[ep], (ep, sorted(k for k in seen[ep] if k[0] == "it"))
        assert all_pairs <= seen[ep], ep
    assert {("it-pair", b, x, y) for b in IT_BUCKETS for x, y in PAIRS_2T} <= seen["layernorm_fwd"]
    for ep in ("layernorm_bwd", "layernorm_combine_bwd"):
        assert {("fold", "one"), ("fold", "two")} <= seen[ep], ep
    for ep in ("layernorm_bwd", "layernorm_combine_bwd", "moe_gather_ln_bwd"):
        assert {("lds", "<=48K"), ("lds", ">48K"), ("lds", ">64K")} <= seen[ep], ep
    assert {("form", "plain"), ("form", "full")} <= seen["layernorm_bwd"]
    for ep in ("router_fwd", "router_bwd_rows", "dropout_add_layernorm_router_fwd", "boundary_router_bwd"):
        assert {("it", b) for b in (1, 2, 3, 4)} <= seen[ep] and {("N", n) for n in (2, 4, 8)} <= seen[ep], ep
    # both ends of every bucket, the upper one ragged where the bucket is not a whole number of 256-wide chunks
    for b in IT_BUCKETS:
        ws = [H for H in WIDTHS if _bucket(H) == b]
        lo = 4 if b == 1 else 256 * IT_BUCKETS[IT_BUCKETS.index(b) - 1] + 4
        assert min(ws) == lo and max(ws) >= 256 * b - 4, (b, ws)
    assert any(H % 256 for H in WIDTHS if _bucket(H) > 4) and any(H % 256 for H in ROUTER_WIDTHS)
    # the fold threshold and a short last group
    fold_T = {T for *_, T, _ in LN_CASES}
    assert _ln_fold(8160) == "one" and _ln_fold(8161) == "two" and {8160, 8161, 8225} <= fold_T
    nblk = -(-8225 // LN_ROWS_PER_BLOCK)
    rpg = -(-nblk // LN_FOLD_GROUPS)
    assert nblk % rpg != 0, "8225 rows must leave the last fold group short"
    # dropout_add_fwd past its grid cap
    assert DROP_N_CAP // 4 > 256 * DROP_BLOCK_CAP


# ---------------------------------------------------------------------------------------------------------------------------
# the keep mask: a numpy copy of drop_keep (csrc/common.h)
def keep_mask(seed, lin, p):
    """keep[i] for the linear element indices `lin` (uint64) under (seed, p): drop_keep / drop_keep4, bit for bit."""
    lin = np.asarray(lin, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = (lin >> np.uint64(1)).astype(np.uint32) ^ np.uint32(seed & 0xFFFFFFFF)
        h = h + (lin >> np.uint64(33)).astype(np.uint32) * np.uint32(0x9E3779B9) + np.uint32(seed >> 32)
        h ^= h >> np.uint32(16)
        h *= np.uint32(0x85EBCA6B)
        h ^= h >> np.uint32(13)
        h *= np.uint32(0xC2B2AE35)
        h ^= h >> np.uint32(16)
    r16 = np.where((lin & np.uint64(1)) != 0, h >> np.uint32(16), h & np.uint32(0xFFFF))
    thresh16 = np.uint32(int(np.float32(p) * np.float32(65536.0)))
    return r16 >= thresh16


def _keep_rows(seed, T, H, p):
    """[T, H] bool keep mask of the row kernels (linear index r * H + c), as a torch tensor."""
    if p <= 0:
        return torch.ones(T, H, dtype=torch.bool)
    lin = np.arange(T * H, dtype=np.uint64)
    return torch.from_numpy(keep_mask(seed, lin, p).reshape(T, H))


def test_keep_mask_mirror_basics():
    """The mirror itself: about 1 - p kept, thresh16 from a float32 multiply, and both hash halves of a pair used."""
    lin = np.arange(1 << 20, dtype=np.uint64)
    for p in (0.1, 0.5):
        k = keep_mask(0xDEADBEEF12345678, lin, p)
        assert abs(k.mean() - (1 - p)) < 3e-3
    assert int(np.float32(0.1) * np.float32(65536.0)) == 6553
    assert keep_mask(7, lin, 0.0).all()


SEEDS = [0x9E3779B97F4A7C15, 0xFFFFFFFF00000001, 0x0000000100000000 + 12345]
DROP_N_CAP = 8_388_608 + 65_540          # n / 4 > 256 * 8192: the grid-stride loop walks a second pass


# ---------------------------------------------------------------------------------------------------------------------------
# helpers
def _lib():
    from apertis_llm_amd import _lib
    return _lib.load(), _lib.ptr, _lib.stream_ptr


def _code(t):
    from apertis_llm_amd import _lib
    return _lib.BF16 if t == BF16 else _lib.F32


GUARD = 67          # elements of NaN on each side of an output


def _out(shape, dt, dev, fill=NAN):
    """(buffer, view): the view of `shape` carved from a NaN-filled buffer with GUARD elements on each side."""
    n = int(np.prod(shape)) if len(shape) else 1
    buf = torch.full((n + 2 * GUARD,), NAN, dtype=dt, device=dev)
    v = buf[GUARD:GUARD + n].view(*shape)
    if fill is not None and not (isinstance(fill, float) and math.isnan(fill)):
        v.fill_(fill)
    return buf, v


def _guards_nan(*bufs):
    for i, b in enumerate(bufs):
        g = torch.cat([b[:GUARD], b[-GUARD:]]).float()
        assert torch.isnan(g).all(), f"output {i}: {int((~torch.isnan(g)).sum())} guard elements written"


def _close(got, ref, name, rtol, atol_scale=1e-5):
    ref = torch.as_tensor(ref).detach().cpu().to(torch.float64)
    got = got.detach().cpu().to(torch.float64)
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), f"{name}: {int((~torch.isfinite(got)).sum())} non-finite values"
    atol = atol_scale * float(ref.abs().max()) + 1e-30
    bad = (got - ref).abs() > atol + rtol * ref.abs()
    assert not bad.any(), f"{name}: {int(bad.sum())} / {bad.numel()} outside rtol {rtol}; max abs diff " \
                          f"{float((got - ref).abs().max()):.3e} (ref max {float(ref.abs().max()):.3e})"


def _rtol(*dts):
    return 8e-3 if BF16 in dts else 1e-4


def _sum_close(got, ref, n, name, scale=1.0):
    """An fp32 sum over n terms of order `scale`: |err| <= 1.6e-4 sqrt(n) scale, as test_conv_gate_gpu's."""
    ref = torch.as_tensor(ref).detach().cpu().to(torch.float64)
    got = got.detach().cpu().to(torch.float64)
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), name
    err, tol = float((got - ref).abs().max()), 2e-5 * 8 * max(1.0, math.sqrt(n)) * scale
    assert err <= tol, f"{name}: max abs err {err:.3e} > {tol:.3e} (ref max {float(ref.abs().max()):.3e})"


def _rnd(t, dt):
    """t rounded to dt (RNE) and back to float64: what a kernel reading dt sees."""
    return t.to(dt).double()


def _ln64(x, g, b, eps):
    """float64 LayerNorm of the rows of x: (y, mean, rstd, xhat)."""
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (x - mean) * rstd
    return xh * g + b, mean[..., 0], rstd[..., 0], xh


def _ln_bwd64(xh, rstd, g, dy):
    """float64 LayerNorm backward: (dx, per-row dy * xhat, dy)."""
    gd = dy * g
    m1, m2 = gd.mean(-1, keepdim=True), (gd * xh).mean(-1, keepdim=True)
    return rstd[..., None] * (gd - m1 - xh * m2), dy * xh, dy


def _rows(T, H, gen, scale=2.0, offset=0.5):
    """[T, H] rows with a per-row offset (means well away from zero) - float64."""
    return torch.randn(T, H, generator=gen, dtype=torch.float64) * scale + offset * torch.randn(T, 1, generator=gen,
                                                                                               dtype=torch.float64)


def _dyadic(shape, gen, den, lim):
    return (torch.randn(*shape, generator=gen, dtype=torch.float64) * lim / 2).round().clamp(-lim, lim) / den


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the keep mask, bit for bit, in every kernel that makes or regenerates it
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("tx,tr", PAIRS_DROP_ADD, ids=[f"{_tag(a)}-{_tag(b)}" for a, b in PAIRS_DROP_ADD])
def test_dropout_add_fwd_and_bwd_mask_and_values(dev, tx, tr, p):
    """apertis_dropout_add_fwd (y = res + keep / (1 - p) * x over a flat index) and apertis_dropout_bwd (dx = keep / (1 - p) *
    g): the kept set is the mirror's bit for bit, for seeds whose high word is non-zero, and the values are fp64's on it.
    The f32 pair runs past the forward's 8192-block grid cap (each thread then makes a second pass)."""
    lib, P, S = _lib()
    big = tx == F32 and tr == F32
    n = DROP_N_CAP if big else 3 * 4096 + 12
    gen = torch.Generator().manual_seed(n + int(p * 10))
    x = (torch.rand(n, generator=gen, dtype=torch.float64) + 0.5) * torch.sign(torch.randn(n, generator=gen, dtype=torch.float64))
    res = torch.rand(n, generator=gen, dtype=torch.float64) * 2 - 1
    xq, rq = _rnd(x, tx), _rnd(res, tr)
    X, R = xq.to(tx).to(dev), rq.to(tr).to(dev)
    ks = 1.0 / (1.0 - float(np.float32(p)))
    for seed in SEEDS[:2]:
        keep = torch.from_numpy(keep_mask(seed, np.arange(n, dtype=np.uint64), p))
        ybuf, y = _out((n,), tr, dev)
        assert lib.apertis_dropout_add_fwd(P(X), P(R), P(y), n, p, seed, _code(tx), _code(tr), S()) == OK
        torch.cuda.synchronize()
        _guards_nan(ybuf)
        yc = y.cpu().double()
        got_keep = yc != rq
        assert torch.equal(got_keep, keep), f"seed {seed:#x}: {int((got_keep != keep).sum())} mask bits differ"
        _close(yc, rq + keep.double() * xq * ks, "y", _rtol(tr))
    # backward: g -> dx, dtype pairs (g, dx) of the entry point
    tg, tdx = {(BF16, F32): (F32, BF16), (F32, F32): (F32, F32), (BF16, BF16): (BF16, BF16)}[(tx, tr)]
    seed = SEEDS[2]
    keep = torch.from_numpy(keep_mask(seed, np.arange(n, dtype=np.uint64), p))
    gq = _rnd(x, tg)
    dxbuf, dx = _out((n,), tdx, dev)
    assert lib.apertis_dropout_bwd(P(gq.to(tg).to(dev)), P(dx), n, p, seed, _code(tg), _code(tdx), S()) == OK
    torch.cuda.synchronize()
    _guards_nan(dxbuf)
    dxc = dx.cpu().double()
    assert torch.equal(dxc != 0, keep), f"dropout_bwd: {int(((dxc != 0) != keep).sum())} mask bits differ"
    _close(dxc, keep.double() * gq * ks, "dx", _rtol(tg, tdx))


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("seed", SEEDS[:2], ids=["s0", "s1"])
def test_row_kernel_masks_equal_the_mirror(dev, seed, p):
    """The mask of the boundary forward (apertis_dropout_add_layernorm_fwd, linear index r * H + c via drop_keep4) and the one
    apertis_layernorm_bwd regenerates for dblk: each the mirror's bit for bit, over 2.1 M elements (a keep test off by one
    - r16 > thresh16 - flips about 32 of them at either p).  blk = 1, res = 0 make y the scaled mask; dy = 0, dres = 1 make
    dx = 1 and dblk the scaled mask."""
    lib, P, S = _lib()
    T, H = 2050, 1028
    keep = _keep_rows(seed, T, H, p)
    ones, zeros = torch.ones(T, H, device=dev), torch.zeros(T, H, device=dev)
    g, b = torch.ones(H, device=dev), torch.zeros(H, device=dev)
    y, xn = torch.full((T, H), NAN, device=dev), torch.full((T, H), NAN, device=dev)
    mean, rstd = torch.full((T,), NAN, device=dev), torch.full((T,), NAN, device=dev)
    assert lib.apertis_dropout_add_layernorm_fwd(P(ones), None, None, 0, P(zeros), P(g), P(b), 1e-5, P(y), P(xn), P(mean),
                                                 P(rstd), T, H, p, seed, _code(F32), _code(F32), S()) == OK
    torch.cuda.synchronize()
    got = (y != 0).cpu()
    assert torch.equal(got, keep), f"boundary forward: {int((got != keep).sum())} mask bits differ"
    nblk = lib.apertis_layernorm_bwd_blocks(T, H)
    part = torch.full((nblk, 2, H), NAN, device=dev)
    dx, dblk = torch.full((T, H), NAN, device=dev), torch.full((T, H), NAN, device=dev)
    dg, db = torch.full((H,), NAN, device=dev), torch.full((H,), NAN, device=dev)
    x = torch.randn(T, H, device=dev)
    m1, r1 = torch.zeros(T, device=dev), torch.ones(T, device=dev)
    assert lib.apertis_layernorm_bwd(P(x), P(g), P(m1), P(r1), P(zeros), P(ones), P(dx), P(dblk), p, seed, P(part), P(dg),
                                     P(db), T, H, _code(F32), _code(F32), S()) == OK
    torch.cuda.synchronize()
    assert torch.equal(dx, ones)
    got = (dblk != 0).cpu()
    assert torch.equal(got, keep), f"layernorm_bwd dblk: {int((got != keep).sum())} mask bits differ"
    ks = 1.0 / (1.0 - float(np.float32(p)))
    _close(dblk, keep.double() * ks, "dblk", 1e-6)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. plain LayerNorm forward and backward
def _ln_run(lib, P, S, dev, x, g, b, eps, dy, dres, p, seed, tx, ty, T, H):
    """apertis_layernorm_fwd then _bwd into guarded NaN buffers: dict of outputs (device views) and the guard buffers."""
    X, G, B = x.to(tx).to(dev), g.float().to(dev), b.float().to(dev)
    ybuf, y = _out((T, H), ty, dev)
    mbuf, mean = _out((T,), F32, dev)
    rbuf, rstd = _out((T,), F32, dev)
    assert lib.apertis_layernorm_fwd(P(X), P(G), P(B), eps, P(y), P(mean), P(rstd), T, H, _code(tx), _code(ty), S()) == OK
    nblk = lib.apertis_layernorm_bwd_blocks(T, H)
    part = torch.full((nblk, 2, H), NAN, device=dev)
    dxbuf, dx = _out((T, H), tx, dev)
    dgbuf, dg = _out((H,), F32, dev)
    dbbuf, db = _out((H,), F32, dev)
    bufs = [ybuf, mbuf, rbuf, dxbuf, dgbuf, dbbuf]
    DY = dy.to(ty).to(dev)
    DR = dres.to(tx).to(dev) if dres is not None else None
    dblk = None
    if dres is not None:
        dkbuf, dblk = _out((T, H), ty, dev)
        bufs.append(dkbuf)
    assert lib.apertis_layernorm_bwd(P(X), P(G), P(mean), P(rstd), P(DY), P(DR), P(dx), P(dblk), p, seed, P(part), P(dg), P(db),
                                     T, H, _code(tx), _code(ty), S()) == OK
    torch.cuda.synchronize()
    return dict(y=y, mean=mean, rstd=rstd, dx=dx, dg=dg, db=db, dblk=dblk, part=part, X=X, G=G, DY=DY, DR=DR), bufs


@pytest.mark.parametrize("H,tx,ty,T,form", LN_CASES,
                         ids=[f"H{c[0]}-{_tag(c[1])}-{_tag(c[2])}-T{c[3]}-{c[4]}" for c in LN_CASES])
def test_layernorm_fwd_bwd_against_fp64(dev, H, tx, ty, T, form):
    """apertis_layernorm_fwd (y, mean, rstd) and apertis_layernorm_bwd (dx, dgamma, dbeta; 'full': with the residual gradient
    dres folded in and dblk = the masked copy of dx at p = 0.1) against fp64 on the rounded inputs, at the bucket's ends and
    every dtype pair, at the fold threshold and past it; the partial-row workspace starts NaN (a fold reading past its
    rows would show).  At a two-level T the backward is repeated and must give the same bits."""
    lib, P, S = _lib()
    gen = torch.Generator().manual_seed(H * 31 + T)
    x = _rnd(_rows(T, H, gen), tx)
    g = torch.randn(H, generator=gen, dtype=torch.float64) * 0.5 + 1
    b = torch.randn(H, generator=gen, dtype=torch.float64) * 0.2
    g, b = g.float().double(), b.float().double()
    dy = _rnd(torch.randn(T, H, generator=gen, dtype=torch.float64), ty)
    full = form == "full"
    dres = _rnd(torch.randn(T, H, generator=gen, dtype=torch.float64), tx) if full else None
    p, seed = (0.1, SEEDS[0]) if full else (0.0, 0)
    eps = 1e-12
    o, bufs = _ln_run(lib, P, S, dev, x, g, b, eps, dy, dres, p, seed, tx, ty, T, H)
    _guards_nan(*bufs)
    y_ref, mean_ref, rstd_ref, xh = _ln64(x, g, b, eps)
    _close(o["y"], y_ref, "y", _rtol(ty))
    _close(o["mean"], mean_ref, "mean", 1e-4, 1e-5)
    _close(o["rstd"], rstd_ref, "rstd", 1e-4)
    dx_ref, dgr, dbr = _ln_bwd64(xh, rstd_ref, g, dy)
    if full:
        dx_ref = dx_ref + dres
    _close(o["dx"], dx_ref, "dx", _rtol(tx))
    _sum_close(o["dg"], dgr.sum(0), T, "dgamma")
    _sum_close(o["db"], dbr.sum(0), T, "dbeta")
    if full:
        keep = _keep_rows(seed, T, H, p)
        ks = 1.0 / (1.0 - float(np.float32(p)))
        # dblk = mask * dx as stored (rounded to x's dtype) / (1 - p), rounded to the gradient dtype
        _close(o["dblk"], keep.double() * o["dx"].cpu().double() * ks, "dblk", _rtol(ty), 1e-6)
        assert torch.equal((o["dblk"].cpu() != 0) | (o["dx"].cpu() == 0), keep | (o["dx"].cpu() == 0))
    if _ln_fold(T) == "two":
        dg1, db1, dx1 = o["dg"].clone(), o["db"].clone(), o["dx"].clone()
        dx2, dg2, db2 = torch.empty_like(dx1), torch.empty_like(dg1), torch.empty_like(db1)
        dblk2 = torch.empty_like(o["dblk"]) if full else None
        o["part"].fill_(NAN)
        assert lib.apertis_layernorm_bwd(P(o["X"]), P(o["G"]), P(o["mean"]), P(o["rstd"]), P(o["DY"]), P(o["DR"]), P(dx2),
                                         P(dblk2), p, seed, P(o["part"]), P(dg2), P(db2), T, H, _code(tx), _code(ty), S()) == OK
        torch.cuda.synchronize()
        assert torch.equal(dg1, dg2) and torch.equal(db1, db2) and torch.equal(dx1, dx2), "the backward is not deterministic"


# ---------------------------------------------------------------------------------------------------------------------------
# 3. numerical edges: rows whose fp32 mean / variance are ill-conditioned, against stock fp32 F.layer_norm's own error
EDGE_ROWS = ["constant", "constant-outlier", "mean50", "gamma-zero-neg"]


def _edge_inputs(kind, T, H, gen):
    x = torch.randn(T, H, generator=gen, dtype=torch.float64)
    g = torch.randn(H, generator=gen, dtype=torch.float64) * 0.5 + 1
    b = torch.randn(H, generator=gen, dtype=torch.float64) * 0.2
    if kind == "constant":
        x = torch.full((T, 1), 0.3, dtype=torch.float64) * torch.arange(1, T + 1, dtype=torch.float64)[:, None] / 7 + 0 * x
    elif kind == "constant-outlier":
        x = torch.full((T, H), 0.3, dtype=torch.float64) + 0 * x
        x[torch.arange(T), torch.randint(0, H, (T,), generator=gen)] = 7.0
    elif kind == "mean50":
        x = 50.0 + x
    else:
        g[::3] = 0.0
        g[1::3] = -g[1::3].abs()
    return x.float().double(), g.float().double(), b.float().double()


@pytest.mark.parametrize("eps", [1e-12, 1e-5])
@pytest.mark.parametrize("kind", EDGE_ROWS)
@pytest.mark.parametrize("H", [260, 1028, 4096])
def test_layernorm_numerical_edges_within_twice_stock(dev, H, kind, eps):
    """Constant rows (rstd = eps^-1/2: 1e6 at the default eps, magnifying any rounding of the mean), constant rows with one
    outlier, rows of mean 50 and spread 1, and gamma with zeros and negative entries: the kernels' y and dx may be no
    further from fp64 than twice stock fp32 F.layer_norm (forward and autograd backward on the GPU), plus a floor of 1e-5
    of the reference's largest entry."""
    lib, P, S = _lib()
    T = 37
    gen = torch.Generator().manual_seed(H + len(kind))
    x, g, b = _edge_inputs(kind, T, H, gen)
    dy = torch.randn(T, H, generator=gen, dtype=torch.float64).float().double()
    o, bufs = _ln_run(lib, P, S, dev, x, g, b, eps, dy, None, 0.0, 0, F32, F32, T, H)
    _guards_nan(*bufs)
    xr = x.clone().requires_grad_(True)
    y_ref = F.layer_norm(xr, (H,), g, b, eps)
    y_ref.backward(dy)
    xs = x.float().to(dev).requires_grad_(True)
    ys = F.layer_norm(xs, (H,), g.float().to(dev), b.float().to(dev), eps)
    ys.backward(dy.float().to(dev))
    for name, got, stock, ref in (("y", o["y"], ys, y_ref), ("dx", o["dx"], xs.grad, xr.grad)):
        ref = ref.detach()
        e_k = float((got.cpu().double() - ref).abs().max())
        e_s = float((stock.detach().cpu().double() - ref).abs().max())
        floor = 1e-5 * float(ref.abs().max()) + 1e-30
        assert torch.isfinite(got).all(), name
        assert e_k <= 2 * e_s + floor, f"{kind} {name}: kernel err {e_k:.3e} > 2 x stock {e_s:.3e} + {floor:.3e}"


# ---------------------------------------------------------------------------------------------------------------------------
# 4. block boundary forward (dense and combine forms) and the combine's backward inside the LayerNorm backward
def _slots(T, K, rows, gen, drop_every=5):
    """slot_of [T, K] int32: distinct rows per token, every drop_every-th slot dropped (-1); wk dyadic m / 64."""
    perm = torch.randperm(rows, generator=gen)
    slot = perm[torch.arange(T * K) % rows].view(T, K).to(torch.int32)
    flat = slot.view(-1)
    flat[::drop_every] = -1
    wk = _dyadic((T, K), gen, 64, 63)
    return slot, wk


def _combine64(blk, slot, wk):
    T, K = slot.shape
    out = torch.zeros(T, blk.shape[1], dtype=torch.float64)
    for k in range(K):
        s = slot[:, k].long()
        m = s >= 0
        out[m] += wk[m, k, None] * blk[s[m]]
    return out


@pytest.mark.parametrize("H,tx,ty,T,K", BOUNDARY_CASES,
                         ids=[f"H{c[0]}-{_tag(c[1])}-{_tag(c[2])}-T{c[3]}-K{c[4]}" for c in BOUNDARY_CASES])
def test_boundary_fwd_against_fp64(dev, H, tx, ty, T, K):
    """apertis_dropout_add_layernorm_fwd: y = res + dropout(blk) (dense blk [T, H], or with slot_of / wk the combine
    sum_k wk * blk[slot] of expert rows, dropped slots skipped, rounded to the block dtype) and xn = LayerNorm(y as stored),
    at p 0.1 with the mirror's mask.  y against fp64; xn, mean and rstd against the fp64 LayerNorm of the stored y."""
    lib, P, S = _lib()
    gen = torch.Generator().manual_seed(H * 7 + T * 3 + K)
    p, seed, eps = 0.1, SEEDS[1], 1e-5
    res = _rnd(_rows(T, H, gen), tx)
    g = (torch.randn(H, generator=gen, dtype=torch.float64) * 0.5 + 1).float().double()
    b = (torch.randn(H, generator=gen, dtype=torch.float64) * 0.2).float().double()
    if K:
        rows = 3 * T + 2
        blk = _dyadic((rows, H), gen, 32, 255)
        slot, wk = _slots(T, K, rows, gen)
        a = _rnd(_combine64(blk, slot, wk), ty)
        SL, WK = slot.to(dev), wk.float().to(dev)
    else:
        blk = _rnd(torch.randn(T, H, generator=gen, dtype=torch.float64), ty)
        a, SL, WK = blk, None, None
    keep = _keep_rows(seed, T, H, p)
    ks = 1.0 / (1.0 - float(np.float32(p)))
    ybuf, y = _out((T, H), tx, dev)
    xbuf, xn = _out((T, H), ty, dev)
    mbuf, mean = _out((T,), F32, dev)
    rbuf, rstd = _out((T,), F32, dev)
    assert lib.apertis_dropout_add_layernorm_fwd(P(blk.to(ty).to(dev)), P(SL), P(WK), K, P(res.to(tx).to(dev)),
                                                 P(g.float().to(dev)), P(b.float().to(dev)), eps, P(y), P(xn), P(mean),
                                                 P(rstd), T, H, p, seed, _code(tx), _code(ty), S()) == OK
    torch.cuda.synchronize()
    _guards_nan(ybuf, xbuf, mbuf, rbuf)
    _close(y, res + keep.double() * a * ks, "y", _rtol(tx))
    ys = y.cpu().double()
    xn_ref, m_ref, r_ref, _ = _ln64(ys, g, b, eps)
    _close(xn, xn_ref, "xn", _rtol(ty))
    _close(mean, m_ref, "mean", 1e-4, 1e-5)
    _close(rstd, r_ref, "rstd", 1e-4)


@pytest.mark.parametrize("H,tx,tg,T,K", COMB_BWD_CASES,
                         ids=[f"H{c[0]}-{_tag(c[1])}-{_tag(c[2])}-T{c[3]}-K{c[4]}" for c in COMB_BWD_CASES])
def test_layernorm_combine_bwd_against_fp64(dev, H, tx, tg, T, K):
    """apertis_layernorm_combine_bwd: dx = LayerNorm backward + dres against fp64; dgamma / dbeta as sums; and the combine's
    backward on d = the masked gradient row as stored (dx rounded to x's dtype, masked, scaled, rounded to the gradient
    dtype): dyr[slot] = wk * d, dwk = <d, yr[slot]> in fp64.  Dropped slots leave dwk untouched and no expert row written."""
    lib, P, S = _lib()
    gen = torch.Generator().manual_seed(H * 13 + T + K)
    p, seed, eps = 0.1, SEEDS[2], 1e-5
    x = _rnd(_rows(T, H, gen), tx)
    g = (torch.randn(H, generator=gen, dtype=torch.float64) * 0.5 + 1).float().double()
    dy = _rnd(torch.randn(T, H, generator=gen, dtype=torch.float64), tg)
    dres = _rnd(torch.randn(T, H, generator=gen, dtype=torch.float64), tx)
    rows = 2 * T + 3
    yr = _dyadic((rows, H), gen, 32, 255)
    slot, wk = _slots(T, K, rows, gen, drop_every=3)
    _, m64, r64, xh = _ln64(x, g, torch.zeros(H, dtype=torch.float64), eps)
    X = x.to(tx).to(dev)
    mean, rstd = m64.float().to(dev), r64.float().to(dev)
    nblk = lib.apertis_layernorm_bwd_blocks(T, H)
    part = torch.full((nblk, 2, H), NAN, device=dev)
    dxbuf, dx = _out((T, H), tx, dev)
    dgbuf, dg = _out((H,), F32, dev)
    dbbuf, db = _out((H,), F32, dev)
    dyrbuf, dyr = _out((rows, H), tg, dev)
    dwkbuf, dwk = _out((T, K), F32, dev)
    assert lib.apertis_layernorm_combine_bwd(P(X), P(g.float().to(dev)), P(mean), P(rstd), P(dy.to(tg).to(dev)),
                                             P(dres.to(tx).to(dev)), P(dx), p, seed, P(part), P(dg), P(db), P(slot.to(dev)),
                                             P(wk.float().to(dev)), P(yr.to(tg).to(dev)), P(dyr), P(dwk), T, H, K, _code(tx),
                                             _code(tg), S()) == OK
    torch.cuda.synchronize()
    _guards_nan(dxbuf, dgbuf, dbbuf, dyrbuf, dwkbuf)
    dx_ref, dgr, dbr = _ln_bwd64(xh, r64.float().double(), g, dy)
    _close(dx, dx_ref + dres, "dx", _rtol(tx))
    _sum_close(dg, dgr.sum(0), T, "dgamma")
    _sum_close(db, dbr.sum(0), T, "dbeta")
    keep = _keep_rows(seed, T, H, p)
    ks = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    d = (dx.cpu().float() * keep.float() * float(ks)).to(tg).double()     # the row as apertis_moe_combine_bwd would read it
    yrq = _rnd(yr, tg)
    written = torch.zeros(rows, dtype=torch.bool)
    for k in range(K):
        s = slot[:, k].long()
        m = s >= 0
        written[s[m]] = True
        _close(dyr.cpu()[s[m]], wk[m, k, None] * d[m], f"dyr k{k}", _rtol(tg))
        _sum_close(dwk.cpu()[m, k], (d[m] * yrq[s[m]]).sum(-1), H, f"dwk k{k}", scale=4.0)
        assert torch.isnan(dwk.cpu()[~m, k]).all(), "a dropped slot's weight gradient was written"
    assert torch.isnan(dyr.cpu()[~written].float()).all(), "an expert row no slot points at was written"


# ---------------------------------------------------------------------------------------------------------------------------
# 5. MoE gather-LN and combine
def _plan(S, E, K, shape, gen, pad=37):
    """A dispatch plan built by hand (apertis_moe_plan's canonical order: expert-major, then k, then token): 'mixed' leaves
    one expert empty and cuts another to one row (its other slots dropped); 'edge' cuts expert 0 to exactly 64 rows (the
    gather-LN backward's 64-row block edge) and empties expert 1.  max_rows = kept rows + pad (capacity padding)."""
    Ef = list(range(E))
    empty = {E - 1} if E > 2 and shape == "mixed" else ({1} if shape == "edge" else set())
    allowed = torch.tensor([e for e in Ef if e not in empty])
    idx = torch.stack([allowed[torch.randperm(len(allowed), generator=gen)[:K]] for _ in range(S)])
    lists = {e: [] for e in Ef}
    for e in Ef:
        for k in range(K):
            for s in range(S):
                if int(idx[s, k]) == e:
                    lists[e].append((s, k))
    if shape == "mixed" and E > 2:
        lists[0] = lists[0][:1]
    if shape == "edge":
        assert len(lists[0]) >= 64
        lists[0] = lists[0][:64]
    counts = [len(lists[e]) for e in Ef]
    offsets = torch.tensor([0] + list(np.cumsum(counts)), dtype=torch.int32)
    total = int(offsets[-1])
    max_rows = total + pad
    row_token = torch.zeros(max_rows, dtype=torch.int32)
    row_k = torch.zeros(max_rows, dtype=torch.int32)
    slot_of = torch.full((S, K), -1, dtype=torch.int32)
    expert = torch.zeros(total, dtype=torch.long)
    r = 0
    for e in Ef:
        for s, k in lists[e]:
            row_token[r], row_k[r], slot_of[s, k], expert[r] = s, k, r, e
            r += 1
    return dict(offsets=offsets, row_token=row_token, row_k=row_k, slot_of=slot_of, total=total, max_rows=max_rows,
                expert=expert, counts=counts)


@pytest.mark.parametrize("cid,H,tx,to,S,E,K,shape", GATHER_CASES, ids=[c[0] for c in GATHER_CASES])
def test_gather_ln_and_combine_against_fp64(dev, cid, H, tx, to, S, E, K, shape):
    """apertis_moe_gather_ln_fwd / _bwd and apertis_moe_combine_fwd / _bwd against fp64 on a hand-built plan: experts with 0
    and 1 rows, an expert boundary on the 64-row block edge, E up to 64 and K up to 8, max_rows past the kept rows (the
    padding rows of the outputs stay NaN, the padding rows of the incoming gradient are NaN and must not be read), dropped
    slots.  The gather-LN backward runs with dxr and with dxr = NULL (affine gradients only: the same dgamma / dbeta); blocks
    straddling experts add with atomics, so its dgamma / dbeta are held to the sum bound, not to bits."""
    lib, P, Sx = _lib()
    gen = torch.Generator().manual_seed(H + S * 3 + E * 5 + K)
    pl = _plan(S, E, K, shape, gen)
    if shape == "edge":
        assert pl["counts"][0] == 64 and pl["counts"][1] == 0
    elif E > 2:
        assert 0 in pl["counts"] and 1 in pl["counts"]
    total, R = pl["total"], pl["max_rows"]
    eps = 1e-12
    x = _rnd(_rows(S, H, gen), tx)
    gam = (torch.randn(E, H, generator=gen, dtype=torch.float64) * 0.5 + 1).float().double()
    bet = (torch.randn(E, H, generator=gen, dtype=torch.float64) * 0.2).float().double()
    OFF, RT, RK, SL = (pl[k].to(dev) for k in ("offsets", "row_token", "row_k", "slot_of"))
    X, GA, BE = x.to(tx).to(dev), gam.float().to(dev), bet.float().to(dev)
    rt, ex = pl["row_token"][:total].long(), pl["expert"]

    # ---- gather-LN forward
    xgbuf, xg = _out((R, H), to, dev)
    mbuf, mean = _out((R,), F32, dev)
    rbuf, rstd = _out((R,), F32, dev)
    assert lib.apertis_moe_gather_ln_fwd(P(X), P(RT), P(OFF), P(GA), P(BE), eps, P(xg), P(mean), P(rstd), R, H, E, _code(tx),
                                         _code(to), Sx()) == OK
    torch.cuda.synchronize()
    _guards_nan(xgbuf, mbuf, rbuf)
    xr = x[rt]
    y_ref, m_ref, r_ref, xh = _ln64(xr, gam[ex], bet[ex], eps)
    _close(xg[:total], y_ref, "xg", _rtol(to))
    _close(mean[:total], m_ref, "mean", 1e-4, 1e-5)
    _close(rstd[:total], r_ref, "rstd", 1e-4)
    assert torch.isnan(xg[total:].float()).all() and torch.isnan(mean[total:]).all(), "padding rows written"

    # ---- gather-LN backward (dxg in the output dtype), with dxr and without
    dxg = _rnd(torch.randn(R, H, generator=gen, dtype=torch.float64), to)
    dxg[total:] = NAN
    DXG = dxg.to(to).to(dev)
    nblk = lib.apertis_moe_gather_ln_bwd_blocks(R)
    dx_ref, dgr, dbr = _ln_bwd64(xh, r_ref, gam[ex], dxg[:total])
    dg_ref = torch.zeros(E, H, dtype=torch.float64).index_add_(0, ex, dgr)
    db_ref = torch.zeros(E, H, dtype=torch.float64).index_add_(0, ex, dbr)
    for with_dxr in (True, False):
        part = torch.full((nblk, 2 * H), NAN, device=dev)
        bexp = torch.full((nblk,), -7, dtype=torch.int32, device=dev)
        dgbuf, dg = _out((E, H), F32, dev, fill=0.0)
        dbbuf, db = _out((E, H), F32, dev, fill=0.0)
        dxrbuf, dxr = _out((R, H), to, dev)
        assert lib.apertis_moe_gather_ln_bwd(P(X), P(RT), P(OFF), P(GA), P(mean), P(rstd), P(DXG), P(dxr) if with_dxr else None,
                                             P(dg), P(db), P(part), P(bexp), R, H, E, _code(tx), _code(to), Sx()) == OK
        torch.cuda.synchronize()
        _guards_nan(dgbuf, dbbuf, dxrbuf)
        if with_dxr:
            _close(dxr[:total], dx_ref, "dxr", _rtol(to))
            assert torch.isnan(dxr[total:].float()).all(), "padding rows of dxr written"
        else:
            assert torch.isnan(dxr.float()).all(), "dxr = NULL, yet rows were written"
        _sum_close(dg, dg_ref, max(pl["counts"]), f"dgamma (dxr {with_dxr})")
        _sum_close(db, db_ref, max(pl["counts"]), f"dbeta (dxr {with_dxr})")

    # ---- combine forward (weighted and not) and backward on expert rows yr [R, H] in the output dtype
    yr = _dyadic((R, H), gen, 32, 255)
    yr[total:] = NAN                                      # rows past the kept ones are never read
    YR = yr.to(to).to(dev)
    wk = _dyadic((S, K), gen, 64, 63)
    WK = wk.float().to(dev)
    slot = pl["slot_of"]
    for with_w in (1, 0):
        obuf, out = _out((S, H), tx, dev)
        assert lib.apertis_moe_combine_fwd(P(YR), P(SL), P(WK), P(out), S, H, K, with_w, _code(to), _code(tx), Sx()) == OK
        torch.cuda.synchronize()
        _guards_nan(obuf)
        _close(out, _rnd(_combine64(yr, slot, wk if with_w else torch.ones_like(wk)), tx), f"combine (w {with_w})", _rtol(tx))
    dout = _rnd(torch.randn(S, H, generator=gen, dtype=torch.float64), tx)
    dyrbuf, dyr = _out((R, H), to, dev)
    dwkbuf, dwk = _out((S, K), F32, dev)
    assert lib.apertis_moe_combine_bwd(P(dout.to(tx).to(dev)), P(YR), P(RT), P(RK), P(OFF), P(WK), P(dyr), P(dwk), R, S, H, K, E,
                                       _code(tx), _code(to), Sx()) == OK
    torch.cuda.synchronize()
    _guards_nan(dyrbuf, dwkbuf)
    rk = pl["row_k"][:total].long()
    _close(dyr[:total], wk[rt, rk, None] * dout[rt], "dyr", _rtol(to))
    assert torch.isnan(dyr[total:].float()).all(), "padding rows of dyr written"
    kept = slot >= 0
    dwk_ref = torch.zeros(S, K, dtype=torch.float64)
    dwk_ref[rt, rk] = (dout[rt] * yr[:total]).sum(-1)
    _sum_close(dwk.cpu()[kept], dwk_ref[kept], H, "dwk", scale=4.0)
    assert torch.isnan(dwk.cpu()[~kept]).all(), "a dropped slot's weight gradient was written"


# ---------------------------------------------------------------------------------------------------------------------------
# 6. router family (IT 1..4)
def _router_ref(xn_in, rg, rb, reps, W, bW, dlogits):
    """fp64 logits = Linear(LayerNorm(x)) and the gradients of <logits, dlogits>: (logits, mean, rstd, dx, dW, db, dg, dbeta)."""
    x = xn_in.clone().requires_grad_(True)
    g, b, w, bb = (t.clone().requires_grad_(True) for t in (rg, rb, W, bW))
    u = F.layer_norm(x, (x.shape[-1],), g, b, reps)
    lg = u @ w.T + bb
    lg.backward(dlogits)
    _, m, r, _ = _ln64(xn_in, rg, rb, reps)
    return lg.detach(), m, r, x.grad, w.grad, bb.grad, g.grad, b.grad


def _router_params(H, N, gen):
    rg = (torch.randn(H, generator=gen, dtype=torch.float64) * 0.2 + 1).float().double()
    rb = (torch.randn(H, generator=gen, dtype=torch.float64) * 0.1).float().double()
    W = (torch.randn(N, H, generator=gen, dtype=torch.float64) * 0.05).float().double()
    bW = (torch.randn(N, generator=gen, dtype=torch.float64) * 0.1).float().double()
    return rg, rb, W, bW


@pytest.mark.parametrize("H,N,tx", ROUTER_CASES, ids=[f"H{c[0]}-N{c[1]}-{_tag(c[2])}" for c in ROUTER_CASES])
def test_router_fwd_and_bwd_rows_against_fp64(dev, H, N, tx):
    """apertis_router_fwd (logits, mean, rstd) and apertis_router_bwd_rows (dx with dres and the gradient rows of two slots per
    row - dyadic, so their sum is exact in bf16 - added; dW, db, dgamma, dbeta) against fp64 autograd."""
    lib, P, S = _lib()
    T, KS = 45, 2
    gen = torch.Generator().manual_seed(H * 3 + N)
    x = _rnd(_rows(T, H, gen), tx)
    rg, rb, W, bW = _router_params(H, N, gen)
    reps = 1e-5
    dl = torch.randn(T, N, generator=gen, dtype=torch.float64).float().double()
    dres = _rnd(torch.randn(T, H, generator=gen, dtype=torch.float64), tx)
    rows = 2 * T
    grows = _dyadic((rows, H), gen, 32, 127)
    slot, _ = _slots(T, KS, rows, gen, drop_every=4)
    lg_ref, m_ref, r_ref, dx_ref, dW_ref, db_ref, dg_ref, dbe_ref = _router_ref(x, rg, rb, reps, W, bW, dl)
    X, RG, RB, WW, BW = x.to(tx).to(dev), rg.float().to(dev), rb.float().to(dev), W.float().to(dev), bW.float().to(dev)
    lbuf, lg = _out((T, N), F32, dev)
    mbuf, mean = _out((T,), F32, dev)
    rbuf, rstd = _out((T,), F32, dev)
    assert lib.apertis_router_fwd(P(X), P(RG), P(RB), reps, P(WW), P(BW), P(lg), P(mean), P(rstd), T, H, N, _code(tx), S()) == OK
    torch.cuda.synchronize()
    _guards_nan(lbuf, mbuf, rbuf)
    _close(lg, lg_ref, "logits", 1e-4)
    _close(mean, m_ref, "mean", 1e-4, 1e-5)
    _close(rstd, r_ref, "rstd", 1e-4)
    nblk = lib.apertis_router_bwd_blocks(T)
    cols = N * H + N + 2 * H
    part = torch.full((nblk, cols), NAN, device=dev)
    dxbuf, dx = _out((T, H), tx, dev)
    gbuf, grads = _out((cols,), F32, dev)
    assert lib.apertis_router_bwd_rows(P(X), P(RG), P(RB), P(mean), P(rstd), P(WW), P(dl.float().to(dev)), P(dres.to(tx).to(dev)),
                                       P(grows.to(tx).to(dev)), P(slot.to(dev)), KS, P(dx), P(part), P(grads), T, H, N,
                                       _code(tx), S()) == OK
    torch.cuda.synchronize()
    _guards_nan(dxbuf, gbuf)
    rsum = _combine64(grows, slot, torch.ones(T, KS, dtype=torch.float64))
    _close(dx, dx_ref + dres + rsum, "dx", _rtol(tx))
    gc = grads.cpu()
    _sum_close(gc[:N * H].view(N, H), dW_ref, T, "dW")
    _sum_close(gc[N * H:N * H + N], db_ref, T, "db")
    _sum_close(gc[N * H + N:N * H + N + H], dg_ref, T, "dgamma_r", scale=0.2)
    _sum_close(gc[N * H + N + H:], dbe_ref, T, "dbeta_r", scale=0.2)


@pytest.mark.parametrize("H,N,tx", ROUTER_CASES, ids=[f"H{c[0]}-N{c[1]}-{_tag(c[2])}" for c in ROUTER_CASES])
def test_boundary_router_fwd_and_bwd_against_fp64(dev, H, N, tx):
    """apertis_dropout_add_layernorm_router_fwd (y, xn, mean, rstd of the boundary; the router's logits, rmean, rrstd on xn as
    stored) and apertis_boundary_router_bwd (fp32 stream; gradient dtype tx): dx, dblk (the mirror's mask) and the boundary's
    dgamma / dbeta against fp64 of the stored xn's router gradient plus rows, rounded to the gradient dtype as the kernel
    hands it over; the router's dW, db, dgamma, dbeta against fp64."""
    lib, P, S = _lib()
    T, KS, p, seed, eps, reps = 45, 2, 0.1, SEEDS[0], 1e-5, 1e-5
    gen = torch.Generator().manual_seed(H * 5 + N)
    ty = tx                         # blk / xn dtype (the stream y is fp32 here)
    res = _rows(T, H, gen).float().double()
    blk = _rnd(torch.randn(T, H, generator=gen, dtype=torch.float64), ty)
    g = (torch.randn(H, generator=gen, dtype=torch.float64) * 0.5 + 1).float().double()
    b = (torch.randn(H, generator=gen, dtype=torch.float64) * 0.2).float().double()
    rg, rb, W, bW = _router_params(H, N, gen)
    keep = _keep_rows(seed, T, H, p)
    ks = 1.0 / (1.0 - float(np.float32(p)))
    G, B, RG, RB, WW, BW = (t.float().to(dev) for t in (g, b, rg, rb, W, bW))
    ybuf, y = _out((T, H), F32, dev)
    xbuf, xn = _out((T, H), ty, dev)
    mbuf, mean = _out((T,), F32, dev)
    rbuf, rstd = _out((T,), F32, dev)
    lbuf, lg = _out((T, N), F32, dev)
    m2buf, rmean = _out((T,), F32, dev)
    r2buf, rrstd = _out((T,), F32, dev)
    assert lib.apertis_dropout_add_layernorm_router_fwd(P(blk.to(ty).to(dev)), P(res.float().to(dev)), P(G), P(B), eps, P(y),
                                                        P(xn), P(mean), P(rstd), P(RG), P(RB), reps, P(WW), P(BW), P(lg),
                                                        P(rmean), P(rrstd), T, H, N, p, seed, _code(F32), _code(ty), S()) == OK
    torch.cuda.synchronize()
    _guards_nan(ybuf, xbuf, mbuf, rbuf, lbuf, m2buf, r2buf)
    _close(y, res + keep.double() * blk * ks, "y", 1e-4)
    ys = y.cpu().double()
    xn_ref, m_ref, r_ref, xh = _ln64(ys, g, b, eps)
    _close(xn, xn_ref, "xn", _rtol(ty))
    _close(mean, m_ref, "mean", 1e-4, 1e-5)
    _close(rstd, r_ref, "rstd", 1e-4)
    xns = xn.cpu().double()
    dl = torch.randn(T, N, generator=gen, dtype=torch.float64).float().double()
    lg_ref, rm_ref, rr_ref, dxn_ref, dW_ref, db_ref, dg_ref, dbe_ref = _router_ref(xns, rg, rb, reps, W, bW, dl)
    _close(lg, lg_ref, "logits", 1e-4)
    _close(rmean, rm_ref, "rmean", 1e-4, 1e-5)
    _close(rrstd, rr_ref, "rrstd", 1e-4)

    # backward
    dres = torch.randn(T, H, generator=gen, dtype=torch.float64).float().double()
    rows = 2 * T
    grows = _dyadic((rows, H), gen, 32, 127)
    slot, _ = _slots(T, KS, rows, gen, drop_every=4)
    gxn = dxn_ref + _combine64(grows, slot, torch.ones(T, KS, dtype=torch.float64))     # total gradient of xn
    gxn_q = _rnd(gxn, ty)                                   # handed to the boundary norm's backward in the gradient dtype
    dx_ref, dgr, dbr = _ln_bwd64(xh, r_ref, g, gxn_q)
    dx_ref = dx_ref + dres
    nblk = lib.apertis_router_bwd_blocks(T)
    cols = N * H + N + 2 * H
    part = torch.full((nblk, cols + 2 * H), NAN, device=dev)
    dxbuf, dx = _out((T, H), F32, dev)
    dkbuf, dblk = _out((T, H), ty, dev)
    gbuf, rgrads = _out((cols,), F32, dev)
    dgbuf, dg = _out((H,), F32, dev)
    dbbuf, db = _out((H,), F32, dev)
    assert lib.apertis_boundary_router_bwd(P(y), P(G), P(mean), P(rstd), P(dres.float().to(dev)), P(dx), P(dblk), p, seed, P(xn),
                                           P(RG), P(RB), P(rmean), P(rrstd), P(WW), P(dl.float().to(dev)),
                                           P(grows.to(ty).to(dev)), P(slot.to(dev)), KS, P(part), P(rgrads), P(dg), P(db), T, H,
                                           N, _code(F32), _code(ty), S()) == OK
    torch.cuda.synchronize()
    _guards_nan(dxbuf, dkbuf, gbuf, dgbuf, dbbuf)
    # the handed-over gradient is rounded once in the kernel too; a bf16 tie apart moves dx by up to one bf16 step of it
    _close(dx, dx_ref, "dx", _rtol(ty), 1e-5 if ty == F32 else 8e-3)
    _close(dblk, keep.double() * dx.cpu().double() * ks, "dblk", _rtol(ty), 1e-6)
    gsc = 1.0 if ty == F32 else 64.0      # (bf16: a hand-over a tie apart moves one term by a bf16 step of dy ~ 4)
    _sum_close(dg, dgr.sum(0), T, "dgamma", scale=gsc)
    _sum_close(db, dbr.sum(0), T, "dbeta", scale=gsc)
    gc = rgrads.cpu()
    _sum_close(gc[:N * H].view(N, H), dW_ref, T, "dW")
    _sum_close(gc[N * H:N * H + N], db_ref, T, "db")
    _sum_close(gc[N * H + N:N * H + N + H], dg_ref, T, "dgamma_r", scale=0.2)
    _sum_close(gc[N * H + N + H:], dbe_ref, T, "dbeta_r", scale=0.2)


# ---------------------------------------------------------------------------------------------------------------------------
# 7. refusals: shapes the entry points do not take leave their outputs untouched
REFUSE = [("H0", 0), ("H4098", 4098), ("H4100", 4100)]


@pytest.mark.parametrize("what,H", REFUSE, ids=[r[0] for r in REFUSE])
def test_entry_points_refuse_widths_they_do_not_take(dev, what, H):
    """H = 0, H % 4 != 0 and H > 4096: APERTIS_ERR_UNSUPPORTED from every entry point of the family, nothing written."""
    lib, P, S = _lib()
    T, E, K = 8, 4, 2
    Hb = max(H, 4)
    f = lambda *s: torch.randn(*s, device=dev)                                       # noqa: E731
    x, g, b = f(T, Hb), f(Hb), f(Hb)
    out = torch.full((T * Hb + 64,), NAN, device=dev)
    m, r = torch.full((T,), NAN, device=dev), torch.full((T,), NAN, device=dev)
    part = torch.full((64, 2 * Hb), NAN, device=dev)
    offs = torch.tensor([0, 2, 4, 6, 8], dtype=torch.int32, device=dev)
    rt = torch.arange(T, dtype=torch.int32, device=dev)
    slot = torch.arange(T * K, dtype=torch.int32, device=dev).view(T, K) % T
    wk = f(T, K)
    be = torch.zeros(64, dtype=torch.int32, device=dev)
    F_ = _code(F32)
    U = ERR_UNSUPPORTED
    assert lib.apertis_layernorm_fwd(P(x), P(g), P(b), 1e-5, P(out), P(m), P(r), T, H, F_, F_, S()) == U
    assert lib.apertis_layernorm_bwd(P(x), P(g), P(m), P(r), P(x), None, P(out), None, 0.0, 0, P(part), P(out), P(out), T, H, F_, F_,
                                     S()) == U
    assert lib.apertis_layernorm_combine_bwd(P(x), P(g), P(m), P(r), P(x), None, P(out), 0.0, 0, P(part), P(out), P(out), P(slot),
                                             P(wk), P(x), P(out), P(out), T, H, K, F_, F_, S()) == U
    for sl, kk in ((None, 0), (slot, K)):
        assert lib.apertis_dropout_add_layernorm_fwd(P(x), P(sl), P(wk) if sl is not None else None, kk, P(x), P(g), P(b), 1e-5,
                                                     P(out), P(out), P(m), P(r), T, H, 0.1, 1, F_, F_, S()) == U
    assert lib.apertis_moe_gather_ln_fwd(P(x), P(rt), P(offs), P(x), P(x), 1e-5, P(out), P(m), P(r), T, H, E, F_, F_, S()) == U
    assert lib.apertis_moe_gather_ln_bwd(P(x), P(rt), P(offs), P(x), P(m), P(r), P(x), P(out), P(out), P(out), P(part), P(be), T, H,
                                         E, F_, F_, S()) == U
    assert lib.apertis_moe_combine_fwd(P(x), P(slot), P(wk), P(out), T, H, K, 1, F_, F_, S()) == U
    assert lib.apertis_moe_combine_bwd(P(x), P(x), P(rt), P(rt), P(offs), P(wk), P(out), P(out), T, T, H, K, E, F_, F_, S()) == U
    assert lib.apertis_router_fwd(P(x), P(g), P(b), 1e-5, P(x), P(b), P(out), P(m), P(r), T, H, 4, F_, S()) == U
    assert lib.apertis_router_bwd_rows(P(x), P(g), P(b), P(m), P(r), P(x), P(wk), None, None, None, 0, P(out), P(part), P(out), T,
                                       H, 4, F_, S()) == U
    assert lib.apertis_dropout_add_layernorm_router_fwd(P(x), P(x), P(g), P(b), 1e-5, P(out), P(out), P(m), P(r), P(g), P(b), 1e-5,
                                                        P(x), P(b), P(out), P(m), P(r), T, H, 4, 0.1, 1, F_, F_, S()) == U
    assert lib.apertis_boundary_router_bwd(P(x), P(g), P(m), P(r), None, P(out), P(out), 0.0, 0, P(x), P(g), P(b), P(m), P(r),
                                           P(x), P(wk), None, None, 0, P(part), P(out), P(out), P(out), T, H, 4, F_, F_, S()) == U
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(m).all() and torch.isnan(r).all() and torch.isnan(part).all()


def test_entry_points_refuse_expert_and_slot_counts_they_do_not_take(dev):
    """E = 65 (gather-LN, combine backward) and K = 9 (combine forward and backward): APERTIS_ERR_UNSUPPORTED; K = 9 in the
    boundary forward's combine form: APERTIS_ERR_ARG; K = 3 in apertis_layernorm_combine_bwd (it takes K <= 2):
    APERTIS_ERR_UNSUPPORTED.  Nothing written."""
    lib, P, S = _lib()
    T, H = 8, 64
    f = lambda *s: torch.randn(*s, device=dev)                                       # noqa: E731
    x, g, b = f(T, H), f(H), f(H)
    out = torch.full((T * H + 64,), NAN, device=dev)
    m, r = torch.full((T,), NAN, device=dev), torch.full((T,), NAN, device=dev)
    part = torch.full((64, 2 * H), NAN, device=dev)
    offs = torch.zeros(66, dtype=torch.int32, device=dev)
    offs[1:] = T
    rt = torch.arange(T, dtype=torch.int32, device=dev)
    slot9 = torch.arange(T * 9, dtype=torch.int32, device=dev).view(T, 9) % T
    wk9 = f(T, 9)
    be = torch.zeros(64, dtype=torch.int32, device=dev)
    F_, U = _code(F32), ERR_UNSUPPORTED
    assert lib.apertis_moe_gather_ln_fwd(P(x), P(rt), P(offs), P(x), P(x), 1e-5, P(out), P(m), P(r), T, H, 65, F_, F_, S()) == U
    assert lib.apertis_moe_gather_ln_bwd(P(x), P(rt), P(offs), P(x), P(m), P(r), P(x), P(out), P(out), P(out), P(part), P(be), T, H,
                                         65, F_, F_, S()) == U
    assert lib.apertis_moe_combine_bwd(P(x), P(x), P(rt), P(rt), P(offs), P(wk9), P(out), P(out), T, T, H, 2, 65, F_, F_, S()) == U
    assert lib.apertis_moe_combine_fwd(P(x), P(slot9), P(wk9), P(out), T, H, 9, 1, F_, F_, S()) == U
    assert lib.apertis_moe_combine_bwd(P(x), P(x), P(rt), P(rt), P(offs), P(wk9), P(out), P(out), T, T, H, 9, 4, F_, F_, S()) == U
    assert lib.apertis_dropout_add_layernorm_fwd(P(x), P(slot9), P(wk9), 9, P(x), P(g), P(b), 1e-5, P(out), P(out), P(m), P(r), T,
                                                 H, 0.1, 1, F_, F_, S()) == ERR_ARG
    assert lib.apertis_layernorm_combine_bwd(P(x), P(g), P(m), P(r), P(x), None, P(out), 0.0, 0, P(part), P(out), P(out), P(slot9),
                                             P(wk9), P(x), P(out), P(out), T, H, 3, F_, F_, S()) == U
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(m).all() and torch.isnan(r).all() and torch.isnan(part).all()


@pytest.mark.parametrize("H", [4098, 4100])
def test_hip_layer_norm_takes_the_stock_path_past_the_kernels(dev, H):
    """HipLayerNorm at H = 4100 (> 4096) and 4098 (% 4 != 0): the stock F.layer_norm path, forward and backward against fp64."""
    from apertis_llm_amd.model import HipLayerNorm
    torch.manual_seed(H)
    ln = HipLayerNorm(H, eps=1e-5).to(dev)
    with torch.no_grad():
        ln.weight.normal_(1.0, 0.3)
        ln.bias.normal_(0.0, 0.2)
    x0 = torch.randn(3, 5, H) * 2 + 0.5
    dy = torch.randn(3, 5, H)
    x = x0.to(dev).requires_grad_(True)
    y = ln(x)
    y.backward(dy.to(dev))
    xr = x0.double().requires_grad_(True)
    wr, br = ln.weight.detach().cpu().double().requires_grad_(True), ln.bias.detach().cpu().double().requires_grad_(True)
    yr = F.layer_norm(xr, (H,), wr, br, 1e-5)
    yr.backward(dy.double())
    _close(y, yr, "y", 1e-4)
    _close(x.grad, xr.grad, "dx", 1e-4)
    _sum_close(ln.weight.grad, wr.grad, 15, "dgamma")
    _sum_close(ln.bias.grad, br.grad, 15, "dbeta")


# ---------------------------------------------------------------------------------------------------------------------------
# 8. whole models whose norms run at IT 8 and 16
@pytest.mark.parametrize("H", [2048, 4096])
def test_wide_moe_model_vs_oracle(dev, H):
    """ApertisForCausalLM (1 layer, selective_ssm, MoE feed-forward with 4 experts, fp32, eval mode) at H = 2048 and 4096 - the
    pre-norms, the block boundaries, the gather-LN and the combine at IT 8 and 16: logits, loss and every parameter gradient
    against fp64 autograd through the CPU oracle at the BASELINE bar (rtol 1e-4, floor 1e-5 of each tensor's largest entry)."""
    import apertis_llm_amd as A
    from oracle import ref_cpu
    torch.manual_seed(H + 1)
    cfg = A.ApertisConfig(vocab_size=96, hidden_size=H, num_hidden_layers=1, num_attention_heads=2, ssm_d_state=16,
                          intermediate_size=64, attention_type="selective_ssm", use_expert_system=True, num_experts=4,
                          experts_per_token=2)
    model = A.ApertisForCausalLM(cfg).to(dev).eval()
    ids = torch.randint(4, 96, (2, 40), device=dev)
    out = model(input_ids=ids, labels=ids, use_cache=False)
    out[0].backward()
    torch.cuda.synchronize()
    sd = {n: v.detach().cpu().double().requires_grad_(True) for n, v in model.state_dict().items() if n != "lm_head.weight"}
    o_loss, o_logits = ref_cpu.model_forward(sd, dict(cfg.to_dict()), ids.cpu(), None, ids.cpu())
    o_loss.backward()
    rel_error_report(f"H{H} moe logits", out[1], o_logits, rtol=1e-4, atol_scale=1e-5)
    assert abs(float(out[0]) - float(o_loss)) <= 1e-4 * abs(float(o_loss)), (float(out[0]), float(o_loss))
    ours = {n: p.grad for n, p in model.named_parameters()}
    checked = []
    for n, ref in sd.items():
        if ref.grad is None:
            continue
        if ".experts." in n:                                  # the stock per-expert Linear of the checkpoint: a stacked slice
            pre, rest = n.split(".experts.")
            e, suffix = rest.split(".", 1)
            got = ours[f"{pre}.{dict(A.AdaptiveExpertSystem._STACKED)[suffix]}"][int(e)]
        else:
            got = ours.get(n)
        if got is None:
            assert float(ref.grad.abs().max()) == 0.0, n
            continue
        rec = rel_error_report(f"H{H} moe grad {n}", got, ref.grad, rtol=1e-4, atol_scale=1e-5, check=False)
        assert rec["worst_excess"] <= 1.0, rec
        checked.append(n)
    assert len(checked) >= 15 and sum(".experts." in n for n in checked) == 4 * len(A.AdaptiveExpertSystem._STACKED), checked
