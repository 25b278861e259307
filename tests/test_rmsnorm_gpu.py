"""The RMSNorm row kernels (csrc/rmsnorm.hip) against float64 references on the same rounded inputs, through the C ABI and the
ops: apertis_rmsnorm_fwd / _bwd and the block boundary apertis_dropout_add_rmsnorm_fwd (dense and combine forms).

Per row of width H: r = sqrt(sum x^2 / H), s = r + eps, y = scale * x / s; backward dx = scale * dy / s - x * c / (H r s^2) with
c = sum_j scale_j dy_j x_j (second term 0 where r == 0), dscale = sum over rows of dy * x / s.

The kernels are templates on IT = ceil(H / 256) rounded up by DISPATCH_IT, as the LayerNorm family's; the cases sit at both
ends of every bucket in all four (x, y) dtype pairs, the backward on both sides of its two-level fold.  The helpers (NaN-guarded
outputs, tolerances, the numpy copy of drop_keep) are tests/test_row_kernels_gpu.py's, and so are the tolerances: fp32 outputs
rtol 1e-4 with a floor of 1e-5 of the tensor's largest entry, bf16 outputs one bf16 rounding (rtol 8e-3), dscale an absolute
bound growing with sqrt(T).  Where a step reads an output the kernel rounded (the norm of a boundary reads the y it stored, dblk
is the masked copy of dx as stored) the reference starts from that stored output, itself checked against fp64."""
import numpy as np
import pytest
import torch

from test_row_kernels_gpu import (BF16, F32, IT_BUCKETS, NAN, OK, PAIRS_2T, SEEDS, WIDTHS, _bucket, _close, _code, _combine64, _dyadic,
                                  _guards_nan, _h_ok, _keep_rows, _lib, _out, _rnd, _rows, _rtol, _slots, _sum_close, _tag)

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------------------------------
# mirror of the dispatch in csrc/rmsnorm.hip (rms_part_rows / rms_two_level): a change there must be made here too
RMS_ROWS_PER_BLOCK = 4 * 8          # four waves x RMS_RPW (8) rows
RMS_FOLD_GROUPS = 32


def _rms_fold(T):
    """'two' when apertis_rmsnorm_bwd folds its partial rows in two levels (rms_two_level), else 'one'."""
    return "two" if -(-max(T, 1) // RMS_ROWS_PER_BLOCK) >= 8 * RMS_FOLD_GROUPS else "one"


# forward + backward: (H, dtype_x, dtype_y = dtype_g, T, form); 'plain' = no dres / dblk, 'full' = dres and dblk at p 0.1
RMS_CASES = ([(H, tx, ty, 1, "plain") for H in WIDTHS for tx, ty in PAIRS_2T] +
             [(H, tx, ty, 3, "full") for H in WIDTHS for tx, ty in PAIRS_2T] +
             # row counts that are no multiple of the 32 rows of a block
             [(4096, F32, F32, 97, "full"), (3076, BF16, BF16, 65, "plain"), (772, F32, BF16, 300, "full"),
              # the fold threshold (8160 rows: 255 partial rows, one level; 8161: 256, two) and a short last fold group (8225:
              # 258 partial rows in groups of 9 - the last has 6)
              (252, F32, F32, 8160, "plain"), (252, BF16, BF16, 8161, "full"), (244, F32, BF16, 8225, "full"),
              (260, BF16, F32, 8225, "plain")])

# boundary forward: (H, dtype_x, dtype_y, T, K): K = 0 the dense form, else the combine form with K slots per token
RMS_BOUNDARY_CASES = ([(H, *PAIRS_2T[i % 4], 5, 0) for i, H in enumerate(WIDTHS)] +
                      [(H, *PAIRS_2T[(i + 1) % 4], 6, (1, 2, 3, 8)[i % 4]) for i, H in enumerate(WIDTHS)] +
                      [(H, tx, ty, 9, 0) for H in (260, 3076) for tx, ty in PAIRS_2T] +
                      [(1028, tx, ty, 7, 2) for tx, ty in PAIRS_2T])


def test_case_tables_cover_every_dispatch_path():
    """From the mirror: every entry point meets every IT bucket (both ends) in every dtype pair, the backward both forms and
    both fold levels with a short last group, the boundary both forms and K in {1, 2, 3, 8}."""
    seen = {}

    def add(ep, *key):
        seen.setdefault(ep, set()).add(key)
    for H, tx, ty, T, form in RMS_CASES:
        assert _h_ok(H)
        add("fwd", "it-pair", _bucket(H), tx, ty)
        add("fwd", "T", T)
        add("bwd", "it-pair-form", _bucket(H), tx, ty, form)
        add("bwd", "fold", _rms_fold(T))
    for H, tx, ty, T, K in RMS_BOUNDARY_CASES:
        ep = "boundary[combine]" if K else "boundary[dense]"
        add(ep, "it", _bucket(H))
        add(ep, "pair", tx, ty)
        add(ep, "K", K)
    assert {("it-pair", b, x, y) for b in IT_BUCKETS for x, y in PAIRS_2T} <= seen["fwd"]
    assert {("T", 1), ("T", 3)} <= seen["fwd"]
    assert {("it-pair-form", b, x, y, f) for b in IT_BUCKETS for x, y in PAIRS_2T for f in ("plain", "full")} <= seen["bwd"]
    assert {("fold", "one"), ("fold", "two")} <= seen["bwd"]
    for ep in ("boundary[dense]", "boundary[combine]"):
        assert {("it", b) for b in IT_BUCKETS} <= seen[ep], ep
        assert {("pair", a, b) for a, b in PAIRS_2T} <= seen[ep], ep
    assert {("K", k) for k in (1, 2, 3, 8)} <= seen["boundary[combine]"]
    for b in IT_BUCKETS:
        ws = [H for H in WIDTHS if _bucket(H) == b]
        lo = 4 if b == 1 else 256 * IT_BUCKETS[IT_BUCKETS.index(b) - 1] + 4
        assert min(ws) == lo and max(ws) >= 256 * b - 4, (b, ws)
    Ts = {c[3] for c in RMS_CASES}
    assert _rms_fold(8160) == "one" and _rms_fold(8161) == "two" and {65, 97, 300, 8160, 8161, 8225} <= Ts
    assert all(T % RMS_ROWS_PER_BLOCK for T in (65, 97, 300))
    nblk = -(-8225 // RMS_ROWS_PER_BLOCK)
    assert nblk % -(-nblk // RMS_FOLD_GROUPS) != 0, "8225 rows must leave the last fold group short"


# ---------------------------------------------------------------------------------------------------------------------------
# float64 references
def _rms64(x, g, eps):
    """(y, r) of the rows of x in float64."""
    r = torch.sqrt((x * x).mean(-1, keepdim=True))
    return g * x / (r + eps), r[..., 0]


def _rms_bwd64(x, g, eps, dy):
    """(dx, per-row dy * x / s) in float64; the second term of dx is 0 for a row with r == 0."""
    H = x.shape[-1]
    r = torch.sqrt((x * x).mean(-1, keepdim=True))
    s = r + eps
    gd = g * dy
    c = (gd * x).sum(-1, keepdim=True)
    second = torch.where(r > 0, x * c / (H * r.clamp_min(1e-300) * s * s), torch.zeros_like(x))
    return gd / s - second, dy * x / s


def _rms_run(lib, P, S, dev, x, g, eps, dy, dres, p, seed, tx, ty, T, H):
    """apertis_rmsnorm_fwd then _bwd into guarded NaN buffers: dict of outputs (device views) and the guard buffers."""
    X, G = x.to(tx).to(dev), g.float().to(dev)
    ybuf, y = _out((T, H), ty, dev)
    rbuf, rms = _out((T,), F32, dev)
    assert lib.apertis_rmsnorm_fwd(P(X), P(G), eps, P(y), P(rms), T, H, _code(tx), _code(ty), S()) == OK
    nblk = lib.apertis_rmsnorm_bwd_blocks(T, H)
    part = torch.full((nblk, H), NAN, device=dev)
    dxbuf, dx = _out((T, H), tx, dev)
    dgbuf, dg = _out((H,), F32, dev)
    bufs = [ybuf, rbuf, dxbuf, dgbuf]
    DY = dy.to(ty).to(dev)
    DR = dres.to(tx).to(dev) if dres is not None else None
    dblk = None
    if dres is not None:
        dkbuf, dblk = _out((T, H), ty, dev)
        bufs.append(dkbuf)
    assert lib.apertis_rmsnorm_bwd(P(X), P(G), P(rms), eps, P(DY), P(DR), P(dx), P(dblk), p, seed, P(part), P(dg), T, H,
                                   _code(tx), _code(ty), S()) == OK
    torch.cuda.synchronize()
    return dict(y=y, rms=rms, dx=dx, dg=dg, dblk=dblk, part=part, X=X, G=G, DY=DY, DR=DR), bufs


def _bwd_again(lib, P, S, o, eps, p, seed, tx, ty, T, H):
    """The backward once more on the same device inputs, into fresh buffers and a NaN workspace: (dx, dscale, dblk)."""
    dx2, dg2 = torch.empty_like(o["dx"]), torch.empty_like(o["dg"])
    dblk2 = torch.empty_like(o["dblk"]) if o["dblk"] is not None else None
    o["part"].fill_(NAN)
    assert lib.apertis_rmsnorm_bwd(P(o["X"]), P(o["G"]), P(o["rms"]), eps, P(o["DY"]), P(o["DR"]), P(dx2), P(dblk2), p, seed,
                                   P(o["part"]), P(dg2), T, H, _code(tx), _code(ty), S()) == OK
    torch.cuda.synchronize()
    return dx2, dg2, dblk2


# ---------------------------------------------------------------------------------------------------------------------------
# 1. forward and backward through the C ABI
@pytest.mark.parametrize("H,tx,ty,T,form", RMS_CASES, ids=[f"H{c[0]}-{_tag(c[1])}-{_tag(c[2])}-T{c[3]}-{c[4]}" for c in RMS_CASES])
def test_rmsnorm_fwd_bwd_against_fp64(dev, H, tx, ty, T, form):
    """apertis_rmsnorm_fwd (y, rms) and apertis_rmsnorm_bwd (dx, dscale; 'full': with the residual gradient dres folded in and
    dblk = the masked copy of dx at p = 0.1) against fp64 on the rounded inputs; the partial-row workspace starts NaN (a fold
    reading past its rows would show).  The backward is repeated and must give the same bits."""
    lib, P, S = _lib()
    gen = torch.Generator().manual_seed(H * 29 + T)
    x = _rnd(_rows(T, H, gen), tx)
    g = (torch.randn(H, generator=gen, dtype=torch.float64) * 0.5 + 1).float().double()
    dy = _rnd(torch.randn(T, H, generator=gen, dtype=torch.float64), ty)
    full = form == "full"
    dres = _rnd(torch.randn(T, H, generator=gen, dtype=torch.float64), tx) if full else None
    p, seed = (0.1, SEEDS[0]) if full else (0.0, 0)
    eps = 1e-12
    o, bufs = _rms_run(lib, P, S, dev, x, g, eps, dy, dres, p, seed, tx, ty, T, H)
    _guards_nan(*bufs)
    y_ref, r_ref = _rms64(x, g, eps)
    _close(o["y"], y_ref, "y", _rtol(ty))
    _close(o["rms"], r_ref, "rms", 1e-4)
    dx_ref, dgr = _rms_bwd64(x, g, eps, dy)
    if full:
        dx_ref = dx_ref + dres
    _close(o["dx"], dx_ref, "dx", _rtol(tx))
    _sum_close(o["dg"], dgr.sum(0), T, "dscale")
    if full:
        keep = _keep_rows(seed, T, H, p)
        ks = 1.0 / (1.0 - float(np.float32(p)))
        # dblk = mask * dx as stored (rounded to x's dtype) / (1 - p), rounded to the gradient dtype; the mask bit for bit
        _close(o["dblk"], keep.double() * o["dx"].cpu().double() * ks, "dblk", _rtol(ty), 1e-6)
        assert torch.equal((o["dblk"].cpu() != 0) | (o["dx"].cpu() == 0), keep | (o["dx"].cpu() == 0))
    dx2, dg2, dblk2 = _bwd_again(lib, P, S, o, eps, p, seed, tx, ty, T, H)
    assert torch.equal(o["dx"], dx2) and torch.equal(o["dg"], dg2), "the backward is not deterministic"
    assert not full or torch.equal(o["dblk"], dblk2)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("seed", SEEDS[:2], ids=["s0", "s1"])
def test_rmsnorm_masks_equal_the_mirror(dev, seed, p):
    """The mask of apertis_dropout_add_rmsnorm_fwd (linear index r * H + c) and the one apertis_rmsnorm_bwd regenerates for
    dblk: each the numpy mirror's bit for bit over 0.5 M elements, more than one block of rows.  blk = 1, res = 0 make y the
    scaled mask; dy = 0, dres = 1 make dx = 1 and dblk the scaled mask."""
    lib, P, S = _lib()
    T, H = 514, 1028
    keep = _keep_rows(seed, T, H, p)
    ones, zeros, g = torch.ones(T, H, device=dev), torch.zeros(T, H, device=dev), torch.ones(H, device=dev)
    y, xn, rms = torch.full((T, H), NAN, device=dev), torch.full((T, H), NAN, device=dev), torch.full((T,), NAN, device=dev)
    assert lib.apertis_dropout_add_rmsnorm_fwd(P(ones), None, None, 0, P(zeros), P(g), 1e-5, P(y), P(xn), P(rms), T, H, p, seed,
                                               _code(F32), _code(F32), S()) == OK
    torch.cuda.synchronize()
    got = (y != 0).cpu()
    assert torch.equal(got, keep), f"boundary forward: {int((got != keep).sum())} mask bits differ"
    part = torch.full((lib.apertis_rmsnorm_bwd_blocks(T, H), H), NAN, device=dev)
    dx, dblk, dg = torch.full((T, H), NAN, device=dev), torch.full((T, H), NAN, device=dev), torch.full((H,), NAN, device=dev)
    x, r1 = torch.randn(T, H, device=dev), torch.ones(T, device=dev)
    assert lib.apertis_rmsnorm_bwd(P(x), P(g), P(r1), 1e-5, P(zeros), P(ones), P(dx), P(dblk), p, seed, P(part), P(dg), T, H,
                                   _code(F32), _code(F32), S()) == OK
    torch.cuda.synchronize()
    assert torch.equal(dx, ones)
    got = (dblk != 0).cpu()
    assert torch.equal(got, keep), f"rmsnorm_bwd dblk: {int((got != keep).sum())} mask bits differ"
    _close(dblk, keep.double() / (1.0 - float(np.float32(p))), "dblk", 1e-6)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. edge rows
@pytest.mark.parametrize("eps", [1e-12, 1e-6])
@pytest.mark.parametrize("H,tx,ty", [(260, F32, F32), (1028, F32, BF16), (3076, BF16, F32)],
                         ids=["H260-f32-f32", "H1028-f32-bf16", "H3076-bf16-f32"])
def test_all_zero_row_among_ordinary_ones(dev, H, tx, ty, eps):
    """A row of zeros has r = 0 and s = eps: its y is exactly 0, its dx is finite and equal to scale * dy / eps (the second
    term of dx is 0 there, as torch's norm backward has it), and it adds nothing to dscale; the rows around it are ordinary."""
    lib, P, S = _lib()
    T, z = 7, 3
    gen = torch.Generator().manual_seed(H + 5)
    x = _rnd(_rows(T, H, gen), tx)
    x[z] = 0.0
    g = (torch.randn(H, generator=gen, dtype=torch.float64) * 0.5 + 1).float().double()
    dy = _rnd(torch.randn(T, H, generator=gen, dtype=torch.float64), ty)
    o, bufs = _rms_run(lib, P, S, dev, x, g, eps, dy, None, 0.0, 0, tx, ty, T, H)
    _guards_nan(*bufs)
    assert float(o["rms"][z]) == 0.0 and torch.equal(o["y"][z].float().cpu(), torch.zeros(H)), "y of the zero row is not exactly 0"
    assert torch.isfinite(o["dx"].float()).all() and torch.isfinite(o["y"].float()).all() and torch.isfinite(o["dg"]).all()
    eps32 = float(np.float32(eps))                 # (the ABI takes eps as a float)
    _close(o["dx"][z], g * dy[z] / eps32, "dx of the zero row", _rtol(tx))
    keep = [i for i in range(T) if i != z]
    y_ref, r_ref = _rms64(x, g, eps32)
    dx_ref, dgr = _rms_bwd64(x, g, eps32, dy)
    _close(o["y"][keep], y_ref[keep], "y", _rtol(ty))
    _close(o["dx"][keep], dx_ref[keep], "dx", _rtol(tx))
    _sum_close(o["dg"], dgr.sum(0), T, "dscale")


@pytest.mark.parametrize("H", [260, 1028, 4096])
def test_rows_of_equal_values(dev, H):
    """Rows whose elements are all equal (0.3 k / 7, negative ones among them): r = |x|, y = scale * sign(x) to rounding."""
    lib, P, S = _lib()
    T = 9
    gen = torch.Generator().manual_seed(H + 11)
    v = 0.3 * torch.arange(1, T + 1, dtype=torch.float64) / 7 * torch.tensor([1, -1, 1] * 3, dtype=torch.float64)
    x = v[:, None].expand(T, H).float().double()
    g = (torch.randn(H, generator=gen, dtype=torch.float64) * 0.5 + 1).float().double()
    dy = torch.randn(T, H, generator=gen, dtype=torch.float64).float().double()
    o, bufs = _rms_run(lib, P, S, dev, x, g, 1e-12, dy, None, 0.0, 0, F32, F32, T, H)
    _guards_nan(*bufs)
    y_ref, r_ref = _rms64(x, g, 1e-12)
    _close(o["y"], y_ref, "y", 1e-4)
    _close(o["rms"], r_ref, "rms", 1e-4)
    dx_ref, dgr = _rms_bwd64(x, g, 1e-12, dy)
    _close(o["dx"], dx_ref, "dx", 1e-4)
    _sum_close(o["dg"], dgr.sum(0), T, "dscale")


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the block boundary forward
@pytest.mark.parametrize("H,tx,ty,T,K", RMS_BOUNDARY_CASES,
                         ids=[f"H{c[0]}-{_tag(c[1])}-{_tag(c[2])}-T{c[3]}-K{c[4]}" for c in RMS_BOUNDARY_CASES])
def test_boundary_fwd_against_fp64(dev, H, tx, ty, T, K):
    """apertis_dropout_add_rmsnorm_fwd: y = res + dropout(blk) (dense blk [T, H], or with slot_of / wk the combine
    sum_k wk * blk[slot] of dyadic expert rows - exact - dropped slots skipped, rounded to the block dtype) at p 0.1 with the
    mirror's mask, against fp64; xn and rms against the fp64 RMSNorm of the stored y."""
    lib, P, S = _lib()
    gen = torch.Generator().manual_seed(H * 7 + T * 3 + K + 1)
    p, seed, eps = 0.1, SEEDS[1], 1e-6
    res = _rnd(_rows(T, H, gen), tx)
    g = (torch.randn(H, generator=gen, dtype=torch.float64) * 0.5 + 1).float().double()
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
    rbuf, rms = _out((T,), F32, dev)
    assert lib.apertis_dropout_add_rmsnorm_fwd(P(blk.to(ty).to(dev)), P(SL), P(WK), K, P(res.to(tx).to(dev)), P(g.float().to(dev)),
                                               eps, P(y), P(xn), P(rms), T, H, p, seed, _code(tx), _code(ty), S()) == OK
    torch.cuda.synchronize()
    _guards_nan(ybuf, xbuf, rbuf)
    y_ref = res + keep.double() * a * ks
    _close(y, y_ref, "y", _rtol(tx))
    if tx == F32:       # where the block output is not zero the mask shows in the fp32 y bit for bit
        nz = a.abs() > 1e-4
        assert torch.equal(((y.cpu().double() != res) & nz), keep & nz)
    xn_ref, r_ref = _rms64(y.cpu().double(), g, eps)
    _close(xn, xn_ref, "xn", _rtol(ty))
    _close(rms, r_ref, "rms", 1e-4)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the ops: autograd wiring of rms_norm / rms_norm_pass / dropout_add_rms_norm against fp64 autograd
def _rms_t(x, g, eps):
    return g * (x / (torch.sqrt((x * x).mean(-1, keepdim=True)) + eps))


@pytest.mark.parametrize("cd", [F32, BF16], ids=["f32", "bf16"])
def test_ops_rms_norm_and_pass_autograd(dev, cd):
    """ops.rms_norm and ops.rms_norm_pass on a [2, 5, 260] fp32 stream: the pass-through's gradient is added inside the backward
    kernel, so d(sum(w1 * RMSNorm(x)) + sum(w2 * x)) / dx matches fp64 autograd, and so does dscale."""
    from apertis_llm_amd import ops
    gen = torch.Generator().manual_seed(3)
    B, L, H, eps = 2, 5, 260, 1e-6
    x64 = torch.randn(B, L, H, generator=gen, dtype=torch.float64).float().double().requires_grad_(True)
    g64 = (torch.randn(H, generator=gen, dtype=torch.float64) * 0.5 + 1).float().double().requires_grad_(True)
    w1 = _rnd(torch.randn(B, L, H, generator=gen, dtype=torch.float64), cd)
    w2 = torch.randn(B, L, H, generator=gen, dtype=torch.float64).float().double()
    (_rms_t(x64, g64, eps) * w1).sum().add((x64 * w2).sum()).backward()
    x = x64.detach().float().to(dev).requires_grad_(True)
    g = g64.detach().float().to(dev).requires_grad_(True)
    y, xp = ops.rms_norm_pass(x, g, eps, out_dtype=cd)
    assert y.dtype == cd and xp.dtype == F32 and y.shape == x.shape
    _close(y, _rms_t(x64, g64, eps).detach(), "y", _rtol(cd))
    ((y.float() * w1.float().to(dev)).sum() + (xp * w2.float().to(dev)).sum()).backward()
    _close(x.grad, x64.grad, "dx", 1e-4 if cd == F32 else 8e-3)
    _sum_close(g.grad, g64.grad, B * L, "dscale", scale=1.0 if cd == F32 else 4.0)
    x2 = x.detach().clone().requires_grad_(True)
    y2 = ops.rms_norm(x2, g.detach(), eps, out_dtype=cd)
    assert torch.equal(y2, y)
    (y2.float() * w1.float().to(dev)).sum().backward()
    xr = x64.detach().clone().requires_grad_(True)
    (_rms_t(xr, g64.detach(), eps) * w1).sum().backward()
    _close(x2.grad, xr.grad, "dx (plain)", 1e-4 if cd == F32 else 8e-3)


@pytest.mark.parametrize("form", ["dense", "combine", "xn-unused"])
def test_ops_dropout_add_rms_norm_autograd(dev, form):
    """ops.dropout_add_rms_norm at p = 0 in fp32 against fp64 autograd of res + blk followed by RMSNorm: the gradients of blk
    (through apertis_moe_combine_bwd in the combine form: of the expert rows and the weights), res and scale; with the
    normalised output unused only the residual path carries gradient (the apertis_dropout_bwd branch)."""
    from apertis_llm_amd import ops
    gen = torch.Generator().manual_seed(17)
    T, H, E, K, eps = 24, 132, 4, 2, 1e-6
    res64 = torch.randn(T, H, generator=gen, dtype=torch.float64).float().double().requires_grad_(True)
    g64 = (torch.randn(H, generator=gen, dtype=torch.float64) * 0.5 + 1).float().double().requires_grad_(True)
    w1 = torch.randn(T, H, generator=gen, dtype=torch.float64).float().double()
    w2 = torch.randn(T, H, generator=gen, dtype=torch.float64).float().double()
    res = res64.detach().float().to(dev).requires_grad_(True)
    g = g64.detach().float().to(dev).requires_grad_(True)
    if form == "combine":
        idx = torch.stack([torch.randperm(E, generator=gen)[:K] for _ in range(T)]).to(torch.int32)
        wk64 = torch.rand(T, K, generator=gen, dtype=torch.float64).float().double().requires_grad_(True)
        plan = ops.moe_plan(idx.to(dev), wk64.detach().float().to(dev), E, None, None)
        rows = int(plan.offsets[-1])
        yr64 = torch.randn(rows, H, generator=gen, dtype=torch.float64).float().double().requires_grad_(True)
        slot = plan.slot_of.cpu().long()
        blk64 = sum(wk64[:, k, None] * yr64[slot[:, k]] for k in range(K))
        yr = torch.zeros(plan.max_rows, H, device=dev)
        yr[:rows] = yr64.detach().float().to(dev)
        yr.requires_grad_(True)
        wk = wk64.detach().float().to(dev).requires_grad_(True)
        y, xn = ops.dropout_add_rms_norm(yr, res, g, eps, 0.0, True, combine=(wk, plan))
    else:
        blk64 = torch.randn(T, H, generator=gen, dtype=torch.float64).float().double().requires_grad_(True)
        blk = blk64.detach().float().to(dev).requires_grad_(True)
        y, xn = ops.dropout_add_rms_norm(blk, res, g, eps, 0.0, True)
    y64 = res64 + blk64
    xn64 = _rms_t(y64, g64, eps)
    _close(y, y64.detach(), "y", 1e-4)
    _close(xn, xn64.detach(), "xn", 1e-4)
    if form == "xn-unused":
        (y64 * w2).sum().backward()
        (y * w2.float().to(dev)).sum().backward()
        assert g.grad is None or not g.grad.any()
    else:
        ((xn64 * w1).sum() + (y64 * w2).sum()).backward()
        ((xn * w1.float().to(dev)).sum() + (y * w2.float().to(dev)).sum()).backward()
        _sum_close(g.grad, g64.grad, T, "dscale")
    _close(res.grad, res64.grad, "dres", 1e-4)
    if form == "combine":
        _close(yr.grad[:rows], yr64.grad, "dyr", 1e-4)
        _close(wk.grad, wk64.grad, "dwk", 1e-4, 1e-4)       # (a dot product over H: the floor grows with its length)
    else:
        _close(blk.grad, blk64.grad, "dblk", 1e-4)


def test_switch_off_means_the_stock_module(dev, monkeypatch):
    """ops.RMSNORM_FUSED = False: model.RMSNorm computes with stock torch (no kernel entry point is reached) and agrees with the
    kernel path to rounding."""
    from apertis_llm_amd import model as M, ops
    norm = M.RMSNorm(260, eps=1e-6).to(dev)
    x = torch.randn(3, 260, device=dev)
    y_on = norm(x)
    calls = []
    monkeypatch.setattr(ops.norm._RMSNorm, "forward", staticmethod(lambda *a: calls.append(a)))
    monkeypatch.setattr(ops, "RMSNORM_FUSED", False)
    y_off = norm(x)
    assert not calls and ops.norm.RMSNORM_FUSED is False
    _close(y_on, y_off.double(), "y", 1e-5)
