"""apertis_swiglu_fwd / apertis_swiglu_bwd through the C ABI against fp64 on the CPU, the reference formed from the values the
kernel actually reads (bf16 inputs upcast).  With s = sigmoid(g):  h = g s u,  dg = dh u s (1 + g (1 - s)),  du = dh g s.

Shapes: rows {1, 3, 65, 1000} x F {8, 256, 264, 1024} (264: a row whose vector count is no multiple of the wave), one shape
past one pass of the capped grid (GRID_CAP blocks of 256 lanes, a 16-byte vector per lane and pass), both dtypes, and one bf16
case each way whose gu is past 2^32 bytes.  g is drawn over +-12 (both sigmoid tails) with 0 and +-88 planted, where fp32 exp
overflows / underflows: the results must be finite and right.

Bounds, derived (REL = 2^-8 bf16 / 2^-20 fp32, ABS = 2^-16 bf16 / 2^-22 fp32):
  forward   |err| <= REL |ref| + ABS |u| (1 + |g|)     REL is the format's unit roundoff: one rounding of the fp32 result to 8
                                                       (bf16) significant bits, or a few fp32 ulps with headroom; the second
                                                       term covers exp / reciprocal (a few fp32 ulps, 4x headroom; in bf16 the
                                                       fast exp2 / rcp and the rounding of g log2(e))
  dg        |err| <= REL |ref| + ABS |dh u| (1 + |g|)  silu' crosses zero near g = -1.278: no purely relative bound there
  du        |err| <= REL |ref| + ABS |dh| (1 + |g|)    (du is the forward with dh in the place of u)
  h_out     the forward's bound, and in bf16 the bits of apertis_swiglu_fwd on the same gu."""
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
GRID_CAP = 2048                 # SWIGLU_MAX_BLOCKS of csrc/swiglu.hip: one pass covers GRID_CAP * 256 vectors of 16 bytes
DT = {F32: torch.float32, BF16: torch.bfloat16}
REL = {F32: 2.0 ** -20, BF16: 2.0 ** -8}
ABS = {F32: 2.0 ** -22, BF16: 2.0 ** -16}


def _lib():
    from apertis_llm_amd import _lib
    return _lib.load()


def _call(fn, name, *args):
    from apertis_llm_amd._lib import check, stream_ptr
    check(fn(*args, stream_ptr()), name)


def _fwd(gu, F, code):
    from apertis_llm_amd._lib import ptr
    rows = gu.shape[0]
    h = torch.full((rows, F), float("nan"), device=gu.device, dtype=gu.dtype)
    _call(_lib().apertis_swiglu_fwd, "apertis_swiglu_fwd", ptr(gu), ptr(h), rows, F, code)
    return h


def _bwd(dh, gu, F, code, with_h=True):
    from apertis_llm_amd._lib import ptr
    rows = gu.shape[0]
    dgu = torch.full_like(gu, float("nan"))
    h = torch.full_like(dh, float("nan")) if with_h else None
    _call(_lib().apertis_swiglu_bwd, "apertis_swiglu_bwd", ptr(dh), ptr(gu), ptr(dgu), ptr(h), rows, F, code)
    return dgu, h


def _reference(gu, dh, F):
    """fp64 on the CPU from the stored values: (h, dg, du, g, u, dh)."""
    gu64 = gu.detach().cpu().double()
    g, u = gu64[:, :F], gu64[:, F:]
    s = torch.sigmoid(g)
    d = None if dh is None else dh.detach().cpu().double()
    h = g * s * u
    if d is None:
        return h, None, None, g, u, None
    return h, d * u * s * (1 + g * (1 - s)), d * g * s, g, u, d


def _hold(name, got, ref, scale, code):
    got = got.detach().cpu().double()
    assert torch.isfinite(got).all(), f"{name}: not finite"
    err, bound = (got - ref).abs(), REL[code] * ref.abs() + ABS[code] * scale
    worst = float((err / (bound + 1e-300)).max())
    print(f"SWIGLU {name}: worst err / bound {worst:.3f}, max abs err {float(err.max()):.3e}")
    assert bool((err <= bound).all()), (name, worst, float(err.max()))


def _inputs(rows, F, code, dev, seed):
    gen = torch.Generator().manual_seed(seed)
    g = torch.rand(rows, F, generator=gen) * 24 - 12
    u = torch.randn(rows, F, generator=gen) * 2
    dh = torch.randn(rows, F, generator=gen)
    # the points where fp32 exp(-g) overflows (g = -88: e^88 = 1.65e38, its reciprocal a denormal) or underflows (g = +88), and 0
    for i, v in enumerate((0.0, 88.0, -88.0, -1.278)):
        g[i % rows, (i * 3) % F] = v
        u[i % rows, (i * 3) % F] = 1.5
    gu = torch.cat([g, u], dim=1).to(DT[code]).to(dev).contiguous()
    return gu, dh.to(DT[code]).to(dev).contiguous()


def _check_case(rows, F, code, dev, seed, h_optional=False):
    gu, dh = _inputs(rows, F, code, dev, seed)
    h_ref, dg_ref, du_ref, g, u, d = _reference(gu, dh, F)
    tag = f"rows={rows} F={F} {'bf16' if code == BF16 else 'fp32'}"
    fscale = u.abs() * (1 + g.abs())
    h = _fwd(gu, F, code)
    _hold(tag + " h", h, h_ref, fscale, code)
    dgu, h2 = _bwd(dh, gu, F, code)
    _hold(tag + " dg", dgu[:, :F], dg_ref, (d * u).abs() * (1 + g.abs()), code)
    _hold(tag + " du", dgu[:, F:], du_ref, d.abs() * (1 + g.abs()), code)
    _hold(tag + " h_out", h2, h_ref, fscale, code)
    if code == BF16:
        assert torch.equal(h2, h), tag + ": h_out is not the forward's h bit for bit"
    if h_optional:
        dgu0, none = _bwd(dh, gu, F, code, with_h=False)
        assert none is None and torch.equal(dgu0, dgu), tag + ": dgu differs without h_out"


@pytest.mark.parametrize("code", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("F", [8, 256, 264, 1024])
@pytest.mark.parametrize("rows", [1, 3, 65, 1000])
def test_kernels_against_fp64(dev, rows, F, code):
    _check_case(rows, F, code, dev, seed=rows * 4099 + F, h_optional=(rows == 65))


@pytest.mark.parametrize("code", [F32, BF16], ids=["fp32", "bf16"])
def test_more_vectors_than_one_pass_of_the_capped_grid(dev, code):
    """1100 x 4096: 563 200 (bf16) / 1 126 400 (fp32) vectors against GRID_CAP * 256 = 524 288 per pass: some lanes take a second
    (fp32: a third) vector.  A pass is a whole number of rows here (512 / 1024 vectors each); the next test takes one that is not."""
    rows, F = 1100, 4096
    assert rows * F // (8 if code == BF16 else 4) > GRID_CAP * 256
    _check_case(rows, F, code, dev, seed=7)


def test_stride_that_is_no_multiple_of_the_row(dev):
    """2100 x 2056 bf16: 257 vectors per row, so a pass of GRID_CAP * 256 lanes ends mid-row and the (row, vector) carry of the
    grid-stride walk wraps on most steps."""
    rows, F = 2100, 2056
    assert rows * (F // 8) > GRID_CAP * 256 and (GRID_CAP * 256) % (F // 8) != 0
    _check_case(rows, F, BF16, dev, seed=9)


BIG_ROWS, BIG_F = 262400, 4096


def _big_rows():
    """The rows checked of the 2^32-byte cases: the first 64, the last 64 and the 64 around the row where gu's byte offset
    passes 2^32 (row 2^32 / (2 F * 2) = 262 144)."""
    cross = (1 << 32) // (2 * BIG_F * 2)
    assert BIG_ROWS * 2 * BIG_F * 2 > 1 << 32 and 32 <= cross and cross + 32 <= BIG_ROWS - 64
    return torch.cat([torch.arange(0, 64), torch.arange(cross - 32, cross + 32), torch.arange(BIG_ROWS - 64, BIG_ROWS)])


def _big_gu(dev):
    gu = torch.empty(BIG_ROWS, 2 * BIG_F, device=dev, dtype=torch.bfloat16)
    gu.uniform_(-12.0, 12.0, generator=torch.Generator(device=dev).manual_seed(21))      # filled on the device
    return gu


def test_forward_past_4_gib_of_gu(dev):
    rows = _big_rows()
    gu = _big_gu(dev)
    h = _fwd(gu, BIG_F, BF16)
    sub, hs = gu[rows.to(dev)], h[rows.to(dev)]
    del gu, h
    torch.cuda.empty_cache()
    h_ref, _, _, g, u, _ = _reference(sub, None, BIG_F)
    _hold("4 GiB forward h", hs, h_ref, u.abs() * (1 + g.abs()), BF16)


def test_backward_past_4_gib_of_gu(dev):
    rows = _big_rows()
    gu = _big_gu(dev)
    dh = torch.empty(BIG_ROWS, BIG_F, device=dev, dtype=torch.bfloat16)
    dh.uniform_(-2.0, 2.0, generator=torch.Generator(device=dev).manual_seed(22))
    dgu, h = _bwd(dh, gu, BIG_F, BF16)
    idx = rows.to(dev)
    sub, ds, dgs, hs = gu[idx], dh[idx], dgu[idx], h[idx]
    del gu, dh, dgu, h
    torch.cuda.empty_cache()
    h_ref, dg_ref, du_ref, g, u, d = _reference(sub, ds, BIG_F)
    _hold("4 GiB backward dg", dgs[:, :BIG_F], dg_ref, (d * u).abs() * (1 + g.abs()), BF16)
    _hold("4 GiB backward du", dgs[:, BIG_F:], du_ref, d.abs() * (1 + g.abs()), BF16)
    _hold("4 GiB backward h_out", hs, h_ref, u.abs() * (1 + g.abs()), BF16)
