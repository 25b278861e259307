"""The SSM block's depthwise causal conv + SiLU (apertis_dwconv_silu_fwd / _bwd / _bwd2) and its stand-alone post-scan gate
(apertis_ssm_gate_fwd / _bwd, csrc/ssm_elementwise.hip) against float64 references on the same rounded inputs, at every
dispatch path of the entry points: the conv forward's LDS tile and run-per-thread kernels on both sides of the tile's LDS
bound, the widths 2..16, the backward's multi-pass chunk loop (CPR > 256) and its 4096-block grid cap; the gate's three dtype
pairs, its multi-pass dD reduction and T = 0.  Then whole models at conv widths 2, 3, 5 and 8 and at Dn = 768 against the CPU
oracle, and their single-token decode steps against the general path.

References (float64, CPU):
  conv  F.conv1d(x^T, w, b, padding=k-1, groups=Dn)[..., :L] -> (bf16: the pre-activation rounded to bf16, as the kernel
        stores it) -> SiLU; gradients by fp64 autograd (the rounding passed straight through, as the kernel's backward does).
  gate  (y + D*xc) * silu(z); gradients by fp64 autograd.
Tolerances: fp32 outputs rtol 1e-4 with an absolute floor of 1e-5 of the tensor's largest entry (the project's bar); bf16
outputs one bf16 rounding (rtol 8e-3); dw, db and dD - fp32 sums over B*L tokens - an absolute bound growing with sqrt(B*L),
as test_grouped_gemm_tn_bf16's.  The bf16 conv inputs sit on a dyadic grid (x = n/32, |n| <= 255; w = m/64; b = j/2048), where
every tap product and partial sum is exact in fp32: the kernel's pre-activation is then the reference's to the bit and both
round it to the same bf16 value, so the one-rounding bound holds elementwise (a pre-activation a bf16 tie apart would move
silu by several bf16 ulps where it is steep)."""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_error_report

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
ERR_UNSUPPORTED = -2

# ---------------------------------------------------------------------------------------------------------------------------
# mirror of the dispatch in csrc/ssm_elementwise.hip (make_geo, conv_blocks, gate_blocks, conv_tile_ok): a change there must
# be made here too, and then test_case_tables_cover_every_dispatch_path says whether the cases below still reach every path
CONV_TT, CONV_TILE_T, CONV_KMAX = 16, 64, 16
TILE_LDS_MAX = 160 * 1024            # one work-group's LDS (the CU's 160 KiB)
CONV_BLOCK_CAP, GATE_BLOCK_CAP = 4096, 2048


def _geo(Dn):
    """(CPR, RP): 4-channel chunks per row, rows per 256-thread block (make_geo)."""
    cpr = Dn // 4
    return cpr, (1 if cpr >= 256 else 256 // cpr)


def _conv_blocks(B, L, Dn):
    runs = B * -(-L // CONV_TT)
    return max(1, min(-(-runs // _geo(Dn)[1]), CONV_BLOCK_CAP))


def _gate_blocks(T, Dn):
    return max(1, min(-(-T // (_geo(Dn)[1] * 8)), GATE_BLOCK_CAP))


def _tile_lds(Dn, k, dt):
    return (CONV_TILE_T + k - 1) * (Dn // (16 // _esize(dt))) * 16


def _esize(dt):
    return 2 if dt == BF16 else 4


def _conv_fwd_path(dt, Dn, k, ptrs, strides):
    """'tile' (LDS tile, k = 2..4), 'thread' (templated run per thread, k = 2..4) or 'kn' (runtime width, k = 5..16): the
    kernel apertis_dwconv_silu_fwd launches for these rows (conv_tile_ok)."""
    es, epc = _esize(dt), 16 // _esize(dt)
    tile = (Dn % epc == 0 and Dn // epc <= 256 and 2 <= k <= 4 and _tile_lds(Dn, k, dt) <= TILE_LDS_MAX
            and all(p % 16 == 0 for p in ptrs) and all((s * es) % 16 == 0 for s in strides))
    return "tile" if tile else ("thread" if k <= 4 else "kn")


# ---------------------------------------------------------------------------------------------------------------------------
# conv cases: (id, dtype, k, B, L, Dn, layout, forward path).  L counts the conv's input rows (the window form: L new tokens
# after k - 1 cached ones).  Layouts:
#   dense     x [B, L, Dn]
#   xz        x = xz[..., :Dn] of a [B, L, 2 Dn] buffer whose z half is NaN (the model's form: row stride 2 Dn)
#   window    x = cat(window [B, k-1, Dn], xp [B, L, Dn]): the prefill-with-cache form, the first L outputs kept
#   rs_pad    x at row stride Dn + 4 (bf16: 8-byte rows, not whole 16-byte pieces)
#   base_off  x at a base 8 bytes past a 16-byte boundary (bf16, row stride Dn + 8)
CONV_CASES = [
    # tile forward: PCS dividing 256 and not (176 bf16: PCS 22, RG 11; 176 fp32: PCS 44), above 48 KiB of LDS, at the bound
    ("f32-k2-pcs16", F32, 2, 3, 130, 64, "dense", "tile"),
    ("f32-k3-pcs16-xz", F32, 3, 3, 65, 64, "xz", "tile"),
    ("f32-k4-pcs44-xz", F32, 4, 4, 64, 176, "xz", "tile"),
    ("f32-k4-window-L1", F32, 4, 3, 1, 64, "window", "tile"),
    ("f32-k4-lds67k", F32, 4, 3, 130, 256, "xz", "tile"),
    ("bf16-k2-pcs8", BF16, 2, 3, 63, 64, "dense", "tile"),
    ("bf16-k3-pcs22-xz", BF16, 3, 3, 130, 176, "xz", "tile"),
    ("bf16-k4-pcs22-xz", BF16, 4, 3, 65, 176, "xz", "tile"),                # the bench's Dn, dtype and width
    ("bf16-k4-window", BF16, 4, 3, 20, 176, "window", "tile"),
    # the tile's LDS bound (64 + k - 1) * PCS * 16 <= 160 KiB: the last PCS inside it and one piece past it
    ("f32-k2-lds-at", F32, 2, 3, 63, 628, "dense", "tile"),                  # PCS 157: 163 280 B
    ("f32-k2-lds-past", F32, 2, 3, 63, 632, "dense", "thread"),              # PCS 158
    ("bf16-k3-lds-at", BF16, 3, 3, 130, 1240, "xz", "tile"),                 # PCS 155: 163 680 B
    ("bf16-k3-lds-past", BF16, 3, 3, 130, 1248, "xz", "thread"),             # PCS 156
    ("f32-k4-lds-at", F32, 4, 3, 65, 608, "xz", "tile"),                     # PCS 152: 162 944 B
    ("f32-k4-lds-past", F32, 4, 3, 65, 612, "xz", "thread"),                 # PCS 153 (12 heads x 51)
    ("bf16-k4-lds-at", BF16, 4, 3, 64, 1216, "dense", "tile"),
    ("bf16-k4-lds-past", BF16, 4, 3, 64, 1224, "dense", "thread"),
    # run per thread: Dn % (16 B / element) != 0, PCS > 256 (CPR > 256: the backward's multi-pass chunk loop), unaligned rows
    ("bf16-k2-dn12", BF16, 2, 3, 65, 12, "dense", "thread"),
    ("bf16-k4-dn36-L2", BF16, 4, 3, 2, 36, "dense", "thread"),
    ("f32-k4-dn1032-xz", F32, 4, 3, 130, 1032, "xz", "thread"),
    ("f32-k3-dn1032", F32, 3, 3, 63, 1032, "dense", "thread"),
    ("bf16-k4-rs-pad", BF16, 4, 3, 65, 176, "rs_pad", "thread"),
    ("bf16-k3-base-off", BF16, 3, 3, 64, 176, "base_off", "thread"),
    # widths 5..16 (runtime-width kernels)
    ("f32-k5-xz", F32, 5, 3, 130, 64, "xz", "kn"),
    ("bf16-k5-xz", BF16, 5, 3, 65, 176, "xz", "kn"),
    ("bf16-k5-dn36", BF16, 5, 3, 64, 36, "dense", "kn"),
    ("f32-k8-L6", F32, 8, 3, 6, 176, "dense", "kn"),
    ("f32-k8-L1", F32, 8, 4, 1, 12, "dense", "kn"),
    ("bf16-k8-window", BF16, 8, 3, 130, 64, "window", "kn"),
    ("f32-k16-L14", F32, 16, 3, 14, 64, "dense", "kn"),
    ("f32-k16-window-L1", F32, 16, 3, 1, 64, "window", "kn"),
    ("bf16-k16-xz", BF16, 16, 3, 63, 176, "xz", "kn"),
    ("bf16-k16-dn1032", BF16, 16, 3, 65, 1032, "dense", "kn"),
    ("f32-k16-dn1032-rs-pad", F32, 16, 3, 64, 1032, "rs_pad", "kn"),
    # the backward's grid at its 4096-block cap (CPR 129, RP 1: 4 500 runs of 16 tokens), so blocks walk several runs
    ("bf16-k4-cap", BF16, 4, 3, 24000, 516, "dense", "thread"),
    ("f32-k4-cap", F32, 4, 3, 24000, 516, "dense", "tile"),                  # tile forward at 138 288 B of LDS
    ("f32-k5-cap", F32, 5, 3, 24000, 516, "xz", "kn"),
]

GATE_PAIRS = [(F32, F32), (F32, BF16), (BF16, BF16)]
GATE_DN = [4, 12, 176, 1028, 4100]
GATE_T = [0, 1, 7, "big"]


def _gate_T(T, Dn):
    """'big': 100 000 rows up to Dn 176 (the grid at its 2048-block cap); 2 500 at Dn 1028 / 4100 (hundreds of blocks)."""
    return T if T != "big" else (100_000 if Dn <= 176 else 2_500)


def _case_ptr_layout(layout, Dn, dt):
    """(byte offset of x's base from a 16-byte boundary, x's row stride) of a layout (the output rows: offset 0, stride
    2 Dn for 'xz' and Dn otherwise)."""
    es = _esize(dt)
    return {"dense": (0, Dn), "xz": (0, 2 * Dn), "window": (0, Dn), "rs_pad": (0, Dn + 4), "base_off": (4 * es, Dn + 8)}[layout]


def test_case_tables_cover_every_dispatch_path():
    """The coverage the cases below are for, from the mirror of the dispatch: both conv forward paths at every width 2..4 and
    both dtypes, both sides of the tile's LDS bound at every tile width (and the tile above 48 KiB, where the launch raises
    the work-group's LDS limit), the runtime-width kernels at 5, 8 and 16 in both dtypes, the backward's multi-pass chunk
    loop (CPR > 256) and its 4096-block cap; for the gate: the three dtype pairs, CPR > 256 and the 2048-block cap."""
    seen = set()
    for _, dt, k, B, L, Dn, layout, path in CONV_CASES:
        off, rs = _case_ptr_layout(layout, Dn, dt)
        out_rs = 2 * Dn if layout == "xz" else Dn
        got = _conv_fwd_path(dt, Dn, k, [off, 0], [rs, out_rs])
        assert got == path, (k, Dn, layout, got, path)
        seen.add(("fwd", path, k, dt))
        if k <= 4:
            lds = _tile_lds(Dn, k, dt)
            seen.add(("lds", k, "inside" if lds <= TILE_LDS_MAX else "past", path))
            if path == "tile" and lds > 48 * 1024:
                seen.add(("tile>48K",))
        cpr, rp = _geo(Dn)
        if cpr > 256:
            seen.add(("bwd cpr>256", "kn" if k > 4 else "templated"))
        if -(-B * -(-L // CONV_TT) // rp) > CONV_BLOCK_CAP:
            seen.add(("bwd cap", path))
    for k in (2, 3, 4):
        for dt in (F32, BF16):
            assert ("fwd", "tile", k, dt) in seen and ("fwd", "thread", k, dt) in seen, (k, dt)
        assert ("lds", k, "inside", "tile") in seen and ("lds", k, "past", "thread") in seen, k
    for k in (5, 8, 16):
        for dt in (F32, BF16):
            assert ("fwd", "kn", k, dt) in seen, (k, dt)
    assert ("tile>48K",) in seen
    assert ("bwd cpr>256", "templated") in seen and ("bwd cpr>256", "kn") in seen
    assert {("bwd cap", p) for p in ("tile", "thread", "kn")} <= seen
    assert any(_geo(Dn)[0] > 256 for Dn in GATE_DN)
    assert any(-(-_gate_T("big", Dn) // (_geo(Dn)[1] * 8)) > GATE_BLOCK_CAP for Dn in GATE_DN)
    assert any(1 < _gate_blocks(_gate_T("big", Dn), Dn) < GATE_BLOCK_CAP and _geo(Dn)[0] > 256 for Dn in GATE_DN)


# ---------------------------------------------------------------------------------------------------------------------------
def _close(got, ref, name, rtol, atol_scale=1e-5):
    ref = torch.as_tensor(ref).detach().cpu().to(torch.float64)
    got = got.detach().cpu().to(torch.float64)
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), f"{name}: {int((~torch.isfinite(got)).sum())} non-finite values"
    atol = atol_scale * float(ref.abs().max()) + 1e-30
    bad = (got - ref).abs() > atol + rtol * ref.abs()
    assert not bad.any(), f"{name}: {int(bad.sum())} / {bad.numel()} outside rtol {rtol}; max abs diff " \
                          f"{float((got - ref).abs().max()):.3e} (ref max {float(ref.abs().max()):.3e})"


def _rtol(dt):
    return 1e-4 if dt == F32 else 8e-3


def _sum_close(got, ref, n, name):
    """An fp32 sum over n terms of order one (parameter gradients): |err| <= 1.6e-4 sqrt(n), as test_grouped_gemm_tn_bf16."""
    ref = torch.as_tensor(ref).detach().cpu().to(torch.float64)
    got = got.detach().cpu().to(torch.float64)
    assert torch.isfinite(got).all(), name
    err, tol = float((got - ref).abs().max()), 2e-5 * 8 * max(1.0, math.sqrt(n))
    assert err <= tol, f"{name}: max abs err {err:.3e} > {tol:.3e} (ref max {float(ref.abs().max()):.3e})"


def _conv_inputs(dt, k, B, L, Dn, seed):
    """x [B, L, Dn] in dt, w [Dn, 1, k], b [Dn] fp32, two output gradients in dt (CPU).  bf16: the dyadic grid (module doc)."""
    g = torch.Generator().manual_seed(seed)
    if dt == BF16:
        x = (torch.randn(B, L, Dn, generator=g) * 32).round().clamp(-255, 255) / 32
        w = (torch.randn(Dn, 1, k, generator=g) * 0.3 * 64).round().clamp(-63, 63) / 64
        b = (torch.randn(Dn, generator=g) * 0.1 * 2048).round() / 2048
    else:
        x = torch.randn(B, L, Dn, generator=g)
        w = torch.randn(Dn, 1, k, generator=g) * 0.3
        b = torch.randn(Dn, generator=g) * 0.1
    g1, g2 = torch.randn(B, L, Dn, generator=g).to(dt), torch.randn(B, L, Dn, generator=g).to(dt)
    return x.to(dt), w, b, g1, g2


def _conv_ref(x, w, b, gout, dt):
    """float64 (y, dx, dw, db) of silu(conv) for output gradient gout; bf16: the pre-activation rounded to bf16 before SiLU
    (the rounding passed straight through by the gradient, as the kernel's backward does)."""
    x64 = x.double().requires_grad_(True)
    w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    L, Dn, k = x.shape[1], x.shape[2], w.shape[-1]
    pre = F.conv1d(x64.transpose(1, 2), w64, b64, padding=k - 1, groups=Dn)[..., :L].transpose(1, 2)
    if dt == BF16:
        pre = pre + (pre.detach().to(BF16).double() - pre.detach())
    y = F.silu(pre)
    y.backward(gout.double())
    return y.detach(), x64.grad, w64.grad, b64.grad


def _place(x, layout, dev):
    """x on the device in the layout: (leaf buffer, view handed to the kernels)."""
    B, L, Dn = x.shape
    nan = float("nan")
    if layout == "xz":
        buf = torch.full((B, L, 2 * Dn), nan, dtype=x.dtype)
        buf[..., :Dn] = x
        buf = buf.to(dev)
        return buf, buf[..., :Dn]
    if layout == "rs_pad":
        buf = torch.full((B, L, Dn + 4), nan, dtype=x.dtype)
        buf[..., :Dn] = x
        buf = buf.to(dev)
        return buf, buf[..., :Dn]
    if layout == "base_off":
        buf = torch.full((B, L, Dn + 8), nan, dtype=x.dtype)
        buf[..., 4:4 + Dn] = x
        buf = buf.to(dev)
        return buf, buf[..., 4:4 + Dn]
    buf = x.to(dev).contiguous()
    return buf, buf


def _dtc(dt):
    from apertis_llm_amd import _lib
    return _lib.BF16 if dt == BF16 else _lib.F32


@pytest.mark.parametrize("cid,dt,k,B,L,Dn,layout,path", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_dwconv_silu_against_fp64(dev, cid, dt, k, B, L, Dn, layout, path):
    """Forward, backward (one gradient) and bwd2 (two gradients, added in the kernel) of the depthwise causal conv + SiLU at
    the case's dispatch path (CONV_CASES: 'tile' = the LDS tile forward, 'thread' = the templated run-per-thread forward,
    'kn' = the runtime-width forward; the backward is the run-per-thread kernel - templated at k <= 4, runtime width above -
    on every case), through the C ABI and through ops.dwconv_silu / ops.dwconv_silu_pair:
      - outputs into NaN-filled buffers; the xz layout's output and bwd2's dx go to one half of a [B, L, 2 Dn] buffer whose
        other half must stay NaN, and x's own neighbouring columns are NaN (a read outside the rows would show);
      - three different sequences per case, so a window leaking across a sequence boundary shows;
      - dw / db against fp64 across the backward's per-block partials."""
    from apertis_llm_amd import _lib, ops
    lib, P, S = _lib.load(), _lib.ptr, _lib.stream_ptr
    Lc = L + (k - 1 if layout == "window" else 0)           # rows the conv runs over
    x, w, b, g1, g2 = _conv_inputs(dt, k, B, Lc, Dn, seed=k * 1000 + Dn + Lc)
    xbuf, xv = _place(x, layout, dev)
    nan = float("nan")
    if layout == "xz":
        obuf = torch.full((B, Lc, 2 * Dn), nan, device=dev, dtype=dt)
        out = obuf[..., Dn:]
    else:
        obuf = out = torch.full((B, Lc, Dn), nan, device=dev, dtype=dt)
    assert _conv_fwd_path(dt, Dn, k, [xv.data_ptr(), out.data_ptr()], [xv.stride(1), out.stride(1)]) == path
    wd, bd = w.reshape(Dn, k).to(dev), b.to(dev)
    dc = _dtc(dt)

    # ---- forward, C ABI
    rc = lib.apertis_dwconv_silu_fwd(P(xv), xv.stride(1), P(wd), P(bd), P(out), out.stride(1), B, Lc, Dn, k, dc, S())
    assert rc == 0, rc
    torch.cuda.synchronize()
    gs = (g1.float() + g2.float()).to(dt)                       # the kernel adds the two gradients rounded to the io dtype
    y_ref, dx_ref, dw_ref, db_ref = _conv_ref(x, w, b, gs, dt)
    _close(out, y_ref, f"{cid} y", _rtol(dt))
    if layout == "xz":
        assert torch.isnan(obuf[..., :Dn]).all(), "the forward wrote outside its output rows"

    # ---- bwd2 (two gradients) and bwd (one), C ABI; dx at row stride 2 Dn into a NaN buffer
    nblk = lib.apertis_dwconv_bwd_blocks(B, Lc, Dn)
    assert nblk == _conv_blocks(B, Lc, Dn), (nblk, _conv_blocks(B, Lc, Dn))
    G1, G2 = g1.to(dev), g2.to(dev)
    for two in (True, False):
        dxbuf = torch.full((B, Lc, 2 * Dn), nan, device=dev, dtype=dt)
        dx = dxbuf[..., :Dn]
        dw_part = torch.full((nblk, Dn, k), nan, device=dev)
        db_part = torch.full((nblk, Dn), nan, device=dev)
        dw, db = torch.full((Dn, k), nan, device=dev), torch.full((Dn,), nan, device=dev)
        if two:
            rc = lib.apertis_dwconv_silu_bwd2(P(xv), xv.stride(1), P(wd), P(bd), P(G1), Dn, P(G2), Dn, P(dx), 2 * Dn,
                                              P(dw_part), P(db_part), P(dw), P(db), B, Lc, Dn, k, dc, S())
            ref = (dx_ref, dw_ref, db_ref)
        else:
            rc = lib.apertis_dwconv_silu_bwd(P(xv), xv.stride(1), P(wd), P(bd), P(G1), Dn, P(dx), 2 * Dn,
                                             P(dw_part), P(db_part), P(dw), P(db), B, Lc, Dn, k, dc, S())
            ref = _conv_ref(x, w, b, g1, dt)[1:]
        assert rc == 0, rc
        torch.cuda.synchronize()
        tag = f"{cid} {'bwd2' if two else 'bwd'}"
        assert torch.isnan(dxbuf[..., Dn:]).all(), f"{tag}: dx written outside its rows"
        _close(dx, ref[0], f"{tag} dx", _rtol(dt))
        _sum_close(dw, ref[1].reshape(Dn, k), B * Lc, f"{tag} dw")
        _sum_close(db, ref[2], B * Lc, f"{tag} db")

    # ---- ops (autograd), the pair form with both views used; the window form keeps the first L outputs
    xl = xbuf.clone().requires_grad_(True)
    xin = xl[..., :Dn] if layout in ("xz", "rs_pad") else (xl[..., 4:4 + Dn] if layout == "base_off" else xl)
    wl, bl = w.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    ya, yb = ops.dwconv_silu_pair(xin, wl, bl)
    keep = slice(0, L) if layout == "window" else slice(0, Lc)
    (ya[:, keep].float() * G1[:, keep].float() + yb[:, keep].float() * G2[:, keep].float()).sum().backward()
    torch.cuda.synchronize()
    gk = torch.zeros_like(gs)
    gk[:, keep] = gs[:, keep]
    _, dx_r, dw_r, db_r = _conv_ref(x, w, b, gk, dt) if layout == "window" else (None, dx_ref, dw_ref, db_ref)
    _close(ya[:, keep], y_ref[:, keep], f"{cid} ops y", _rtol(dt))
    assert torch.equal(ya, out), "ops and the C ABI forward differ"
    xg = xl.grad[..., :Dn] if layout in ("xz", "rs_pad") else (xl.grad[..., 4:4 + Dn] if layout == "base_off" else xl.grad)
    _close(xg, dx_r, f"{cid} ops dx", _rtol(dt))
    _sum_close(wl.grad, dw_r, B * Lc, f"{cid} ops dw")
    _sum_close(bl.grad, db_r, B * Lc, f"{cid} ops db")


@pytest.mark.parametrize("k", [0, 1, 17, 32])
def test_dwconv_refuses_widths_outside_2_to_16(dev, k):
    """Conv widths outside 2..16 (the range the decode entry points accept) are refused with APERTIS_ERR_UNSUPPORTED by the
    forward and both backward entry points, with nothing written."""
    from apertis_llm_amd import _lib
    lib, P, S = _lib.load(), _lib.ptr, _lib.stream_ptr
    B, L, Dn = 2, 20, 64
    x = torch.randn(B, L, Dn, device=dev)
    w, b = torch.randn(Dn, max(k, 1), device=dev), torch.randn(Dn, device=dev)
    out = torch.full((B, L, Dn), float("nan"), device=dev)
    assert lib.apertis_dwconv_silu_fwd(P(x), Dn, P(w), P(b), P(out), Dn, B, L, Dn, k, _lib.F32, S()) == ERR_UNSUPPORTED
    nblk = lib.apertis_dwconv_bwd_blocks(B, L, Dn)
    part, bpart = torch.empty(nblk, Dn, max(k, 1), device=dev), torch.empty(nblk, Dn, device=dev)
    dw, db = torch.empty(Dn, max(k, 1), device=dev), torch.empty(Dn, device=dev)
    assert lib.apertis_dwconv_silu_bwd(P(x), Dn, P(w), P(b), P(x), Dn, P(out), Dn, P(part), P(bpart), P(dw), P(db), B, L, Dn, k,
                                       _lib.F32, S()) == ERR_UNSUPPORTED
    assert lib.apertis_dwconv_silu_bwd2(P(x), Dn, P(w), P(b), P(x), Dn, P(x), Dn, P(out), Dn, P(part), P(bpart), P(dw), P(db),
                                        B, L, Dn, k, _lib.F32, S()) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ---------------------------------------------------------------------------------------------------------------------------
def _gate_ref(y, xc, z, D, dout):
    y64, xc64, z64, D64 = (t.double().requires_grad_(True) for t in (y, xc, z, D))
    out = (y64 + D64 * xc64) * F.silu(z64)
    out.backward(dout.double())
    return out.detach(), y64.grad, xc64.grad, z64.grad, D64.grad


@pytest.mark.parametrize("T", GATE_T)
@pytest.mark.parametrize("Dn", GATE_DN)
@pytest.mark.parametrize("ty,tio", GATE_PAIRS, ids=["f32-f32", "f32-bf16", "bf16-bf16"])
def test_ssm_gate_against_fp64(dev, ty, tio, Dn, T):
    """apertis_ssm_gate_fwd / _bwd: out = (y + D*xc) * silu(z) and its gradients, through the C ABI (and ops.ssm_gate for
    T > 0).  One kernel path per direction; what varies is the geometry: Dn 4 / 12 / 176 give CPR 1 / 3 / 44 (RP 256 / 85 / 5
    rows per block), Dn 1028 / 4100 give CPR 257 / 1025 > 256 (RP 1: the backward's multi-pass c0 loop and its LDS reduction
    in every pass); T 'big' puts the grid at its 2048-block cap up to Dn 176 (blocks walk many rows), T = 0 runs the backward
    anyway - no early return - and must leave dD exactly zero.  z is a column view at row stride 2 Dn + 4 with NaN
    neighbours; dy, dxc and dz go to column views of NaN-filled buffers whose other columns must stay NaN."""
    from apertis_llm_amd import _lib, ops
    lib, P, S = _lib.load(), _lib.ptr, _lib.stream_ptr
    T = _gate_T(T, Dn)
    g = torch.Generator().manual_seed(Dn * 7 + T)
    R = max(T, 1)                                             # rows allocated (T = 0: valid pointers, nothing read)
    y = torch.randn(R, Dn, generator=g).to(ty)
    xc, z, dout = (torch.randn(R, Dn, generator=g).to(tio) for _ in range(3))
    D = 1.0 + 0.5 * torch.randn(Dn, generator=g)
    nan = float("nan")
    zs = 2 * Dn + 4
    zbuf = torch.full((R, zs), nan, dtype=tio)
    zbuf[:, Dn + 4:] = z
    Y, XC, DO, DD = y.to(dev), xc.to(dev), dout.to(dev), D.to(dev)
    zbuf = zbuf.to(dev)
    Z = zbuf[:, Dn + 4:]
    cy, cio = _dtc(ty), _dtc(tio)

    out = torch.full((R, Dn), nan, device=dev, dtype=tio)
    assert lib.apertis_ssm_gate_fwd(P(Y), Dn, P(XC), Dn, P(Z), zs, P(DD), P(out), Dn, T, Dn, cy, cio, S()) == 0
    nblk = lib.apertis_ssm_gate_bwd_blocks(T, Dn)
    assert nblk == _gate_blocks(T, Dn), (nblk, _gate_blocks(T, Dn))
    dybuf = torch.full((R, 2 * Dn), nan, device=dev, dtype=ty)
    dxbuf = torch.full((R, 2 * Dn), nan, device=dev, dtype=tio)
    dzbuf = torch.full((R, zs), nan, device=dev, dtype=tio)
    dy, dxc, dz = dybuf[:, :Dn], dxbuf[:, Dn:], dzbuf[:, 4:4 + Dn]
    part = torch.full((nblk, Dn), nan, device=dev)
    dD = torch.full((Dn,), nan, device=dev)
    assert lib.apertis_ssm_gate_bwd(P(DO), Dn, P(Y), Dn, P(XC), Dn, P(Z), zs, P(DD), P(dy), 2 * Dn, P(dxc), 2 * Dn, P(dz), zs,
                                    P(part), P(dD), T, Dn, cy, cio, S()) == 0
    torch.cuda.synchronize()
    assert torch.isnan(zbuf[:, :Dn + 4]).all()
    if T == 0:
        assert torch.isnan(out).all() and torch.isnan(dybuf).all() and torch.isnan(dxbuf).all() and torch.isnan(dzbuf).all()
        assert torch.equal(dD, torch.zeros_like(dD)), "T = 0: dD must be exactly zero"
        return
    assert torch.isnan(dybuf[:, Dn:]).all() and torch.isnan(dxbuf[:, :Dn]).all()
    assert torch.isnan(dzbuf[:, :4]).all() and torch.isnan(dzbuf[:, 4 + Dn:]).all()
    o_ref, dy_ref, dxc_ref, dz_ref, dD_ref = _gate_ref(y, xc, z, D, dout)
    _close(out, o_ref, "out", _rtol(tio))
    _close(dy, dy_ref, "dy", _rtol(ty))
    _close(dxc, dxc_ref, "dxc", _rtol(tio))
    _close(dz, dz_ref, "dz", _rtol(tio))
    _sum_close(dD, dD_ref, T, "dD")

    # ops.ssm_gate (autograd) on [1, T, Dn] views, z strided
    yl, xl = Y.clone().requires_grad_(True), XC.clone().requires_grad_(True)
    zl = zbuf.clone().requires_grad_(True)
    Dl = DD.clone().requires_grad_(True)
    o = ops.ssm_gate(yl.view(1, T, Dn), xl.view(1, T, Dn), zl[:, Dn + 4:].view(1, T, Dn), Dl)
    assert torch.equal(o.reshape(T, Dn), out)
    o.backward(DO.view(1, T, Dn))
    torch.cuda.synchronize()
    assert torch.equal(yl.grad, dy) and torch.equal(xl.grad, dxc) and torch.equal(zl.grad[:, Dn + 4:], dz)
    assert float(zl.grad[:, :Dn + 4].abs().max()) == 0.0
    _sum_close(Dl.grad, dD_ref, T, "ops dD")


def test_ssm_gate_refuses_bf16_y_with_fp32_io(dev):
    """The dtype pair (bf16 y, fp32 xc / z / out) has no kernel: APERTIS_ERR_UNSUPPORTED from both directions."""
    from apertis_llm_amd import _lib
    lib, P, S = _lib.load(), _lib.ptr, _lib.stream_ptr
    T, Dn = 8, 16
    y = torch.randn(T, Dn, device=dev).bfloat16()
    a = torch.randn(T, Dn, device=dev)
    D = torch.ones(Dn, device=dev)
    out = torch.full((T, Dn), float("nan"), device=dev)
    part, dD = torch.empty(1, Dn, device=dev), torch.empty(Dn, device=dev)
    dy = torch.empty(T, Dn, device=dev).bfloat16()
    assert lib.apertis_ssm_gate_fwd(P(y), Dn, P(a), Dn, P(a), Dn, P(D), P(out), Dn, T, Dn, _lib.BF16, _lib.F32, S()) == ERR_UNSUPPORTED
    assert lib.apertis_ssm_gate_bwd(P(a), Dn, P(y), Dn, P(a), Dn, P(a), Dn, P(D), P(dy), Dn, P(out), Dn, P(out), Dn, P(part),
                                    P(dD), T, Dn, _lib.BF16, _lib.F32, S()) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ---------------------------------------------------------------------------------------------------------------------------
MODEL_CASES = [  # (ssm_conv_kernel, heads, ssm_d_state, hidden): Dn = heads * d_state
    (2, 4, 16, 128),
    (3, 4, 16, 128),
    (5, 4, 16, 128),
    (8, 4, 16, 128),
    (4, 12, 64, 192),        # Dn 768 fp32: PCS 192, a tile of 205 824 B - past the CU's LDS: the run-per-thread forward
]


@pytest.mark.parametrize("k,heads,N,H", MODEL_CASES, ids=[f"k{c[0]}-dn{c[1] * c[2]}" for c in MODEL_CASES])
def test_model_at_conv_width_and_wide_dn_vs_oracle(dev, k, heads, N, H):
    """ApertisForCausalLM (2 layers, selective_ssm, dense FFN, fp32, eval mode) at conv widths 2, 3, 5, 8 (Dn 64: the tile
    forward at k 2 / 3, the runtime-width kernels at 5 / 8) and at Dn = 768 (k = 4: past the tile's LDS bound, the templated
    run-per-thread forward): logits, loss and every parameter gradient against fp64 autograd through the CPU oracle, at the
    BASELINE bar (rtol 1e-4, absolute floor 1e-5 of each tensor's largest entry).  Then a 20-token prefill and 8 cached
    single-token steps through the decode kernels (no_grad: apertis_ssm_decode_conv) against the same steps through the general
    path (grad mode: the training conv over [cached window | new token]): logits, conv windows and states at the same bar (the
    windows hold in_proj_x rows, which the two paths reach through different LayerNorm / GEMM launches: not the same bits)."""
    import apertis_llm_amd as A
    from oracle import ref_cpu
    torch.manual_seed(100 + k + heads)
    cfg = A.ApertisConfig(vocab_size=256, hidden_size=H, num_hidden_layers=2, num_attention_heads=heads, ssm_d_state=N,
                          ssm_conv_kernel=k, intermediate_size=2 * H, attention_type="selective_ssm", use_expert_system=False)
    model = A.ApertisForCausalLM(cfg).to(dev).eval()
    ids = torch.randint(4, 256, (3, 40), device=dev)
    out = model(input_ids=ids, labels=ids, use_cache=False)
    out[0].backward()
    torch.cuda.synchronize()
    cfgd = dict(cfg.to_dict())
    sd = {n: v.detach().cpu().double().requires_grad_(True) for n, v in model.state_dict().items() if n != "lm_head.weight"}
    o_loss, o_logits = ref_cpu.model_forward(sd, cfgd, ids.cpu(), None, ids.cpu())
    o_loss.backward()
    rel_error_report(f"k{k} Dn{heads * N} logits", out[1], o_logits, rtol=1e-4, atol_scale=1e-5)
    assert abs(float(out[0]) - float(o_loss)) <= 1e-4 * abs(float(o_loss)), (float(out[0]), float(o_loss))
    ours = {n: p.grad for n, p in model.named_parameters()}
    checked = []
    for n, ref in sd.items():
        if ref.grad is None:
            continue
        got = ours.get(n)
        if got is None:
            assert float(ref.grad.abs().max()) == 0.0, n
            continue
        rec = rel_error_report(f"k{k} Dn{heads * N} grad {n}", got, ref.grad, rtol=1e-4, atol_scale=1e-5, check=False)
        assert rec["worst_excess"] <= 1.0, rec
        checked.append(n)
    assert len(checked) >= 20 and sum("conv1d." in n for n in checked) == 4, checked

    # decode: the single-token kernels against the general path from the same prefilled caches
    with torch.no_grad():
        o = model(input_ids=ids[:, :20], use_cache=True)
    past0 = o[4]
    steps = torch.randint(4, 256, (3, 8), device=dev)
    pa = [(c.clone(), s.clone()) for c, s in past0]
    pb = [(c.clone(), s.clone()) for c, s in past0]
    for t in range(8):
        with torch.no_grad():
            oa = model(input_ids=steps[:, t:t + 1], past_key_values=pa, use_cache=True)
        with torch.enable_grad():
            ob = model(input_ids=steps[:, t:t + 1], past_key_values=pb, use_cache=True)
        pa, pb = oa[4], ob[4]
        rel_error_report(f"k{k} Dn{heads * N} decode step {t} logits", oa[1].detach(), ob[1].detach(), rtol=1e-4, atol_scale=1e-5)
        for (ca, sa), (cb, sb) in zip(pa, pb):
            assert ca.shape[-1] == k - 1
            _close(ca.detach().reshape(cb.shape), cb.detach(), f"step {t} conv window", rtol=1e-4)
            _close(sa.detach(), sb.detach(), f"step {t} state", rtol=1e-4)
