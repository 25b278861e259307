"""The single-token decode-step kernels, each called directly and compared with a float64 reference of the same operation on the
inputs as stored (tests/decode_step_ref.py), at every path of their entry points:
  apertis_decode_pre_conv / _pre_state / _post / _dense_gemv   (csrc/decode_step.hip)
  apertis_decode_inproj: xn form with epilogue, boundary form, xz output form   (decode_ln_inproj_k, csrc/layernorm.hip)
  apertis_ssm_decode_conv / _state / _state_dt   (csrc/scan_gate.hip)
The cases are the tables of decode_step_ref.py, each row with the path it reaches; test_case_tables_cover_every_dispatch_path
holds the tables to the mirror of the dispatch kept there.

Assertions and where their bounds come from:
  exact (torch.equal on the bits)
    - the window push (values are moved, not computed), and that a kernel leaves its inputs alone;
    - the bf16 output of both GEMV kernels on the dyadic grid (x = n/16, W = m/32, bias = j/64, |n|, |m|, |j| <= 31: every
      partial sum up to K = 1024 is an integer below 2^20 over 512, inside an fp32 significand in any summation order -
      decode_step_ref.py's module doc; the single rounding left is the bf16 one of an exactly known value), the window entries
      the in_proj epilogue pushes included;
    - y of the boundary form: one fp32 addition of stored values (the combine's operands on a dyadic grid, so its bf16 value is
      known exactly too);
    - every "the same bits as the launches it replaces" claim of the kernels' comments: dense GEMV and in_proj against
      ops.grouped_linear's skinny kernel (followed by ops.decode_post), the boundary form against moe_combine ->
      dropout_add_layer_norm (p = 0) -> the xn form, the stacked pre-pass against the per-layer kernels.
  fp32 outputs (state, pre, fp32 xc / gated): rtol 1e-4 with a floor of 1e-5 of the tensor's largest entry (the project's bar).
  bf16 outputs computed from exactly known or stored operands (xc, gated, xn): one bf16 rounding, rtol 8e-3, same floor.
  GEMV outputs on random operands: rtol 2e-2, atol 1e-2 of the tensor's maximum (test_grouped_linear_skinny_rows's bound).
Memory a kernel must not read is NaN (window entries 1..k-2 for the conv, the columns of p outside Bt / C / dt, W's columns
K..ldw-1, the z half where only xp is read and the xp half where only z is, xz's columns past 2 Dn); behind every output lie 64
sentinel elements that must survive."""
import math

import pytest
import torch

import decode_step_ref as R
from decode_step_ref import (BF16, BOUNDARY_CASES, CHAIN_CASES, CHAIN_SHAPE, ELEM_CASES, ERR_ARG, ERR_UNSUPPORTED, F32, GEMV_CASES,
                             GEMV_REFUSED, INPROJ_CASES, INPROJ_REFUSED, STATE_CASES, XZ_CASES)

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT = -768.0                   # exact in bf16


def test_case_tables_cover_every_dispatch_path():
    R.check_case_tables_cover_every_dispatch_path()


# ---------------------------------------------------------------------------------------------------------------------------
def _close(got, ref, name, rtol, atol_scale=1e-5):
    ref = torch.as_tensor(ref).detach().cpu().to(torch.float64)
    got = got.detach().cpu().to(torch.float64)
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), f"{name}: {int((~torch.isfinite(got)).sum())} non-finite values"
    atol = atol_scale * float(ref.abs().max()) + 1e-30
    err = (got - ref).abs()
    print(f"FIGURE {name}: max abs err {float(err.max()):.3e}, worst excess {float((err / (atol + rtol * ref.abs())).max()):.3f} "
          f"(rtol {rtol}, ref max {float(ref.abs().max()):.3e})")
    bad = err > atol + rtol * ref.abs()
    assert not bad.any(), f"{name}: {int(bad.sum())} / {bad.numel()} outside rtol {rtol}; max abs diff " \
                          f"{float(err.max()):.3e} (ref max {float(ref.abs().max()):.3e})"


def _rtol(dt):
    return 1e-4 if dt == F32 else 8e-3


def _dtc(dt):
    from apertis_llm_amd import _lib
    return _lib.BF16 if dt == BF16 else _lib.F32


def _guarded(n, dt, dev, init=None):
    """A flat device buffer of n elements (NaN, or `init`) with 64 sentinel elements behind it."""
    buf = torch.full((n + 64,), SENT, dtype=dt, device=dev)
    buf[:n] = NAN if init is None else init.reshape(-1).to(dev)
    return buf


def _guard_ok(buf, n, name):
    assert bool((buf[n:] == SENT).all()), f"{name}: written past its end"


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def _same_bits(got, ref, name):
    assert got.shape == ref.shape and got.dtype == ref.dtype, (name, got.shape, ref.shape, got.dtype, ref.dtype)
    same = _bits(got) == _bits(ref)
    assert bool(same.all()), f"{name}: {int((~same).sum())} / {same.numel()} elements differ"


def _ceil(a, b):
    return -(-a // b) * b


def _api():
    from apertis_llm_amd import _lib, ops
    return _lib.load(), _lib.ptr, _lib.stream_ptr, ops


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,dt,k,NL,B,Dn,pad", ELEM_CASES, ids=[c[0] for c in ELEM_CASES])
def test_pre_conv_post_and_per_layer_conv_against_fp64(dev, cid, dt, k, NL, B, Dn, pad):
    """decode_pre_conv (all layers in one launch), ssm_decode_step (a layer: conv + push, out of place and in place) and
    decode_post (gate + push in place) at ELEM_CASES: per-layer weights that differ, so a wrong layer index shows.
      - the stacked conv reads a window whose entries 1..k-2 are NaN and must not write it;
      - the per-layer conv reads xp as the front half of an xz row whose z half is NaN, and equals the stacked one bit for bit;
      - decode_post reads xz at row stride 2 Dn + pad with NaN in the pad, gates within the dtype's bar and pushes exactly."""
    lib, P, ST, ops = _api()
    g = torch.Generator().manual_seed(1000 * k + NL * B * Dn)
    win = torch.randn(NL, B, Dn, k - 1, generator=g).to(dt)
    w, bias = torch.randn(NL, Dn, k, generator=g) * 0.5, torch.randn(NL, Dn, generator=g) * 0.2
    xz, pre = torch.randn(NL, B, 2 * Dn, generator=g).to(dt), torch.randn(NL, B, Dn, generator=g)
    n, dc = NL * B * Dn, _dtc(dt)
    xc_ref = R.conv_ref(win, w, bias)
    wd, bd, pre_d = w.to(dev), bias.to(dev), pre.to(dev)

    # ---- the stacked conv, C ABI
    poisoned = win.clone()
    poisoned[..., 1:] = NAN
    pw = poisoned.to(dev)
    xcb = _guarded(n, dt, dev)
    assert lib.apertis_decode_pre_conv(P(pw), P(wd), P(bd), P(xcb), NL, B, Dn, k, dc, ST()) == 0
    torch.cuda.synchronize()
    _guard_ok(xcb, n, f"{cid} xc")
    xc = xcb[:n].view(NL, B, Dn)
    _close(xc, xc_ref, f"{cid} pre_conv xc", _rtol(dt))
    _same_bits(pw, poisoned, f"{cid} pre_conv left the window alone")
    assert torch.equal(ops.decode_pre_conv(win.to(dev), wd, bd), xc), "ops.decode_pre_conv and the C ABI differ"

    for l in range(NL):
        new_win = R.push_ref(win[l], xz[l][:, :Dn])
        # ---- the per-layer conv + push
        xzp = xz[l].clone()
        xzp[:, Dn:] = NAN
        xzp = xzp.to(dev)
        win_d = win[l].to(dev)
        xc_l, cs = ops.ssm_decode_step(xzp[:, :Dn], win_d, wd[l], bd[l])
        torch.cuda.synchronize()
        assert torch.equal(xc_l, xc[l]), f"{cid} layer {l}: ssm_decode_step and decode_pre_conv differ"
        _close(xc_l, xc_ref[l], f"{cid} layer {l} ssm_decode_step xc", _rtol(dt))
        _same_bits(cs, new_win, f"{cid} layer {l} ssm_decode_step window")
        _same_bits(win_d, win[l], f"{cid} layer {l} out-of-place push left its input alone")
        xc_i, cs_i = ops.ssm_decode_step(xzp[:, :Dn], win_d, wd[l], bd[l], inplace=True)
        torch.cuda.synchronize()
        assert cs_i.data_ptr() == win_d.data_ptr() and torch.equal(xc_i, xc_l)
        _same_bits(win_d, new_win, f"{cid} layer {l} in-place push")

        # ---- gate + push, C ABI
        rs = 2 * Dn + pad
        xzb = torch.full((B, rs), NAN, dtype=dt)
        xzb[:, :2 * Dn] = xz[l]
        xzb = xzb.to(dev)
        m = B * Dn
        csb, gb = _guarded(m * (k - 1), dt, dev, win[l]), _guarded(m, dt, dev)
        assert lib.apertis_decode_post(P(pre_d[l]), P(xzb), rs, P(csb), P(gb), B, Dn, k, dc, ST()) == 0
        torch.cuda.synchronize()
        _guard_ok(csb, m * (k - 1), f"{cid} layer {l} post window")
        _guard_ok(gb, m, f"{cid} layer {l} gated")
        _close(gb[:m].view(B, Dn), R.gate_ref(pre[l], xz[l][:, Dn:]), f"{cid} layer {l} post gated", _rtol(dt))
        _same_bits(csb[:m * (k - 1)].view(B, Dn, k - 1), new_win, f"{cid} layer {l} post window")
        win_o = win[l].to(dev)
        assert torch.equal(ops.decode_post(pre_d[l], xzb, win_o), gb[:m].view(B, Dn)), "ops.decode_post and the C ABI differ"
        _same_bits(win_o, new_win, f"{cid} layer {l} ops.decode_post window")


def test_conv_and_post_refuse_widths_outside_2_to_16(dev):
    lib, P, ST, _ = _api()
    a = torch.zeros(64, device=dev)
    for k in (1, 17):
        assert lib.apertis_decode_pre_conv(P(a), P(a), P(a), P(a), 1, 1, 2, k, 0, ST()) == ERR_UNSUPPORTED
        assert lib.apertis_decode_post(P(a), P(a), 4, P(a), P(a), 1, 2, k, 0, ST()) == ERR_UNSUPPORTED
    assert lib.apertis_decode_post(P(a), P(a), 3, P(a), P(a), 1, 2, 4, 0, ST()) == ERR_ARG          # xz_rs < 2 Dn
    torch.cuda.synchronize()
    assert float(a.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------
def _state_inputs(dt, NL, B, h, N, Rk, bias, lead, seed, steps):
    g = torch.Generator().manual_seed(seed)
    Dn = h * N
    Wb, Wr = _ceil(Dn, 64), _ceil(Rk, 64)
    o_bt, o_c, o_dt, prs = lead, lead + Wb, lead + 2 * Wb, lead + 2 * Wb + Wr
    par = dict(W_dt=torch.randn(NL, h, Rk, generator=g) * 0.5 / math.sqrt(Rk), b_dt=torch.randn(NL, h, generator=g) * 0.3 if bias else None,
               A_log=torch.rand(NL, h, N, generator=g) * 1.5 - 1.0, D=1.0 + 0.5 * torch.randn(NL, Dn, generator=g),
               s0=torch.randn(NL, B, Dn, generator=g), offs=(o_bt, o_c, o_dt), prs=prs)
    seq = []
    for _ in range(steps):
        Bt, C, xc, z = (torch.randn(NL, B, Dn, generator=g).to(dt) for _ in range(4))
        xdt = (torch.randn(NL, B, Rk, generator=g) * 0.5).to(dt)
        p = torch.full((NL * B, prs), NAN, dtype=dt)
        p[:, o_bt:o_bt + Dn], p[:, o_c:o_c + Dn], p[:, o_dt:o_dt + Rk] = Bt.reshape(-1, Dn), C.reshape(-1, Dn), xdt.reshape(-1, Rk)
        seq.append(dict(Bt=Bt, C=C, xc=xc, z=z, xdt=xdt, p=p))
    return par, seq


@pytest.mark.parametrize("cid,dt,NL,B,h,N,Rk,bias,sp,lead", STATE_CASES, ids=[c[0] for c in STATE_CASES])
def test_pre_state_and_per_layer_state_against_fp64(dev, cid, dt, NL, B, h, N, Rk, bias, sp, lead):
    """decode_pre_state (all layers at once) over THREE consecutive steps on one state buffer - an error in the in-place update
    compounds - against the fp64 recurrence from the same start; p is the model's padded row (64-column blocks, NaN outside
    Bt / C / dt, `lead` columns in front), A_log, D, W_dt and b_dt differ per layer.  Then the per-layer kernels on the first
    step: ssm_decode_state_dt (dt_proj_head inside) on row-strided views of p and a z view whose xp half is NaN must leave the
    stacked kernel's state bit for bit; ssm_decode_state takes the logits (fp64, rounded to fp32) instead."""
    lib, P, ST, ops = _api()
    Dn, n, dc = h * N, NL * B * h * N, _dtc(dt)
    par, seq = _state_inputs(dt, NL, B, h, N, Rk, bias, lead, seed=NL * 1000 + Dn + Rk, steps=3)
    o_bt, o_c, o_dt = par["offs"]
    Wd, Ad, Dd = par["W_dt"].to(dev), par["A_log"].to(dev), par["D"].to(dev)
    bd = None if par["b_dt"] is None else par["b_dt"].to(dev)
    sb = _guarded(n, F32, dev, par["s0"])
    s_ref = par["s0"].double()
    first = None
    for t, st in enumerate(seq):
        pd, xcd = st["p"].to(dev), st["xc"].to(dev)
        preb = _guarded(n, F32, dev)
        if t == 0:
            s_ops = par["s0"].to(dev).clone()
            with torch.no_grad():
                pre_ops = ops.decode_pre_state(pd, o_bt, o_c, o_dt, Wd, bd, Ad, Dd, xcd, s_ops, delta_softplus=sp)
        assert lib.apertis_decode_pre_state(P(pd), par["prs"], o_bt, o_c, o_dt, P(Wd), P(bd), Rk, P(Ad), P(Dd), P(xcd), P(sb), P(preb),
                                            NL, B, h, N, int(sp), dc, ST()) == 0
        torch.cuda.synchronize()
        _guard_ok(sb, n, f"{cid} step {t} state")
        _guard_ok(preb, n, f"{cid} step {t} pre")
        s_ref, pre_ref = R.state_ref(st["xdt"], par["W_dt"], par["b_dt"], par["A_log"], st["Bt"], st["C"], par["D"], st["xc"], s_ref, sp)
        _close(sb[:n].view(NL, B, Dn), s_ref, f"{cid} step {t} state", 1e-4)
        _close(preb[:n].view(NL, B, Dn), pre_ref, f"{cid} step {t} pre", 1e-4)
        _same_bits(pd, st["p"], f"{cid} step {t}: p left alone")
        if t == 0:
            first = (sb[:n].view(NL, B, Dn).clone(), s_ref, pre_ref)
            assert torch.equal(s_ops, first[0]) and torch.equal(pre_ops, preb[:n].view(NL, B, Dn)), "ops and the C ABI differ"

    # ---- the per-layer kernels, first step
    st, (s1, s1_ref, pre1_ref) = seq[0], first
    pd, xcd = st["p"].to(dev), st["xc"].to(dev)
    for l in range(NL):
        rows = pd[l * B:(l + 1) * B]
        zb = torch.full((B, 2 * Dn), NAN, dtype=dt)
        zb[:, Dn:] = st["z"][l]
        zv = zb.to(dev)[:, Dn:]
        out_ref = R.gate_ref(pre1_ref[l], st["z"][l])
        s_l = par["s0"][l].to(dev).clone()
        out = ops.ssm_decode_state_dt(rows[:, o_dt:o_dt + Rk], Wd[l], None if bd is None else bd[l], Ad[l], rows[:, o_bt:o_bt + Dn],
                                      rows[:, o_c:o_c + Dn], xcd[l], zv, Dd[l], s_l, delta_softplus=sp)
        torch.cuda.synchronize()
        assert torch.equal(s_l, s1[l]), f"{cid} layer {l}: ssm_decode_state_dt and decode_pre_state leave different states"
        _close(out, out_ref, f"{cid} layer {l} state_dt out", _rtol(dt))
        logits = torch.einsum("br,hr->bh", st["xdt"][l].double(), par["W_dt"][l].double())
        if par["b_dt"] is not None:
            logits = logits + par["b_dt"][l].double()
        s_l = par["s0"][l].to(dev).clone()
        out = ops.ssm_decode_state(logits.float().to(dev), Ad[l], rows[:, o_bt:o_bt + Dn], rows[:, o_c:o_c + Dn], xcd[l], zv, Dd[l], s_l,
                                   delta_softplus=sp)
        torch.cuda.synchronize()
        _close(s_l, s1_ref[l], f"{cid} layer {l} ssm_decode_state state", 1e-4)
        _close(out, out_ref, f"{cid} layer {l} ssm_decode_state out", _rtol(dt))


def test_pre_state_refuses_columns_outside_the_row(dev):
    lib, P, ST, _ = _api()
    a = torch.zeros(256, device=dev)
    for off in ((0, 0, 60), (60, 0, 0), (0, 60, 0), (-1, 0, 0)):             # Dn = 8, R = 8 in rows of 64 columns
        assert lib.apertis_decode_pre_state(P(a), 64, off[0], off[1], off[2], P(a), None, 8, P(a), P(a), P(a), P(a), P(a), 1, 1, 1, 8, 1,
                                            0, ST()) == ERR_ARG
    torch.cuda.synchronize()
    assert float(a.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,dt", CHAIN_CASES, ids=[f"k{k}" for k, _ in CHAIN_CASES])
def test_stacked_prepass_equals_the_per_layer_chain_bit_for_bit(dev, k, dt):
    """decode_pre_conv -> x_param product (ops.grouped_linear, one group per layer) -> decode_pre_state -> decode_post against,
    per layer, ssm_decode_step -> the same product -> ssm_decode_state_dt: gated values, windows and states bit for bit, at
    conv widths 2 and 16 with Dn = 80, N = 8 (bf16: both products run on the skinny NT kernel)."""
    _, _, _, ops = _api()
    NL, B, h, N, Rk = (CHAIN_SHAPE[x] for x in ("NL", "B", "h", "N", "R"))
    Dn, Wb, Wr = h * N, _ceil(h * N, 64), _ceil(Rk, 64)
    g = torch.Generator().manual_seed(77 + k)
    rnd = lambda *s: torch.randn(*s, generator=g)                                     # noqa: E731
    win, xz = rnd(NL, B, Dn, k - 1).to(dt).to(dev), rnd(NL, B, 2 * Dn).to(dt).to(dev)
    cw, cb = (rnd(NL, Dn, k) * 0.5).to(dev), (rnd(NL, Dn) * 0.2).to(dev)
    wp = torch.zeros(NL, 2 * Wb + Wr, Dn)
    for lo, cnt in ((0, Dn), (Wb, Dn), (2 * Wb, Rk)):
        wp[:, lo:lo + cnt] = rnd(NL, cnt, Dn) / math.sqrt(Dn)
    wp = wp.to(dev)
    W_dt, b_dt = (rnd(NL, h, Rk) * 0.5 / math.sqrt(Rk)).to(dev), (rnd(NL, h) * 0.3).to(dev)
    A_log, D, s0 = (torch.rand(NL, h, N, generator=g) * 1.5 - 1.0).to(dev), (1.0 + 0.5 * rnd(NL, Dn)).to(dev), rnd(NL, B, Dn).to(dev)
    with torch.no_grad():
        # the stacked form
        win_a, s_a = win.clone(), s0.clone()
        xc_all = ops.decode_pre_conv(win_a, cw, cb)
        offs = torch.arange(0, (NL + 1) * B, B, dtype=torch.int32, device=dev)
        p_all = ops.grouped_linear(xc_all.reshape(NL * B, Dn), wp, None, offs, NL * B, compute_dtype=dt)
        pre = ops.decode_pre_state(p_all, 0, Wb, 2 * Wb, W_dt, b_dt, A_log, D, xc_all, s_a)
        gated_a = [ops.decode_post(pre[l], xz[l], win_a[l]) for l in range(NL)]
        # the per-layer form
        for l in range(NL):
            xc, cs = ops.ssm_decode_step(xz[l][:, :Dn], win[l], cw[l], cb[l])
            p = ops.grouped_linear(xc, wp[l:l + 1], None, ops.dense_offsets(B, dev), B, compute_dtype=dt)
            s_b = s0[l].clone()
            out = ops.ssm_decode_state_dt(p[:, 2 * Wb:2 * Wb + Rk], W_dt[l], b_dt[l], A_log[l], p[:, :Dn], p[:, Wb:Wb + Dn], xc,
                                          xz[l][:, Dn:], D[l], s_b)
            torch.cuda.synchronize()
            assert torch.equal(xc, xc_all[l]) and torch.equal(p, p_all[l * B:(l + 1) * B]), f"layer {l}: conv or x_param product"
            assert torch.equal(out, gated_a[l]), f"layer {l}: gated"
            assert torch.equal(cs, win_a[l]), f"layer {l}: window"
            assert torch.equal(s_b, s_a[l]), f"layer {l}: state"
    assert torch.isfinite(torch.stack(gated_a).float()).all() and not torch.equal(win_a, win)


# ---------------------------------------------------------------------------------------------------------------------------
def _gemv_inputs(B, K, N, use_bias, grid, seed):
    """(x bf16, W fp32 holding bf16 values, bias fp32 or None) on the CPU."""
    if grid == "dyadic":
        x, W, b = R.dyadic_gemv_inputs(B, K, N, use_bias, seed)
    else:
        g = torch.Generator().manual_seed(seed)
        x, W = torch.randn(B, K, generator=g), (torch.randn(N, K, generator=g) / math.sqrt(K)).bfloat16().float()
        b = torch.randn(N, generator=g) if use_bias else None
    return x.bfloat16(), W, b


def _padded_w(W, ldw, dev):
    """W [N, K] as a bf16 device buffer of row pitch ldw with NaN in the columns K..ldw-1."""
    buf = torch.full((W.shape[0], ldw), NAN, dtype=BF16)
    buf[:, :W.shape[1]] = W.bfloat16()
    return buf.to(dev)


def _skinny_linear(ops, xd, W, b, dev):
    """x @ W.T + b through ops.grouped_linear's skinny NT kernel (one group).  That entry point wants 16-byte output rows, so
    N is filled up to a multiple of 8 with zero rows of W: a column of the output depends on its own row of W only."""
    N, K = W.shape
    Np = _ceil(N, 8)
    Wg = torch.zeros(1, Np, K)
    Wg[0, :N] = W
    bg = None
    if b is not None:
        bg = torch.zeros(1, Np)
        bg[0, :N] = b
        bg = bg.to(dev)
    rows = xd.shape[0]
    return ops.grouped_linear(xd, Wg.to(dev), bg, ops.dense_offsets(rows, dev), rows, compute_dtype=BF16)


@pytest.mark.parametrize("cid,B,K,N,pad,use_bias,grid", GEMV_CASES, ids=[c[0] for c in GEMV_CASES])
def test_dense_gemv_against_fp64(dev, cid, B, K, N, pad, use_bias, grid):
    """apertis_decode_dense_gemv at GEMV_CASES: one and two K batches (the second with a single live chunk and ragged at its
    end), full and partial 16-column work-groups, 1 / 7 / 16 rows, W at row pitch K and at a wider pitch with NaN behind every
    row.  On the dyadic grid the bf16 output EQUALS the fp64 reference rounded once (module doc); random operands are held to
    test_grouped_linear_skinny_rows's bound.  ops.decode_dense_gemv and ops.grouped_linear's skinny kernel give the same bits."""
    lib, P, ST, ops = _api()
    x, W, b = _gemv_inputs(B, K, N, use_bias, grid, seed=K * 31 + N + B)
    ldw = K + pad
    assert R.gemv_rc(B, K, N, ldw) == 0
    xd, Wd = x.to(dev), _padded_w(W, ldw, dev)
    bd = None if b is None else b.to(dev)
    ob = _guarded(B * N, BF16, dev)
    assert lib.apertis_decode_dense_gemv(P(xd), P(Wd), ldw, P(bd), P(ob), B, K, N, ST()) == 0
    torch.cuda.synchronize()
    _guard_ok(ob, B * N, f"{cid} out")
    out = ob[:B * N].view(B, N)
    ref = R.gemv_ref(x, W, b, K)
    if grid == "dyadic":
        _same_bits(out, R.round_bf16(ref), f"{cid} out against the exact sum")
    else:
        _close(out, ref, f"{cid} out", rtol=2e-2, atol_scale=1e-2)
    with torch.no_grad():
        o2 = ops.decode_dense_gemv(xd, W.to(dev), bd)
        o3 = _skinny_linear(ops, xd, W, b, dev)
    assert o2 is not None and torch.equal(o2, out), "ops.decode_dense_gemv and the C ABI differ"
    assert torch.equal(o3[:, :N], out), "decode_dense_gemv_k and grouped_gemm_nt_skinny_k differ"


def test_dense_gemv_refusals(dev):
    """Shapes outside the kernel's: -2 from the C ABI with nothing written (ldw < K: the argument error); None from
    ops.decode_dense_gemv for fp32 input, a non-contiguous x, grad mode on and K = 512."""
    lib, P, ST, ops = _api()
    x, W = torch.zeros(17 * 512, dtype=BF16, device=dev), torch.zeros(64 * 512, dtype=BF16, device=dev)
    out = torch.full((17 * 64,), NAN, dtype=BF16, device=dev)
    for B, K, N, ldw in GEMV_REFUSED:
        assert R.gemv_rc(B, K, N, ldw) == ERR_UNSUPPORTED
        assert lib.apertis_decode_dense_gemv(P(x), P(W), ldw, None, P(out), B, K, N, ST()) == ERR_UNSUPPORTED, (B, K, N, ldw)
    assert lib.apertis_decode_dense_gemv(P(x), P(W), 56, None, P(out), 1, 64, 64, ST()) == ERR_ARG
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    xb, w = torch.randn(4, 64, device=dev).bfloat16(), torch.randn(16, 64, device=dev)
    with torch.no_grad():
        assert ops.decode_dense_gemv(xb, w) is not None
        assert ops.decode_dense_gemv(xb.float(), w) is None
        assert ops.decode_dense_gemv(torch.randn(4, 128, device=dev).bfloat16()[:, ::2], w) is None
        assert ops.decode_dense_gemv(torch.randn(4, 512, device=dev).bfloat16(), torch.randn(16, 512, device=dev)) is None
    with torch.enable_grad():
        assert ops.decode_dense_gemv(xb, w) is None


# ---------------------------------------------------------------------------------------------------------------------------
def _inproj_abi(lib, P, ST, *, xn=None, W, ldw, xz=None, pre=None, conv=None, k=0, gated=None, S, H, N, Dn=0, bnd=None):
    blk = slot = wk = res = gam = bet = y = None
    KK, eps = 0, 0.0
    if bnd is not None:
        blk, slot, wk, KK, res, gam, bet, eps, y = bnd
    return lib.apertis_decode_inproj(P(blk), P(slot), P(wk), KK, P(res), P(gam), P(bet), float(eps), P(y), P(xn), P(W), ldw, P(xz), P(pre),
                                     P(conv), k, P(gated), S, H, N, Dn, ST())


@pytest.mark.parametrize("cid,S,H,Dn,k,pad", INPROJ_CASES, ids=[c[0] for c in INPROJ_CASES])
def test_inproj_with_epilogue_against_fp64(dev, cid, S, H, Dn, k, pad):
    """apertis_decode_inproj, xn given, gate and window push in the epilogue, at INPROJ_CASES: IT = 2 / 3 / 4, a last K quarter
    that is short and one that ends inside a 32-deep step, Dn = 130 (N = 260: one 4-column group pushes two window entries AND
    gates two values; the last work-group is partial), conv widths 2 / 4 / 16, W's rows padded with NaN.  xn and W on the dyadic
    grid, so xz = bf16(xn W^T) is known exactly: the pushed window entries EQUAL it, gated is within one bf16 rounding of
    pre * silu(z) with z the exact bf16 value.  Bit for bit the same as ops.grouped_linear (skinny, four K quarters) followed by
    ops.decode_post, and as ops.decode_inproj."""
    lib, P, ST, ops = _api()
    N = 2 * Dn
    x, W, _ = _gemv_inputs(S, H, N, False, "dyadic", seed=H * 7 + Dn + S)
    g = torch.Generator().manual_seed(H + k)
    pre, win = torch.randn(S, Dn, generator=g), torch.randn(S, Dn, k - 1, generator=g).bfloat16()
    ldw = H + pad
    assert R.inproj_rc(S, H, N, ldw, k) == 0
    xd, Wd, pre_d = x.to(dev), _padded_w(W, ldw, dev), pre.to(dev)
    m = S * Dn
    gb, cb = _guarded(m, BF16, dev), _guarded(m * (k - 1), BF16, dev, win)
    assert _inproj_abi(lib, P, ST, xn=xd, W=Wd, ldw=ldw, pre=pre_d, conv=cb, k=k, gated=gb, S=S, H=H, N=N, Dn=Dn) == 0
    torch.cuda.synchronize()
    _guard_ok(gb, m, f"{cid} gated")
    _guard_ok(cb, m * (k - 1), f"{cid} window")
    xz_ref = R.round_bf16(R.gemv_ref(x, W, None, H))                        # exact
    new_win = R.push_ref(win, xz_ref[:, :Dn])
    gated, win_k = gb[:m].view(S, Dn), cb[:m * (k - 1)].view(S, Dn, k - 1)
    _same_bits(win_k, new_win, f"{cid} window: the shift and the exact xp")
    _close(gated, R.gate_ref(pre, xz_ref[:, Dn:]), f"{cid} gated", rtol=8e-3)
    with torch.no_grad():
        win_o = win.to(dev)
        g2 = ops.decode_inproj(W.to(dev), pre_d, win_o, xn=xd)
        assert g2 is not None and torch.equal(g2, gated), "ops.decode_inproj and the C ABI differ"
        _same_bits(win_o, new_win, f"{cid} ops.decode_inproj window")
        xzg = _skinny_linear(ops, xd, W, None, dev)                         # [S, N rounded up to 8]
        _same_bits(xzg[:, :N].contiguous(), xz_ref, f"{cid} the skinny kernel's xz")
        win_p = win.to(dev)
        g3 = ops.decode_post(pre_d, xzg, win_p)
        assert torch.equal(g3, gated), "the epilogue's gate and grouped_linear -> decode_post differ"
        _same_bits(win_p, new_win, f"{cid} decode_post window")


@pytest.mark.parametrize("cid,S,H,N", XZ_CASES, ids=[c[0] for c in XZ_CASES])
def test_inproj_xz_output_form_is_exact_on_the_dyadic_grid(dev, cid, S, H, N):
    """pre == NULL: the product alone, xz written (the form only the C ABI reaches), at N = 20 and 260 - partial last
    work-groups - with NaN behind W's rows: equal to the exact sum rounded once to bf16."""
    lib, P, ST, _ = _api()
    x, W, _ = _gemv_inputs(S, H, N, False, "dyadic", seed=H + N + S)
    ldw = _ceil(H, 64) + 8
    xd, Wd = x.to(dev), _padded_w(W, ldw, dev)
    ob = _guarded(S * N, BF16, dev)
    assert _inproj_abi(lib, P, ST, xn=xd, W=Wd, ldw=ldw, xz=ob, S=S, H=H, N=N) == 0
    torch.cuda.synchronize()
    _guard_ok(ob, S * N, f"{cid} xz")
    _same_bits(ob[:S * N].view(S, N), R.round_bf16(R.gemv_ref(x, W, None, H)), f"{cid} xz against the exact sum")


def test_inproj_refusals(dev):
    """S = 17, H = 504, H = 1032 and kconv = 17 return -2 with nothing written; ops.decode_inproj returns None for a boundary
    form of more than four rows."""
    lib, P, ST, ops = _api()
    x, W = torch.zeros(17 * 1032, dtype=BF16, device=dev), torch.zeros(128 * 1032, dtype=BF16, device=dev)
    pre = torch.zeros(17 * 64, device=dev)
    conv, gated = torch.full((17 * 64 * 16,), NAN, dtype=BF16, device=dev), torch.full((17 * 64,), NAN, dtype=BF16, device=dev)
    for S, H, N, ldw, k in INPROJ_REFUSED:
        assert _inproj_abi(lib, P, ST, xn=x, W=W, ldw=ldw, pre=pre, conv=conv, k=k, gated=gated, S=S, H=H, N=N, Dn=N // 2) == ERR_UNSUPPORTED
    for S, H, N, ldw, _ in INPROJ_REFUSED[:3]:
        assert _inproj_abi(lib, P, ST, xn=x, W=W, ldw=ldw, xz=gated, S=S, H=H, N=N) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isnan(conv).all() and torch.isnan(gated).all()
    S, H, Dn = 5, 512, 64
    res, blk = torch.randn(S, 1, H, device=dev), torch.randn(S, 1, H, device=dev).bfloat16()
    w, ga = torch.randn(2 * Dn, H, device=dev), torch.ones(H, device=dev)
    win = torch.zeros(S, Dn, 3, dtype=BF16, device=dev)
    with torch.no_grad():
        assert ops.decode_inproj(w, torch.zeros(S, Dn, device=dev), win, boundary=(blk, res, ga, ga, 1e-5, None)) is None
        assert ops.decode_inproj(w, torch.zeros(S, Dn, device=dev), win, xn=blk) is not None


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,S,H,Dn,k,form", BOUNDARY_CASES, ids=[c[0] for c in BOUNDARY_CASES])
def test_inproj_boundary_form_against_fp64_and_the_launches_it_replaces(dev, cid, S, H, Dn, k, form):
    """apertis_decode_inproj with the block boundary as its prologue (LN = true), S = 1 and 4, IT = 2 / 3 / 4, blk dense or the
    MoE combine taken on the fly (two slots per row, at least one dropped; one row with both dropped where S = 4):
      - y EQUALS the fp32 sum res + blk (the combine's yr and weights on a dyadic grid: its bf16 value is exact);
      - (y, gated) and the window are bit for bit those of moe_combine -> dropout_add_layer_norm (p = 0) -> the xn form;
      - the xn of those launches is within one bf16 rounding of the fp64 LayerNorm of y;
      - the pushed xp and the gated values are within the random-operand GEMV bound of fp64 on that xn as stored."""
    _, _, _, ops = _api()
    g = torch.Generator().manual_seed(H * 3 + S + k)
    N = 2 * Dn
    res = torch.randn(S, 1, H, generator=g)
    gamma, beta, eps = 1.0 + 0.2 * torch.randn(H, generator=g), 0.1 * torch.randn(H, generator=g), 1e-5
    W = (torch.randn(N, H, generator=g) / math.sqrt(H)).bfloat16().float()
    pre, win = torch.randn(S, Dn, generator=g), torch.randn(S, Dn, k - 1, generator=g).bfloat16()
    Wd, pre_d, res_d, gd, bd = W.to(dev), pre.to(dev), res.to(dev), gamma.to(dev), beta.to(dev)
    with torch.no_grad():
        if form == "combine":
            rows = 2 * S
            yr = R.dyadic((rows, H), 16, g).bfloat16()
            wk = R.dyadic((S, 2), 8, g, bound=7)
            slot = torch.tensor([[2 * s, 2 * s + 1] for s in range(S)], dtype=torch.int32)
            slot[0, 1] = -1
            if S == 4:
                slot[2] = -1
                slot[3, 0] = -1
            plan = ops.MoePlan()
            plan.S, plan.E, plan.K, plan.max_rows, plan.slot_of = S, 4, 2, rows, slot.to(dev)
            blk_d, comb = yr.to(dev), (wk.to(dev), plan)
            y_ref, xn_ref = R.boundary_ref(res, yr, gamma, beta, eps, (wk, slot))
            blk_two = ops.moe_combine(blk_d, comb[0], plan, out_dtype=BF16)
            _same_bits(blk_two, R.round_bf16(R.combine_ref(yr, wk, slot)), f"{cid} moe_combine against the exact sum")
        else:
            blk = torch.randn(S, 1, H, generator=g).bfloat16()
            blk_d, comb = blk.to(dev), None
            y_ref, xn_ref = R.boundary_ref(res, blk.reshape(S, H), gamma, beta, eps)
            blk_two = blk_d
        win_a = win.to(dev)
        r = ops.decode_inproj(Wd, pre_d, win_a, boundary=(blk_d, res_d, gd, bd, eps, comb))
        assert r is not None
        y, gated = r
        torch.cuda.synchronize()
        # the launches it replaces
        y2, xn2 = ops.dropout_add_layer_norm(blk_two.reshape(S, 1, H), res_d, gd, bd, eps, 0.0, False, out_dtype=BF16)
        win_b = win.to(dev)
        gated2 = ops.decode_inproj(Wd, pre_d, win_b, xn=xn2)
        torch.cuda.synchronize()
    assert y.shape == res.shape
    _same_bits(y.reshape(S, H), y_ref, f"{cid} y against the fp32 sum")
    assert torch.equal(y, y2) and torch.equal(gated, gated2), "the boundary form and the launches it replaces differ"
    _same_bits(win_a, win_b.cpu(), f"{cid} window against the launches it replaces")
    _close(xn2.reshape(S, H), xn_ref, f"{cid} xn", rtol=8e-3)
    xz_ref = R.gemv_ref(xn2.reshape(S, H).cpu(), W, None, H)
    _same_bits(win_a[..., :k - 2], win[..., 1:], f"{cid} window shift")
    _close(win_a[..., k - 2], xz_ref[:, :Dn], f"{cid} pushed xp", rtol=2e-2, atol_scale=1e-2)
    _close(gated, R.gate_ref(pre, xz_ref[:, Dn:]), f"{cid} gated", rtol=2e-2, atol_scale=1e-2)
