"""ops.linear_cross_entropy at a vocabulary that is no multiple of the cross entropy kernels' 16-byte chunk (LCE_PAD_VOCAB): the
chunk's logits are formed Vp = ceil(V / VN) * VN wide (VN = 8 bf16, 4 fp32), the columns [V, Vp) hold -inf, and the existing
entry points run with V = Vp.

Reference: _lce_ref of test_loss_kernels_gpu (F.linear + F.cross_entropy in float64 on the rounded operands) at the caller's V.
Bounds, for every case, are those of test_linear_cross_entropy_two_kernel_path: loss 1e-5 (fp32) / 2e-3 (bf16) times
max(1, |ref|); d hidden and d W _close(rtol 1e-4, atol 1e-5 max|ref|) fp32 / (3e-2, 2e-2) bf16.

Widths: V = 1 (a row of one logit and 7 or 3 pads), one chunk and a bit, 513 (7 / 3 pads behind a full chunk per thread),
1007 / 1001 / 1003 (1 and 7 pads), both sides of the one-pass form's last width (Vp = 32768 / 32776 bf16, 16384 / 16388
fp32), and V = 31999 at H = 704 in two chunks, where the weight gradient runs on apertis_grouped_gemm_tn at Vp = 32000."""
import pytest
import torch

from test_loss_kernels_gpu import BF16, F32, CE_ENTRIES, CE_KEEP, CE_NT, _close, _code, _lce_ref, _lib, _spy, _tag, _vn

pytestmark = pytest.mark.gpu
NEG_INF = float("-inf")
SCALE = 1.3


def _vp(V, dt):
    return -(-V // _vn(dt)) * _vn(dt)


def _inputs(V, dt, B=2, L=9, H=32, wstd=0.1):
    """test_linear_cross_entropy_two_kernel_path's operands: labels [B, L + 2] with one -100 and one V - 1."""
    gen = torch.Generator().manual_seed(V + 1)
    h = (torch.randn(B, L, H, generator=gen) * 0.7).to(dt)
    W = torch.randn(V, H, generator=gen) * wstd
    lab = torch.randint(0, V, (B, L + 2), generator=gen)
    lab[0, 3], lab[1, 1] = -100, V - 1
    return h, W, lab


def _run(dev, h, W, lab, dt, grad=True):
    from apertis_llm_amd import ops
    hd, Wd = h.to(dev).requires_grad_(grad), W.to(dev).requires_grad_(grad)
    loss = ops.linear_cross_entropy(hd, Wd, lab.to(dev), compute_dtype=dt)
    if grad:
        (loss * SCALE).backward()
    return loss.detach(), hd.grad, Wd.grad


def _bounds(got, ref, dt, W):
    loss, dh, dW = got
    ref, dh_ref, dW_ref = ref
    ltol = 1e-5 if dt == F32 else 2e-3
    print(f"LCE {_tag(dt)} V={W.shape[0]}: loss {float(loss):.7f} ref {float(ref):.7f}, max |d hidden err| "
          f"{float((dh.double().cpu() - dh_ref).abs().max()):.3e} (ref max {float(dh_ref.abs().max()):.3e}), max |d W err| "
          f"{float((dW.double().cpu() - dW_ref).abs().max()):.3e} (ref max {float(dW_ref.abs().max()):.3e})")
    assert abs(float(loss) - float(ref)) <= ltol * max(1.0, abs(float(ref))), (float(loss), float(ref))
    rtol, asc = (1e-4, 1e-5) if dt == F32 else (3e-2, 2e-2)
    assert dW.shape == W.shape and dW.dtype == W.dtype and dh.dtype == dt
    _close(dh, dh_ref, "d hidden", rtol=rtol, atol_scale=asc)
    _close(dW, dW_ref, "d W", rtol=rtol, atol_scale=asc)


@pytest.fixture
def pad_on(monkeypatch):
    from apertis_llm_amd import ops
    monkeypatch.setattr(ops.loss, "LCE_PAD_VOCAB", True)


ODD = [(BF16, V) for V in (1, 9, 513, 1007, 1001)] + [(F32, V) for V in (1, 5, 513, 1003)]


# ---------------------------------------------------------------------------------------------------------------------------
# a. odd widths against fp64
@pytest.mark.parametrize("dt,V", ODD, ids=[f"{_tag(dt)}-V{V}" for dt, V in ODD])
def test_odd_vocabulary_against_fp64(dev, monkeypatch, pad_on, dt, V):
    """Loss, d hidden and d W [V, H] against float64; every CE launch sees Vp; without gradients only the forward kernel runs
    and gives the same loss."""
    from apertis_llm_amd import ops
    lib, _, _ = _lib()
    h, W, lab = _inputs(V, dt)
    assert ops.linear_cross_entropy_supported(h.to(dev), W.to(dev), lab.to(dev))
    calls = _spy(monkeypatch, lib, CE_ENTRIES)
    got = _run(dev, h, W, lab, dt)
    assert [c[0] for c in calls] == ["apertis_cross_entropy_fwd_bwd"] and calls[0][1][8] == _vp(V, dt) > V
    _bounds(got, _lce_ref(h, W, lab, dt, SCALE), dt, W)
    assert float(got[1][:, h.shape[1] - 1:].abs().max()) == 0.0
    del calls[:]
    with torch.no_grad():
        loss_ng, _, _ = _run(dev, h, W, lab, dt, grad=False)
    assert [c[0] for c in calls] == ["apertis_cross_entropy_fwd"] and calls[0][1][6] == _vp(V, dt)
    assert torch.equal(loss_ng, got[0])


def test_label_on_a_pad_column_is_out_of_range(dev, pad_on):
    """A label in [V, Vp) is outside the caller's vocabulary: skipped like any other out-of-range label, in the kernels and in
    the count."""
    dt, V = BF16, 1001
    h, W, lab = _inputs(V, dt)
    ref = _lce_ref(h, W, torch.where(lab == lab[0, 5], -100, lab), dt, SCALE)
    lab = torch.where(lab == lab[0, 5], V + 3, lab)
    assert int((lab == V + 3).sum()) >= 1 and V + 3 < _vp(V, dt)
    _bounds(_run(dev, h, W, lab, dt), ref, dt, W)


# ---------------------------------------------------------------------------------------------------------------------------
# b. the padding is exact
@pytest.mark.parametrize("fused", [False, True], ids=["two-kernels", "one-pass"])
@pytest.mark.parametrize("dt,V", [(BF16, 1001), (F32, 1003)], ids=["bf16-V1001", "f32-V1003"])
def test_padding_is_exact(dev, monkeypatch, dt, V, fused):
    """What the CE entry points saw and left: V = Vp, the backward in place, -inf in the pad columns at the forward call, exact
    zeros there after the backward, and lse of every live row bit for bit that of apertis_cross_entropy_fwd by hand on the
    op's own logits with -inf pads.  (The tensors behind the captured pointers are kept through ops.loss.ptr.)  Today's
    path at Vp, on the weight extended by rows that put the pad logits at -1e4 (exp underflows to an exact 0), meets the
    same float64 reference; its bits are not compared."""
    from apertis_llm_amd import ops
    lib, P, S = _lib()
    Vp = _vp(V, dt)
    h, W, lab = _inputs(V, dt)
    h[..., 0] = 1.0
    ref = _lce_ref(h, W, lab, dt, SCALE)
    W_ext = torch.cat([W, torch.zeros(Vp - V, W.shape[1])])
    W_ext[V:, 0] = -1e4
    monkeypatch.setattr(ops.loss, "LCE_PAD_VOCAB", False)
    ext = _run(dev, h, W_ext, lab, dt)
    _bounds((ext[0], ext[1], ext[2][:V]), ref, dt, W)
    assert float(ext[2][V:].abs().max()) == 0.0

    monkeypatch.setattr(ops.loss, "LCE_PAD_VOCAB", True)
    monkeypatch.setattr(ops.loss, "LCE_FUSED_CE", fused)
    held = {}
    real_ptr = ops.loss.ptr
    monkeypatch.setattr(ops.loss, "ptr", lambda t: real_ptr(t) if t is None else held.setdefault(real_ptr(t), t).data_ptr())
    calls = _spy(monkeypatch, lib, CE_ENTRIES)
    first = "apertis_cross_entropy_fwd_bwd" if fused else "apertis_cross_entropy_fwd"
    seen = {}
    spied = getattr(lib, first)

    def snapshot(*a):                                      # the chunk's logits as the op's first CE call meets them
        if "logits" not in seen:
            seen["logits"] = held[a[0]].clone()
        return spied(*a)
    monkeypatch.setattr(lib, first, snapshot)
    got = _run(dev, h, W, lab, dt)
    _bounds(got, ref, dt, W)
    assert [c[0] for c in calls] == ([first] if fused else ["apertis_cross_entropy_fwd", "apertis_cross_entropy_bwd"])
    n, L = h.shape[:2]
    for name, a in calls:
        assert a[8 if name.endswith("fwd_bwd") else 7 if name.endswith("_bwd") else 6] == Vp, (name, a)
    bwd = calls[-1][1]
    assert (bwd[0] == bwd[5]) if fused else (bwd[0] == bwd[4]), "the backward of the chunk runs in place on its logits"
    x = seen["logits"].reshape(n * L, Vp)
    assert bool((x[:, V:] == NEG_INF).all()) and bool(torch.isfinite(x[:, :V]).all())
    dl = held[bwd[0]].reshape(n * L, Vp)
    assert dl.dtype == dt and float(dl[:, V:].float().abs().max()) == 0.0
    assert float(dl[:, :V].float().abs().max()) > 0.0
    # lse by hand
    hand = torch.full((n * L, Vp), NEG_INF, dtype=dt, device=dev)
    hand[:, :V] = x[:, :V]
    lse, loss = torch.full((n * L,), 7.0, device=dev), torch.full((n * L,), 7.0, device=dev)
    labd = lab.to(dev)
    assert lib.apertis_cross_entropy_fwd(P(hand), P(labd), P(lse), P(loss), n, L, Vp, lab.shape[1], L - 1, -100, _code(dt), S()) == 0
    op_lse = held[calls[0][1][2]][:n * L]
    tgt = lab[:, 1:L]
    live = torch.zeros(n, L, dtype=torch.bool)
    live[:, :L - 1] = (tgt != -100) & (tgt >= 0) & (tgt < V)
    assert int(live.sum()) == n * (L - 1) - 1
    assert torch.equal(op_lse.view(torch.int32).cpu()[live.reshape(-1)], lse.view(torch.int32).cpu()[live.reshape(-1)])
    assert float(op_lse.cpu()[~live.reshape(-1)].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# c. both kernel regimes
REGIMES = [(BF16, CE_KEEP * CE_NT * 8 - 7, True), (BF16, CE_KEEP * CE_NT * 8 + 1, False),
           (F32, CE_KEEP * CE_NT * 4 - 3, True), (F32, CE_KEEP * CE_NT * 4 + 1, False)]


@pytest.mark.parametrize("dt,V,one_pass", REGIMES, ids=[f"{_tag(dt)}-V{V}" for dt, V, _ in REGIMES])
def test_both_kernel_regimes(dev, monkeypatch, pad_on, dt, V, one_pass):
    """Vp at the one-pass form's last width (one launch) and at the first it declines (it is asked, declines, and the two
    kernels run in place)."""
    lib, _, _ = _lib()
    assert [r[1] for r in REGIMES] == [32761, 32769, 16381, 16385]
    h, W, lab = _inputs(V, dt)
    ref = _lce_ref(h, W, lab, dt, SCALE)
    calls = _spy(monkeypatch, lib, CE_ENTRIES)
    got = _run(dev, h, W, lab, dt)
    names = [c[0] for c in calls]
    assert names == ["apertis_cross_entropy_fwd_bwd"] + ([] if one_pass else ["apertis_cross_entropy_fwd", "apertis_cross_entropy_bwd"])
    assert calls[0][1][8] == _vp(V, dt) == V + (_vn(dt) - 1)
    if not one_pass:
        assert calls[-1][1][0] == calls[-1][1][4] and calls[-1][1][7] == _vp(V, dt)
    _bounds(got, ref, dt, W)


# ---------------------------------------------------------------------------------------------------------------------------
# d. several chunks and the library's weight-gradient kernel
def test_two_chunks_on_the_library_weight_gradient_kernel(dev, monkeypatch, pad_on):
    """H = 704, V = 31999 (Vp = 32000: apertis_grouped_gemm_tn_dense_variant accepts it), three sequences in chunks of two: the
    first chunk writes the [Vp, H] fp32 sum, the second adds; the -inf fill runs for both (a reused buffer would hold the
    first backward's zeros)."""
    from apertis_llm_amd import ops
    lib, _, _ = _lib()
    dt, B, L, H, V = BF16, 3, 8, 704, 31999
    assert lib.apertis_grouped_gemm_tn_dense_variant(_vp(V, dt), H) >= 0
    monkeypatch.setattr(ops.loss, "_LCE_CHUNK_ROWS", 2 * L)
    h, W, lab = _inputs(V, dt, B=B, L=L, H=H, wstd=0.05)
    ref = _lce_ref(h, W, lab, dt, SCALE)
    calls = _spy(monkeypatch, lib, CE_ENTRIES + ("apertis_grouped_gemm_tn",))
    got = _run(dev, h, W, lab, dt)
    assert [c[0] for c in calls] == ["apertis_cross_entropy_fwd_bwd", "apertis_grouped_gemm_tn"] * 2
    assert [c[1][6] for c in calls if c[0] == "apertis_cross_entropy_fwd_bwd"] == [2, 1]
    tn = [c[1] for c in calls if c[0] == "apertis_grouped_gemm_tn"]
    assert [(a[5], a[6], a[7]) for a in tn] == [(2 * L, 32000, H), (L, 32000, H)] and tn[0][3] != tn[1][3]
    _bounds(got, ref, dt, W)


# ---------------------------------------------------------------------------------------------------------------------------
# e. an aligned V under the switch is today's path
@pytest.mark.parametrize("dt", [BF16, F32], ids=_tag)
def test_aligned_vocabulary_is_unchanged_by_the_switch(dev, monkeypatch, dt):
    """V = 512 with the switch on and off: the same launches with the same shapes, the same bits of loss, d hidden and d W."""
    from apertis_llm_amd import ops
    lib, _, _ = _lib()
    V = 512
    h, W, lab = _inputs(V, dt)
    calls = _spy(monkeypatch, lib, CE_ENTRIES + ("apertis_grouped_gemm_tn",))
    out = {}
    for on in (False, True):
        monkeypatch.setattr(ops.loss, "LCE_PAD_VOCAB", on)
        del calls[:]
        res = _run(dev, h, W, lab, dt)
        # (name and the shape arguments: B, L, V of the CE call, rows, M, N of the weight-gradient GEMM; pointers differ)
        out[on] = (res, [(name, a[5:8] if name == "apertis_grouped_gemm_tn" else a[6:9]) for name, a in calls])
    assert out[True][1] == out[False][1] and out[True][1][0] == ("apertis_cross_entropy_fwd_bwd", (2, 9, V))
    for a, b, name in zip(out[True][0], out[False][0], ("loss", "d hidden", "d W")):
        assert torch.equal(a, b), name + ": the switch changed an aligned vocabulary's bits"


# ---------------------------------------------------------------------------------------------------------------------------
# f. model level
@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16-autocast", "f32"])
def test_model_trains_an_odd_vocabulary_on_the_fused_path(dev, monkeypatch, dt):
    """A 2-layer selective_ssm ApertisForCausalLM with vocab_size = 1001 in training mode under fused_lm_head_loss: with the
    switch on the logits slot is None, and loss, the LM head's weight gradient and the first block's in_proj_x weight gradient
    match the same model's switch-off run (the stock branch: logits, F.cross_entropy) within the bounds above."""
    import contextlib
    import apertis_llm_amd as A
    from apertis_llm_amd import ops
    V = 1001
    torch.manual_seed(0)
    cfg = A.ApertisConfig(vocab_size=V, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                          attention_type="selective_ssm", use_expert_system=True, num_experts=4, hidden_dropout_prob=0.0,
                          attention_probs_dropout_prob=0.0, use_noisy_top_k_routing=False, use_expert_dropout=False)
    model = A.ApertisForCausalLM(cfg).to(dev).train()
    model.fused_lm_head_loss = True
    ids = torch.randint(4, V, (3, 40), device=dev)
    ids[0, 7] = V - 1
    labels = ids.clone()
    labels[1, :5] = -100
    head, block = model.lm_head.weight, model.model.layers[0].attention.attention_mechanism_impl.in_proj_x.weight

    def step(on):
        monkeypatch.setattr(ops.loss, "LCE_PAD_VOCAB", on, raising=False)
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16) if dt == BF16 else contextlib.nullcontext():
            out = model(input_ids=ids, labels=labels)
        out[0].backward()
        return out, head.grad.clone(), block.grad.clone()
    off, head_off, block_off = step(False)
    assert off[1] is not None and off[1].shape == (3, 40, V)
    on, head_on, block_on = step(True)
    assert on[1] is None and len(on) == 7, "an odd vocabulary under LCE_PAD_VOCAB takes the fused LM head + loss"
    ltol = 1e-5 if dt == F32 else 2e-3
    print(f"model {_tag(dt)}: loss {float(on[0]):.7f} against the stock branch's {float(off[0]):.7f}")
    assert abs(float(on[0]) - float(off[0])) <= ltol * max(1.0, abs(float(off[0]))), (float(on[0]), float(off[0]))
    rtol, asc = (1e-4, 1e-5) if dt == F32 else (3e-2, 2e-2)
    assert head_on.shape == (V, 128) and head_on.dtype == head_off.dtype
    _close(head_on, head_off, "grad lm_head.weight", rtol=rtol, atol_scale=asc)
    _close(block_on, block_off, "grad layers.0 in_proj_x.weight", rtol=rtol, atol_scale=asc)


# ---------------------------------------------------------------------------------------------------------------------------
# g. switch off keeps today
@pytest.mark.parametrize("dt", [BF16, F32], ids=_tag)
def test_switch_off_keeps_the_alignment_rule(dev, monkeypatch, dt):
    """V = 1001 with the switch off: not supported (the model takes the stock branch), and the op itself raises the library's
    error from the first CE entry point."""
    from apertis_llm_amd import ops
    monkeypatch.setattr(ops.loss, "LCE_PAD_VOCAB", False)
    V = 1001
    h, W, lab = _inputs(V, dt)
    assert not ops.linear_cross_entropy_supported(h.to(dev), W.to(dev), lab.to(dev))
    with pytest.raises(ops.ApertisHipError, match="not supported"):
        _run(dev, h, W, lab, dt)
    with torch.no_grad(), pytest.raises(ops.ApertisHipError, match="not supported"):
        _run(dev, h, W, lab, dt, grad=False)
