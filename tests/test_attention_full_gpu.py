"""Bidirectional attention (ops.full_attention, ops.full_attention_qkv; csrc/attention.hip with CAUSAL = false) against an
explicit fp64 softmax: every mask kind, both dtypes, dropout against the numpy restatement of the hash, determinism, a fully
masked sequence, the packed form, and that the causal instantiation is not what runs.

Shapes (D, L, B, H) are the smallest at which the kernels can go wrong: one row, less than one MFMA tile, one key tile plus one
key, exactly one work-group, the tower's 197 (three work-groups and a ragged tail), and 257 (one row into a fifth
work-group), at both head dims."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_error_report
from test_attention_gpu import NAMES, _fwd_bwd, _keep_mask, _zero_floor

pytestmark = pytest.mark.gpu

SHAPES = [(64, 1, 2, 3), (64, 5, 2, 3), (64, 33, 2, 2), (64, 64, 3, 2), (64, 197, 2, 3), (64, 257, 2, 2),
          (128, 1, 1, 2), (128, 31, 2, 1), (128, 197, 1, 2), (128, 257, 2, 2)]
MASKS = ["none", "right", "holes"]


def _mask(kind, B, L, dev):
    if kind == "none":
        return None
    kv = torch.ones(B, L, dtype=torch.long, device=dev)
    for b in range(B):
        if kind == "right":
            kv[b, max(1, (L * (b + 1)) // (B + 1)):] = 0        # right padding, a different length per sequence
        elif L > 1:                                             # holes: key 0 and scattered interior keys
            kv[b, 0] = 0
            kv[b, 3 + b::5 + b] = 0
            kv[b, L - 1] = 1                                    # every sequence keeps at least one key
    return kv


def _inputs(dev, B, L, H, D, dtype, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    return tuple(torch.randn(B, L, H * D, device=dev, generator=gen).to(dtype) for _ in range(4))


def _ref_full(q, k, v, H, key_valid=None, keep=None, p=0.0):
    """Explicit softmax over ALL keys in whatever dtype q has: [B, L, H*D] in and out."""
    B, L, W = q.shape
    D = W // H
    qh, kh, vh = (t.view(B, L, H, D).transpose(1, 2) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) * (1.0 / float(np.sqrt(np.float32(D))))
    if key_valid is not None:
        s = s.masked_fill(~key_valid.bool()[:, None, None, :], float("-inf"))
    pr = torch.softmax(s, dim=-1)
    if keep is not None:
        pr = pr * torch.as_tensor(keep, device=q.device).to(pr.dtype) / (1.0 - p)
    return (pr @ vh).transpose(1, 2).reshape(B, L, W)


def _ref64(q, k, v, do, H, kv, keep=None, p=0.0):
    return _fwd_bwd(lambda a, b, c: _ref_full(a, b, c, H, kv, keep, p), q.double(), k.double(), v.double(), do.double())


def _hold_fp32(name, got, ref, v, do):
    for n, g_, r in zip(NAMES, got, ref):
        if float(r.abs().max()) == 0.0:
            # (dQ at L = 1 is exactly zero: P (dP - rowsum(dO*O)) cancels, to the summation order of two fp32 dot products)
            rep = rel_error_report(f"{name} {n}", g_, r, check=False)
            assert rep["max_abs"] <= _zero_floor(v, do), rep
        else:
            rel_error_report(f"{name} {n}", g_, r, rtol=1e-4)


@pytest.mark.parametrize("D,L,B,H", SHAPES)
@pytest.mark.parametrize("mask", MASKS)
def test_full_attention_fp32_matches_fp64(dev, D, L, B, H, mask):
    from apertis_llm_amd import ops
    q, k, v, do = _inputs(dev, B, L, H, D, torch.float32, 11 + L + D)
    kv = _mask(mask, B, L, dev)
    got = _fwd_bwd(lambda a, b, c: ops.full_attention(a, b, c, H, kv), q, k, v, do)
    _hold_fp32(f"full attention fp32 D{D} L{L} B{B} H{H} {mask}", got, _ref64(q, k, v, do, H, kv), v, do)


@pytest.mark.parametrize("D,L,B,H", SHAPES)
@pytest.mark.parametrize("mask", MASKS)
def test_full_attention_bf16_within_twice_stock_sdpa_error(dev, D, L, B, H, mask):
    """The project's bf16 rule (no absolute bound has been measured): the kernel's max error against fp64 is at most twice that
    of stock bf16 SDPA on the same inputs, plus 1e-6 of the reference's magnitude (and _zero_floor for dQ at L = 1, exactly
    zero)."""
    from apertis_llm_amd import ops
    q, k, v, do = _inputs(dev, B, L, H, D, torch.bfloat16, 23 + L + D)
    kv = _mask(mask, B, L, dev)
    allow = None if kv is None else kv.bool()[:, None, None, :].expand(B, 1, L, L)

    def stock(a, b, c):
        ah, bh, ch = (t.view(B, L, H, D).transpose(1, 2) for t in (a, b, c))
        return F.scaled_dot_product_attention(ah, bh, ch, attn_mask=allow).transpose(1, 2).reshape(B, L, H * D)
    got = _fwd_bwd(lambda a, b, c: ops.full_attention(a, b, c, H, kv), q, k, v, do)
    base = _fwd_bwd(stock, q, k, v, do)
    ref = _ref64(q, k, v, do, H, kv)
    for n, g_, s_, r in zip(NAMES, got, base, ref):
        rep = rel_error_report(f"full attention bf16 D{D} L{L} B{B} H{H} {mask} {n}", g_, r, check=False)
        srep = rel_error_report(f"stock SDPA bf16 (non-causal) D{D} L{L} B{B} H{H} {mask} {n}", s_, r, check=False)
        assert rep["max_abs"] <= 2 * srep["max_abs"] + 1e-6 * rep["ref_absmax"] + \
            (_zero_floor(v, do) if rep["ref_absmax"] == 0.0 else 0.0), (n, rep, srep)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_full_attention_dropout_mask_matches_numpy_hash(dev, dtype):
    from apertis_llm_amd import ops
    B, L, H, D, p, seed = 2, 200, 2, 64, 0.1, 0x1234_5678_9abc
    q, k, v, do = _inputs(dev, B, L, H, D, dtype, 5)
    kv = _mask("holes", B, L, dev)
    keep = _keep_mask(seed, B, H, L, p)
    fn = lambda a, b, c: ops.attention._Attention.apply("full", a, b, c, H, kv, p, seed)     # noqa: E731
    got = _fwd_bwd(fn, q, k, v, do)
    ref = _ref64(q, k, v, do, H, kv, keep, p)
    if dtype == torch.float32:
        for n_, g_, r in zip(NAMES, got, ref):
            rel_error_report(f"full attention dropout fp32 {n_}", g_, r, rtol=1e-4)
    else:
        base = _fwd_bwd(lambda a, b, c: _ref_full(a, b, c, H, kv, keep, p), q, k, v, do)   # the same math in bf16
        for n_, g_, s_, r in zip(NAMES, got, base, ref):
            rep = rel_error_report(f"full attention dropout bf16 {n_}", g_, r, check=False)
            srep = rel_error_report(f"explicit bf16 dropout (non-causal) {n_}", s_, r, check=False)
            assert rep["max_abs"] <= 2 * srep["max_abs"] + 1e-6 * rep["ref_absmax"], (n_, rep, srep)
    # same seed: the same bits; another seed: another mask
    again = _fwd_bwd(fn, q, k, v, do)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    other = _fwd_bwd(lambda a, b, c: ops.attention._Attention.apply("full", a, b, c, H, kv, p, seed + 1), q, k, v, do)
    assert not torch.equal(got[0], other[0])
    # the public op draws its seed from torch's RNG, and only in training
    torch.manual_seed(7)
    a = ops.full_attention(q, k, v, H, kv, 0.3, training=True)
    torch.manual_seed(7)
    b = ops.full_attention(q, k, v, H, kv, 0.3, training=True)
    c = ops.full_attention(q, k, v, H, kv, 0.3, training=True)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert torch.equal(ops.full_attention(q, k, v, H, kv, 0.3, training=False), ops.full_attention(q, k, v, H, kv))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_full_attention_backward_is_deterministic(dev, dtype):
    from apertis_llm_amd import ops
    B, L, H, D = 2, 257, 2, 64
    q, k, v, do = _inputs(dev, B, L, H, D, dtype, 9)
    kv = _mask("holes", B, L, dev)
    fn = lambda a, b, c: ops.attention._Attention.apply("full", a, b, c, H, kv, 0.1, 99)     # noqa: E731
    runs = [_fwd_bwd(fn, q, k, v, do) for _ in range(3)]
    assert all(torch.equal(a, b) for r in runs[1:] for a, b in zip(runs[0], r))


@pytest.mark.parametrize("D", [64, 128])
def test_fully_masked_sequence_is_zeros_and_the_others_are_right(dev, D):
    """One sequence of three without a single valid key: its O rows and its dQ, dK, dV are exactly zero (no NaN from the
    +inf LSE), and the two other sequences - one unmasked, one with holes - meet the fp64 bar."""
    from apertis_llm_amd import ops
    B, L, H = 3, 70, 2
    q, k, v, do = _inputs(dev, B, L, H, D, torch.float32, 31 + D)
    kv = torch.ones(B, L, dtype=torch.long, device=dev)
    kv[1] = 0
    kv[2] = _mask("holes", 1, L, dev)[0]
    got = _fwd_bwd(lambda a, b, c: ops.full_attention(a, b, c, H, kv), q, k, v, do)
    for n, g_ in zip(NAMES, got):
        assert torch.isfinite(g_).all(), n
        assert torch.equal(g_[1], torch.zeros_like(g_[1])), n
    live = [0, 2]
    ref = _ref64(q[live], k[live], v[live], do[live], H, kv[live])
    _hold_fp32(f"full attention fp32 D{D} beside a fully masked sequence", [g_[live] for g_ in got], ref, v, do)
    gb = _fwd_bwd(lambda a, b, c: ops.full_attention(a, b, c, H, kv), *(t.bfloat16() for t in (q, k, v, do)))
    assert all(torch.isfinite(g_).all() and torch.equal(g_[1], torch.zeros_like(g_[1])) for g_ in gb)


@pytest.mark.parametrize("dtype,D,L", [(torch.float32, 64, 197), (torch.bfloat16, 64, 197), (torch.bfloat16, 128, 33)])
def test_packed_form_is_bit_identical_and_returns_one_gradient(dev, dtype, D, L):
    from apertis_llm_amd import ops
    B, H = 2, 3
    W = H * D
    gen = torch.Generator(device=dev).manual_seed(77)
    qkv = torch.randn(B, L, 3 * W, device=dev, generator=gen).to(dtype).requires_grad_()
    do = torch.randn(B, L, W, device=dev, generator=gen).to(dtype)
    timer = ops.KernelTimer(["apertis_attention_full_fwd", "apertis_attention_full_bwd"])
    for p in (0.0, 0.1):
        ops.set_kernel_timer(timer)
        try:
            torch.manual_seed(3)
            o = ops.full_attention_qkv(qkv, H, p, training=True)
            (d,) = torch.autograd.grad(o, (qkv,), do)
        finally:
            ops.set_kernel_timer(None)
        assert d.shape == qkv.shape and d.is_contiguous() and d.dtype == dtype
        parts = [qkv.detach()[..., i * W:(i + 1) * W].contiguous() for i in range(3)]
        torch.manual_seed(3)
        ref = _fwd_bwd(lambda a, b, c: ops.full_attention(a, b, c, H, None, p, training=True), *parts, do)
        assert torch.equal(o.detach(), ref[0])
        for i, n in enumerate(("dQ", "dK", "dV")):
            assert torch.equal(d[..., i * W:(i + 1) * W], ref[1 + i]), (n, p)
    s = timer.summary()
    assert s["apertis_attention_full_fwd"]["launches"] == 2 and s["apertis_attention_full_bwd"]["launches"] == 2
    assert s["apertis_attention_full_fwd"]["work"] == 2 * 4.0 * B * H * D * L * L
    assert s["apertis_attention_full_bwd"]["work"] == 2 * 2.5 * 4.0 * B * H * D * L * L


def test_it_is_not_the_causal_kernel(dev):
    """(64, 33, 2, 2), no mask: only the LAST query of a sequence sees the same keys under both forms - there the two agree
    within the fp32 bar, and every other row differs."""
    from apertis_llm_amd import ops
    D, L, B, H = 64, 33, 2, 2
    q, k, v, _ = _inputs(dev, B, L, H, D, torch.float32, 41)
    full = ops.full_attention(q, k, v, H)
    causal = ops.causal_attention(q, k, v, H)
    differs = (full != causal).any(dim=-1)                       # [B, L]
    assert bool(differs[:, :L - 1].all()), differs
    rel_error_report("full vs causal attention, last row", full[:, L - 1], causal[:, L - 1].double(), rtol=1e-4)
