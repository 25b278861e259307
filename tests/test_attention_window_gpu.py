"""Sliding-window causal attention on the GPU: ops.window_attention and the entry points apertis_attention_window_fwd / _bwd.

The tile geometry is 16 rows per wave, 32-key tiles and 64 rows per work-group; L = 200 with W in {1, 16, 17, 32, 33, 65, 199}
puts the window's edge inside a tile, on a tile boundary, on a wave boundary and across work-groups; L = 1 and 7 are rows
shorter than every tile.  Three yardsticks: the document kernels fed ops.window_layout's arrays (bit for bit: a skipped tile
adds exact zeros), the causal kernels at window >= L (bit for bit) and an fp64 explicit softmax under the band mask."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_error_report

pytestmark = pytest.mark.gpu

B, H = 2, 2
LENGTHS = (1, 7, 200)
WINDOWS = (1, 16, 17, 32, 33, 65, 199)
NAMES = ("O", "dQ", "dK", "dV")
PAD = 37                                                     # row 1 is left-padded by this many keys (L - 1 when shorter)


def _inputs(dev, L, D, dtype, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    return tuple(torch.randn(B, L, H * D, device=dev, generator=gen).to(dtype) for _ in range(4))


def _key_valid(dev, L):
    kv = torch.ones(B, L, dtype=torch.long, device=dev)
    kv[1, :min(PAD, L - 1)] = 0
    return kv


def _allow(dev, L, W, kv=None):
    """[B, 1, L, L] bool: key j counts for query i."""
    i, j = torch.arange(L, device=dev)[:, None], torch.arange(L, device=dev)[None, :]
    allow = ((j <= i) & (i - j < W))[None].expand(B, L, L)
    if kv is not None:
        allow = allow & kv.bool()[:, None, :]
    return allow[:, None]


def _ref_attention(q, k, v, allow):
    """Explicit softmax in whatever dtype q has: [B, L, H*D] in and out; a row with no key is zero (what the kernels write)."""
    L, W = q.shape[1:]
    D = W // H
    qh, kh, vh = (t.view(B, L, H, D).transpose(1, 2) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) * (1.0 / float(np.sqrt(np.float32(D))))
    pr = torch.softmax(s.masked_fill(~allow, float("-inf")), dim=-1)
    pr = torch.where(allow.any(-1, keepdim=True), pr, torch.zeros_like(pr))
    return (pr @ vh).transpose(1, 2).reshape(B, L, W)


def _fwd_bwd(fn, q, k, v, do):
    q, k, v = (t.detach().clone().requires_grad_() for t in (q, k, v))
    o = fn(q, k, v)
    grads = torch.autograd.grad(o, (q, k, v), do)
    return (o.detach(), *grads)


def _zero_floor(v, do):
    """Absolute bound for a product whose exact value is zero: 1e-5 of the size of one dP = dO . V term."""
    return 1e-5 * float(v.abs().max().float() * do.abs().max().float()) * v.shape[-1] ** 0.5


# ------------------------------------------------------------------------------- against the document kernels, bit for bit
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("D", [64, 128])
def test_window_attention_has_the_document_kernels_bits(dev, D, dtype):
    """Every (L, W), with and without key_valid, with and without dropout p = 0.1 under the same torch seed: O, dQ, dK, dV of
    the window form are torch.equal to the document form on ops.window_layout's arrays."""
    from apertis_llm_amd import ops
    for L in LENGTHS:
        q, k, v, do = _inputs(dev, L, D, dtype, 11 + L + D)
        for W in WINDOWS:
            layout = ops.window_layout((B, L), W, dev)
            for kv in (None, _key_valid(dev, L)):
                for p in (0.0, 0.1):
                    torch.manual_seed(5)
                    got = _fwd_bwd(lambda a, b, c: ops.window_attention(a, b, c, H, W, kv, p, training=True), q, k, v, do)
                    torch.manual_seed(5)
                    want = _fwd_bwd(lambda a, b, c: ops.document_attention(a, b, c, H, layout, kv, p, training=True), q, k, v, do)
                    for n, g_, w in zip(NAMES, got, want):
                        assert torch.equal(g_, w), (n, L, W, kv is not None, p)
                    assert bool(got[0].any()) and not bool(torch.isnan(got[0]).any())


# ----------------------------------------------------------------------------------- against the causal kernels, bit for bit
def _raw(window, q, k, v, do, kv, p=0.0, seed=0):
    """(rc, O, LSE, dQ, dK, dV) straight from the entry points: the causal pair (window None) or the window pair; outputs
    start out as sevens."""
    from apertis_llm_amd import _lib
    lib, ptr = _lib.load(), _lib.ptr
    L, W = q.shape[1:]
    D, dt, st = W // H, _lib.dtype_code(q), _lib.stream_ptr()
    out, lse = torch.full_like(q, 7.0), torch.full((B, H, L), 7.0, device=q.device)
    dq, dk, dv = torch.full_like(q, 7.0), torch.full_like(q, 7.0), torch.full_like(q, 7.0)
    ws = torch.zeros(B * H * L, device=q.device, dtype=torch.float32)
    extra = () if window is None else (window,)
    fwd = lib.apertis_attention_fwd if window is None else lib.apertis_attention_window_fwd
    bwd = lib.apertis_attention_bwd if window is None else lib.apertis_attention_window_bwd
    rc_f = fwd(ptr(q), W, ptr(k), W, ptr(v), W, ptr(kv), *extra, ptr(out), W, ptr(lse), B, L, H, D, p, seed, dt, st)
    rc_b = bwd(ptr(q), W, ptr(k), W, ptr(v), W, ptr(out), W, ptr(do), W, ptr(lse), ptr(kv), *extra, ptr(ws), ptr(dq), ptr(dk),
               ptr(dv), W, B, L, H, D, p, seed, dt, st)
    torch.cuda.synchronize()
    return (rc_f, rc_b), out, lse, dq, dk, dv


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("D", [64, 128])
def test_a_window_of_the_whole_row_has_the_causal_kernels_bits(dev, D, dtype):
    """The raw entry points (the op's callers never reach them with window >= L): window = L and window = 2**40 add a
    predicate that is true everywhere and bounds that are the causal loops', so every bit is apertis_attention_fwd / _bwd's.
    2**63 - 1 as well: the comparisons are 64-bit and cannot wrap."""
    for L in LENGTHS:
        q, k, v, do = _inputs(dev, L, D, dtype, 23 + L + D)
        for kv in (None, _key_valid(dev, L)):
            for p in (0.0, 0.1):
                want = _raw(None, q, k, v, do, kv, p, 99)
                assert want[0] == (0, 0)
                for W in (L, 2 ** 40, 2 ** 63 - 1):
                    got = _raw(W, q, k, v, do, kv, p, 99)
                    assert got[0] == (0, 0)
                    for n, g_, w in zip(("O", "LSE") + NAMES[1:], got[1:], want[1:]):
                        assert torch.equal(g_, w), (n, L, W, kv is not None, p)


# ------------------------------------------------------------------------------------------------------------ against fp64
@pytest.mark.parametrize("D", [64, 128])
def test_window_attention_fp32_matches_fp64(dev, D):
    from apertis_llm_amd import ops
    for L in LENGTHS:
        q, k, v, do = _inputs(dev, L, D, torch.float32, 31 + L + D)
        for W in WINDOWS:
            for kv in (None, _key_valid(dev, L)):
                allow = _allow(dev, L, W, kv)
                got = _fwd_bwd(lambda a, b, c: ops.window_attention(a, b, c, H, W, kv), q, k, v, do)
                ref = _fwd_bwd(lambda a, b, c: _ref_attention(a, b, c, allow), q.double(), k.double(), v.double(), do.double())
                for n, g_, r in zip(NAMES, got, ref):
                    name = f"window attention fp32 D{D} L{L} W{W} kv{int(kv is not None)} {n}"
                    if float(r.abs().max()) == 0.0:                 # (dQ when every query sees one key: W = 1, L = 1)
                        rep = rel_error_report(name, g_, r, check=False)
                        assert rep["max_abs"] <= _zero_floor(v, do), rep
                    else:
                        rel_error_report(name, g_, r, rtol=1e-4)


@pytest.mark.parametrize("D", [64, 128])
def test_window_attention_bf16_within_twice_stock_sdpa_error(dev, D):
    """The kernel's max error against fp64 is held to twice that of stock bf16 SDPA given the same band as an ADDITIVE mask
    (plus 1e-6 of the reference's magnitude, and _zero_floor where the reference is zero).  Under key_valid the query rows
    in front of row 1's first valid key have no key: the kernels write zeros there and an additive mask makes them uniform
    rows, so their incoming gradient is zeroed and their output left out - nothing else depends on them."""
    from apertis_llm_amd import ops
    lo = torch.finfo(torch.bfloat16).min
    for L in LENGTHS:
        q, k, v, do = _inputs(dev, L, D, torch.bfloat16, 47 + L + D)
        for W in WINDOWS:
            for kv in (None, _key_valid(dev, L)):
                allow = _allow(dev, L, W, kv)
                live = allow.any(-1)[:, 0, :, None]                                              # [B, L, 1]
                do_ = do * live
                additive = torch.zeros(allow.shape, device=dev, dtype=torch.bfloat16).masked_fill_(~allow, lo)

                def stock(a, b, c):
                    ah, bh, ch = (t.view(B, L, H, D).transpose(1, 2) for t in (a, b, c))
                    return F.scaled_dot_product_attention(ah, bh, ch, attn_mask=additive).transpose(1, 2).reshape(B, L, H * D)
                got = _fwd_bwd(lambda a, b, c: ops.window_attention(a, b, c, H, W, kv), q, k, v, do_)
                base = _fwd_bwd(stock, q, k, v, do_)
                ref = _fwd_bwd(lambda a, b, c: _ref_attention(a, b, c, allow), q.double(), k.double(), v.double(), do_.double())
                base = (base[0] * live, *base[1:])
                for n, g_, s_, r in zip(NAMES, got, base, ref):
                    tag = f"bf16 D{D} L{L} W{W} kv{int(kv is not None)} {n}"
                    rep = rel_error_report(f"window attention {tag}", g_, r, check=False)
                    srep = rel_error_report(f"stock SDPA band mask {tag}", s_, r, check=False)
                    assert rep["max_abs"] <= 2 * srep["max_abs"] + 1e-6 * rep["ref_absmax"] + \
                        (_zero_floor(v, do) if rep["ref_absmax"] == 0.0 else 0.0), (tag, rep, srep)


# ------------------------------------------------------------------------------------------------------------- locality
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_a_key_reaches_the_window_after_it_and_nothing_else(dev, dtype):
    from apertis_llm_amd import ops
    L, D = 200, 64
    q, k, v, do = _inputs(dev, L, D, dtype, 77)
    for W in (1, 17, 32, 65):
        o = ops.window_attention(q, k, v, H, W)
        for j in (0, 15, 31, 64, 130, L - 1):
            k2, v2 = k.clone(), v.clone()
            k2[:, j] = k2[:, j] * 3 + 1
            v2[:, j] = v2[:, j] * 3 + 1
            o2 = ops.window_attention(q, k2, v2, H, W)
            inside = torch.zeros(L, dtype=torch.bool, device=dev)
            inside[j:j + W] = True
            assert torch.equal(o2[:, ~inside], o[:, ~inside]), (W, j)
            assert not torch.equal(o2[:, j], o[:, j]) and not torch.equal(o2[:, min(j + W, L) - 1], o[:, min(j + W, L) - 1]), (W, j)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_dk_dv_do_not_depend_on_queries_past_the_window(dev, dtype):
    """Queries (and their incoming gradient) at or past row t change: dK[j], dV[j] keep their bits for every j + W <= t."""
    from apertis_llm_amd import ops
    L, D = 200, 64
    q, k, v, do = _inputs(dev, L, D, dtype, 78)
    for W in (1, 17, 32, 65):
        got = _fwd_bwd(lambda a, b, c: ops.window_attention(a, b, c, H, W), q, k, v, do)
        for t in (W, 70, 131, L - 1):
            q2, do2 = q.clone(), do.clone()
            q2[:, t:] = q2[:, t:] * 2 - 1
            do2[:, t:] = do2[:, t:] * 2 - 1
            oth = _fwd_bwd(lambda a, b, c: ops.window_attention(a, b, c, H, W), q2, k, v, do2)
            keep = t - W + 1                                  # keys 0 .. t - W see no changed query
            for n in (2, 3):
                assert torch.equal(oth[n][:, :keep], got[n][:, :keep]), (NAMES[n], W, t)
                if n == 3 or W > 1:                           # (dK under W = 1 is exactly zero: P = 1, dS = 0)
                    assert not torch.equal(oth[n][:, keep:t + 1], got[n][:, keep:t + 1]), (NAMES[n], W, t)


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_outputs_untouched(dev):
    from apertis_llm_amd import ops
    L = 7
    for D, dtype, window, want in ((64, torch.float32, 0, -1), (64, torch.float32, -5, -1), (128, torch.bfloat16, 0, -1),
                                   (32, torch.float32, 3, -2)):
        q = torch.randn(B, L, H * D, device=dev).to(dtype)
        rc, *outs = _raw(window, q, q, q, q, None)
        assert rc == (want, want)
        assert all(bool((t == 7.0).all()) for t in outs)
    x = torch.zeros(B, L, H * 64, device=dev)
    for bad in (0, -1, 2.0, None):
        with pytest.raises(ValueError):
            ops.window_attention(x, x, x, H, bad)
    with pytest.raises(ops.ApertisHipError):                 # key_valid of another shape
        ops.window_attention(x, x, x, H, 3, torch.ones(B, L + 1, dtype=torch.long, device=dev))
    x32 = torch.zeros(B, L, H * 32, device=dev)
    with pytest.raises(ops.ApertisHipError):                 # head dim 32
        ops.window_attention(x32, x32, x32, H, 3)
    x16 = x.half()
    with pytest.raises(ops.ApertisHipError):
        ops.window_attention(x16, x16, x16, H, 3)
    with pytest.raises(ops.ApertisHipError):                 # dead_rows is inference only
        ops.window_attention(x.requires_grad_(), x, x, H, 3, torch.ones(B, L, dtype=torch.long, device=dev), dead_rows=True)


def test_dead_rows_are_filled_as_the_causal_form_fills_them(dev):
    """Left padding under the window: a query row with no valid key at or before it gets the column mean of v (inference
    only), every other row keeps its bits."""
    from apertis_llm_amd import ops
    L, D, W = 200, 64, 33
    q, k, v, _ = _inputs(dev, L, D, torch.float32, 91)
    kv = _key_valid(dev, L)
    plain = ops.window_attention(q, k, v, H, W, kv)
    filled = ops.window_attention(q, k, v, H, W, kv, dead_rows=True)
    assert not bool(plain[1, :PAD].any()) and torch.equal(filled[0], plain[0]) and torch.equal(filled[1, PAD:], plain[1, PAD:])
    want = ops.causal_attention(q, k, v, H, kv, dead_rows=True)[1, :PAD]
    assert torch.equal(filled[1, :PAD], want)


# --------------------------------------------------------------------------------------------------- launch accounting
def test_the_window_form_launches_its_own_pair_and_counts_its_own_work(dev):
    from apertis_llm_amd import ops
    D, L, W = 64, 97, 40
    names = [n for form in ops.attention._FORMS.values() for n in form[:2]]
    assert len(names) == 8
    q, k, v, do = _inputs(dev, L, D, torch.float32, 3)
    timer = ops.KernelTimer(names)
    ops.set_kernel_timer(timer)
    try:
        _fwd_bwd(lambda a, b, c: ops.window_attention(a, b, c, H, W), q, k, v, do)
    finally:
        ops.set_kernel_timer(None)
    s = timer.summary()
    pairs = sum(min(i + 1, W) for i in range(L))
    assert ops.window_pairs(L, W) == pairs
    fwd_work = 4.0 * B * H * D * pairs
    assert {n: r["launches"] for n, r in s.items()} == {"apertis_attention_window_fwd": 1, "apertis_attention_window_bwd": 1}
    assert s["apertis_attention_window_fwd"]["work"] == fwd_work and s["apertis_attention_window_bwd"]["work"] == 2.5 * fwd_work


# ------------------------------------------------------------------------------------------------------- decode window
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_attention_decode_reads_the_last_window_rows_only(dev, dtype):
    """attention_decode(window=W) with Lk > W: the bits of the same call on a cache that holds the last W rows only, with
    the launch seeing Lk = W; rows in front of the window may hold anything (NaN here).  Lk <= W: the call without a window."""
    from apertis_llm_amd import ops
    D, cap, Lk, W = 64, 96, 80, 33
    width = H * D
    gen = torch.Generator(device=dev).manual_seed(4)
    kc, vc, q = (torch.randn(*s, device=dev, generator=gen).to(dtype) for s in ((B, cap, width), (B, cap, width), (B, width)))
    kv = torch.ones(B, Lk, dtype=torch.long, device=dev)
    kv[1, :60] = 0
    cache = ops.KVCache([kc.clone()], [vc.clone()], Lk)
    cache.k[0][:, :Lk - W] = float("nan")
    cache.v[0][:, :Lk - W] = float("nan")
    short = ops.KVCache([kc[:, Lk - W:].contiguous()], [vc[:, Lk - W:].contiguous()], W)
    for mask in (None, kv):
        want = ops.attention_decode(q, short, 0, H, None if mask is None else mask[:, Lk - W:].contiguous())
        timer = ops.KernelTimer(["apertis_attention_decode"])
        ops.set_kernel_timer(timer)
        try:
            got = ops.attention_decode(q, cache, 0, H, mask, window=W)
        finally:
            ops.set_kernel_timer(None)
        assert torch.equal(got, want) and not bool(torch.isnan(got).any())
        assert timer.summary()["apertis_attention_decode"]["work"] == 4.0 * B * W * width
        assert torch.equal(ops.attention_decode(q, short, 0, H, None, window=W), ops.attention_decode(q, short, 0, H))
    with pytest.raises(ValueError):
        ops.attention_decode(q, short, 0, H, window=0)
