"""Document-masked causal attention (packed rows) on the GPU: ops.document_layout / ops.document_attention and the entry
points apertis_attention_doc_fwd / _bwd against an fp64 explicit softmax under the block-diagonal causal mask.

Layouts are document lengths per row, chosen so that boundaries fall inside a 32-key tile, on a tile edge, on a 64-row
work-group edge, with documents of one token and with documents that span several work-groups."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_error_report

pytestmark = pytest.mark.gpu

LAYOUTS = {
    257: ([257], [1, 31, 32, 33, 64, 96]),
    97: ([5, 92], [96, 1], [40, 17, 40]),
    512: ([200, 312], [300, 1, 211]),
    7: ([3, 4], [7]),
    1: ([1],),
}
CASES = [(L, D, 2 + (L + D // 64) % 2) for L in LAYOUTS for D in (64, 128)]        # heads 2 or 3
NAMES = ("O", "dQ", "dK", "dV")


def _doc_ids(L, dev):
    rows = []
    for lens in LAYOUTS[L]:
        assert sum(lens) == L
        rows.append(torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens)))
    return torch.stack(rows).to(dev)


def _allow(ids, key_valid=None):
    """[B, 1, L, L] bool: key j counts for query i."""
    L = ids.shape[1]
    allow = torch.ones(L, L, dtype=torch.bool, device=ids.device).tril()[None] & (ids[:, :, None] == ids[:, None, :])
    if key_valid is not None:
        allow = allow & key_valid.bool()[:, None, :]
    return allow[:, None]


def _ref_attention(q, k, v, H, allow, keep=None, p=0.0):
    """Explicit softmax in whatever dtype q has: [B, L, H*D] in and out."""
    B, L, W = q.shape
    D = W // H
    qh, kh, vh = (t.view(B, L, H, D).transpose(1, 2) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) * (1.0 / float(np.sqrt(np.float32(D))))
    pr = torch.softmax(s.masked_fill(~allow, float("-inf")), dim=-1)
    if keep is not None:
        pr = pr * torch.as_tensor(keep, device=q.device).to(pr.dtype) / (1.0 - p)
    return (pr @ vh).transpose(1, 2).reshape(B, L, W)


def _inputs(dev, B, L, H, D, dtype, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    return tuple(torch.randn(B, L, H * D, device=dev, generator=gen).to(dtype) for _ in range(4))


def _fwd_bwd(fn, q, k, v, do):
    q, k, v = (t.detach().clone().requires_grad_() for t in (q, k, v))
    o = fn(q, k, v)
    grads = torch.autograd.grad(o, (q, k, v), do)
    return (o.detach(), *grads)


def _zero_floor(v, do):
    """Absolute bound for a product whose exact value is zero: 1e-5 of the size of one dP = dO . V term."""
    return 1e-5 * float(v.abs().max().float() * do.abs().max().float()) * v.shape[-1] ** 0.5


@pytest.mark.parametrize("L,D,H", CASES)
def test_document_attention_fp32_matches_fp64(dev, L, D, H):
    from apertis_llm_amd import ops
    ids = _doc_ids(L, dev)
    B = ids.shape[0]
    q, k, v, do = _inputs(dev, B, L, H, D, torch.float32, 31 + L + D)
    layout, allow = ops.document_layout(ids), _allow(ids)
    got = _fwd_bwd(lambda a, b, c: ops.document_attention(a, b, c, H, layout), q, k, v, do)
    ref = _fwd_bwd(lambda a, b, c: _ref_attention(a, b, c, H, allow), q.double(), k.double(), v.double(), do.double())
    for n, g_, r in zip(NAMES, got, ref):
        name = f"document attention fp32 D{D} L{L} B{B} H{H} {n}"
        if float(r.abs().max()) == 0.0:                       # (dQ when every document has one token)
            rep = rel_error_report(name, g_, r, check=False)
            assert rep["max_abs"] <= _zero_floor(v, do), rep
        else:
            rel_error_report(name, g_, r, rtol=1e-4)
    # dQ of a one-token document is exactly zero (P (dP - rowsum(dO*O)) cancels): held to the zero floor on its own
    single = (layout.end - layout.start) == 1
    if bool(single.any()):
        assert float(got[1][single].abs().max()) <= _zero_floor(v, do)


@pytest.mark.parametrize("L,D,H", CASES)
def test_document_attention_bf16_within_twice_stock_sdpa_error(dev, L, D, H):
    """No absolute bf16 bound has been measured: the kernel's max error against fp64 is held to twice that of stock bf16
    SDPA under the same boolean mask (plus 1e-6 of the reference's magnitude, and _zero_floor where the reference is zero)."""
    from apertis_llm_amd import ops
    ids = _doc_ids(L, dev)
    B = ids.shape[0]
    q, k, v, do = _inputs(dev, B, L, H, D, torch.bfloat16, 47 + L + D)
    layout, allow = ops.document_layout(ids), _allow(ids)

    def stock(a, b, c):
        ah, bh, ch = (t.view(B, L, H, D).transpose(1, 2) for t in (a, b, c))
        return F.scaled_dot_product_attention(ah, bh, ch, attn_mask=allow).transpose(1, 2).reshape(B, L, H * D)
    got = _fwd_bwd(lambda a, b, c: ops.document_attention(a, b, c, H, layout), q, k, v, do)
    base = _fwd_bwd(stock, q, k, v, do)
    ref = _fwd_bwd(lambda a, b, c: _ref_attention(a, b, c, H, allow), q.double(), k.double(), v.double(), do.double())
    for n, g_, s_, r in zip(NAMES, got, base, ref):
        rep = rel_error_report(f"document attention bf16 D{D} L{L} B{B} H{H} {n}", g_, r, check=False)
        srep = rel_error_report(f"stock SDPA bf16 doc mask D{D} L{L} B{B} H{H} {n}", s_, r, check=False)
        assert rep["max_abs"] <= 2 * srep["max_abs"] + 1e-6 * rep["ref_absmax"] + \
            (_zero_floor(v, do) if rep["ref_absmax"] == 0.0 else 0.0), (n, rep, srep)


# ------------------------------------------------------------------------------------------------ one document per row
def _raw(ops, doc, q, k, v, do, H, kv, layout):
    """(O, LSE, dQ, dK, dV) straight from the entry points: the causal pair (doc=False) or the document pair."""
    from apertis_llm_amd import _lib
    lib, ptr = _lib.load(), _lib.ptr
    B, L, W = q.shape
    D, dt, st = W // H, _lib.dtype_code(q), _lib.stream_ptr()
    out, lse = torch.empty_like(q), torch.empty(B, H, L, device=q.device, dtype=torch.float32)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
    ws = torch.empty(B * H * L, device=q.device, dtype=torch.float32)
    extra = (ptr(layout.start), ptr(layout.end)) if doc else ()
    fwd = lib.apertis_attention_doc_fwd if doc else lib.apertis_attention_fwd
    bwd = lib.apertis_attention_doc_bwd if doc else lib.apertis_attention_bwd
    assert fwd(ptr(q), W, ptr(k), W, ptr(v), W, ptr(kv), *extra, ptr(out), W, ptr(lse), B, L, H, D, 0.0, 0, dt, st) == 0
    assert bwd(ptr(q), W, ptr(k), W, ptr(v), W, ptr(out), W, ptr(do), W, ptr(lse), ptr(kv), *extra, ptr(ws), ptr(dq), ptr(dk),
               ptr(dv), W, B, L, H, D, 0.0, 0, dt, st) == 0
    return out, lse, dq, dk, dv


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("L,D", [(257, 64), (97, 128), (7, 64), (1, 128)])
def test_one_document_per_row_has_the_causal_kernels_bits(dev, dtype, padded, L, D):
    """The arithmetic per element is the same sequence and the added predicate is true everywhere."""
    from apertis_llm_amd import ops
    B, H = 2, 3
    q, k, v, do = _inputs(dev, B, L, H, D, dtype, 5 + L)
    kv = None
    if padded:
        kv = torch.ones(B, L, dtype=torch.long, device=dev)
        kv[1, max(1, (2 * L) // 3):] = 0
    layout = ops.document_layout(torch.zeros(B, L, dtype=torch.long, device=dev))
    assert int(layout.start.max()) == 0 and int(layout.end.min()) == L
    want = _raw(ops, False, q, k, v, do, H, kv, None)
    got = _raw(ops, True, q, k, v, do, H, kv, layout)
    for n, g_, w in zip(("O", "LSE", "dQ", "dK", "dV"), got, want):
        assert torch.equal(g_, w), n
    # and through the ops
    a = _fwd_bwd(lambda x, y, z: ops.document_attention(x, y, z, H, layout, kv), q, k, v, do)
    b = _fwd_bwd(lambda x, y, z: ops.causal_attention(x, y, z, H, kv), q, k, v, do)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ independence
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_documents_do_not_see_each_other(dev, dtype):
    from apertis_llm_amd import ops
    L, H, D = 257, 2, 64
    ids = _doc_ids(L, dev)[1:]                               # [1, 31, 32, 33, 64, 96]
    layout = ops.document_layout(ids)
    q, k, v, do = _inputs(dev, 1, L, H, D, dtype, 77)
    o = ops.document_attention(q, k, v, H, layout)
    for d in range(6):
        sel = (ids[0] == d)
        q2, k2, v2 = (t.clone() for t in (q, k, v))
        for t in (q2, k2, v2):
            t[0, sel] = t[0, sel] * 3 + 1
        o2 = ops.document_attention(q2, k2, v2, H, layout)
        assert torch.equal(o2[0, ~sel], o[0, ~sel]), d
        assert not torch.equal(o2[0, sel], o[0, sel]), d


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_dk_dv_of_a_document_do_not_depend_on_what_follows(dev, dtype):
    from apertis_llm_amd import ops
    L, H, D, head = 512, 2, 64, 200
    q, k, v, do = _inputs(dev, 2, L, H, D, dtype, 78)
    for t in (q, k, v, do):
        t[1, :head] = t[0, :head]                            # the same first document, different tokens after it
    ids = torch.stack([torch.repeat_interleave(torch.arange(2), torch.tensor([200, 312])),
                       torch.repeat_interleave(torch.arange(4), torch.tensor([200, 1, 100, 211]))]).to(dev)
    got = _fwd_bwd(lambda a, b, c: ops.document_attention(a, b, c, H, ops.document_layout(ids)), q, k, v, do)
    for n, g_ in zip(NAMES, got):
        assert torch.equal(g_[0, :head], g_[1, :head]), n
        assert not torch.equal(g_[0, head:], g_[1, head:]), n


# ------------------------------------------------------------------------------------------------ dropout
def _drop_keep_np(seed, row, col, ncols, thresh16):
    """common.h drop_keep restated: 16 random bits per element from a 32-bit avalanche of (element pair, seed)."""
    lin = row.astype(np.uint64) * np.uint64(ncols) + col.astype(np.uint64)
    s_lo, s_hi = np.uint32(seed & 0xffffffff), np.uint32((seed >> 32) & 0xffffffff)
    with np.errstate(over="ignore"):
        h = (lin >> np.uint64(1)).astype(np.uint32) ^ s_lo
        h = h + (lin >> np.uint64(33)).astype(np.uint32) * np.uint32(0x9E3779B9) + s_hi
        h ^= h >> np.uint32(16)
        h = h * np.uint32(0x85ebca6b)
        h ^= h >> np.uint32(13)
        h = h * np.uint32(0xc2b2ae35)
        h ^= h >> np.uint32(16)
    r16 = np.where((lin & np.uint64(1)) != 0, h >> np.uint32(16), h & np.uint32(0xffff))
    return r16 >= thresh16


def _keep_mask(seed, B, H, L, p):
    bh, i, j = np.meshgrid(np.arange(B * H), np.arange(L), np.arange(L), indexing="ij")
    return _drop_keep_np(seed, bh * L + i, j, L, int(p * 65536)).reshape(B, H, L, L)


def test_document_attention_dropout_mask_matches_numpy_hash(dev):
    """The kept set is drop_keep's (row (b*H+h)*L + i, key j, L columns: the causal kernels' indices) intersected with the
    document mask: fp32 results within 1e-4 of fp64 under exactly that mask; the same seed gives the same bits."""
    from apertis_llm_amd import ops
    L, H, D, p, seed = 97, 2, 64, 0.1, 0x1234_5678_9abc
    ids = _doc_ids(L, dev)
    B = ids.shape[0]
    layout, allow = ops.document_layout(ids), _allow(ids)
    q, k, v, do = _inputs(dev, B, L, H, D, torch.float32, 6)
    keep = _keep_mask(seed, B, H, L, p)
    fn = lambda a, b, c: ops.attention._Attention.apply("doc", a, b, c, H, None, p, seed, layout)     # noqa: E731
    got = _fwd_bwd(fn, q, k, v, do)
    ref = _fwd_bwd(lambda a, b, c: _ref_attention(a, b, c, H, allow, keep, p), q.double(), k.double(), v.double(), do.double())
    for n, g_, r in zip(NAMES, got, ref):
        rel_error_report(f"document attention dropout fp32 {n}", g_, r, rtol=1e-4)
    again = _fwd_bwd(fn, q, k, v, do)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    other = _fwd_bwd(lambda a, b, c: ops.attention._Attention.apply("doc", a, b, c, H, None, p, seed + 1, layout), q, k, v, do)
    assert not torch.equal(got[0], other[0])
    # through the op: the seed comes from torch's RNG, training only
    torch.manual_seed(7)
    a = ops.document_attention(q, k, v, H, layout, None, 0.3, training=True)
    torch.manual_seed(7)
    b = ops.document_attention(q, k, v, H, layout, None, 0.3, training=True)
    assert torch.equal(a, b)
    assert torch.equal(ops.document_attention(q, k, v, H, layout, None, 0.3, training=False),
                       ops.document_attention(q, k, v, H, layout))


# ------------------------------------------------------------------------------------------------ every form of the node
# (causal, full and doc run through ONE autograd node and one table of what differs, ops.attention._FORMS: these hold every
#  row of that table, here because the document ids live here)
LAUNCHES = {"causal": ("apertis_attention_fwd", "apertis_attention_bwd"),
            "full": ("apertis_attention_full_fwd", "apertis_attention_full_bwd"),
            "doc": ("apertis_attention_doc_fwd", "apertis_attention_doc_bwd")}


def _form_fn(ops, form, H, layout):
    if form == "qkv":                                        # one [B, L, 3W] input: q | k | v stacked along the width
        return lambda a, b, c: ops.full_attention_qkv(torch.cat((a, b, c), dim=-1), H)
    return {"causal": lambda a, b, c: ops.causal_attention(a, b, c, H),
            "full": lambda a, b, c: ops.full_attention(a, b, c, H),
            "doc": lambda a, b, c: ops.document_attention(a, b, c, H, layout)}[form]


@pytest.mark.parametrize("form", ["causal", "full", "doc"])
def test_every_form_launches_its_own_pair_and_counts_its_own_work(dev, form):
    """One forward + backward of each form under a timer on all six launch names: exactly one launch of the form's own two
    and none of the other four, with the form's flops (L = 97: no multiple of the 64-row work-group or the 32-key tile)."""
    from apertis_llm_amd import ops
    B, H, D, L = 2, 2, 64, 97
    layout = ops.document_layout(_doc_ids(L, dev)[:B])
    pairs = sum(n * (n + 1) // 2 for lens in LAYOUTS[L][:B] for n in lens)
    assert layout.pairs == pairs
    fwd_work = {"causal": 4.0 * B * H * D * L * (L + 1) / 2, "full": 4.0 * B * H * D * L * L, "doc": 4.0 * H * D * pairs}[form]
    q, k, v, do = _inputs(dev, B, L, H, D, torch.float32, 3)
    timer = ops.KernelTimer([n for pair in LAUNCHES.values() for n in pair])
    ops.set_kernel_timer(timer)
    try:
        _fwd_bwd(_form_fn(ops, form, H, layout), q, k, v, do)
    finally:
        ops.set_kernel_timer(None)
    s = timer.summary()
    fwd, bwd = LAUNCHES[form]
    assert {n: r["launches"] for n, r in s.items()} == {fwd: 1, bwd: 1}
    assert s[fwd]["work"] == fwd_work and s[bwd]["work"] == 2.5 * fwd_work


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("form", ["causal", "full", "doc", "qkv"])
def test_misaligned_gradient_is_copied_and_gives_the_same_bits(dev, form, dtype):
    """A gradient whose rows (a [B, L, W + 1] buffer's first W columns: 516- and 258-byte rows) or whose pointer (one element
    into a flat buffer) is off a 16-byte boundary is not what the kernels' 16-byte loads take: every form copies it, and dQ,
    dK, dV have the bits a packed copy of the same gradient gives."""
    from apertis_llm_amd import ops
    B, L, H, D = 2, 33, 2, 64
    W = H * D
    q, k, v, _ = _inputs(dev, B, L, H, D, dtype, 13)
    ids = torch.stack([torch.repeat_interleave(torch.arange(2), torch.tensor(lens)) for lens in ([5, 28], [32, 1])]).to(dev)
    fn = _form_fn(ops, form, H, ops.document_layout(ids))
    gen = torch.Generator(device=dev).manual_seed(14)
    rows = torch.randn(B, L, W + 1, device=dev, generator=gen).to(dtype)[..., :W]
    shifted = torch.randn(B * L * W + 1, device=dev, generator=gen).to(dtype)[1:].view(B, L, W)
    assert (rows.stride(1) * rows.element_size()) % 16 and shifted.data_ptr() % 16
    q, k, v = (t.requires_grad_() for t in (q, k, v))
    o = fn(q, k, v)
    for what, g in (("row stride", rows), ("pointer", shifted)):
        packed = g.clone(memory_format=torch.contiguous_format)     # (a fresh allocation: .contiguous() keeps the shifted view)
        assert packed.is_contiguous() and packed.data_ptr() % 16 == 0
        got = torch.autograd.grad(o, (q, k, v), g, retain_graph=True)
        want = torch.autograd.grad(o, (q, k, v), packed, retain_graph=True)
        for n, g_, w in zip(NAMES[1:], got, want):
            assert torch.equal(g_, w) and bool(g_.any()), (what, n)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_outputs_untouched(dev):
    from apertis_llm_amd import _lib, ops
    lib, ptr = _lib.load(), _lib.ptr
    B, L, H = 2, 7, 2
    layout = ops.document_layout(_doc_ids(L, dev))

    def run(D, dtype, code, start, end):
        W = H * D
        q = torch.randn(B, L, W, device=dev).to(dtype)
        out, lse = torch.full_like(q, 7.0), torch.full((B, H, L), 7.0, device=dev)
        dq, dk, dv = torch.full_like(q, 7.0), torch.full_like(q, 7.0), torch.full_like(q, 7.0)
        ws = torch.zeros(B * H * L, device=dev)
        st = _lib.stream_ptr()
        rc_f = lib.apertis_attention_doc_fwd(ptr(q), W, ptr(q), W, ptr(q), W, None, start, end, ptr(out), W, ptr(lse), B, L, H, D,
                                             0.0, 0, code, st)
        rc_b = lib.apertis_attention_doc_bwd(ptr(q), W, ptr(q), W, ptr(q), W, ptr(out), W, ptr(q), W, ptr(lse), None, start, end,
                                             ptr(ws), ptr(dq), ptr(dk), ptr(dv), W, B, L, H, D, 0.0, 0, code, st)
        torch.cuda.synchronize()
        assert all(bool((t == 7.0).all()) for t in (out, lse, dq, dk, dv))
        return rc_f, rc_b

    s, e = ptr(layout.start), ptr(layout.end)
    assert run(32, torch.float32, _lib.F32, s, e) == (-2, -2)                 # head dim 32: unsupported
    assert run(64, torch.float16, 2, s, e) == (-1, -1)                         # fp16: not a dtype of the library
    assert run(64, torch.float32, _lib.F32, None, e) == (-1, -1)               # null layout pointers
    assert run(64, torch.float32, _lib.F32, s, None) == (-1, -1)
    x = torch.zeros(B, L, 2 * 64, device=dev, dtype=torch.float16)
    with pytest.raises(ops.ApertisHipError):
        ops.document_attention(x, x, x, H, layout)
    x32 = torch.zeros(B, L, 2 * 32, device=dev)
    with pytest.raises(ops.ApertisHipError):
        ops.document_attention(x32, x32, x32, H, layout)
