"""Sliding-window attention without a GPU: the library exports the window pair under ABI 4.12 and refuses bad arguments before
any launch; ops.window_layout against a brute-force mask; the model's stock branch under ops.ATTN_WINDOW (a band-masked softmax
over the same projections, a cached step equal to the uncached forward, and nothing at all with the switch off)."""
import ctypes
import math
import os
import re

import pytest
import torch

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -2
F32, BF16 = 0, 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = (("apertis_attention_window_fwd", "apertis_attention_doc_fwd"), ("apertis_attention_window_bwd", "apertis_attention_doc_bwd"))


def _lib():
    from apertis_llm_amd import _lib
    return _lib.load()


def _params(hdr, name):
    m = re.search(r"\bint " + name + r"\(([^)]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/apertis_hip.h"
    return [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]


@pytest.fixture
def window_switch():
    from apertis_llm_amd import ops
    before = ops.ATTN_WINDOW
    ops.ATTN_WINDOW = True
    yield ops
    ops.ATTN_WINDOW = before


# ------------------------------------------------------------------------------------------------ exports
def test_library_exports_header_declares_and_binding_matches():
    from apertis_llm_amd import _lib
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "apertis_hip.h")) as f:
        hdr = f.read()
    for name, doc in PAIRS:
        assert hasattr(cdll, name), name
        params, base = _params(hdr, name), _params(hdr, doc)
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(params), (name, params)
        # the document entry point's argument list with one int64 in place of the two int32 pointers
        at = base.index("const int32_t *doc_start")
        assert params == base[:at] + ["int64_t window"] + base[at + 2:]
        dargs = list(_lib.SIGNATURES[doc][1])
        assert list(argtypes) == dargs[:at] + [ctypes.c_int64] + dargs[at + 2:]
    assert _lib.ABI_VERSION == (4 << 16) | 12 and int(_lib.load().apertis_abi_version()) == (4 << 16) | 12
    assert re.search(r"#define APERTIS_ABI_VERSION \(\(4 << 16\) \| 12\)", hdr)
    assert len(_lib.SIGNATURES) == 123


# ------------------------------------------------------------------------------------------------ refusals
# non-null, 16-byte aligned stand-ins: validation happens before any launch, nothing is dereferenced
P = 0x1000


def _fwd(name, **kw):
    a = {**dict(q=P, k=P, v=P, kv=None, start=P, end=P, window=3, out=P, lse=P, q_rs=192, k_rs=192, v_rs=192, o_rs=192, B=2, L=5,
                H=3, D=64, p=0.0, seed=0, dt=BF16), **kw}
    mid = (a["start"], a["end"]) if "doc" in name else (a["window"],)
    return getattr(_lib(), name)(a["q"], a["q_rs"], a["k"], a["k_rs"], a["v"], a["v_rs"], a["kv"], *mid, a["out"], a["o_rs"],
                                 a["lse"], a["B"], a["L"], a["H"], a["D"], a["p"], a["seed"], a["dt"], None)


def _bwd(name, **kw):
    a = {**dict(q=P, k=P, v=P, out=P, dout=P, lse=P, kv=None, start=P, end=P, window=3, ws=P, dq=P, dk=P, dv=P, q_rs=192, k_rs=192,
                v_rs=192, o_rs=192, do_rs=192, d_rs=192, B=2, L=5, H=3, D=64, p=0.0, seed=0, dt=BF16), **kw}
    mid = (a["start"], a["end"]) if "doc" in name else (a["window"],)
    return getattr(_lib(), name)(a["q"], a["q_rs"], a["k"], a["k_rs"], a["v"], a["v_rs"], a["out"], a["o_rs"], a["dout"], a["do_rs"],
                                 a["lse"], a["kv"], *mid, a["ws"], a["dq"], a["dk"], a["dv"], a["d_rs"], a["B"], a["L"], a["H"],
                                 a["D"], a["p"], a["seed"], a["dt"], None)


def _refusals(call, ptrs, strides):
    got = [(f"null {n}", call(**{n: None})) for n in ptrs]
    got += [(f"p {p}", call(p=p)) for p in (-0.1, 1.0, 1.5, float("nan"))]
    got += [("D 32", call(D=32, **{s: 96 for s in strides}))]
    got += [("fp16", call(dt=2))]
    got += [("B*H 65536", call(B=16384, H=4, D=64, **{s: 256 for s in strides}))]
    got += [(f"misaligned {s}", call(**{s: 196})) for s in strides]            # bf16: 392-byte rows
    got += [(f"misaligned {n}", call(**{n: P + 8})) for n in ptrs]
    return dict(got)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    fs, bs = ("q_rs", "k_rs", "v_rs", "o_rs"), ("q_rs", "k_rs", "v_rs", "o_rs", "do_rs", "d_rs")
    fp, bp = ("q", "k", "v", "out", "lse"), ("q", "k", "v", "out", "dout", "lse", "ws", "dq", "dk", "dv")
    for (win, doc), call, ptrs, strides in zip(PAIRS, (_fwd, _bwd), (fp, bp), (fs, bs)):
        got = _refusals(lambda **kw: call(win, **kw), ptrs, strides)
        want = _refusals(lambda **kw: call(doc, **kw), ptrs, strides)
        assert got == want, (win, got, want)                                   # the document pair's checks and codes
        assert all(got[f"null {n}"] == ERR_ARG for n in ptrs) and got["fp16"] == ERR_ARG
        assert got["D 32"] == ERR_UNSUPPORTED and got["B*H 65536"] == ERR_UNSUPPORTED
        assert all(got[f"misaligned {s}"] == ERR_UNSUPPORTED for s in strides)
        # the window: below one is an argument error, whatever else is asked, work or no work
        for w in (0, -1, -2 ** 63):
            assert call(win, window=w) == ERR_ARG, w
            assert call(win, window=w, L=0) == ERR_ARG and call(win, window=w, B=0) == ERR_ARG
        assert call(win, B=0) == OK and call(win, L=0) == OK
        assert call(win, B=0, window=2 ** 63 - 1) == OK
        assert call(win, L=2 ** 31) == call(doc, L=2 ** 31) == ERR_ARG         # rows the document pair refuses


# ------------------------------------------------------------------------------------------------ layout
def _brute(L, W, start=None):
    """allow[i, j]: j <= i, i - j < W and (packed) j at or after the first token of i's document."""
    i, j = torch.arange(L)[:, None], torch.arange(L)[None, :]
    allow = (j <= i) & (i - j < W)
    if start is not None:
        allow = allow & (j >= start[:, None])
    return allow


def _check_layout(lay, allow):
    """start / end describe `allow` [B, L, L], read from the query side and from the key side; pairs is its popcount."""
    B, L, _ = allow.shape
    i, j = torch.arange(L)[None, :, None], torch.arange(L)[None, None, :]
    assert lay.start.dtype == torch.int32 and lay.end.dtype == torch.int32
    assert tuple(lay.start.shape) == tuple(lay.end.shape) == (B, L) and lay.start.is_contiguous() and lay.end.is_contiguous()
    query_side = (j <= i) & (j >= lay.start.long()[:, :, None])
    key_side = (j <= i) & (i < lay.end.long()[:, None, :])
    assert torch.equal(query_side, allow) and torch.equal(key_side, allow)
    assert lay.pairs == int(allow.sum())


@pytest.mark.parametrize("L", [1, 7, 200])
@pytest.mark.parametrize("W", [1, 5, 200, 1000])
def test_window_layout_matches_a_brute_force_mask(L, W):
    from apertis_llm_amd import ops
    lay = ops.window_layout((2, L), W, "cpu")
    _check_layout(lay, _brute(L, W)[None].expand(2, L, L))
    assert lay.positions.tolist() == [list(range(L))] * 2
    assert ops.window_pairs(L, W) * 2 == lay.pairs
    # the unclipped arrays are built once per (L, W, device)
    assert (L, min(W, L), "cpu") in ops.attention._WINDOW_ARRAYS
    # clipped into three documents (the last one a single token when L allows)
    cuts = sorted({0, L // 3, L - 1})
    ids = torch.zeros(2, L, dtype=torch.long)
    for c in cuts[1:]:
        ids[0, c:] += 1
    docs = ops.document_layout(ids)
    clipped = ops.window_layout(docs, W)
    allow = torch.stack([_brute(L, W, docs.start[b].long()) for b in range(2)])
    _check_layout(clipped, allow)
    assert clipped.positions is docs.positions
    if W >= L:
        assert torch.equal(clipped.start, docs.start) and torch.equal(clipped.end, docs.end) and clipped.pairs == docs.pairs


def test_window_arguments_that_raise():
    from apertis_llm_amd import ops
    for bad in (0, -3, 2.0, None, True, "4"):
        with pytest.raises(ValueError):
            ops.window_layout((1, 4), bad, "cpu")
    x = torch.zeros(1, 4, 128)
    with pytest.raises(ValueError):
        ops.window_attention(x, x, x, 2, 0)
    with pytest.raises(ops.ApertisHipError):                                   # a CPU tensor: no fallback
        ops.window_attention(x, x, x, 2, 2)
    assert ops.ATTN_WINDOW is False or os.environ.get("APERTIS_MHA_WINDOW") == "1"          # off by default
    for name in ("window_attention", "window_layout", "window_pairs", "ATTN_WINDOW"):
        assert hasattr(ops, name), name
    assert "window" in ops.attention._FORMS


# ------------------------------------------------------------------------------------------------ model, stock path
L_MODEL, W_MODEL = 48, 13


def _model(A, **kw):
    base = dict(vocab_size=64, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128,
                attention_type="standard_mha", position_embedding_type="rotary", max_position_embeddings=64,
                hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, sliding_window=W_MODEL)
    base.update(kw)
    torch.manual_seed(0)
    return A.ApertisForCausalLM(A.ApertisConfig(**base)).eval()


def _ids(B=2):
    return torch.randint(4, 64, (B, L_MODEL), generator=torch.Generator().manual_seed(1))


def _band_sdpa(W):
    """A straight band-masked softmax in place of the stock branch's SDPA call: it ignores the mask it is handed."""
    def sdpa(q, k, v, attn_mask=None, dropout_p=0.0):
        Lq, Lk = q.shape[-2], k.shape[-2]
        i, j = torch.arange(Lq)[:, None] + (Lk - Lq), torch.arange(Lk)[None, :]
        s = (q @ k.transpose(-1, -2)) / math.sqrt(q.shape[-1])
        s = s.masked_fill(~((j <= i) & (i - j < W)), float("-inf"))
        return torch.softmax(s, dim=-1) @ v
    return sdpa


def test_model_logits_are_a_band_masked_softmax(window_switch, monkeypatch):
    import apertis_llm_amd as A
    import apertis_llm_amd.model as M
    model, ids = _model(A), _ids()
    with torch.no_grad():
        got = model(input_ids=ids)[1]
        window_switch.ATTN_WINDOW = False
        full = model(input_ids=ids)[1]
        monkeypatch.setattr(M.F, "scaled_dot_product_attention", _band_sdpa(W_MODEL))
        want = model(input_ids=ids)[1]
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5 * float(want.abs().max()))
    assert not torch.allclose(got, full, rtol=1e-3, atol=1e-3 * float(full.abs().max()))      # the band does something
    torch.testing.assert_close(got[:, :W_MODEL], full[:, :W_MODEL], rtol=1e-5, atol=1e-5 * float(full.abs().max()))  # not inside it


def test_switch_off_ignores_the_field():
    import apertis_llm_amd as A
    from apertis_llm_amd import ops
    assert not ops.ATTN_WINDOW
    ids = _ids()
    with torch.no_grad():
        a = _model(A)(input_ids=ids)[1]
        b = _model(A, sliding_window=None)(input_ids=ids)[1]
        c = _model(A, sliding_window="not a number")(input_ids=ids)[1]
    assert torch.equal(a, b) and torch.equal(a, c)


def test_window_none_under_the_switch_changes_nothing(window_switch):
    import apertis_llm_amd as A
    ids = _ids()
    with torch.no_grad():
        on = _model(A, sliding_window=None)(input_ids=ids)[1]
        wide = _model(A, sliding_window=L_MODEL)(input_ids=ids)[1]
        window_switch.ATTN_WINDOW = False
        off = _model(A, sliding_window=None)(input_ids=ids)[1]
    assert torch.equal(on, off) and torch.equal(wide, off)


@pytest.mark.parametrize("bad", [0, -1, 2.5, "13", True])
def test_bad_sliding_window_raises_at_the_first_forward(window_switch, bad):
    import apertis_llm_amd as A
    model = _model(A, sliding_window=bad)
    with pytest.raises(ValueError), torch.no_grad():
        model(input_ids=_ids())


def test_cached_step_equals_the_uncached_last_row(window_switch):
    import apertis_llm_amd as A
    model, ids = _model(A), _ids()
    with torch.no_grad():
        want = model(input_ids=ids)[1][:, -1]
        past = model(input_ids=ids[:, :-1], use_cache=True)[4]
        assert past[0][0].shape[1] == L_MODEL - 1 > W_MODEL                                     # the prefill keeps every row
        got = model(input_ids=ids[:, -1:], past_key_values=past, use_cache=True)[1][:, -1]
        # and a multi-token continuation (cached Lq < Lk) carries the band too
        past = model(input_ids=ids[:, :20], use_cache=True)[4]
        tail = model(input_ids=ids[:, 20:], past_key_values=past, use_cache=True)[1]
        whole = model(input_ids=ids)[1][:, 20:]
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5 * float(want.abs().max()))
    torch.testing.assert_close(tail, whole, rtol=1e-5, atol=1e-5 * float(whole.abs().max()))


def test_packed_rows_under_the_window_equal_documents_alone(window_switch):
    import apertis_llm_amd as A
    model, ids = _model(A), _ids()
    lens = ([30, 5, 13], [48])
    docs = torch.stack([torch.repeat_interleave(torch.arange(len(l)), torch.tensor(l)) for l in lens])
    with torch.no_grad():
        logits = model(input_ids=ids, document_ids=docs)[1]
        for b, ll in enumerate(lens):
            at = 0
            for n in ll:
                alone = model(input_ids=ids[b:b + 1, at:at + n])[1]
                torch.testing.assert_close(logits[b, at:at + n], alone[0], rtol=1e-5, atol=1e-5 * float(alone.abs().max()))
                at += n
