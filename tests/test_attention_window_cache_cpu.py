"""The sliding-window KV-cache entry points without a GPU (include/apertis_hip_ext.h, csrc/attention_decode.hip, ops/attention.py):
apertis_attention_decode_window_at and apertis_attention_chunk_window are exported, declared in the extension header only and
bound in _lib.EXT_SIGNATURES, the 4.12 table keeps its 123 entries, both refuse window < 1 and everything their base entry points
refuse before any launch, ops.ATTN_WINDOW_CACHE is off by default, and KVCache.step_state_begin refuses a window below one."""
import ctypes
import glob
import os
import re

import pytest
import torch

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -2
F32, BF16 = 0, 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 4096            # a 16-byte aligned stand-in for a device pointer: nothing is dereferenced before the checks pass
# (new entry point, the entry point whose argument list it extends, the argument `window` follows)
PAIRS = (("apertis_attention_decode_window_at", "apertis_attention_decode_at", "const int64_t *len"),
         ("apertis_attention_chunk_window", "apertis_attention_chunk", "int64_t n"))


def _lib():
    from apertis_llm_amd import _lib
    return _lib.load()


def _params(hdr, name):
    m = re.search(r"\bint " + name + r"\(([^)]*)\)\s*;", hdr)
    assert m, f"{name} is not declared"
    return [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]


# ------------------------------------------------------------------------------------------------ exports
def test_exported_declared_in_the_extension_header_only_and_bound_in_the_second_table():
    from apertis_llm_amd import _lib
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "apertis_hip.h")) as f:
        base_hdr = f.read()
    with open(os.path.join(ROOT, "include", "apertis_hip_ext.h")) as f:
        ext_hdr = f.read()
    assert re.search(r'#include "apertis_hip.h"', ext_hdr)
    assert "entry points added after the 4.12 table" in ext_hdr
    assert "APERTIS_ABI_VERSION" not in re.sub(r"/\*.*?\*/", "", ext_hdr, flags=re.S)         # it defines no version of its own
    others = [p for p in glob.glob(os.path.join(ROOT, "include", "*.h")) if os.path.basename(p) != "apertis_hip_ext.h"]
    assert os.path.join(ROOT, "include", "apertis_hip.h") in others
    for name, base, after in PAIRS:
        assert hasattr(cdll, name), name
        for p in others:
            with open(p) as f:
                assert not re.search(r"\b" + name + r"\b", f.read()), (name, p)
        assert name not in _lib.SIGNATURES and name in _lib.EXT_SIGNATURES
        params, bparams = _params(ext_hdr, name), _params(base_hdr, base)
        at = bparams.index(after) + 1
        assert params == bparams[:at] + ["int64_t window"] + bparams[at:]                      # the base list plus one int64
        restype, argtypes = _lib.EXT_SIGNATURES[name]
        bargs = list(_lib.SIGNATURES[base][1])
        assert restype is ctypes.c_int and len(argtypes) == len(params)
        assert list(argtypes) == bargs[:at] + [ctypes.c_int64] + bargs[at:]
        fn = getattr(_lib.load(), name)                                                        # _Lib.__getattr__ finds it
        assert list(fn.argtypes) == list(argtypes)
    assert set(re.findall(r"\b(apertis_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", ext_hdr, flags=re.S))) == set(_lib.EXT_SIGNATURES)
    assert not set(_lib.SIGNATURES) & set(_lib.EXT_SIGNATURES)
    with pytest.raises(AttributeError):
        _lib.load().apertis_no_such_entry_point


def test_the_4_12_table_is_as_it_was():
    from apertis_llm_amd import _lib
    with open(os.path.join(ROOT, "include", "apertis_hip.h")) as f:
        hdr = f.read()
    assert len(_lib.SIGNATURES) == 123
    assert set(re.findall(r"\b(apertis_\w+)\s*\(", hdr)) == set(_lib.SIGNATURES)
    assert _lib.ABI_VERSION == (4 << 16) | 12 == int(_lib.load().apertis_abi_version())
    assert re.search(r"#define APERTIS_ABI_VERSION \(\(4 << 16\) \| 12\)", hdr)


# ------------------------------------------------------------------------------------------------ refusals
def _decode(name, q=P, q_rs=256, k=P, k_rs=256, k_bs=None, v=P, v_rs=256, v_bs=None, cap=64, len_=P, window=5, kv=None, kv_rs=0,
            out=P, out_rs=256, ws=None, B=2, H=4, D=64, splits=1, dtype=F32):
    k_bs = cap * k_rs if k_bs is None else k_bs
    v_bs = cap * v_rs if v_bs is None else v_bs
    mid = (len_, window) if "window" in name else (len_,)
    return getattr(_lib(), name)(q, q_rs, k, k_rs, k_bs, v, v_rs, v_bs, cap, *mid, kv, kv_rs, out, out_rs, ws, B, H, D, splits,
                                 dtype, None)


def _chunk(name, q=P, q_rs=256, k=P, k_rs=256, k_bs=None, v=P, v_rs=256, v_bs=None, cap=64, kv=None, kv_rs=0, out=P, out_rs=256,
           ws=None, B=2, Lq=8, n=20, window=5, H=4, D=64, splits=1, dtype=F32):
    k_bs = cap * k_rs if k_bs is None else k_bs
    v_bs = cap * v_rs if v_bs is None else v_bs
    mid = (n, window) if "window" in name else (n,)
    return getattr(_lib(), name)(q, q_rs, k, k_rs, k_bs, v, v_rs, v_bs, cap, kv, kv_rs, out, out_rs, ws, B, Lq, *mid, H, D, splits,
                                 dtype, None)


# every call below asks for work (B = 2) unless it says B=0: a call that passed its checks would launch on stand-in pointers
DECODE_CASES = [dict(B=0), dict(q=None), dict(k=None), dict(v=None), dict(out=None), dict(len_=None), dict(len_=None, B=0),
                dict(H=0), dict(dtype=2), dict(cap=0), dict(B=-1), dict(q_rs=255), dict(out_rs=128), dict(k_rs=128), dict(v_rs=128),
                dict(k_bs=63 * 256), dict(v_bs=63 * 256), dict(kv=P, kv_rs=63), dict(kv=P, kv_rs=64, B=0),
                dict(splits=0), dict(splits=-1), dict(splits=65, ws=P), dict(splits=2, ws=None), dict(splits=64, ws=P, B=0),
                dict(D=48, q_rs=192, k_rs=192, v_rs=192, out_rs=192), dict(k_rs=258), dict(v_rs=257), dict(dtype=BF16, k_rs=260),
                dict(q=P + 4), dict(k=P + 8), dict(v=P + 8), dict(B=65536), dict(H=65536, q_rs=2 ** 22, k_rs=2 ** 22, v_rs=2 ** 22,
                                                                                  out_rs=2 ** 22)]
CHUNK_CASES = [dict(B=0), dict(q=None), dict(k=None), dict(v=None), dict(out=None), dict(Lq=0), dict(n=-1), dict(n=57),
               dict(n=56, B=0), dict(n=2 ** 62, Lq=2 ** 62), dict(H=0), dict(dtype=2), dict(q_rs=255), dict(out_rs=128),
               dict(k_rs=128), dict(k_bs=63 * 256), dict(v_bs=63 * 256), dict(kv=P, kv_rs=27), dict(kv=P, kv_rs=28, B=0),
               dict(splits=-1), dict(splits=65, ws=P), dict(splits=2, ws=None),
               dict(splits=0, ws=None, B=1, H=1, n=4000, Lq=8, cap=4096, window=4000),
               dict(D=48, H=4, q_rs=192, k_rs=192, v_rs=192, out_rs=192), dict(k_rs=258), dict(v_rs=257),
               dict(dtype=BF16, k_rs=260), dict(q=P + 4), dict(k=P + 8), dict(out=P + 4), dict(B=16384)]


@pytest.mark.parametrize("call,cases,names", [(_decode, DECODE_CASES, PAIRS[0]), (_chunk, CHUNK_CASES, PAIRS[1])],
                         ids=["decode_window_at", "chunk_window"])
def test_window_entry_points_refuse_before_any_launch(call, cases, names):
    win, base = names[:2]
    for kw in cases:
        got, want = call(win, **kw), call(base, **kw)
        assert got == want, (win, kw, got, want)                               # the base entry point's checks and codes
        assert got in (ERR_ARG, ERR_UNSUPPORTED) or (got == OK and kw.get("B") == 0), (kw, got)
    assert {call(win, **kw) for kw in cases} == {OK, ERR_ARG, ERR_UNSUPPORTED}
    # the window: below one is an argument error, whatever else is asked, work or no work
    for w in (0, -1, -2 ** 63):
        assert call(win, window=w) == ERR_ARG and call(win, window=w, B=0) == ERR_ARG, w
    for w in (1, 64, 2 ** 63 - 1):
        assert call(win, window=w, B=0) == OK, w


# ------------------------------------------------------------------------------------------------ ops
def test_the_switch_is_off_by_default_and_forwarded():
    from apertis_llm_amd import ops
    assert ops.ATTN_WINDOW_CACHE is False or os.environ.get("APERTIS_MHA_WINDOW_CACHE") == "1"
    assert ops._FORWARDED["ATTN_WINDOW_CACHE"] is ops.attention is ops._FORWARDED["ATTN_WINDOW"]
    before = ops.ATTN_WINDOW_CACHE
    try:
        ops.ATTN_WINDOW_CACHE = True
        assert ops.attention.ATTN_WINDOW_CACHE is True and "ATTN_WINDOW_CACHE" not in vars(ops)
    finally:
        ops.ATTN_WINDOW_CACHE = before
    assert ops.attention.ATTN_WINDOW_CACHE is before


def test_step_state_begin_refuses_a_window_below_one_before_anything_else():
    from apertis_llm_amd import ops
    cache = ops.KVCache.empty(1, 2, 8, 128)
    assert cache.step_window is None
    for bad in (0, -3, 2.0, True, "4"):
        with pytest.raises(ValueError):
            cache.step_state_begin(2, window=bad)
    assert cache.step_active is False and cache.step_window is None and cache.dev_len is None
    x = torch.zeros(2, 3, 128)
    cache.lengths = [3]
    with pytest.raises(ops.ApertisHipError):                                   # a CPU tensor: no fallback, window or not
        ops.attention_chunk(x, cache, 0, 2, window=2)
