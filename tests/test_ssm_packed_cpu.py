"""Packed selective_ssm rows without a GPU (ops.ssm.SSM_PACKED): the library exports the three entry points under ABI 4.12, the
header declares them and the binding has as many arguments; with the switch forced on a CPU model and a CPU trainer still refuse
packed rows; the state reset that rides on delta (ops.SSM_DOC_RESET) has the fp32 properties DESIGN.md section 3 claims at the
documented A_log floor; and the fp64 restatement the GPU tests compare with (tests/ssm_packed_ref.py) gives every document of a
packed row what it gives that document alone."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import ssm_packed_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"apertis_dwconv_silu_doc_fwd": 13, "apertis_dwconv_silu_doc_bwd": 22, "apertis_tiny_linear_doc_fwd": 13}


@pytest.fixture
def packed_on():
    from apertis_llm_amd import ops
    prev = ops.SSM_PACKED
    ops.SSM_PACKED = True
    yield ops
    ops.SSM_PACKED = prev


def test_library_exports_header_declares_and_binding_matches():
    from apertis_llm_amd import _lib
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "apertis_hip.h")) as f:
        hdr = f.read()
    for name, nargs in NAMES.items():
        assert hasattr(cdll, name), name
        m = re.search(r"\bint " + name + r"\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/apertis_hip.h"
        params = [p for p in re.sub(r"/\*.*?\*/", "", m.group(1)).split(",") if p.strip()]
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(params) == nargs, (name, params)
    # the layout pointers are int32, as ops.document_layout builds them
    assert "const int32_t *start /* [B, L] */, const int32_t *end /* [B, L] */" in hdr
    assert _lib.ABI_VERSION == (4 << 16) | 12 and int(_lib.load().apertis_abi_version()) == (4 << 16) | 12
    assert re.search(r"#define APERTIS_ABI_VERSION \(\(4 << 16\) \| 12\)", hdr)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from apertis_llm_amd import _lib
    lib, P = _lib.load(), 0x1000          # non-null aligned stand-ins: validation happens first, nothing is dereferenced
    fwd = lambda **kw: lib.apertis_dwconv_silu_doc_fwd(*{**dict(x=P, x_rs=64, w=P, b=P, s=P, o=P, o_rs=64, B=2, L=5, Dn=64, k=4,
                                                                dt=1, st=None), **kw}.values())
    bwd = lambda **kw: lib.apertis_dwconv_silu_doc_bwd(*{**dict(x=P, x_rs=64, w=P, b=P, g=P, g_rs=64, g2=None, g2_rs=0, s=P, e=P,
                                                                dx=P, dx_rs=64, dwp=P, dbp=P, dw=P, db=P, B=2, L=5, Dn=64, k=4, dt=1,
                                                                st=None), **kw}.values())
    tl = lambda **kw: lib.apertis_tiny_linear_doc_fwd(*{**dict(x=P, ldx=64, W=P, b=P, s=P, r=2.0 ** 40, y=P, T=10, L=5, K=44, N=11,
                                                               dt=1, st=None), **kw}.values())
    assert all(fwd(**{n: None}) == -1 for n in ("x", "w", "b", "s", "o")) and fwd(dt=2) == -1
    assert all(fwd(**kw) == -2 for kw in (dict(k=1), dict(k=17), dict(Dn=6), dict(x_rs=62), dict(o_rs=32), dict(x=P + 4)))
    assert all(bwd(**{n: None}) == -1 for n in ("x", "w", "b", "g", "s", "e", "dx", "dwp", "dbp", "dw", "db")) and bwd(dt=2) == -1
    assert all(bwd(**kw) == -2 for kw in (dict(k=1), dict(k=17), dict(Dn=6), dict(g_rs=62)))
    assert all(tl(**kw) == -1 for kw in (dict(s=None), dict(y=None), dict(T=11), dict(L=0), dict(r=float("nan")), dict(W=None),
                                         dict(ldx=40)))
    assert all(tl(**kw) == -2 for kw in (dict(K=65, ldx=72), dict(N=17)))
    assert fwd(B=0) == 0 and tl(T=0) == 0 and tl(x=None, T=0) == 0          # nothing to do: no launch


def _model(A, **kw):
    base = dict(vocab_size=16, hidden_size=64, num_hidden_layers=1, num_attention_heads=4, intermediate_size=64,
                attention_type="selective_ssm", position_embedding_type="rotary", max_position_embeddings=64,
                hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    base.update(kw)
    torch.manual_seed(0)
    return A.ApertisForCausalLM(A.ApertisConfig(**base))


def test_switch_is_off_by_default_and_forwarded():
    from apertis_llm_amd import ops
    assert ops.SSM_PACKED is (os.environ.get("APERTIS_SSM_PACKED", "0") == "1")
    assert ops.ssm.SSM_PACKED is ops.SSM_PACKED and "SSM_PACKED" in dir(ops)


def test_cpu_model_and_cpu_trainer_still_refuse(packed_on, tmp_path):
    import apertis_llm_amd as A
    from apertis_llm_amd import data as D
    from apertis_llm_amd.trainer import ApertisTrainer
    model = _model(A).eval()
    ids = torch.randint(4, 16, (2, 16), generator=torch.Generator().manual_seed(1))
    docs = R.document_ids([[5, 1, 10], [16]])
    with torch.no_grad(), pytest.raises(ValueError, match="not a ROCm device"):
        model(input_ids=ids, document_ids=docs)
    with pytest.raises(ValueError, match="generate"):
        model.generate(input_ids=ids, document_ids=docs, max_new_tokens=2)
    words = list("abcdefgh")
    path = tmp_path / "d.jsonl"
    path.write_text("\n".join(json.dumps({"text": " ".join(words[(i + j) % 8] for j in range(n))}) for i, n in enumerate([3, 5, 2, 6])),
                    encoding="utf-8")
    train = D.ApertisPretrainDataset(str(path), {c: i + 4 for i, c in enumerate(words)}, 16, max_length=16)
    with pytest.raises(ValueError, match="ROCm device"):
        ApertisTrainer(_model(A), train, None, output_dir=str(tmp_path / "o"), fp16=False, device="cpu", num_workers=0,
                       pack_sequences=True)
    packed_on.SSM_PACKED = False
    with pytest.raises(ValueError, match="SSM_PACKED"):
        ApertisTrainer(_model(A), train, None, output_dir=str(tmp_path / "o"), fp16=False, device="cpu", num_workers=0,
                       pack_sequences=True)
    with torch.no_grad(), pytest.raises(ValueError, match="is off"):
        model(input_ids=ids, document_ids=docs)


def test_a_log_floor_check_reads_the_parameters():
    import apertis_llm_amd as A
    from apertis_llm_amd import ops
    model = _model(A)
    ops.doc_reset_check(model)                                    # the initialisation lies in [ln 0.5, ln 0.99]
    with torch.no_grad():
        model.model.layers[0].attention.attention_mechanism_impl.A_log[1, 3] = ops.SSM_DOC_A_LOG_FLOOR - 0.5
    with pytest.raises(ops.ApertisHipError, match="A_log"):
        ops.doc_reset_check(model)
    with torch.no_grad():
        model.model.layers[0].attention.attention_mechanism_impl.A_log[1, 3] = float("nan")
    with pytest.raises(ops.ApertisHipError, match="A_log"):
        ops.doc_reset_check(model)


def test_reset_value_in_fp32_at_the_a_log_floor():
    """What DESIGN.md section 3 claims of ops.SSM_DOC_RESET, in numpy fp32 arithmetic as the kernels do it: softplus returns the
    logit itself, the decay at the documented A_log floor - and at every A_log above it - is exactly 0, the state after the
    reset is Bt, every term of the backward that crosses the boundary is 0, and the sums of delta the kernels form over ranges
    of tokens stay finite for rows of up to 2^27 tokens."""
    from apertis_llm_amd import ops
    f = np.float32
    reset, log2e = f(ops.SSM_DOC_RESET), f(1.4426950408889634)
    assert np.isfinite(reset) and float(reset) == ops.SSM_DOC_RESET == 2.0 ** 40
    with np.errstate(under="ignore", over="raise", invalid="raise"):
        # softplus: the library form (threshold 20) and the hardware form max(x, 0) + log1p(exp(-|x|))
        e = np.exp2(-np.abs(reset) * log2e)
        assert e == 0 and np.maximum(reset, f(0)) + e == reset
        for a_log in (ops.SSM_DOC_A_LOG_FLOOR, -10.0, math.log(0.5), math.log(0.99), 3.0):
            A2 = -np.exp(f(a_log)) * log2e                       # the kernels' A2 = -exp(A_log) * log2(e)
            a = np.exp2(reset * A2)
            assert a == 0 and np.signbit(a) == False, (a_log, a)          # noqa: E712
            assert float(reset) * math.exp(a_log) * 1.4426950408889634 >= 150          # below the smallest fp32 denormal
            s_prev, bt, lam = f(123.456), f(-0.75), f(0.3)
            assert a * s_prev + bt == bt                          # s_t = fma(0, s_{t-1}, Bt_t)
            assert a * lam == 0                                   # mu = a * lambda: nothing crosses the boundary
            q = lam * s_prev * a * A2
            assert q == 0 and q * reset == 0                      # d delta and the dA_log term q * delta
            assert f(1) - np.exp2(-reset * log2e) == 1            # the sigmoid factor 1 - exp(-softplus(x))
            # range sums of delta that contain resets: finite, and their product with A2 too (a decay of 0, never NaN)
            for n_resets in (1, 2 ** 10, 2 ** 27):
                total = f(n_resets) * reset + f(37.5)
                assert np.isfinite(total) and np.isfinite(total * A2) and np.exp2(total * A2) == 0
    # just below the floor the product is still far from the denormal range's edge only by the margin the floor documents
    assert float(reset) * math.exp(ops.SSM_DOC_A_LOG_FLOOR - 0.2) * 1.4426950408889634 < 150


LENS = [[1, 1, 1, 13, 48, 1], [16, 21, 1, 1, 25, 1]]           # rows of 65 tokens


def _per_document(fn, tensors, lens, names):
    """fn on every document alone: outputs written back to the packed positions, gradients of the [B, L, ...] inputs too, the
    others summed."""
    out, grads = None, {}
    for b, s, e in R.documents(lens):
        lv = R.leaves({k: (v[b:b + 1, s:e] if k in names else v) for k, v in tensors.items() if k != "dout"})
        o = fn(lv, torch.zeros(1, e - s, dtype=torch.int64))
        if out is None:
            out = torch.zeros(len(lens), sum(lens[0]), o.shape[-1], dtype=torch.float64)
        out[b, s:e] = o.detach()[0]
        o.backward(tensors["dout"][b:b + 1, s:e].double())
        for k, v in lv.items():
            if k in names:
                grads.setdefault(k, torch.zeros_like(tensors[k], dtype=torch.float64))[b, s:e] = v.grad[0]
            else:
                grads[k] = grads.get(k, 0) + v.grad
    return out, grads


def test_restated_conv_equals_the_documents_alone():
    g = torch.Generator().manual_seed(5)
    B, L, Dn, k = 2, 65, 8, 4
    t = dict(x=torch.randn(B, L, Dn, generator=g), w=torch.randn(Dn, k, generator=g), b=torch.randn(Dn, generator=g))
    dout = torch.randn(B, L, Dn, generator=g)
    start, _ = R.starts_ends(LENS)
    lv = R.leaves(t)
    out = R.conv_silu(lv["x"], lv["w"], lv["b"], start)
    out.backward(dout.double())
    alone, ga = _per_document(lambda v, st: R.conv_silu(v["x"], v["w"], v["b"], st), {**t, "dout": dout}, LENS, ("x",))
    torch.testing.assert_close(out.detach(), alone, rtol=1e-13, atol=1e-13)
    for n in ("x", "w", "b"):
        torch.testing.assert_close(lv[n].grad, ga[n], rtol=1e-12, atol=1e-12, msg=n)
    # ... and not what the rows give as one sequence each
    whole = R.conv_silu(lv["x"], lv["w"], lv["b"], torch.zeros_like(start))
    assert float((whole - out).detach().abs().max()) > 1e-3


def test_restated_scan_equals_the_documents_alone():
    g = torch.Generator().manual_seed(6)
    B, L, h, N = 2, 65, 2, 4
    Dn = h * N
    t = dict(logits=torch.randn(B, L, h, generator=g) - 1.0, A_log=torch.empty(h, N).uniform_(math.log(0.5), math.log(0.99), generator=g),
             Bt=torch.randn(B, L, Dn, generator=g), C=torch.randn(B, L, Dn, generator=g), xc=torch.randn(B, L, Dn, generator=g),
             z=torch.randn(B, L, Dn, generator=g), D=torch.randn(Dn, generator=g))
    dout = torch.randn(B, L, Dn, generator=g)
    start, _ = R.starts_ends(LENS)
    call = lambda v, st: R.scan_gate(v["logits"], v["A_log"], v["Bt"], v["C"], v["xc"], v["z"], v["D"], st)
    lv = R.leaves(t)
    out = call(lv, start)
    out.backward(dout.double())
    rows = ("logits", "Bt", "C", "xc", "z")
    alone, ga = _per_document(call, {**t, "dout": dout}, LENS, rows)
    torch.testing.assert_close(out.detach(), alone, rtol=1e-13, atol=1e-13)
    for n in lv:
        torch.testing.assert_close(lv[n].grad, ga[n], rtol=1e-12, atol=1e-12, msg=n)
    # the logit of a document's first token is never read: its gradient is exactly 0 (the row's first token aside, which
    # has no state in front of it either and gets an exact 0 through h0 = 0)
    first = start == torch.arange(L).view(1, L)
    assert float(lv["logits"].grad[first].abs().max()) == 0.0
    assert float((call(lv, torch.zeros_like(start)) - out).detach().abs().max()) > 1e-3
