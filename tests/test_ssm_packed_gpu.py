"""Packed selective_ssm rows on the GPU (ops.ssm.SSM_PACKED): the conv that stops at document starts (csrc/ssm_elementwise.hip's
doc pair), the scan whose state reset rides on delta (ops.scan_gate / scan_gate_dt under a layout, every form a packed row can
reach), the model and the trainer.  Exact claims are asserted exactly (bits against the plain kernels on a document alone,
zeros, isolation of documents, run-to-run identity); every tolerance is MEASURED in the test: the error of the packed run
against the fp64 restatement (tests/ssm_packed_ref.py) is held to twice the error of the existing plain op run on the documents
alone against the same restatement."""
import json
import math

import pytest
import torch

import ssm_packed_ref as R
from conftest import rel_error_report

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture
def ops():
    from apertis_llm_amd import ops as o
    prev = (o.SSM_PACKED, o.SCAN_LEAN, o.SCAN_LEAN_BWD, o.SCAN_LOOKBACK, o.SCAN_SINGLE_PASS, o.SCAN_DT_FUSED, o.DWCONV_PAIR)
    o.SSM_PACKED = True
    yield o
    o.SSM_PACKED, o.SCAN_LEAN, o.SCAN_LEAN_BWD, o.SCAN_LOOKBACK, o.SCAN_SINGLE_PASS, o.SCAN_DT_FUSED, o.DWCONV_PAIR = prev


def _layout(ops, lens, dev):
    return ops.document_layout(R.document_ids(lens).to(dev))


def _err(got, ref):
    return float((got.detach().cpu().double() - ref.detach().cpu().double()).abs().max())


def _held(name, packed, alone):
    """The measured bound: the packed run's error against the restatement is at most twice the alone runs'."""
    print(f"{name}: packed {packed:.3e}  alone {alone:.3e}")
    assert packed <= 2.0 * alone, f"{name}: packed error {packed:.3e} > 2 x alone error {alone:.3e}"


# ================================================================================================ conv
CONV_L = (1, 63, 64, 65, 130)
CONV_DN = (4, 64, 176)


def _conv_lens(L):
    """Two rows: boundaries at 1, 2, 3 (a run of one-token documents, shorter than k - 1 for k >= 4), at the tile edge 64 and
    at L - 1; and at 37, 63, 65, 66 (either side of the tile edge)."""
    return [R.lens_from_boundaries(L, (1, 2, 3, 64, L - 1)), R.lens_from_boundaries(L, (37, 63, 65, 66))]


def _conv_inputs(dev, L, Dn, k, dt, seed):
    """x as the model hands it over: a column slice of a wider projection output (strided rows)."""
    g = torch.Generator().manual_seed(seed)
    xz = torch.randn(2, L, 2 * Dn, generator=g).to(dt).to(dev)
    w = (0.5 * torch.randn(Dn, 1, k, generator=g)).to(dev)
    b = (0.5 * torch.randn(Dn, generator=g)).to(dev)
    g1 = torch.randn(2, L, Dn, generator=g).to(dt).to(dev)
    g2 = torch.randn(2, L, Dn, generator=g).to(dt).to(dev)
    return xz[..., :Dn], w, b, g1, g2


@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("k", [2, 4, 5, 16])
def test_conv_forward_has_the_bits_of_every_document_alone(dev, ops, k, dt):
    with torch.no_grad():
        for Dn in CONV_DN:
            for L in CONV_L:
                x, w, b, _, _ = _conv_inputs(dev, L, Dn, k, dt, 1000 * Dn + 10 * L + k)
                lens = _conv_lens(L)
                out = ops.dwconv_silu(x, w, b, layout=_layout(ops, lens, dev))
                assert out.shape == x.shape and out.dtype == dt and out.is_contiguous()
                for r, s, e in R.documents(lens):
                    alone = ops.dwconv_silu(x[r:r + 1, s:e].contiguous(), w, b)
                    assert torch.equal(out[r, s:e], alone[0]), (Dn, L, r, s, e)
                # one document per row: the plain forward's bits
                one = ops.dwconv_silu(x, w, b, layout=_layout(ops, [[L], [L]], dev))
                assert torch.equal(one, ops.dwconv_silu(x, w, b)), (Dn, L)
                if L > 3:
                    assert not torch.equal(one, out)


def _conv_grads(ops, x, w, b, g1, g2, layout):
    """(dx, dw, db) through the pair op (two views of the output, one gradient each; g2 None: the second view is unused)."""
    x, w, b = (t.detach().clone().requires_grad_(True) for t in (x, w, b))
    a, c = ops.dwconv_silu_pair(x, w, b, layout=layout)
    assert a.data_ptr() == c.data_ptr()
    torch.autograd.backward([a] if g2 is None else [a, c], [g1] if g2 is None else [g1, g2])
    return x.grad, w.grad, b.grad


@pytest.mark.parametrize("both", [True, False], ids=["two_grads", "one_grad"])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("k", [4, 16])
def test_conv_backward(dev, ops, k, dt, both):
    ops.DWCONV_PAIR = True
    for Dn in CONV_DN:
        for L in CONV_L:
            x, w, b, g1, g2 = _conv_inputs(dev, L, Dn, k, dt, 2000 * Dn + 10 * L + k)
            if not both:
                g2 = None
            lens = _conv_lens(L)
            tag = f"conv bwd k={k} {dt} Dn={Dn} L={L}"
            # one document per row: dx has the plain backward's bits
            one = _conv_grads(ops, x, w, b, g1, g2, _layout(ops, [[L], [L]], dev))
            plain = _conv_grads(ops, x, w, b, g1, g2, None)
            assert torch.equal(one[0], plain[0]), tag
            lay = _layout(ops, lens, dev)
            dx, dw, db = _conv_grads(ops, x, w, b, g1, g2, lay)
            again = _conv_grads(ops, x, w, b, g1, g2, lay)
            assert all(torch.equal(p, q) for p, q in zip((dx, dw, db), again)), tag + ": two runs differ"
            assert all(bool(torch.isfinite(t).all()) for t in (dx, dw, db))
            # the restatement: the sum of the two gradients is rounded to the io dtype where the kernel reads them
            gsum = g1 if g2 is None else (g1.float() + g2.float()).to(dt)
            start, _ = R.starts_ends(lens)
            lv = R.leaves(dict(x=x.cpu(), w=w.cpu().reshape(Dn, k), b=b.cpu()))
            R.conv_silu(lv["x"], lv["w"], lv["b"], start).backward(gsum.cpu().double())
            # the plain backward on every document alone, dw / db summed in fp64
            ax = torch.zeros(2, L, Dn, dtype=torch.float64)
            aw, ab = torch.zeros(Dn, k, dtype=torch.float64), torch.zeros(Dn, dtype=torch.float64)
            for r, s, e in R.documents(lens):
                d = _conv_grads(ops, x[r:r + 1, s:e].contiguous(), w, b, g1[r:r + 1, s:e].contiguous(),
                                None if g2 is None else g2[r:r + 1, s:e].contiguous(), None)
                ax[r, s:e] = d[0][0].cpu().double()
                aw += d[1].cpu().double().reshape(Dn, k)
                ab += d[2].cpu().double()
            _held(tag + " dx", _err(dx, lv["x"].grad), _err(ax, lv["x"].grad))
            _held(tag + " dw", _err(dw.reshape(Dn, k), lv["w"].grad), _err(aw, lv["w"].grad))
            _held(tag + " db", _err(db, lv["b"].grad), _err(ab, lv["b"].grad))


def test_conv_layout_is_checked(dev, ops):
    x, w, b, _, _ = _conv_inputs(dev, 65, 64, 4, F32, 3)
    lay = _layout(ops, _conv_lens(65), dev)
    with torch.no_grad():
        with pytest.raises(ops.ApertisHipError, match="layout"):
            ops.dwconv_silu(x, w, b, layout=_layout(ops, _conv_lens(64), dev))
        with pytest.raises(ops.ApertisHipError, match="do not go together"):
            ops.dwconv_silu(x, w, b, start=torch.zeros(2, dtype=torch.int32, device=dev), layout=lay)
        with pytest.raises(ops.ApertisHipError, match="layout"):
            ops.dwconv_silu(x, w, b, layout=object())


# ================================================================================================ scan
SCAN_L = 320                                                     # crosses a 256-token super-chunk
SCAN_LENS = [R.lens_from_boundaries(SCAN_L, (16, 37, 38, 39, 64, 256, 319)),       # [37, 38), [38, 39): two one-token documents
             R.lens_from_boundaries(SCAN_L, (1, 100, 257))]
REPLACED = ((0, 16, 37), (0, 64, 256))                           # (row, start, stop) of the documents the isolation run replaces
FORMS = {"lookback": dict(SCAN_LEAN=False, SCAN_LEAN_BWD=False, SCAN_LOOKBACK="all", SCAN_SINGLE_PASS=True),
         "lean": dict(SCAN_LEAN=True, SCAN_LEAN_BWD=True, SCAN_LOOKBACK=False, SCAN_SINGLE_PASS=True),
         "staged_single_pass": dict(SCAN_LEAN=False, SCAN_LEAN_BWD=False, SCAN_LOOKBACK=False, SCAN_SINGLE_PASS=True),
         "staged_two_launch": dict(SCAN_LEAN=False, SCAN_LEAN_BWD=False, SCAN_LOOKBACK=False, SCAN_SINGLE_PASS=False)}
ROWWISE = ("p", "xz", "xc", "logits")                            # inputs [B, L, ...]; the others are parameters


def _scan_inputs(h, dt, seed=11, scale=1.0):
    """p in the model's padded layout [Bt | 0 | C | 0 | dt | 0] (blocks of 64 columns), xz = [xp | z]."""
    g = torch.Generator().manual_seed(seed)
    B, L, N = 2, SCAN_L, 16
    Dn, R_ = h * N, 4 * h
    Wb, Wr = -(-Dn // 64) * 64, 64
    p = scale * torch.randn(B, L, 2 * Wb + Wr, generator=g)
    p[..., Dn:Wb] = 0
    p[..., Wb + Dn:2 * Wb] = 0
    p[..., 2 * Wb + R_:] = 0
    i = dict(p=p.to(dt), xz=(scale * torch.randn(B, L, 2 * Dn, generator=g)).to(dt), xc=(scale * torch.randn(B, L, Dn, generator=g)).to(dt),
             logits=scale * torch.randn(B, L, h, generator=g) - 2.0, W=0.3 * torch.randn(h, R_, generator=g),
             b=torch.randn(h, generator=g) - 2.0, A_log=torch.empty(h, N).uniform_(math.log(0.5), math.log(0.99), generator=g),
             D=1.0 + 0.2 * torch.randn(Dn, generator=g), dout=(scale * torch.randn(B, L, Dn, generator=g)).to(dt))
    return i, dict(Dn=Dn, Wb=Wb, Wr=Wr, R=R_, h=h)


def _scan_run(ops, dev, i, m, op, lens, form):
    """One forward + backward of ops.scan_gate_dt ("dt") or ops.scan_gate ("logits") in the given form; lens None: no layout."""
    for k, v in FORMS[form].items():
        setattr(ops, k, v)
    names = [n for n in i if n != "dout" and not (op == "dt" and n == "logits") and not (op == "logits" and n in ("W", "b"))]
    lv = {n: i[n].to(dev).requires_grad_(True) for n in names}
    Btp, Cp, dt_in, _ = ops.split_cols(lv["p"], (m["Wb"], m["Wb"], m["R"], m["Wr"] - m["R"]))
    _xp, z = ops.split_cols(lv["xz"], (m["Dn"], m["Dn"]))
    lay = None if lens is None else _layout(ops, lens, dev)
    if op == "dt":
        out = ops.scan_gate_dt(dt_in, lv["W"], lv["b"], lv["A_log"], Btp, Cp, lv["xc"], z, lv["D"], layout=lay)
    else:
        out = ops.scan_gate(lv["logits"], lv["A_log"], Btp, Cp, lv["xc"], z, lv["D"], delta_softplus=True, layout=lay)
    out.backward(i["dout"].to(dev))
    assert ops.scan_gate_error() == 0
    return out.detach(), {n: v.grad for n, v in lv.items()}


_RESTATED = {}


def _restated(i, m, op, key):
    """The fp64 restatement of the packed run and its gradients, computed once per (shape, dtype, op) and shared by the forms."""
    if key not in _RESTATED:
        names = [n for n in i if n != "dout" and not (op == "dt" and n == "logits") and not (op == "logits" and n in ("W", "b"))]
        lv = R.leaves({n: i[n] for n in names})
        Dn, Wb, R_ = m["Dn"], m["Wb"], m["R"]
        logits = lv["p"][..., 2 * Wb:2 * Wb + R_] @ lv["W"].t() + lv["b"] if op == "dt" else lv["logits"]
        start, _ = R.starts_ends(SCAN_LENS)
        out = R.scan_gate(logits, lv["A_log"], lv["p"][..., :Dn], lv["p"][..., Wb:Wb + Dn], lv["xc"], lv["xz"][..., Dn:], lv["D"], start)
        out.backward(i["dout"].double())
        _RESTATED[key] = (out.detach(), {n: v.grad for n, v in lv.items()})
    return _RESTATED[key]


@pytest.mark.parametrize("h", [11, 4], ids=["Dn176", "Dn64"])
@pytest.mark.parametrize("form,dt", [(f, BF16) for f in FORMS] + [("staged_single_pass", F32), ("staged_two_launch", F32)],
                         ids=[f + "-bf16" for f in FORMS] + ["staged_single_pass-fp32", "staged_two_launch-fp32"])
def test_scan_under_a_layout(dev, ops, form, dt, h):
    i, m = _scan_inputs(h, dt)
    first = R.starts_ends(SCAN_LENS)[0] == torch.arange(SCAN_L).view(1, -1)
    first[:, 0] = False                                          # the rows of the document starts at t >= 1
    other = torch.ones(2, SCAN_L, dtype=torch.bool)
    for r, s, e in REPLACED:
        other[r, s:e] = False
    j, _ = _scan_inputs(h, dt, seed=12, scale=3.0)               # other finite values for the replaced documents
    swapped = {n: v.clone() for n, v in i.items()}
    for n in ROWWISE + ("dout",):
        for r, s, e in REPLACED:
            swapped[n][r, s:e] = j[n][r, s:e]
    for op in ("dt", "logits"):
        tag = f"scan {form} {dt} Dn={m['Dn']} op={op}"
        out, g = _scan_run(ops, dev, i, m, op, SCAN_LENS, form)
        # (i) everything is finite, dA_log included
        assert bool(torch.isfinite(out).all()) and all(bool(torch.isfinite(v).all()) for v in g.values()), tag
        # (ii) nothing reaches the delta logits of the document starts
        if op == "logits":
            assert float(g["logits"][first.to(dev)].abs().max()) == 0.0, tag
            assert float(g["logits"][~first.to(dev)].abs().max()) > 0.0
        else:
            dt_cols = g["p"][..., 2 * m["Wb"]:2 * m["Wb"] + m["R"]]
            assert float(dt_cols[first.to(dev)].abs().max()) == 0.0 and float(dt_cols[~first.to(dev)].abs().max()) > 0.0, tag
        # (iii) the other documents do not see the replaced ones: bit-identical outputs and row-wise gradients
        out2, g2 = _scan_run(ops, dev, swapped, m, op, SCAN_LENS, form)
        keep = other.to(dev)
        assert torch.equal(out[keep], out2[keep]) and not torch.equal(out[~keep], out2[~keep]), tag
        for n in ROWWISE:
            if n in g:
                assert torch.equal(g[n][keep], g2[n][keep]), f"{tag}: d{n} of the other documents changed"
        # (iv) against the fp64 restatement, held to twice the error of the same op on the documents alone
        ref_out, ref_g = _restated(i, m, op, (h, dt, op))
        a_out = torch.zeros_like(ref_out)
        a_g = {n: torch.zeros_like(v) for n, v in ref_g.items()}
        for r, s, e in R.documents(SCAN_LENS):
            one = {n: (v[r:r + 1, s:e].contiguous() if n in ROWWISE + ("dout",) else v) for n, v in i.items()}
            o, gg = _scan_run(ops, dev, one, m, op, None, form)
            a_out[r, s:e] = o[0].cpu().double()
            for n, v in gg.items():
                if n in ROWWISE:
                    a_g[n][r, s:e] = v[0].cpu().double()
                else:
                    a_g[n] += v.cpu().double()
        _held(tag + " out", _err(out, ref_out), _err(a_out, ref_out))
        for n in ref_g:
            _held(f"{tag} d{n}", _err(g[n], ref_g[n]), _err(a_g[n], ref_g[n]))


def test_scan_refusals_under_a_layout(dev, ops):
    i, m = _scan_inputs(4, BF16)
    lay = _layout(ops, SCAN_LENS, dev)
    t = {n: v.to(dev) for n, v in i.items()}
    Btp, Cp, dt_in = t["p"][..., :m["Wb"]], t["p"][..., m["Wb"]:2 * m["Wb"]], t["p"][..., 2 * m["Wb"]:2 * m["Wb"] + m["R"]]
    z = t["xz"][..., m["Dn"]:]
    h0 = torch.zeros(2, m["Dn"], device=dev)
    with torch.no_grad():
        for kw in (dict(h0=h0), dict(return_last=True)):
            with pytest.raises(ops.ApertisHipError, match="no h0 and no return_last"):
                ops.scan_gate_dt(dt_in, t["W"], t["b"], t["A_log"], Btp, Cp, t["xc"], z, t["D"], layout=lay, **kw)
            with pytest.raises(ops.ApertisHipError, match="no h0 and no return_last"):
                ops.scan_gate(t["logits"], t["A_log"], Btp, Cp, t["xc"], z, t["D"], delta_softplus=True, layout=lay, **kw)
        with pytest.raises(ops.ApertisHipError, match="delta_softplus"):
            ops.scan_gate(t["logits"], t["A_log"], Btp, Cp, t["xc"], z, t["D"], delta_softplus=False, layout=lay)
        ops.SCAN_DT_FUSED = True
        with pytest.raises(ops.ApertisHipError, match="SCAN_DT_FUSED"):
            ops.scan_gate_dt(dt_in, t["W"], t["b"], t["A_log"], Btp, Cp, t["xc"], z, t["D"], layout=lay)
        ops.SCAN_DT_FUSED = False
        # the caller's logits are not written: the kernels read a copy that carries the reset values
        before = t["logits"].clone()
        ops.scan_gate(t["logits"], t["A_log"], Btp, Cp, t["xc"], z, t["D"], delta_softplus=True, layout=lay)
        assert torch.equal(t["logits"], before)


# ================================================================================================ model
M_LENS = ([5, 92], [96, 1], [40, 17, 40])          # rows of 97 tokens: boundaries inside a tile, on a tile edge, one-token documents
M_L = 97
VARIANTS = {"dense": {}, "rmsnorm_swiglu": dict(use_rmsnorm=True, use_swiglu=True),
            "experts": dict(use_expert_system=True, num_experts=4, experts_per_token=2)}


def _model(dev, **kw):
    import apertis_llm_amd as A
    base = dict(vocab_size=512, hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128,
                attention_type="selective_ssm", position_embedding_type="rotary", max_position_embeddings=128,
                hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    base.update(kw)
    torch.manual_seed(0)
    return A.ApertisForCausalLM(A.ApertisConfig(**base)).to(dev)


def _batch(dev):
    gen = torch.Generator().manual_seed(3)
    ids = torch.randint(4, 512, (len(M_LENS), M_L), generator=gen).to(dev)
    return ids, R.document_ids(M_LENS).to(dev)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_packed_logits_equal_the_documents_alone(dev, ops, variant):
    model = _model(dev, **VARIANTS[variant]).eval()
    ids, docs = _batch(dev)
    with torch.no_grad():
        logits = model(input_ids=ids, document_ids=docs)[1]
        alone = {(b, s): model(input_ids=ids[b:b + 1, s:e])[1][0] for b, s, e in R.documents(M_LENS)}
        for b, s, e in R.documents(M_LENS):
            rel_error_report(f"packed ssm logits {variant} row {b} tokens {s}..{e - 1}", logits[b, s:e], alone[(b, s)], rtol=1e-4)
        assert not torch.allclose(logits, model(input_ids=ids)[1], rtol=1e-3, atol=1e-3)      # not the rows as one sequence each
        # bf16 autocast: held to twice the alone run's own error against fp32
        with torch.autocast("cuda", dtype=torch.bfloat16):
            lp = model(input_ids=ids, document_ids=docs)[1].float()
            e_packed = e_alone = 0.0
            for b, s, e in R.documents(M_LENS):
                e_alone = max(e_alone, _err(model(input_ids=ids[b:b + 1, s:e])[1][0].float(), alone[(b, s)]))
                e_packed = max(e_packed, _err(lp[b, s:e], alone[(b, s)]))
        _held(f"packed ssm logits bf16 autocast {variant}", e_packed, e_alone)


def _loss_and_grads(model, **kw):
    model.zero_grad(set_to_none=True)
    loss = model(**kw)[0]
    loss.backward()
    return float(loss), {n: p.grad.detach().double().cpu() for n, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_packed_loss_and_gradients_are_the_documents_weighted_sums(dev, ops, variant):
    """Experts in eval mode: routing noise, capacity and the auxiliary losses are per batch in training, as for any batch."""
    model = _model(dev, **VARIANTS[variant])
    model = model.eval() if variant == "experts" else model.train()
    ids, docs = _batch(dev)
    labels = ids.clone()
    labels[0, 10:20] = -100                                              # some ignored targets inside a document
    loss, grads = _loss_and_grads(model, input_ids=ids, labels=labels, document_ids=docs)
    counts = {(b, s): int((labels[b, s:e][1:] != -100).sum()) for b, s, e in R.documents(M_LENS)}
    total = sum(counts.values())
    want, wg = 0.0, {n: torch.zeros_like(g) for n, g in grads.items()}
    for b, s, e in R.documents(M_LENS):
        if counts[(b, s)]:
            l_i, g_i = _loss_and_grads(model, input_ids=ids[b:b + 1, s:e], labels=labels[b:b + 1, s:e])
            want += l_i * counts[(b, s)] / total
            for n, g in g_i.items():
                wg[n] += g * (counts[(b, s)] / total)
    assert abs(loss - want) <= 1e-4 * abs(want), (loss, want)
    assert grads.keys() == wg.keys() and len(grads) > 0
    for n in grads:
        rel_error_report(f"packed ssm grad fp32 {variant} {n}", grads[n], wg[n], rtol=1e-4)
    # a checkpointed layer is recomputed with the same layout: the same gradients
    if variant != "experts":
        model.model.gradient_checkpointing = True
        loss_c, grads_c = _loss_and_grads(model, input_ids=ids, labels=labels, document_ids=docs)
        assert loss_c == loss
        for n in grads:
            torch.testing.assert_close(grads_c[n], grads[n], rtol=1e-5, atol=1e-7, msg=n)


def test_model_refusals_with_the_switch_on(dev, ops):
    model = _model(dev).eval()
    ids, docs = _batch(dev)
    mask = torch.ones_like(ids)
    mask[0, 90:] = 0
    with torch.no_grad():
        past = model(input_ids=ids[:, :8], use_cache=True)[4]
        for kw in (dict(past_key_values=past), dict(use_cache=True), dict(pixel_values=torch.zeros(3, 3, 8, 8, device=dev)),
                   dict(attention_mask=mask), dict(output_attentions=True), dict(document_ids=docs.flip(1))):
            with pytest.raises(ValueError):
                model(**{**dict(input_ids=ids, document_ids=docs), **kw})
        with pytest.raises(ValueError, match="generate"):
            model.generate(input_ids=ids, document_ids=docs, max_new_tokens=2)
        assert model(input_ids=ids, document_ids=docs)[4] is None                      # no cache comes back
        ops.SSM_PACKED = False
        with pytest.raises(ValueError, match="is off"):
            model(input_ids=ids, document_ids=docs)


def test_trainer_packs_sequences_for_a_selective_ssm_model(dev, ops, tmp_path):
    from apertis_llm_amd import data as D
    from apertis_llm_amd.trainer import ApertisTrainer
    words = list("abcdefgh")
    path = tmp_path / "d.jsonl"
    path.write_text("\n".join(json.dumps({"text": " ".join(words[(i + j) % 8] for j in range(n))})
                              for i, n in enumerate([3, 5, 2, 6, 4, 1, 7, 3, 2, 5])), encoding="utf-8")
    train = D.ApertisPretrainDataset(str(path), {c: i + 4 for i, c in enumerate(words)}, 16, max_length=16)
    model = _model(dev, vocab_size=16, max_position_embeddings=64)
    t = ApertisTrainer(model, train, None, output_dir=str(tmp_path / "out"), batch_size=2, learning_rate=1e-2, num_epochs=2,
                       gradient_accumulation_steps=1, fp16=False, device=str(dev), checkpoint_steps=0, shuffle=False, num_workers=0,
                       pack_sequences=True)
    assert isinstance(t.train_dataset, D.PackedDataset) and len(t.train_dataset) == 3 < len(train)
    t.train()
    assert len(t.history["loss"]) == 4 and all(torch.isfinite(torch.tensor(t.history["loss"])))     # 2 steps per epoch
    assert t.history["loss"][-1] <= t.history["loss"][0]
    assert ops.scan_gate_error() == 0
