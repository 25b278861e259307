"""Left-padded selective_ssm prefills on the GPU (ops.ssm.SSM_LEFT_PAD): every row of a left-padded batch gets what it gets alone.

  1. the kernel, apertis_dwconv_silu_start_fwd through ops.dwconv_silu(start=...): rows before a sequence's start are exact
     zeros and never read (the inputs there are NaN), the rows from it on carry the BITS the plain forward gives that row as a
     sequence of its own (the same k-term sum, term for term: no tolerance), starts of 0 give the plain forward's output,
     a start of L gives zeros - at Dn 12 (three chunks, one work-group per tile) and 176 (the bench's), every conv width class
     (2, 4, 8, 16), both dtypes, dense rows and the model's xz view, L = 70 (two tiles, the second ragged) and starts in the
     first tile, at a tile's first row and inside the second
  2. the layer: the state after a pad prefix is exactly 0 (so is the output there), h_last / the valid output rows / the
     cached conv window against the same row alone on the stock path, through the staged scan (fp32) and the look-back scan
     (bf16 autocast, Dn 176)
  3. the model and generate(): greedy tokens of every row equal its alone run's through the graph tail with one row finishing
     on the way, prefill logits at the 1e-4 bar; with the switch off the start form is never reached and a padded row differs
     from its alone run (the defect); chat's sampling runs on the fused sampler; a multimodal call and an absolute-position
     model stay on the stock path
"""
import functools

import pytest
import torch

from conftest import rel_error_report

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture
def ops():
    from apertis_llm_amd import ops
    prev = ops.SSM_LEFT_PAD
    yield ops
    ops.SSM_LEFT_PAD = prev


def _spy_start(monkeypatch, ops):
    """Every call of the start form of the conv, as (B, L, Dn, starts)."""
    calls, real = [], ops.ssm._dwconv_silu_start

    def spy(x, w, b, start):
        calls.append(tuple(x.shape) + (start.tolist(),))
        return real(x, w, b, start)
    monkeypatch.setattr(ops.ssm, "_dwconv_silu_start", spy)
    return calls


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the kernel
KB, KL, STARTS = 4, 70, [0, 5, 64, 67]


def _conv_inputs(dev, Dn, k, dt, layout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(KB, KL, Dn, generator=g).to(dt)
    w = (torch.randn(Dn, 1, k, generator=g) * 0.5).to(dev)
    b = (torch.randn(Dn, generator=g) * 0.5).to(dev)
    if layout == "xz":                                   # the model's form: x = xz[..., :Dn], row stride 2 Dn, z never read
        buf = torch.full((KB, KL, 2 * Dn), float("nan"), dtype=dt)
        buf[..., :Dn] = x
        x = buf.to(dev)[..., :Dn]
    else:
        x = x.to(dev)
    return x, w, b


@pytest.mark.parametrize("layout", ["dense", "xz"])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("k", [2, 4, 8, 16])
@pytest.mark.parametrize("Dn", [12, 176, 272])     # (272: 68 chunks per row - two channel blocks, the second four chunks wide)
def test_start_kernel_is_the_plain_forward_of_every_row_alone(dev, ops, Dn, k, dt, layout):
    x, w, b = _conv_inputs(dev, Dn, k, dt, layout, 100 * Dn + k)
    start = torch.tensor(STARTS, dtype=torch.int32, device=dev)
    with torch.no_grad():
        plain = ops.dwconv_silu(x, w, b)
        # all starts 0: the plain forward's bits
        zero = ops.dwconv_silu(x, w, b, start=torch.zeros(KB, dtype=torch.int32, device=dev))
        assert zero.shape == plain.shape and zero.dtype == dt and torch.equal(zero, plain)
        # the pads hold NaN: a pad that is loaded - as a tap of a valid row or on the way to a pad row's output - shows
        xp = x.clone() if layout == "dense" else x
        for r, s in enumerate(STARTS):
            xp[r, :s] = float("nan")
        got = ops.dwconv_silu(xp, w, b, start=start)
        assert got.is_contiguous() and tuple(got.shape) == (KB, KL, Dn)
        for r, s in enumerate(STARTS):
            assert bool((got[r, :s] == 0).all()), f"row {r}: a pad output is not zero"
            alone = ops.dwconv_silu(xp[r:r + 1, s:], w, b)
            assert torch.equal(got[r, s:], alone[0]), f"row {r} from its start {s} on differs from the row alone"
        # one row that is all pad (start = L; a start past L is clamped to it)
        for last in (KL, KL + 9):
            ends = torch.tensor([0, KL - 1, last, STARTS[3]], dtype=torch.int32, device=dev)
            xe = xp.clone()
            xe[2] = float("nan")
            got = ops.dwconv_silu(xe, w, b, start=ends)
            assert bool((got[2] == 0).all()) and bool(torch.isfinite(got[0]).all())
            assert torch.equal(got[1, KL - 1:], ops.dwconv_silu(xe[1:2, KL - 1:], w, b)[0]) and bool((got[1, :KL - 1] == 0).all())


def test_start_form_checks_its_arguments(dev, ops):
    x, w, b = _conv_inputs(dev, 12, 4, F32, "dense", 1)
    start = torch.zeros(KB, dtype=torch.int32, device=dev)
    with torch.no_grad():
        for bad in (start.long(), start[:3], start.reshape(KB, 1)):
            with pytest.raises(ops.ApertisHipError, match="start must be int32"):
                ops.dwconv_silu(x, w, b, start=bad)
        with pytest.raises(ops.ApertisHipError, match="no CPU fallback"):
            ops.dwconv_silu(x, w, b, start=start.cpu())
        for k in (1, 17):
            with pytest.raises(ops.ApertisHipError):
                ops.dwconv_silu(x, torch.randn(12, 1, k, device=dev), b, start=start)
    with pytest.raises(ops.ApertisHipError, match="forward only"):
        ops.dwconv_silu(x.clone().requires_grad_(), w, b, start=start)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the layer
LL, LSTARTS = 130, [0, 3, 64, 127]                      # valid lengths 130, 127, 66 and 3 = k - 1


def _layer(dev, heads):
    import apertis_llm_amd as A
    torch.manual_seed(11 + heads)
    cfg = A.ApertisConfig(hidden_size=16 * heads, num_attention_heads=heads, attention_type="selective_ssm", ssm_d_state=16)
    layer = A.model.SelectiveLinearAttention(cfg).eval()
    with torch.no_grad():
        layer.conv1d.bias.uniform_(-0.5, 0.5)           # (the pollution comes through the bias: make it large)
    x = torch.randn(len(LSTARTS), LL, 16 * heads)
    return layer.to(dev), x.to(dev)


def _spy_lookback(monkeypatch, ops):
    """Whether the look-back scan took each scan launch (ops.scan._try_launch is its only caller's helper)."""
    took, real = [], ops.scan._try_launch

    def spy(*a, **k):
        took.append(real(*a, **k))
        return took[-1]
    monkeypatch.setattr(ops.scan, "_try_launch", spy)
    return took


@pytest.mark.parametrize("heads,bf16", [(4, False), (11, True)], ids=["staged-f32", "lookback-bf16"])
def test_layer_rows_equal_the_rows_alone(dev, ops, monkeypatch, heads, bf16):
    import apertis_llm_amd as A
    layer, x = _layer(dev, heads)
    Dn, kw = 16 * heads, layer.conv_kernel_size
    assert kw == 4 and LL - LSTARTS[-1] == kw - 1
    took = _spy_lookback(monkeypatch, ops)
    calls = _spy_start(monkeypatch, ops)

    def run(xs, starts=None, autocast=bf16):
        mask = A.model._SsmStarts(torch.tensor(starts, dtype=torch.int32, device=dev)) if starts is not None else None
        with torch.no_grad(), torch.autocast("cuda", dtype=BF16, enabled=autocast):
            out, _, (window, h_last) = layer(xs, attention_mask=mask, use_cache=True)
        return out.float(), window, h_last
    out, window, h_last = run(x, LSTARTS)
    assert calls == [(len(LSTARTS), LL, Dn, LSTARTS)]
    assert took == ([True] if bf16 else []), "not the scan form this case is about"
    assert tuple(window.shape) == (len(LSTARTS), Dn, kw - 1) and tuple(h_last.shape) == (len(LSTARTS), heads, 16)
    for r, s in enumerate(LSTARTS):
        tag = f"ssm left pad layer {'bf16' if bf16 else 'f32'} Dn{Dn} row {r} start {s}"
        if s:
            # the state after the pad prefix, and everything the layer gives for it: exactly zero
            assert bool((out[r, :s] == 0).all())
            o_pad, _, h_pad = run(x[r:r + 1, :s], [s])
            assert bool((h_pad == 0).all()) and bool((o_pad == 0).all())
        a_out, a_window, a_h = run(x[r:r + 1, s:])           # the row alone, on the stock path
        assert torch.equal(window[r], a_window[0]), f"{tag}: cached conv window"
        if not bf16:
            rel_error_report(tag + " h_last", h_last[r], a_h[0], rtol=1e-4)
            rel_error_report(tag + " output", out[r, s:], a_out[0], rtol=1e-4)
        else:
            r_out, _, r_h = run(x[r:r + 1, s:], autocast=False)      # fp32 alone: the reference of both bf16 runs
            for name, got, base, ref in (("h_last", h_last[r], a_h[0], r_h[0]), ("output", out[r, s:], a_out[0], r_out[0])):
                rep = rel_error_report(f"{tag} {name} (batch, bf16)", got, ref, check=False)
                srep = rel_error_report(f"{tag} {name} (alone, bf16)", base, ref, check=False)
                assert rep["max_abs"] <= 2 * srep["max_abs"] + 1e-6 * rep["ref_absmax"], (name, rep, srep)
    assert len(calls) == 1 + sum(1 for s in LSTARTS if s)      # the alone runs took the plain conv
    # the switch-off form of the same batch: the pads reach the state (what the switch is for)
    _, _, h_off = run(x)
    assert not torch.allclose(h_off[1:], h_last[1:], rtol=1e-3, atol=1e-5)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the model and generate()
PL, LENS, NEW, VOCAB = 20, [20, 17, 9, 3], 30, 64
# Weights: oracle.seeded's rule with a gain on the matrices.  At the constructor's std 0.02 this tiny model repeats one token
# whatever came before - the pads change no token and the defect cannot show; at these gains every row emits some 20 distinct
# tokens.  Chosen on the CPU oracle (fp64, greedy by full forwards, which is not the cached step's arithmetic to the letter:
# a guide): the alone runs' smallest top-2 gap there is 3.0e-3 (dense) and 3.6e-3 (moe) of the largest logit, row 0 emits its
# step-5 token there first and the other rows late or never, and the padded batch changes 27 to 30 of the 30 tokens of every
# padded row.  On the GPU the gaps are 2.2e-3 and 3.4e-3; the test asserts 1e-3 before it compares a token.
GAIN = {"dense": 12.0, "moe": 16.0, "absolute": 12.0, "multimodal": 12.0}


@functools.lru_cache(maxsize=None)
def _model(kind):
    """2 layers, hidden 64, 4 heads (Dn 64), vocab 64, fp32, eval; 'dense', 'moe' (4 experts, top 2), 'absolute' (position
    embeddings) or 'multimodal'."""
    import apertis_llm_amd as A
    from oracle import seeded
    kw = {"dense": {}, "moe": dict(use_expert_system=True, num_experts=4, experts_per_token=2),
          "absolute": dict(position_embedding_type="absolute"),
          "multimodal": dict(multimodal=True, image_size=16, vision_embed_dim=32, vision_patch_size=8, vision_layers=1,
                             vision_heads=2)}[kind]
    cfg = A.ApertisConfig(vocab_size=VOCAB, hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128,
                          attention_type="selective_ssm", max_position_embeddings=128, **kw)
    model = A.ApertisForCausalLM(cfg).eval()
    model.load_state_dict(seeded.fill_state_dict(model.state_dict(), gain=GAIN[kind]))
    return model.to(torch.device("cuda:0"))


def _batch(dev):
    ids = torch.randint(4, VOCAB, (len(LENS), PL), generator=torch.Generator().manual_seed(3))
    mask = torch.ones_like(ids)
    for b, n in enumerate(LENS):
        mask[b, :PL - n] = 0
        ids[b, :PL - n] = 0
    return ids.to(dev), mask.to(dev)


def _generate(model, ids, mask, eos=-1, **kw):
    kw = {**dict(do_sample=False), **kw}
    return model.generate(input_ids=ids, attention_mask=mask, max_new_tokens=NEW, eos_token_id=eos, pad_token_id=0, **kw)


@functools.lru_cache(maxsize=None)
def _alone(kind):
    """Every row of the batch alone, without padding, on the eager loop (so that every step's logits can be looked at):
    (tokens [NEW] per row, prefill logits per row, the smallest top-2 gap over all steps as a share of the largest logit)."""
    import apertis_llm_amd as A
    model, dev = _model(kind), torch.device("cuda:0")
    ids, _ = _batch(dev)
    toks, prefill, gap = [], [], float("inf")
    graph, A.model.DECODE_GRAPH = A.model.DECODE_GRAPH, False
    fwd = model.forward
    try:
        for b, n in enumerate(LENS):
            steps = []

            def spy(*a, **k):
                out = fwd(*a, **k)
                steps.append(out[1].detach().float().clone())
                return out
            model.forward = spy
            row = ids[b:b + 1, PL - n:]
            out = _generate(model, row, torch.ones_like(row))
            assert tuple(out.shape) == (1, n + NEW) and len(steps) == NEW
            toks.append(out[0, n:].clone())
            prefill.append(steps[0][0])
            last = torch.stack([s[0, -1] for s in steps])
            top2 = torch.topk(last, 2, dim=-1).values
            gap = min(gap, float(((top2[:, 0] - top2[:, 1]) / last.abs().amax(-1)).min()))
    finally:
        del model.forward
        A.model.DECODE_GRAPH = graph
    return toks, prefill, gap


def _expected(toks, eos, pad=0):
    """The alone runs' tokens as generate() hands them back with `eos` set: a row's tokens up to and with its first eos,
    `pad` after it."""
    rows = []
    for t in toks:
        t = t.clone()
        hit = (t == eos).nonzero()
        if len(hit):
            t[int(hit[0]) + 1:] = pad
        rows.append(t)
    return torch.stack(rows)


@pytest.mark.parametrize("kind", ["dense", "moe"])
def test_generate_gives_every_row_its_alone_run(dev, ops, monkeypatch, kind):
    import apertis_llm_amd as A
    model = _model(kind)
    ids, mask = _batch(dev)
    toks, prefill, gap = _alone(kind)
    print(f"alone runs ({kind}): smallest top-2 gap {gap:.3e} of the largest logit")
    assert gap > 1e-3, "a near-tie in an alone run: pick other weights (GAIN)"
    eos = int(toks[0][5])                                    # row 0 finishes at step 5 at the latest, mid-way
    want = _expected(toks, eos)
    assert bool((want[0] == 0).any()) and not bool((want == 0).all(1).any())
    assert NEW - 1 >= A.model.DECODE_GRAPH_MIN_STEPS and A.model.DECODE_GRAPH
    calls = _spy_start(monkeypatch, ops)
    tails, tail = [], A.model.ApertisForCausalLM._generate_graph_tail
    monkeypatch.setattr(A.model.ApertisForCausalLM, "_generate_graph_tail",
                        lambda self, *a, **k: (tails.append(1), tail(self, *a, **k))[1])
    pads = [PL - n for n in LENS]

    # the switch on: every row its alone run's tokens, through the graph tail
    ops.SSM_LEFT_PAD = True
    got = _generate(model, ids, mask, eos)
    assert calls == [(len(LENS), PL, 64, pads)] * 2 and tails == [1]       # the prefill, once per layer
    assert tuple(got.shape) == (len(LENS), PL + NEW) and torch.equal(got[:, :PL], ids)
    assert torch.equal(got[:, PL:], want), (got[:, PL:], want)
    with torch.no_grad():
        logits = model(input_ids=ids, attention_mask=mask, use_cache=True)[1]
    for b, n in enumerate(LENS):
        rel_error_report(f"ssm left pad {kind} prefill logits row {b} ({n} tokens)", logits[b, PL - n:], prefill[b], rtol=1e-4)

    # the switch off: the stock path - the mask is not looked at - and the defect
    del calls[:], tails[:]
    ops.SSM_LEFT_PAD = False
    off = _generate(model, ids, mask, eos)
    assert calls == [] and tails == [1]
    assert torch.equal(off, _generate(model, ids, None, eos))
    assert torch.equal(off[0, PL:], want[0])                              # the row without padding is fine either way
    assert any(not torch.equal(off[b, PL:], want[b]) for b in range(1, len(LENS))), "no padded row shows the defect"


def test_sampled_generate_runs_on_the_fused_sampler(dev, ops, monkeypatch):
    model = _model("dense")
    ids, mask = _batch(dev)
    calls = _spy_start(monkeypatch, ops)
    draws, real = [], ops.sample.sample_next
    monkeypatch.setattr(ops.sample, "sample_next", lambda *a, **k: (draws.append(k["do_sample"]), real(*a, **k))[1])
    ops.SSM_LEFT_PAD = True
    torch.manual_seed(1)
    got = _generate(model, ids, mask, do_sample=True, temperature=0.7, top_k=50, top_p=0.9)
    assert len(calls) == 2 and len(draws) >= 1 and all(draws)
    assert tuple(got.shape) == (len(LENS), PL + NEW) and torch.equal(got[:, :PL], ids)
    assert int(got.min()) >= 0 and int(got.max()) < VOCAB


@pytest.mark.parametrize("case", ["multimodal", "absolute", "all_valid", "right_padded", "short_row", "grad", "train", "past",
                                  "output_attentions"])
def test_stays_on_the_stock_path(dev, ops, monkeypatch, case):
    """Under the switch, every forward that does not meet all conditions never reaches the start form and gives the
    switch-off run's logits, bit for bit."""
    import contextlib
    model = _model(case if case in ("multimodal", "absolute") else "dense")
    ids, mask = _batch(dev)
    kw = dict(input_ids=ids, attention_mask=mask, use_cache=True)
    grad = contextlib.nullcontext() if case == "grad" else torch.no_grad()
    if case == "multimodal":
        kw["pixel_values"] = torch.randn(len(LENS), 3, 16, 16, generator=torch.Generator().manual_seed(2)).to(dev)
    elif case == "all_valid":
        kw["attention_mask"] = torch.ones_like(mask)
    elif case == "right_padded":
        kw["attention_mask"] = mask.flip(1)
    elif case == "short_row":
        kw["attention_mask"] = mask.clone()
        kw["attention_mask"][3, :PL - 2] = 0                  # two valid tokens: fewer than ssm_conv_kernel - 1
    elif case == "past":
        with torch.no_grad():
            kw["past_key_values"] = model(input_ids=ids[:, :8], use_cache=True)[4]
        kw["input_ids"], kw["attention_mask"] = ids[:, 8:], mask
    elif case == "output_attentions":
        kw["output_attentions"] = True
    calls = _spy_start(monkeypatch, ops)
    outs = []
    try:
        if case == "train":
            model.train()
        for on in (False, True):
            ops.SSM_LEFT_PAD = on
            torch.manual_seed(4)                              # (a training forward draws its dropout seeds from torch's RNG)
            with grad:
                outs.append(model(**kw)[1].detach())
    finally:
        model.eval()
    assert calls == [] and torch.equal(outs[0], outs[1])
