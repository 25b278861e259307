"""generate()'s fused next-token selection (csrc/sampling.hip, ops.sample_next) against the CPU restatement of the reference's
block (tests/sampling_ref.py, core.py:1605-1627), and generate() with sampling / a repetition penalty, eager and through the
decode graph."""
import contextlib
import json

import numpy as np
import pytest
import torch

from conftest import load_golden
from sampling_ref import inverse_cdf, reference_select, sample_u

pytestmark = pytest.mark.gpu


def _ops():
    from apertis_llm_amd import ops
    return ops


def _run(logits, *, alive=None, probs=True, **kw):
    """One sample_next launch; returns (next, alive_out, probs, err, u_out) on the host."""
    ops = _ops()
    B, V = logits.shape
    dev = logits.device
    alive = torch.ones(B, dtype=torch.long, device=dev) if alive is None else alive
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    p = torch.full((B, V), -1.0, device=dev) if probs else None
    u = torch.full((B,), -1.0, dtype=torch.float64, device=dev)
    a_out = torch.empty_like(alive)
    nxt = ops.sample_next(logits, alive, err, alive_out=a_out, probs_out=p, u_out=u, **kw)
    torch.cuda.synchronize()
    return nxt.cpu(), a_out.cpu(), (p.cpu() if probs else None), int(err[0]), u.cpu()


def test_penalty_and_temperature_are_bit_exact(dev):
    """x[0] divided by the penalty c times (then by the temperature) on the device must equal x[1] = the same divisions done
    by fp32 CPU torch, bit for bit: with top_k = 1 both are then kept as a tie (0.5 / 0.5), one ulp apart only one is."""
    ops = _ops()
    torch.manual_seed(0)
    B, V = 64, 96
    x = torch.randn(B, V) - 20.0
    a = torch.randn(B) * 4 + 10
    c = torch.randint(1, 6, (B,))
    counts = torch.zeros(B, V, dtype=torch.int32)
    for pen, temp in [(1.3, 0.7), (1.1, 1.0), (0.9, 0.6)]:
        for b in range(B):
            x[b, 0] = a[b]
            counts[b, 0] = int(c[b])
            v = a[b].clone()
            for _ in range(int(c[b])):
                v = v / pen
            x[b, 1] = v
        _, _, probs, err, _ = _run(x.to(dev), do_sample=True, temperature=temp, top_k=1, repetition_penalty=pen,
                                   counts=counts.to(dev))
        assert err == 0
        assert (probs[:, :2] == 0.5).all() and (probs[:, 2:] == 0).all(), (pen, temp)
    # ... and the occurrence table from a prompt: ids >= V skipped, negative ids wrapped
    toks = torch.tensor([[3, 3, 96, 200, -1, 5], [0, -96, 7, 7, 7, 95]], device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    cnt = ops.token_counts(toks, V, err).cpu()
    want = torch.zeros(2, V, dtype=torch.int32)
    for b, row in enumerate(toks.tolist()):
        for t in row:
            if t < V:
                want[b, t] += 1
    assert torch.equal(cnt, want) and int(err[0]) == 0
    ops.token_counts(torch.tensor([[1, -97]], device=dev), V, err)
    assert int(err[0]) == ops.ERR_TOKEN_ID
    with pytest.raises(IndexError):
        ops.raise_sample_error(int(err[0]))


@pytest.mark.parametrize("bf16", [False, True])
def test_processed_row_is_bit_exact_against_cpu_torch(dev, bf16):
    """x_out (the row after steps 1-2) equals fp32 CPU torch's penalty loop and temperature division bit for bit, for
    penalties and temperatures whose reciprocal is not exact (a multiply by it would be one ulp away), at every row form."""
    ops = _ops()
    g = torch.Generator().manual_seed(7)
    for V in (96, 4000, 8000, 40000):
        B = 3
        base = torch.randn(B, V, generator=g) * 5
        if bf16:
            base = base.bfloat16().float()
        hist = [torch.randint(0, V, (200,), generator=g).tolist() + [1] * 40 for _ in range(B)]
        counts = torch.zeros(B, V, dtype=torch.int32)
        for b in range(B):
            for t in hist[b]:
                counts[b, t] += 1
        logits = base.to(dev, torch.bfloat16 if bf16 else torch.float32)
        for pen, temp, do_sample in [(1.3, 0.7, True), (1.1, 0.6, True), (0.9, 1.7, True), (1.3, 1.0, False), (1.0, 0.3, True)]:
            want, _, _, _ = reference_select(base, hist, penalty=pen, do_sample=do_sample, temperature=temp)
            xo = torch.full((B, V), float("nan"), device=dev)
            err = torch.zeros(1, dtype=torch.int32, device=dev)
            ops.sample_next(logits, torch.ones(B, dtype=torch.long, device=dev), err, do_sample=do_sample,
                            temperature=max(temp, 1e-6) if do_sample else 1.0, repetition_penalty=pen,
                            counts=counts.to(dev) if pen != 1.0 else None, x_out=xo)
            assert torch.equal(xo.cpu(), want), (V, pen, temp, do_sample, float((xo.cpu() - want).abs().max()))


@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 96, 1000, 2048, 8192, 32000, 50257, 131072, 262144])
@pytest.mark.parametrize("bf16", [False, True])
def test_stages_match_the_restatement_across_vocabularies(dev, V, bf16):
    """top-k (ties at the k-th value, k = 1 and k = V), top-p (tie groups at the cut, top_p <= 0) and all four stages together
    on strided rows: the kept set equals the restatement's, the distribution is its fp64 softmax (rtol 1e-5, exact zeros),
    and the token is a kept one."""
    g = torch.Generator().manual_seed(V)
    B = 3
    base = (torch.randn(B, V, generator=g) * 4).round() / 4          # quarter steps: many exact ties
    if bf16:
        base = base.bfloat16().float()
    wide = torch.zeros(B, V + 8)
    wide[:, 5:5 + V] = base
    dt = torch.bfloat16 if bf16 else torch.float32
    logits = wide.to(dev, dt)[:, 5:5 + V]                           # row stride V + 8
    hist = [torch.randint(0, V, (30,), generator=g).tolist() for _ in range(B)]
    counts = torch.zeros(B, V, dtype=torch.int32)
    for b in range(B):
        for t in hist[b]:
            counts[b, t] += 1
    cases = [dict(top_k=1), dict(top_k=V), dict(top_k=min(7, V)), dict(top_p=0.0), dict(top_p=-0.5), dict(top_p=0.5),
             dict(top_p=0.9), dict(top_k=min(20, V), top_p=0.9, temperature=0.7, repetition_penalty=1.3)]
    for case in cases:
        pen = case.get("repetition_penalty", 1.0)
        x, keep, probs, _ = reference_select(base, hist, penalty=pen, do_sample=True, temperature=case.get("temperature", 1.0),
                                             top_k=case.get("top_k", 0), top_p=case.get("top_p", 1.0))
        nxt, _, p, err, _ = _run(logits, do_sample=True, counts=counts.to(dev) if pen != 1.0 else None, **case)
        assert err == 0, case
        assert torch.equal(p > 0, keep), (V, bf16, case, int((p > 0).sum()), int(keep.sum()))
        assert torch.allclose(p.double()[keep], probs[keep], rtol=1e-5, atol=0), case
        assert (p[~keep] == 0).all()
        assert all(bool(keep[b, int(nxt[b])]) for b in range(B)), case
    with pytest.raises(RuntimeError):
        _run(logits, do_sample=True, top_k=V + 1)


def test_unsupported_vocabulary_is_refused(dev):
    ops = _ops()
    x = torch.zeros(1, ops.SAMPLE_MAX_VOCAB + 1, device=dev)
    assert not ops.sample_supported(x) and ops.sample_supported(x[:, :-1])
    with pytest.raises(ops.ApertisHipError):
        _run(x, do_sample=True)


@pytest.mark.parametrize("B", [1, 3, 16, 64])
def test_batch_sizes_and_greedy_argmax(dev, B):
    """Greedy with a penalty: torch.argmax of the penalised row (lowest index among equal maxima); sampling: a kept token."""
    g = torch.Generator().manual_seed(B)
    V = 1000
    base = (torch.randn(B, V, generator=g) * 2).round()
    hist = [torch.randint(0, V, (50,), generator=g).tolist() for _ in range(B)]
    counts = torch.zeros(B, V, dtype=torch.int32)
    for b in range(B):
        for t in hist[b]:
            counts[b, t] += 1
    x, _, _, _ = reference_select(base, hist, penalty=1.3, do_sample=False)
    nxt, _, _, err, _ = _run(base.to(dev), do_sample=False, repetition_penalty=1.3, counts=counts.to(dev), probs=False)
    assert err == 0 and torch.equal(nxt, torch.argmax(x, dim=-1))
    _, keep, _, _ = reference_select(base, None, do_sample=True, temperature=0.7, top_k=50, top_p=0.9)
    nxt, _, _, err, _ = _run(base.to(dev), do_sample=True, temperature=0.7, top_k=50, top_p=0.9, seed=5)
    assert err == 0 and all(bool(keep[b, int(nxt[b])]) for b in range(B))


def test_draw_is_the_inverse_cdf_at_explicit_uniforms(dev):
    """On a grid of uniforms the token is the fp64 inverse CDF in vocabulary order wherever u is more than 1e-6 from a step,
    and never a removed token; the step counter selects the uniforms' column and is only read."""
    torch.manual_seed(1)
    B, V, S = 4, 500, 64
    base = torch.randn(B, V) * 2
    _, keep, probs, _ = reference_select(base, None, do_sample=True, temperature=0.8, top_k=40, top_p=0.95)
    grid = torch.rand(B, S, dtype=torch.float64)
    grid[:, :4] = torch.tensor([0.0, 1e-9, 0.5, 1 - 1e-12], dtype=torch.float64)
    uni = grid.to(dev)
    step = torch.zeros(1, dtype=torch.long, device=dev)
    checked = 0
    for s in range(S):
        nxt, _, _, err, u = _run(base.to(dev), do_sample=True, temperature=0.8, top_k=40, top_p=0.95, uniforms=uni, step=step,
                                 step_off=s, probs=False)
        assert err == 0 and int(step[0]) == 0
        for b in range(B):
            assert float(u[b]) == float(grid[b, s])
            assert bool(keep[b, int(nxt[b])])
            i, d = inverse_cdf(probs[b].numpy(), float(grid[b, s]))
            if d > 1e-6:
                assert int(nxt[b]) == i, (b, s)
                checked += 1
    assert checked > 0.9 * B * S
    _, _, _, err, _ = _run(base.to(dev), do_sample=True, uniforms=uni, step=step, step_off=S, probs=False)
    assert err == _ops().ERR_UNIFORMS


def test_counter_hash_and_determinism(dev):
    """u_out equals the numpy copy of the hash of (seed, row, step); the same inputs give the same bits twice; over many rows
    of one 8-token distribution the kernel's own draws land within 5 sigma of every probability."""
    B, V = 8192, 8
    logits = torch.log(torch.tensor([0.3, 0.2, 0.15, 0.1, 0.1, 0.08, 0.05, 0.02])).repeat(B, 1).to(dev)
    step = torch.full((1,), 7, dtype=torch.long, device=dev)
    a = _run(logits, do_sample=True, seed=0xDEADBEEF12345, step=step, step_off=3)
    b = _run(logits, do_sample=True, seed=0xDEADBEEF12345, step=step, step_off=3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[4], b[4])
    for r in (0, 1, 17, 4095, 8191):
        assert float(a[4][r]) == sample_u(0xDEADBEEF12345, r, 10)
    p = a[2][0].double().numpy()
    freq = np.bincount(a[0].numpy(), minlength=V) / B
    sig = np.sqrt(p * (1 - p) / B)
    assert (np.abs(freq - p) < 5 * sig).all(), (freq, p)
    c = _run(logits, do_sample=True, seed=0xDEADBEEF12346, step=step, step_off=3)
    assert not torch.equal(a[0], c[0])


def test_bookkeeping_pad_eos_counts(dev):
    """Finished rows get pad and stay finished; an eos list of several ids clears alive; counts grow at the chosen token of
    the rows that were alive; the step tensor is not written."""
    ops = _ops()
    B, V = 4, 50
    logits = torch.full((B, V), -10.0)
    for b, t in enumerate([3, 4, 5, 6]):
        logits[b, t] = 10.0
    logits = logits.to(dev)
    alive = torch.tensor([1, 0, 1, 1], device=dev)
    counts = torch.zeros(B, V, dtype=torch.int32, device=dev)
    eos = torch.tensor([5, 6], device=dev)
    step = torch.zeros(1, dtype=torch.long, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    nxt = ops.sample_next(logits, alive, err, do_sample=True, top_k=1, counts=counts, repetition_penalty=1.2, eos=eos, pad=-7,
                          step=step)
    assert nxt.tolist() == [3, -7, 5, 6] and alive.tolist() == [1, 0, 0, 0]
    want = torch.zeros(B, V, dtype=torch.int32)
    want[0, 3] = want[2, 5] = want[3, 6] = 1
    assert torch.equal(counts.cpu(), want) and int(step[0]) == 0 and int(err[0]) == 0


def test_non_finite_rows_set_the_error_word(dev):
    ops = _ops()
    x = torch.randn(3, 64)
    x[0, 7] = float("nan")
    x[1, :] = float("-inf")
    x[2, 9] = float("inf")
    for b in range(3):
        nxt, _, p, err, _ = _run(x[b:b + 1].to(dev), do_sample=True, top_k=5)
        assert err == ops.ERR_NOT_FINITE and 0 <= int(nxt[0]) < 64 and (p == 0).all()
    nxt, _, _, err, _ = _run(x[2:3].to(dev), do_sample=True, alive=torch.zeros(1, dtype=torch.long, device=dev), pad=0)
    assert err == 0 and int(nxt[0]) == 0                       # (a finished row is not processed)


# ---------------------------------------------------------------------------------------------- generate()
def _model(dev, vocab=97, experts=0, layers=2, attention="selective_ssm", seed=11):
    import apertis_llm_amd as A
    torch.manual_seed(seed)
    cfg = A.ApertisConfig(vocab_size=vocab, hidden_size=128, num_hidden_layers=layers, num_attention_heads=2,
                          intermediate_size=256, attention_type=attention, use_expert_system=experts > 0,
                          num_experts=max(experts, 1), experts_per_token=2, pad_token_id=0)
    return A.ApertisForCausalLM(cfg).to(dev).eval()


CHAT = dict(do_sample=True, temperature=0.7, top_k=50, top_p=0.9)


def test_generate_raises_on_a_non_finite_row(dev):
    model = _model(dev)
    fwd = model.forward

    def bad(*a, **k):
        out = fwd(*a, **k)
        return (out[0], torch.full_like(out[1], float("nan"))) + tuple(out[2:])
    model.forward = bad
    # (ApertisHipError, not the RuntimeError torch.multinomial raises on the stock path: the kernel's error word was read)
    with pytest.raises(_ops().ApertisHipError, match="inf"):
        model.generate(input_ids=torch.randint(4, 97, (2, 8), device=dev), max_new_tokens=4, **CHAT)


@pytest.mark.parametrize("experts,bf16", [(0, False), (0, True), (4, False), (4, True)])
def test_sampled_generate_graph_equals_eager_and_is_seeded(dev, monkeypatch, experts, bf16):
    """A seeded sampled generate() run twice gives the same tokens; the decode graph's tail gives the eager loop's tokens (the
    same (seed, row, step) counter), with and without a penalty and an eos; the graph tail engages for do_sample."""
    from apertis_llm_amd import model as M
    model = _model(dev, experts=experts)
    prompt = torch.randint(4, 97, (3, 20), device=dev)
    ac = (lambda: torch.autocast("cuda", dtype=torch.bfloat16)) if bf16 else contextlib.nullcontext
    tails = {"n": 0}
    tail = M.ApertisForCausalLM._generate_graph_tail

    def tail_spy(self, *a, **k):
        tails["n"] += 1
        return tail(self, *a, **k)
    monkeypatch.setattr(M.ApertisForCausalLM, "_generate_graph_tail", tail_spy)

    def gen(graph, seed=5, **kw):
        monkeypatch.setattr(M, "DECODE_GRAPH", graph)
        torch.manual_seed(seed)
        with ac():
            return model.generate(input_ids=prompt, max_new_tokens=70, use_cache=True, **kw)

    for kw in (dict(CHAT, eos_token_id=-1), dict(CHAT, repetition_penalty=1.3, eos_token_id=-1),
               dict(do_sample=False, repetition_penalty=1.3, eos_token_id=-1)):
        e1 = gen(False, **kw)
        assert e1.shape == (3, 90) and torch.equal(gen(False, **kw), e1)
        n = tails["n"]
        g1 = gen(True, **kw)
        assert tails["n"] == n + 1, "the captured-graph tail did not engage"
        assert torch.equal(g1, e1), kw
    e1 = gen(False, **CHAT, eos_token_id=-1)
    assert not torch.equal(gen(False, seed=6, **CHAT, eos_token_id=-1), e1)
    eos = int(e1[0, 45])
    assert torch.equal(gen(True, **CHAT, eos_token_id=eos), gen(False, **CHAT, eos_token_id=eos))


def test_sampled_tokens_lie_in_their_kept_sets(dev, monkeypatch):
    """Every sampled token, eager and through the graph, is in the kept set recomputed (CPU restatement) from the logits a
    forward spy recorded on the device (a device-side counter: the graph replays the spy too), with the token history for
    the penalty."""
    from apertis_llm_amd import model as M
    model = _model(dev, experts=4)
    prompt = torch.randint(4, 97, (2, 9), device=dev)
    NEW = 40
    kw = dict(do_sample=True, temperature=0.7, top_k=20, top_p=0.9, repetition_penalty=1.3)
    fwd = model.forward
    for graph in (False, True):
        monkeypatch.setattr(M, "DECODE_GRAPH", graph)
        buf = torch.zeros(2, NEW + 8, 97, device=dev)
        ctr = torch.zeros(1, dtype=torch.long, device=dev)

        def spy(*a, **k):
            out = fwd(*a, **k)
            buf.index_copy_(1, ctr, out[1][:, -1:, :].float())
            ctr.add_(1)
            return out
        model.forward = spy
        try:
            toks = model.generate(input_ids=prompt, max_new_tokens=NEW, use_cache=True, eos_token_id=-1, **kw)
        finally:
            model.forward = fwd
        n = int(ctr[0])
        # eager: one forward per step; graph: the prefill, two warm-up steps (state restored after them), then the replays
        assert n == (NEW + 2 if graph else NEW), n
        logits = buf.cpu()
        for s in range(NEW):
            lg = logits[:, s if (not graph or s == 0) else s + 2]
            hist = [toks[b, :prompt.shape[1] + s].tolist() for b in range(2)]
            _, keep, _, _ = reference_select(lg, hist, penalty=1.3, do_sample=True, temperature=0.7, top_k=20, top_p=0.9)
            for b in range(2):
                assert bool(keep[b, int(toks[b, prompt.shape[1] + s])]), (graph, s, b)


def test_an_exception_in_the_graph_tail_leaves_the_model_as_it_was(dev, monkeypatch):
    """A Python exception out of the graph tail's first warm-up step (the second forward of the generate(): the prefill is the
    first) propagates, and nothing of the step stays on the modules (whether a step updates its cache in place, and what the
    pre-pass computed, ride with the cache views): the next generate() gives the eager loop's tokens."""
    from apertis_llm_amd import model as M
    model = _model(dev)
    prompt = torch.randint(4, 97, (2, 8), device=dev)
    kw = dict(input_ids=prompt, max_new_tokens=40, do_sample=False, use_cache=True, eos_token_id=-1)
    monkeypatch.setattr(M, "DECODE_GRAPH", False)
    eager = model.generate(**kw)
    monkeypatch.setattr(M, "DECODE_GRAPH", True)
    seen = {"tail": 0, "fwd": 0}
    tail = M.ApertisForCausalLM._generate_graph_tail

    def tail_spy(self, *a, **k):
        seen["tail"] += 1
        return tail(self, *a, **k)
    monkeypatch.setattr(M.ApertisForCausalLM, "_generate_graph_tail", tail_spy)
    fwd = model.forward

    def second_call_raises(*a, **k):
        seen["fwd"] += 1
        if seen["fwd"] == 2:
            raise RuntimeError("stop")
        return fwd(*a, **k)
    model.forward = second_call_raises
    try:
        with pytest.raises(RuntimeError, match="^stop$"):
            model.generate(**kw)
    finally:
        del model.forward
    assert seen == {"tail": 1, "fwd": 2}
    blocks = [m for m in model.modules() if isinstance(m, M.SelectiveLinearAttention)]
    assert len(blocks) == 2 and not any(hasattr(m, a) for m in blocks for a in ("_inplace_cache", "_decode_pre", "use_cache"))
    assert torch.equal(model.generate(**kw), eager) and seen["tail"] == 2


@pytest.mark.parametrize("name", ["generate_ssm_dense_long", "generate_ssm_moe_long"])
def test_top_k_one_through_the_graph_reproduces_the_greedy_reference(dev, name, monkeypatch):
    """do_sample=True with top_k = 1 keeps only the maximum: through the graph tail it must give the reference's greedy tokens
    (reference generate(), captured by tools/gen_golden.py generate_long), eos and padding included."""
    import apertis_llm_amd as A
    from apertis_llm_amd import model as M
    g = load_golden(name)
    cfg = A.ApertisConfig.from_dict(json.loads(str(g["config_json"])))
    model = A.ApertisForCausalLM(cfg)
    model.load_state_dict(g["sd"])
    model = model.to(dev).eval()
    seen = {"tail": 0}
    tail = M.ApertisForCausalLM._generate_graph_tail

    def tail_spy(self, *a, **k):
        seen["tail"] += 1
        assert k.get("sampler") is not None
        return tail(self, *a, **k)
    monkeypatch.setattr(M.ApertisForCausalLM, "_generate_graph_tail", tail_spy)
    NEW = g["step_logits"].shape[1]
    toks = model.generate(input_ids=g["prompt"].to(dev), max_new_tokens=NEW, do_sample=True, top_k=1, temperature=0.7,
                          use_cache=True, eos_token_id=int(g["eos"]), pad_token_id=0)
    assert seen["tail"] == 1
    assert torch.equal(toks.cpu(), g["tokens"])


def test_greedy_penalty_fused_equals_stock_and_standard_mha_samples(dev, monkeypatch):
    """Greedy with a repetition penalty: the same tokens with SAMPLE_FUSED on (kernel, graph) and off (the stock loop).  A
    standard_mha model samples through the kernel in its eager loop (seeded: twice the same tokens)."""
    ops = _ops()
    model = _model(dev, experts=4)
    prompt = torch.randint(4, 97, (3, 20), device=dev)
    kw = dict(max_new_tokens=40, do_sample=False, repetition_penalty=1.3, use_cache=True, eos_token_id=-1)
    fused = model.generate(input_ids=prompt, **kw)
    monkeypatch.setattr(ops.sample, "SAMPLE_FUSED", False)
    stock = model.generate(input_ids=prompt, **kw)
    monkeypatch.setattr(ops.sample, "SAMPLE_FUSED", True)
    assert torch.equal(fused, stock)
    mha = _model(dev, attention="standard_mha", vocab=128)
    calls = {"n": 0}
    real = ops.sample.sample_next

    def count(*a, **k):
        calls["n"] += 1
        return real(*a, **k)
    monkeypatch.setattr(ops.sample, "sample_next", count)
    p = torch.randint(4, 128, (2, 12), device=dev)
    torch.manual_seed(3)
    t1 = mha.generate(input_ids=p, max_new_tokens=12, use_cache=True, eos_token_id=-1, **CHAT)
    torch.manual_seed(3)
    t2 = mha.generate(input_ids=p, max_new_tokens=12, use_cache=True, eos_token_id=-1, **CHAT)
    assert calls["n"] == 24 and torch.equal(t1, t2) and t1.shape == (2, 24)


# ---------------------------------------------------------------------------------------------- against the reference capture
SAMPLED = ["generate_sampled_ssm_dense", "generate_sampled_ssm_moe", "generate_sampled_mha"]


def _capture(name, dev):
    import apertis_llm_amd as A
    g = load_golden(name)
    cfg = A.ApertisConfig.from_dict(json.loads(str(g["config_json"])))
    model = A.ApertisForCausalLM(cfg)
    model.load_state_dict(g["sd"])
    sp = dict(do_sample=True, temperature=float(g["temperature"]), top_k=int(g["top_k"]), top_p=float(g["top_p"]),
              repetition_penalty=float(g["repetition_penalty"]))
    return g, model.to(dev).eval(), sp


@pytest.mark.parametrize("name", SAMPLED)
def test_kernel_reproduces_the_reference_probs_and_draws(dev, name):
    """Every live step of the reference's sampled generate(): from its raw last-position logits and its token history the
    kernel gives the reference's probs (rtol 1e-5 on kept entries, exact zeros elsewhere) and, at the recorded uniform, the
    reference's token."""
    g = load_golden(name)
    P = int(g["prompt"].shape[1])
    toks, logits, probs, uni, live = g["tokens"], g["step_logits"], g["probs"], g["uniforms"], g["live"]
    rows = [(b, s_) for s_ in range(live.shape[1]) for b in range(2) if live[b, s_]]
    V = logits.shape[-1]
    x = torch.stack([logits[b, s_] for b, s_ in rows]).float()
    counts = torch.zeros(len(rows), V, dtype=torch.int32)
    for r, (b, s_) in enumerate(rows):
        for t in toks[b, :P + s_].tolist():
            if t < V:
                counts[r, t] += 1
    u = torch.tensor([[float(uni[b, s_])] for b, s_ in rows], dtype=torch.float64)
    nxt, _, p, err, _ = _run(x.to(dev), do_sample=True, temperature=float(g["temperature"]), top_k=int(g["top_k"]),
                             top_p=float(g["top_p"]), repetition_penalty=float(g["repetition_penalty"]),
                             counts=counts.to(dev), uniforms=u.to(dev))
    assert err == 0
    ref = torch.stack([probs[b, s_] for b, s_ in rows]).float()
    kept = ref > 0
    assert torch.equal(p > 0, kept)
    assert torch.allclose(p[kept].double(), ref[kept].double(), rtol=1e-5, atol=0)
    want = torch.stack([toks[b, P + s_] for b, s_ in rows])
    assert torch.equal(nxt, want)


@pytest.mark.parametrize("name,graph", [(SAMPLED[0], False), (SAMPLED[0], True), (SAMPLED[1], False), (SAMPLED[1], True),
                                        (SAMPLED[2], False)])        # (standard_mha decodes eagerly: no graph tail)
def test_generate_with_recorded_uniforms_gives_the_reference_tokens(dev, monkeypatch, name, graph):
    """generate() with SAMPLE_UNIFORMS = the capture's uniforms gives the reference's sampled tokens (eos and padding included):
    SSM eager and through the decode graph's tail (spied), standard_mha eager."""
    from apertis_llm_amd import model as M
    ops = _ops()
    g, model, sp = _capture(name, dev)
    tails = {"n": 0}
    tail = M.ApertisForCausalLM._generate_graph_tail

    def tail_spy(self, *a, **k):
        tails["n"] += 1
        assert k.get("sampler") is not None
        return tail(self, *a, **k)
    monkeypatch.setattr(M.ApertisForCausalLM, "_generate_graph_tail", tail_spy)
    monkeypatch.setattr(M, "DECODE_GRAPH", graph)
    monkeypatch.setattr(ops.sample, "SAMPLE_UNIFORMS", g["uniforms"].to(dev))
    NEW = g["uniforms"].shape[1]
    toks = model.generate(input_ids=g["prompt"].to(dev), max_new_tokens=NEW, use_cache=True, eos_token_id=int(g["eos"]),
                          pad_token_id=0, **sp)
    assert tails["n"] == (1 if graph else 0)
    assert torch.equal(toks.cpu(), g["tokens"])


@pytest.mark.parametrize("name", SAMPLED[:2])
@pytest.mark.parametrize("graph", [False, True])
def test_greedy_penalty_gives_the_reference_tokens(dev, monkeypatch, name, graph):
    """Greedy decoding with repetition_penalty 1.3 gives the reference's tokens (its capture: pen_*), eager and through the
    decode graph's tail."""
    from apertis_llm_amd import model as M
    g, model, sp = _capture(name, dev)
    monkeypatch.setattr(M, "DECODE_GRAPH", graph)
    NEW = g["pen_step_logits"].shape[1]
    toks = model.generate(input_ids=g["prompt"].to(dev), max_new_tokens=NEW, do_sample=False, repetition_penalty=sp["repetition_penalty"],
                          use_cache=True, eos_token_id=int(g["pen_eos"]), pad_token_id=0)
    assert torch.equal(toks.cpu(), g["pen_tokens"])
