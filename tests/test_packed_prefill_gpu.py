"""ApertisForCausalLM.prefill_packed - the prefill of several standard_mha prompts as one packed row on the document kernels,
every prompt's (k, v) a view of the row's - and generate_many(prefill_tokens=...), whose refill rounds use it.

Model recipe, weights, prompts and alone runs of tests/test_mha_slots_gpu.py (recomputed here): 2 layers, hidden 128, 2 heads
(D 64), intermediate 256, vocab 64, 128 rotary positions, fp32, oracle.seeded's weights with GAIN 16; prompts of 1, 2, 5, 9,
17, 33 and 40 tokens from PROMPT_SEED 24; 3 slots, 30 new tokens.  The alone runs' precondition - the smallest top-2 logit gap
over all their steps exceeds 1e-3 of the largest logit; searched on the CPU for these weights and prompts: 3.2e-3 plain,
1.4e-3 with the penalty - is asserted again on the GPU before any token is compared, and the gap is printed: a packed row
runs the projections at another row count, which is not the alone call's arithmetic to the last bit.
"""
import functools
import os
import re

import pytest
import torch

from conftest import rel_error_report

pytestmark = pytest.mark.gpu

LENS, NEW, VOCAB, SLOTS = [1, 2, 5, 9, 17, 33, 40], 30, 64, 3
NO_EOS = -1
GAIN = 16.0
PROMPT_SEED = 24
# the packed row of the prefill tests, as indices into the prompts: 33 + 17 + 9 + 5 = 64 tokens, then the 40-token prompt,
# then the 2- and the 1-token prompt (107 tokens).  _packed_order asserts what that does to the kernels' key tiles
ORDER = [5, 4, 3, 2, 6, 1, 0]
# generate_many(prefill_tokens=CAP) on the seven prompts in 3 slots, no eos, equal budgets (the three rows of a refill end
# together): rounds [1, 2, 5] - three free slots, a fourth prompt waits: cut by the slots; [9, 17] - the 33-token prompt
# would make 59 > 30 with a slot still free: cut by the cap; [33] and [40]: one prompt each, the batch-1 forward
CAP = 30
ROUNDS = [[0, 1, 2], [3, 4], [5], [6]]
# bf16: what the packed call's error against fp64 may be, as a multiple of the alone bf16 call's (see the test).  Measured
# on the MI355X before it was set: ratio 1.000 for all three kinds (logits 3.769e-2 both ways, k 3.898e-2, v 3.038e-2 of the
# largest reference value - bf16 through two layers of GAIN-16 weights).  2: one flipped bf16 rounding on the worst element
# stays inside, a document at wrong positions or reading a neighbour (errors of order 1, a factor of 25) does not
BF16_FACTOR = 2.0

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def ops():
    from apertis_llm_amd import ops
    return ops


@pytest.fixture
def slots_on(ops, monkeypatch):
    monkeypatch.setattr(ops, "ATTN_SLOTS", True)


def _config(kind="mha"):
    import apertis_llm_amd as A
    kw = dict(hidden_size=128, num_attention_heads=2, intermediate_size=256, attention_type="standard_mha")
    kw.update({"mha": {}, "d16": dict(hidden_size=64, num_attention_heads=4),
               "ssm": dict(hidden_size=64, num_attention_heads=4, intermediate_size=128, attention_type="selective_ssm")}[kind])
    return A.ApertisConfig(vocab_size=VOCAB, num_hidden_layers=2, max_position_embeddings=128, **kw)


@functools.lru_cache(maxsize=None)
def _cpu_model(kind="mha"):
    import apertis_llm_amd as A
    from oracle import seeded
    model = A.ApertisForCausalLM(_config(kind)).eval()
    if kind == "mha":
        model.load_state_dict(seeded.fill_state_dict(model.state_dict(), gain=GAIN))
    return model


@functools.lru_cache(maxsize=None)
def _model(kind="mha"):
    import copy
    return copy.deepcopy(_cpu_model(kind)).to(torch.device("cuda:0"))


@functools.lru_cache(maxsize=None)
def _prompts():
    g = torch.Generator().manual_seed(PROMPT_SEED)
    return [torch.randint(4, VOCAB, (n,), generator=g).to("cuda:0") for n in LENS]


def _packed_order():
    """The prompts in ORDER, with the offsets asserted: the 40-token prompt starts exactly on a key-tile boundary of the
    document kernels (csrc/attn_tile.h: TILE columns per step of a wave's loop) - and on a work-group's first query row -
    while the 33-token one straddles a key tile, as do the 17- and the 40-token ones."""
    with open(os.path.join(ROOT, "apertis_llm_amd", "csrc", "attn_tile.h")) as f:
        hdr = f.read()
    tile = int(re.search(r"constexpr int TILE = (\d+);", hdr).group(1))
    rows = int(re.search(r"constexpr int ROWS = (\d+);", hdr).group(1)) * int(re.search(r"constexpr int WAVES = (\d+);", hdr).group(1))
    prompts = [_prompts()[i] for i in ORDER]
    starts = [sum(len(p) for p in prompts[:j]) for j in range(len(prompts))]
    at = dict(zip([len(p) for p in prompts], starts))
    assert at[40] % tile == 0 and at[40] % rows == 0 and at[40] > 0
    assert at[33] // tile != (at[33] + 32) // tile and at[17] % tile != 0
    assert sorted(len(p) for p in prompts) == LENS and sum(LENS) > rows          # more than one work-group of query rows
    return prompts


@functools.lru_cache(maxsize=None)
def _fp64():
    """Every prompt alone through the same weights in fp64 on the CPU's stock branch, one prompt per call: per prompt (the
    last token's logits [V], per layer (k, v) [1, L, W]).  Computed once."""
    import copy
    ref = copy.deepcopy(_cpu_model()).double().eval()
    out = []
    with torch.no_grad():
        for p in _prompts():
            o = ref(input_ids=p.cpu()[None], use_cache=True)
            out.append((o[1][0, -1], o[4]))
    return out


def _spy(obj, calls, name="forward"):
    """Every call of obj.<name> as its keyword arguments (an instance attribute: `del obj.<name>` undoes it)."""
    real = getattr(obj, name)

    def spy(*a, **k):
        calls.append((name, a, k))
        return real(*a, **k)
    setattr(obj, name, spy)


def _against_fp64(what, logits, pasts, which, dtype=torch.float32, rtol=1e-4):
    """`logits` [n, V] and `pasts` (per prompt, per layer (k, v)) of the prompts `which` (indices) against _fp64()."""
    ref = _fp64()
    for j, i in enumerate(which):
        want_logits, want_past = ref[i]
        rel_error_report(f"{what} prompt {LENS[i]} logits", logits[j], want_logits, rtol=rtol)
        assert len(pasts[j]) == len(want_past) == 2
        for layer, ((k, v), (rk, rv)) in enumerate(zip(pasts[j], want_past)):
            assert tuple(k.shape) == tuple(v.shape) == (1, LENS[i], 128) and k.dtype == v.dtype == dtype
            rel_error_report(f"{what} prompt {LENS[i]} layer {layer} k", k, rk, rtol=rtol)
            rel_error_report(f"{what} prompt {LENS[i]} layer {layer} v", v, rv, rtol=rtol)


# ------------------------------------------------------------------------------------------------------- prefill_packed
def test_packed_prefill_against_fp64_and_the_alone_fused_call(dev, ops):
    model, prompts = _model(), _packed_order()
    timer = ops.KernelTimer(("apertis_attention_doc_fwd", "apertis_attention_fwd"))
    ops.set_kernel_timer(timer)
    try:
        logits, pasts = model.prefill_packed(prompts)
    finally:
        ops.set_kernel_timer(None)
    assert [r[0] for r in timer.records] == ["apertis_attention_doc_fwd"] * 2        # one per layer, no plain causal launch
    assert tuple(logits.shape) == (len(prompts), VOCAB) and logits.dtype == torch.float32 and len(pasts) == len(prompts)
    # the alone fused call is held to the same bar: a failure shows which side moved
    with torch.no_grad():
        for i in ORDER:
            o = model(input_ids=_prompts()[i][None], use_cache=True)
            _against_fp64("alone fused fp32", o[1][:, -1], [o[4]], [i])
    _against_fp64("prefill_packed fp32", logits, pasts, ORDER)
    # views of one buffer per layer and tensor, each at its document's rows
    firsts = set()
    for layer in range(2):
        for t in range(2):
            views = [past[layer][t] for past in pasts]
            base = views[0]._base
            assert base is not None and base.numel() == sum(LENS) * 128
            at = 0
            for x in views:
                assert x._base is base and x.data_ptr() == base.data_ptr() + at * 128 * base.element_size()
                assert x.stride()[1:] == (128, 1)
                at += x.shape[1]
            firsts.add(base.data_ptr())
    assert len(firsts) == 4                                                          # k and v of each layer: four buffers


def test_documents_do_not_leak(dev):
    model, prompts = _model(), _packed_order()
    mid = 3                                                                          # the 5-token prompt, fourth of seven
    other = list(prompts)
    other[mid] = (prompts[mid] - 4 + 7) % (VOCAB - 4) + 4                            # other tokens, the same length
    assert other[mid].shape == prompts[mid].shape and not bool((other[mid] == prompts[mid]).any())
    la, pa = model.prefill_packed(prompts)
    lb, pb = model.prefill_packed(other)
    for j in range(len(prompts)):
        pairs = [(la[j], lb[j])] + [(x, y) for a, b in zip(pa[j], pb[j]) for x, y in zip(a, b)]
        if j == mid:
            assert all(not torch.equal(x, y) for x, y in pairs)
        else:
            assert all(torch.equal(x, y) for x, y in pairs), j


@pytest.mark.parametrize("i", [0, 6], ids=["1-token", "40-token"])
def test_one_prompt(dev, i):
    logits, pasts = _model().prefill_packed([_prompts()[i]])
    assert tuple(logits.shape) == (1, VOCAB) and len(pasts) == 1
    _against_fp64("prefill_packed fp32 one prompt", logits, pasts, [i])


def test_lists_of_ids_are_prompts_too(dev):
    model, prompts = _model(), _prompts()
    la, pa = model.prefill_packed([prompts[2], prompts[4]])
    lb, pb = model.prefill_packed([prompts[2].tolist(), prompts[4].tolist()])
    assert torch.equal(la, lb) and all(torch.equal(x, y) for a, b in zip(pa, pb) for c, d in zip(a, b) for x, y in zip(c, d))


def _worst(logits, pasts, which):
    """Per kind (logits, k, v): the largest max|got - ref| / max|ref| over the prompts `which` against _fp64()."""
    ref, worst = _fp64(), {"logits": 0.0, "k": 0.0, "v": 0.0}

    def err(got, want):
        return float((got.detach().cpu().double() - want).abs().max() / want.abs().max())
    for j, i in enumerate(which):
        worst["logits"] = max(worst["logits"], err(logits[j], ref[i][0]))
        for (k, v), (rk, rv) in zip(pasts[j], ref[i][1]):
            worst["k"], worst["v"] = max(worst["k"], err(k, rk)), max(worst["v"], err(v, rv))
    return worst


def test_bf16_packed_is_as_close_to_fp64_as_the_alone_bf16_call(dev):
    """bf16 autocast over the fp32 weights; the reference is those weights in fp64.  Per kind of output - last-token logits,
    K, V - the figure is the largest max|got - ref| / max|ref| over the seven prompts.  The packed call may exceed the alone
    fused bf16 call's figure by BF16_FACTOR: the row count changes the GEMMs' tiling (and with it the order of the fp32
    accumulation before the one bf16 rounding), not their precision.
    Measured on the MI355X on the first run, before the factor was set: packed / alone = 1.000 for logits, K and V (3.769e-2,
    3.898e-2 and 3.038e-2 both ways).  Margin chosen: 2 (the constant's comment has the reasoning)."""
    model, prompts = _model(), _packed_order()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        logits, pasts = model.prefill_packed(prompts)
        alone = [model(input_ids=_prompts()[i][None], use_cache=True) for i in ORDER]
    assert logits.dtype == torch.bfloat16 and all(k.dtype == v.dtype == torch.bfloat16 for past in pasts for k, v in past)
    packed = _worst(logits, pasts, ORDER)
    single = _worst(torch.cat([o[1][:, -1] for o in alone]), [o[4] for o in alone], ORDER)
    for kind in packed:
        print(f"bf16 {kind}: packed {packed[kind]:.3e}, alone {single[kind]:.3e}, ratio {packed[kind] / single[kind]:.3f}")
    for kind in packed:
        assert 0 < single[kind] < 0.25, (kind, single)                                # (a bf16 error, and not a wrong answer)
        assert packed[kind] <= BF16_FACTOR * single[kind], (kind, packed, single)


@pytest.mark.parametrize("case", ["ssm", "fused_off", "head_dim", "training", "empty_prompt", "empty_list", "too_long",
                                  "cpu_prompt", "output_attentions"])
def test_refusals_launch_no_forward(dev, ops, monkeypatch, case):
    import copy
    kind = {"ssm": "ssm", "head_dim": "d16"}.get(case, "mha")
    model = copy.copy(_model(kind)) if case in ("training", "output_attentions") else _model(kind)
    prompts = [_prompts()[2], _prompts()[3]]
    match = {"ssm": "no per-document end state and no conv window.*kernel work.*not offered", "fused_off": "ATTN_FUSED is off",
             "head_dim": "head dim 16", "training": "training mode", "empty_prompt": "prompt 1 is empty",
             "empty_list": "no prompts", "too_long": r"prompt 1 of 129 tokens runs past the rotary table \(128 positions\)",
             "cpu_prompt": "prompt 1 is a torch.int64 tensor of shape \\(9,\\) on cpu", "output_attentions": "output_attentions"}[case]
    if case == "fused_off":
        monkeypatch.setattr(ops, "ATTN_FUSED", False)
    elif case == "training":
        model.training = True                     # (a shallow copy: the flag of the copy alone; the sub-modules are shared)
    elif case == "output_attentions":
        model.config = copy.copy(model.config)
        model.config.output_attentions = True
    elif case == "empty_prompt":
        prompts[1] = prompts[1][:0]
    elif case == "empty_list":
        prompts = []
    elif case == "too_long":
        prompts[1] = torch.randint(4, VOCAB, (129,), device=dev)
    elif case == "cpu_prompt":
        prompts[1] = prompts[1].cpu()
    calls = []
    _spy(model, calls)
    _spy(model.model, calls)
    try:
        with pytest.raises(ValueError, match=match):
            model.prefill_packed(prompts)
    finally:
        del model.forward
        del model.model.forward
    assert calls == []


def test_a_row_longer_than_the_rotary_table_is_taken(dev):
    """Five times the 40-token prompt: 200 tokens in one row against 128 rotary positions - the longest document is what
    the table must hold - and every copy gets the one prompt's numbers."""
    p = _prompts()[6]
    logits, pasts = _model().prefill_packed([p] * 5)
    _against_fp64("prefill_packed fp32 5 x 40", logits, pasts, [6] * 5)


def test_the_public_forward_still_refuses_a_cache_from_packed_rows(dev):
    model, p = _model(), _prompts()[3]
    docs = torch.zeros(1, len(p), dtype=torch.long, device=dev)
    with torch.no_grad():
        with pytest.raises(ValueError, match="packed rows take no past_key_values and no use_cache=True"):
            model(input_ids=p[None], document_ids=docs, use_cache=True)
        assert model(input_ids=p[None], document_ids=docs)[4] is None
        with pytest.raises(TypeError):
            model(input_ids=p[None], document_ids=docs, _packed_kv=len(p))


# ---------------------------------------------------------------------------------------- generate_many(prefill_tokens=)
@functools.lru_cache(maxsize=None)
def _alone(penalty=1.0):
    """Every prompt alone through batch-1 generate() on the eager loop, NEW tokens, no eos: (new tokens per prompt, the
    smallest top-2 gap over all steps as a share of the largest logit - of the logits the token is selected from: each
    divided by the penalty once per earlier occurrence of its token)."""
    import apertis_llm_amd as A
    model = _model()
    toks, gap = [], float("inf")
    graph, A.model.DECODE_GRAPH = A.model.DECODE_GRAPH, False
    fwd = model.forward
    try:
        for p in _prompts():
            steps, seen = [], torch.zeros(VOCAB, device=p.device)

            def spy(*a, **k):
                out = fwd(*a, **k)
                seen.add_(torch.bincount(k["input_ids"][0], minlength=VOCAB))
                steps.append(out[1].detach().float()[0, -1] / penalty ** seen)
                return out
            model.forward = spy
            out = model.generate(input_ids=p[None], max_new_tokens=NEW, do_sample=False, repetition_penalty=penalty,
                                 eos_token_id=NO_EOS, pad_token_id=0)
            assert tuple(out.shape) == (1, len(p) + NEW) and len(steps) == NEW
            toks.append(out[0, len(p):].clone())
            last = torch.stack(steps)
            top2 = torch.topk(last, 2, dim=-1).values
            gap = min(gap, float(((top2[:, 0] - top2[:, 1]) / last.abs().amax(-1)).min()))
    finally:
        del model.forward
        A.model.DECODE_GRAPH = graph
    return toks, gap


def _cut(t, eos, budget=NEW):
    t = t[:budget]
    hit = (t == eos).nonzero()
    return t[:int(hit[0]) + 1] if len(hit) else t


def _want(eos=NO_EOS, budgets=None, penalty=1.0):
    toks, gap = _alone(penalty)
    print(f"alone runs (standard_mha, penalty {penalty}): smallest top-2 gap {gap:.3e} of the largest logit")
    assert gap > 1e-3, "a near-tie in an alone run: pick other weights (GAIN) or prompts (PROMPT_SEED)"
    budgets = [NEW] * len(LENS) if budgets is None else budgets
    return [torch.cat((p, _cut(t, eos, m))) for p, t, m in zip(_prompts(), toks, budgets)]


def _same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == torch.int64 and g.dim() == 1 and g.is_cuda
        assert torch.equal(g, w), (i, g.tolist(), w.tolist())


def _early_eos(toks):
    """A token some prompt emits at its step 5 - so that its row ends there at the latest, while others are mid-run - such
    that at least two other prompts never emit it."""
    for t in toks:
        eos = int(t[5])
        if sum(1 for o in toks if not bool((o == eos).any())) >= 2:
            return eos
    raise AssertionError("no step-5 token leaves two rows running to the end: pick other prompts")


def _spied_run(model, **kw):
    """generate_many under spies on prefill_packed and on forward: (what it returned, the prefill rounds as lists of prompt
    indices in call order - a packed call's prompts, or the one prompt of a batch-1 prefill forward)."""
    calls, prompts = [], _prompts()
    _spy(model, calls)
    _spy(model, calls, "prefill_packed")
    try:
        out = model.generate_many(prompts, slots=SLOTS, pad_token_id=0, **kw)
    finally:
        del model.forward
        del model.prefill_packed

    def index(t):
        hit = [i for i, p in enumerate(prompts) if torch.equal(p, t)]
        assert len(hit) == 1
        return hit[0]
    rounds = []
    for name, a, k in calls:
        if name == "prefill_packed":
            assert not k and len(a) == 1 and len(a[0]) >= 2                          # never a packed row of one prompt
            rounds.append([index(t) for t in a[0]])
        elif k.get("past_key_values") is None:
            assert not a and tuple(k["input_ids"].shape)[0] == 1 and k["use_cache"] is True
            rounds.append([index(k["input_ids"][0])])
    return out, rounds


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_greedy_rounds_cut_by_cap_and_by_slots(dev, slots_on, monkeypatch, graph):
    import apertis_llm_amd as A
    assert NEW - 1 >= A.model.DECODE_GRAPH_MIN_STEPS
    monkeypatch.setattr(A.model, "DECODE_GRAPH", graph)
    (got, stats), rounds = _spied_run(_model(), max_new_tokens=NEW, eos_token_id=NO_EOS, return_stats=True, prefill_tokens=CAP)
    want = _want()
    # ROUNDS: one cut by the free slots, one cut by the token cap, two of a single prompt on the batch-1 forward
    assert rounds == ROUNDS
    assert sorted(i for r in rounds for i in r) == list(range(len(LENS)))            # no prompt prefilled twice
    assert sum(LENS[i] for i in ROUNDS[1]) <= CAP < sum(LENS[i] for i in ROUNDS[1]) + LENS[5] and len(ROUNDS[1]) < SLOTS
    assert len(ROUNDS[0]) == SLOTS and sum(LENS[i] for i in ROUNDS[0]) + LENS[3] <= CAP
    _same(got, want)
    assert set(stats) == {"steps", "replays", "graphs", "prefills", "live_slot_steps", "slot_steps", "fallbacks",
                          "prefill_forwards"}
    assert stats["prefills"] == len(LENS) and stats["prefill_forwards"] == len(rounds) and stats["fallbacks"] == []
    assert stats["graphs"] == int(graph) and stats["live_slot_steps"] == len(LENS) * (NEW - 1)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_an_eos_frees_rows_that_packed_rounds_refill(dev, slots_on, monkeypatch, graph):
    import apertis_llm_amd as A
    toks, _ = _alone()
    eos = _early_eos(toks)
    want = _want(eos)
    assert min(len(w) - n for w, n in zip(want, LENS)) <= 6 and sum(len(w) - n == NEW for w, n in zip(want, LENS)) >= 2
    monkeypatch.setattr(A.model, "DECODE_GRAPH", graph)
    (got, stats), rounds = _spied_run(_model(), max_new_tokens=NEW, eos_token_id=eos, return_stats=True, prefill_tokens=64)
    _same(got, want)
    assert sorted(i for r in rounds for i in r) == list(range(len(LENS))) and [i for r in rounds for i in r] == sorted(
        i for r in rounds for i in r)                                                # each once, in arrival order
    assert rounds[0] == [0, 1, 2] and len(rounds) > 2                                # rows were refilled while others ran
    assert stats["prefills"] == len(LENS) and stats["prefill_forwards"] == len(rounds) and stats["graphs"] == int(graph)


def test_repetition_penalty(dev, slots_on):
    want = _want(penalty=1.3)
    assert any(not torch.equal(w, g) for w, g in zip(want, _want())), "the penalty changes no token: it shows nothing"
    got, rounds = _spied_run(_model(), max_new_tokens=NEW, repetition_penalty=1.3, eos_token_id=NO_EOS, prefill_tokens=CAP)
    assert rounds == ROUNDS
    _same(got, want)


def test_budgets_of_one_and_zero_in_a_packed_round(dev, slots_on):
    """Budgets [1, 0, 30, 1, ...]: the prompt with nothing to generate takes no slot and no prefill; the first round packs
    prompts 0, 2 and 3, of which 0 and 3 end at their first token, and their two slots are refilled by the next round."""
    budgets = [1, 0, 30, 1, 30, 16, 3]
    want = _want(budgets=budgets)
    (got, stats), rounds = _spied_run(_model(), max_new_tokens=budgets, eos_token_id=NO_EOS, return_stats=True, prefill_tokens=64)
    assert [len(g) for g in got] == [n + m for n, m in zip(LENS, budgets)]
    _same(got, want)
    assert rounds == [[0, 2, 3], [4, 5], [6]]
    assert stats["prefills"] == 6 and stats["prefill_forwards"] == 3 and stats["fallbacks"] == []
    assert stats["live_slot_steps"] == sum(m - 1 for m in budgets if m > 0)


def test_top_k_one_sampling_is_greedy(dev, slots_on):
    torch.manual_seed(11)
    got, rounds = _spied_run(_model(), max_new_tokens=NEW, do_sample=True, top_k=1, temperature=0.7, eos_token_id=NO_EOS,
                             prefill_tokens=CAP)
    assert rounds == ROUNDS
    _same(got, _want())


def test_a_sampled_run_repeats_under_its_seed_and_first_draws_do_not_depend_on_the_knob(dev, slots_on):
    model, prompts = _model(), _prompts()
    kw = dict(max_new_tokens=NEW, slots=SLOTS, do_sample=True, temperature=0.7, top_k=50, top_p=0.9, eos_token_id=NO_EOS,
              pad_token_id=0)
    runs = []
    for cap in (CAP, CAP, None):
        torch.manual_seed(3)
        runs.append(model.generate_many(prompts, prefill_tokens=cap, **kw))
    _same(runs[0], runs[1])
    for g, p in zip(runs[0], prompts):
        assert len(g) == len(p) + NEW and torch.equal(g[:len(p)], p)
        assert 0 <= int(g.min()) and int(g.max()) < VOCAB
    # a prompt's first token is drawn with its prefill ordinal as the counter, packed round or not
    assert [int(g[len(p)]) for g, p in zip(runs[0], prompts)] == [int(g[len(p)]) for g, p in zip(runs[2], prompts)]
    assert len({int(g[len(p)]) for g, p in zip(runs[0], prompts)}) > 1


def test_without_the_knob_the_stats_keys_are_todays(dev, slots_on):
    (got, stats), rounds = _spied_run(_model(), max_new_tokens=4, eos_token_id=NO_EOS, return_stats=True)
    assert set(stats) == {"steps", "replays", "graphs", "prefills", "live_slot_steps", "slot_steps", "fallbacks"}
    assert rounds == [[i] for i in range(len(LENS))]                                 # one batch-1 forward per prompt, no packed call
    (_, stats), _ = _spied_run(_model(), max_new_tokens=4, eos_token_id=NO_EOS, return_stats=True, prefill_tokens=None)
    assert "prefill_forwards" not in stats


@pytest.mark.parametrize("case", ["zero", "bool", "float", "ssm", "switch_off"])
def test_generate_many_refusals_before_any_forward(dev, ops, monkeypatch, case):
    monkeypatch.setattr(ops, "ATTN_SLOTS", case != "switch_off")
    model = _model("ssm" if case == "ssm" else "mha")
    value, match = {"zero": (0, "prefill_tokens must be None or an integer >= 1, got 0"),
                    "bool": (True, "prefill_tokens must be None or an integer >= 1, got True"),
                    "float": (64.0, "prefill_tokens must be None or an integer >= 1, got 64.0"),
                    "ssm": (64, "no per-document end state and no conv window.*kernel work.*not offered"),
                    "switch_off": (64, r"generate\(past_key_values=.*left-padded")}[case]
    calls = []
    _spy(model, calls)
    _spy(model.model, calls)
    try:
        with pytest.raises(ValueError, match=match):
            model.generate_many(list(_prompts()[2:5]), max_new_tokens=4, slots=2, prefill_tokens=value)
    finally:
        del model.forward
        del model.model.forward
    assert calls == []
