"""ApertisForCausalLM.generate_many on the GPU: every prompt gets the tokens generate() gives it alone, cut after its first eos,
while the rows of one decode batch are refilled as they finish.

Model recipe of tests/test_ssm_leftpad_gpu.py: 2 layers, hidden 64, 4 heads (Dn 64), conv kernel 4, vocab 64, fp32,
oracle.seeded's weights with a gain (at the constructor's std the tiny model repeats one token whatever came before, and
nothing a slot could get wrong would show).  Seven prompts of 3 (= k - 1), 4, 5, 9, 17, 33 and 40 tokens in 3 slots.  The
alone runs come from batch-1 generate() on the eager loop; before any token is compared the smallest top-2 logit gap over
all their steps must exceed 1e-3 of the largest logit (a condition on the inputs: the slots run the stacked token step at
another batch size, which is not the eager step's arithmetic to the last bit).
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

LENS, NEW, VOCAB, SLOTS = [3, 4, 5, 9, 17, 33, 40], 30, 64, 3
GAIN = {"dense": 12.0, "moe": 16.0}
NO_EOS = -1
# The prompts' seed: chosen so that the precondition holds on the GPU for both kinds and under the repetition penalty (gaps
# 1.9e-3 dense, 3.4e-3 moe, 1.3e-3 dense with the penalty; most seeds leave a gap below 1e-3 somewhere in the 210 steps of
# the seven alone runs)
PROMPT_SEED = 13


@functools.lru_cache(maxsize=None)
def _model(kind):
    import apertis_llm_amd as A
    from oracle import seeded
    kw = {"dense": {}, "moe": dict(use_expert_system=True, num_experts=4, experts_per_token=2),
          "absolute": dict(position_embedding_type="absolute"), "mha": dict(attention_type="standard_mha"),
          "multimodal": dict(multimodal=True, image_size=16, vision_embed_dim=32, vision_patch_size=8, vision_layers=1,
                             vision_heads=2)}[kind]
    kw = {**dict(attention_type="selective_ssm"), **kw}
    cfg = A.ApertisConfig(vocab_size=VOCAB, hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128,
                          max_position_embeddings=128, **kw)
    model = A.ApertisForCausalLM(cfg).eval()
    if kind in GAIN:
        model.load_state_dict(seeded.fill_state_dict(model.state_dict(), gain=GAIN[kind]))
    return model.to(torch.device("cuda:0"))


@functools.lru_cache(maxsize=None)
def _prompts():
    g = torch.Generator().manual_seed(PROMPT_SEED)
    return [torch.randint(4, VOCAB, (n,), generator=g).to("cuda:0") for n in LENS]


def _spy_forward(model, calls):
    """Every model.forward call as its keyword arguments (generate() and generate_many() pass keywords only)."""
    fwd = model.forward

    def spy(*a, **k):
        assert not a
        calls.append(k)
        return fwd(**k)
    model.forward = spy


@functools.lru_cache(maxsize=None)
def _alone(kind, penalty=1.0):
    """Every prompt alone through batch-1 generate() on the eager loop, NEW tokens, no eos: (new tokens per prompt, the
    smallest top-2 gap over all steps as a share of the largest logit - of the logits the token is selected from: each
    divided by the penalty once per earlier occurrence of its token)."""
    import apertis_llm_amd as A
    model = _model(kind)
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


def _want(kind, eos=NO_EOS, budgets=None, penalty=1.0):
    toks, gap = _alone(kind, penalty)
    print(f"alone runs ({kind}, penalty {penalty}): smallest top-2 gap {gap:.3e} of the largest logit")
    assert gap > 1e-3, "a near-tie in an alone run: pick other weights (GAIN)"
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


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("kind", ["dense", "moe"])
def test_every_prompt_gets_its_alone_run(dev, monkeypatch, kind, graph):
    import apertis_llm_amd as A
    model = _model(kind)
    toks, _ = _alone(kind)
    eos = _early_eos(toks)
    want = _want(kind, eos)
    assert min(len(w) - n for w, n in zip(want, LENS)) <= 6 and sum(len(w) - n == NEW for w, n in zip(want, LENS)) >= 2
    assert NEW - 1 >= A.model.DECODE_GRAPH_MIN_STEPS
    monkeypatch.setattr(A.model, "DECODE_GRAPH", graph)
    replays, real = [], torch.cuda.CUDAGraph.replay
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", lambda self: (replays.append(id(self)), real(self))[1])
    got, stats = model.generate_many(_prompts(), max_new_tokens=NEW, slots=SLOTS, eos_token_id=eos, pad_token_id=0,
                                     return_stats=True)
    _same(got, want)
    assert stats["prefills"] == len(LENS) and stats["fallbacks"] == []
    if graph:
        assert stats["graphs"] == 1 and len(set(replays)) == 1          # one graph captured for the whole call
        assert stats["replays"] == stats["steps"] == len(replays) > 0
    else:
        assert stats["graphs"] == 0 and stats["replays"] == 0 and replays == [] and stats["steps"] > 0


@pytest.mark.parametrize("kind", ["dense", "moe"])
def test_per_prompt_budgets(dev, kind):
    budgets = [1, 2, 7, 30, 30, 16, 3]
    want = _want(kind, budgets=budgets)
    got = _model(kind).generate_many(_prompts(), max_new_tokens=budgets, slots=SLOTS, eos_token_id=NO_EOS, pad_token_id=0)
    assert [len(g) for g in got] == [n + m for n, m in zip(LENS, budgets)]
    _same(got, want)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16-autocast"])
def test_prefill_is_the_alone_call(dev, bf16):
    model, prompts = _model("dense"), _prompts()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
        # the alone runs' first tokens, under the same autocast state: the prefill is the same call, bit for bit
        first = [int(model.generate(input_ids=p[None], max_new_tokens=1, eos_token_id=NO_EOS, pad_token_id=0)[0, -1])
                 for p in prompts]
        calls = []
        _spy_forward(model, calls)
        try:
            got = model.generate_many(prompts, max_new_tokens=NEW, slots=SLOTS, eos_token_id=NO_EOS, pad_token_id=0)
        finally:
            del model.forward
    prefills = [k for k in calls if k.get("past_key_values") is None]
    assert len(prefills) == len(prompts)
    for k, p in zip(prefills, prompts):                       # one batch-1 prefill per prompt, in arrival order
        assert torch.equal(k["input_ids"], p[None]) and k.get("attention_mask") is None and k.get("pixel_values") is None
    steps = [k for k in calls if k.get("past_key_values") is not None]
    assert steps and all(tuple(k["input_ids"].shape) == (SLOTS, 1) for k in steps)
    assert len(got) == len(prompts)
    for g, p, f in zip(got, prompts, first):
        assert len(g) == len(p) + NEW and torch.equal(g[:len(p)], p) and int(g[len(p)]) == f
        assert 0 <= int(g.min()) and int(g.max()) < VOCAB
    if not bf16:
        _same(got, _want("dense"))


def test_repetition_penalty_and_the_samplers_rows(dev, monkeypatch):
    import apertis_llm_amd as A
    from apertis_llm_amd import ops
    model, prompts = _model("dense"), _prompts()
    # greedy with a penalty: the occurrence row rebuilt from the prompt when it moves into a slot others have used
    want = _want("dense", penalty=1.3)
    plain = model.generate_many(prompts, max_new_tokens=NEW, slots=SLOTS, eos_token_id=NO_EOS, pad_token_id=0)
    assert any(not torch.equal(w, g) for w, g in zip(want, plain)), "the penalty changes no token: it shows nothing"
    _same(model.generate_many(prompts, max_new_tokens=NEW, slots=SLOTS, repetition_penalty=1.3, eos_token_id=NO_EOS,
                              pad_token_id=0), want)
    # top_k = 1: the draw cannot choose otherwise; on the eager loop every step is one call of the fused sampler over S rows
    rows, real = [], ops.sample.sample_next
    monkeypatch.setattr(ops.sample, "sample_next", lambda lg, *a, **k: (rows.append(lg.shape[0]), real(lg, *a, **k))[1])
    monkeypatch.setattr(A.model, "DECODE_GRAPH", False)
    torch.manual_seed(3)
    got, stats = model.generate_many(prompts, max_new_tokens=NEW, slots=SLOTS, do_sample=True, top_k=1, temperature=0.7,
                                     eos_token_id=NO_EOS, pad_token_id=0, return_stats=True)
    _same(got, _want("dense"))
    assert rows == [SLOTS] * stats["steps"] and stats["steps"] > 0


def test_stale_rows_do_no_harm(dev):
    model, prompts, want = _model("dense"), _prompts(), _want("dense")
    # two rows of four are never live: zero state, pad tokens
    got, stats = model.generate_many(prompts[3:5], max_new_tokens=NEW, slots=4, eos_token_id=NO_EOS, pad_token_id=0,
                                     return_stats=True)
    _same(got, want[3:5])
    assert stats["live_slot_steps"] == 2 * (NEW - 1) and stats["slot_steps"] == 4 * (NEW - 1)
    # one slot: every prompt moves into the row the one before it left
    got, stats = model.generate_many(prompts, max_new_tokens=NEW, slots=1, eos_token_id=NO_EOS, pad_token_id=0,
                                     return_stats=True)
    _same(got, want)
    assert stats["prefills"] == len(prompts) and stats["live_slot_steps"] == stats["slot_steps"] == len(prompts) * (NEW - 1)


def test_short_prompts_run_through_generate(dev):
    import apertis_llm_amd as A
    model, prompts, want = _model("dense"), _prompts(), _want("dense")
    g = torch.Generator().manual_seed(8)
    short = [torch.randint(4, VOCAB, (n,), generator=g).to(dev) for n in (1, 2)]
    # (a short prompt's steps are full-sequence forwards - no window to step on - so 12 new tokens: below the length from
    #  which generate() replays them as a graph.  That replay would run the scan on its capture streams, and the look-back
    #  workspace is kept per stream for the life of the process: tests/test_model_gpu.py plants the error word of the only one)
    few = 12
    assert few - 1 < A.model.DECODE_GRAPH_MIN_STEPS
    alone = [model.generate(input_ids=p[None], max_new_tokens=few, eos_token_id=NO_EOS, pad_token_id=0)[0] for p in short]
    mixed = [prompts[4], short[0], prompts[0], prompts[5], short[1], prompts[1]]
    got, stats = model.generate_many(mixed, max_new_tokens=[NEW, few, NEW, NEW, few, NEW], slots=2, eos_token_id=NO_EOS,
                                     pad_token_id=0, return_stats=True)
    _same(got, [want[4], alone[0], want[0], want[5], alone[1], want[1]])
    assert stats["fallbacks"] == [1, 4] and stats["prefills"] == 4
    # lists of ids are taken as they are
    alone3 = model.generate(input_ids=short[0][None], max_new_tokens=3, eos_token_id=NO_EOS, pad_token_id=0)[0]
    got = model.generate_many([p.tolist() for p in mixed[:3]], max_new_tokens=[4, 3, 2], slots=2, eos_token_id=NO_EOS,
                              pad_token_id=0)
    _same(got, [want[4][:LENS[4] + 4], alone3, want[0][:LENS[0] + 2]])
    assert model.generate_many([], slots=2) == []


@pytest.mark.parametrize("case", ["standard_mha", "absolute", "pixel_values", "cpu", "train", "output_attentions", "slots_17",
                                  "slots_0", "budget_list", "empty_prompt"])
def test_refusals_launch_no_forward(dev, case):
    model = _model({"standard_mha": "mha", "absolute": "absolute", "pixel_values": "multimodal"}.get(case, "dense"))
    prompts = list(_prompts()[:3])
    kw, match = dict(max_new_tokens=4, slots=2), case
    if case == "standard_mha":
        match = r"generate\(past_key_values=.*left-padded"
    elif case == "absolute":
        match = "absolute position"
    elif case == "pixel_values":
        kw["pixel_values"] = torch.zeros(1, 3, 16, 16, device=dev)
    elif case == "cpu":
        prompts[1] = prompts[1].cpu()
        match = "on cpu"
    elif case == "train":
        match = "training mode"
    elif case in ("slots_17", "slots_0"):
        kw["slots"] = int(case[6:])
        match = "slots = "
    elif case == "budget_list":
        kw["max_new_tokens"] = [4, 4]
        match = "2 max_new_tokens for 3 prompts"
    elif case == "empty_prompt":
        prompts[2] = prompts[2][:0]
        match = "prompt 2 is empty"
    calls = []
    _spy_forward(model, calls)
    try:
        if case == "train":
            model.train()
        if case == "output_attentions":
            model.config.output_attentions = True
        with pytest.raises(ValueError, match=match):
            model.generate_many(prompts, **kw)
    finally:
        del model.forward
        model.eval()
        model.config.output_attentions = False
    assert calls == []


def test_stats(dev):
    budgets = [1, 2, 7, 30, 30, 16, 3]
    got, stats = _model("dense").generate_many(_prompts(), max_new_tokens=budgets, slots=SLOTS, eos_token_id=NO_EOS,
                                               pad_token_id=0, return_stats=True)
    assert set(stats) == {"steps", "replays", "graphs", "prefills", "live_slot_steps", "slot_steps", "fallbacks"}
    assert stats["prefills"] == len(LENS) and stats["slot_steps"] == SLOTS * stats["steps"]
    assert stats["live_slot_steps"] == sum(m - 1 for m in budgets)        # every kept token but each prompt's first is a live slot-step
    assert 0 < stats["live_slot_steps"] <= stats["slot_steps"]
