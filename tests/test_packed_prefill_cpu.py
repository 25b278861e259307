"""generate_many(prefill_tokens=...) without a GPU: the refill round's choice as a pure function (serving.prefill_round),
SlotSchedule.waiting, the two signatures, and the refusals that need no device."""
import inspect

import pytest


def _round(lens, free, cap):
    from apertis_llm_amd.serving import prefill_round
    return prefill_round(lens, free, cap)


# ------------------------------------------------------------------------------------------------ the round's choice
@pytest.mark.parametrize("lens, free, cap, want", [
    ([9, 17, 33], 3, 30, [0, 1]),              # the cap is honoured: 9 + 17 = 26, the third would make 59
    ([9, 17, 33], 3, 26, [0, 1]),              # a total equal to the cap is inside it
    ([9, 17, 33], 3, 25, [0]),
    ([1, 2, 5, 9], 3, 1000, [0, 1, 2]),        # at most one per free slot
    ([1, 2, 5, 9], 1, 1000, [0]),
    ([33, 1, 1], 3, 30, [0]),                  # a prompt longer than the cap is taken alone: the one after it waits
    ([33], 2, 1, [0]),                         # at least one prompt is taken
    ([1, 40, 1], 3, 2, [0]),                   # arrival order is kept: the 1-token prompt behind the long one is not pulled up
    ([5, 5], 0, 100, []),                      # no free slot
    ([], 3, 100, []),                          # nothing waits
])
def test_round_choice(lens, free, cap, want):
    assert _round(lens, free, cap) == want


def test_round_choice_properties_over_a_sweep():
    import random
    rng = random.Random(5)
    for _ in range(500):
        lens = [rng.randint(1, 50) for _ in range(rng.randint(1, 8))]
        free, cap = rng.randint(1, 6), rng.randint(1, 120)
        got = _round(lens, free, cap)
        assert got == list(range(len(got)))                       # a prefix: arrival order, nobody skipped
        assert 1 <= len(got) <= min(free, len(lens))
        assert len(got) == 1 or sum(lens[j] for j in got) <= cap
        if len(got) < min(free, len(lens)):                       # it stopped for the cap, and only for the cap
            assert sum(lens[j] for j in got) + lens[len(got)] > cap


def test_waiting_lists_what_place_would_take():
    from apertis_llm_amd.serving import SlotSchedule
    s = SlotSchedule(6, [0, 3, 0, 1, 2, 0], 2)
    assert s.head() == 1 and s.waiting(0) == [] and s.waiting(1) == [1] and s.waiting(2) == [1, 3] and s.waiting(9) == [1, 3, 4]
    assert s.head() == 1 and s.pending == 5                       # (asking moves nothing)
    assert s.place(0, 7) and s.waiting(2) == [3, 4]
    assert not s.place(1, 7)                                      # budget 1: done at once, the slot stays free
    assert s.waiting(2) == [4] and s.free() == [1]
    assert s.place(1, 7) and s.waiting(3) == [] and s.head() is None


# ------------------------------------------------------------------------------------------------ signatures
def test_signatures():
    import apertis_llm_amd as A
    sig = inspect.signature(A.ApertisForCausalLM.generate_many)
    assert sig.parameters["prefill_tokens"].default is None
    assert list(inspect.signature(A.ApertisForCausalLM.prefill_packed).parameters) == ["self", "prompts"]
    fwd = inspect.signature(A.ApertisForCausalLM.forward)
    assert not any(n.startswith("_") for n in fwd.parameters)     # the cache-keeping packed path is not on the public forward


# ------------------------------------------------------------------------------------------------ refusals off the GPU
def _cpu_model(kind="standard_mha"):
    import apertis_llm_amd as A
    cfg = A.ApertisConfig(vocab_size=64, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256,
                          max_position_embeddings=128, attention_type=kind)
    return A.ApertisForCausalLM(cfg).eval()


def test_a_cpu_model_is_refused():
    with pytest.raises(ValueError, match="not on a GPU"):
        _cpu_model().prefill_packed([[5, 6, 7], [8]])


def test_a_selective_ssm_model_is_refused_with_the_reason():
    model = _cpu_model("selective_ssm")
    with pytest.raises(ValueError, match="no per-document end state and no conv window.*kernel work.*not offered"):
        model.prefill_packed([[5, 6, 7], [8]])
    with pytest.raises(ValueError, match="no per-document end state and no conv window.*kernel work.*not offered"):
        model.generate_many([[5, 6, 7], [8]], max_new_tokens=2, prefill_tokens=64)


@pytest.mark.parametrize("bad", [0, -3, True, False, 2.0, "64"])
def test_prefill_tokens_must_be_an_integer_of_at_least_one(monkeypatch, bad):
    from apertis_llm_amd import ops
    monkeypatch.setattr(ops, "ATTN_SLOTS", True)
    with pytest.raises(ValueError, match="prefill_tokens must be None or an integer >= 1"):
        _cpu_model().generate_many([[5, 6, 7], [8]], max_new_tokens=2, prefill_tokens=bad)


def test_with_the_switch_off_the_existing_refusal_comes_first(monkeypatch):
    from apertis_llm_amd import ops
    monkeypatch.setattr(ops, "ATTN_SLOTS", False)
    with pytest.raises(ValueError, match=r"generate\(past_key_values=.*left-padded"):
        _cpu_model().generate_many([[5, 6, 7], [8]], max_new_tokens=2, prefill_tokens=0)


def test_rope_bound_is_the_longest_document_when_the_caller_knows_it():
    """ops.attention._positions: in_range=True holds the row's length against the rotary table, an integer holds that
    integer - a packed row may be longer than the table when none of its documents is."""
    import torch
    from apertis_llm_amd.ops.attention import _positions
    pos = torch.arange(6).repeat(2)[None]                         # two documents of 6 tokens in a row of 12
    with pytest.raises(IndexError, match="sequence length 12 exceeds the rotary table"):
        _positions(pos, 1, 12, 8, in_range=True)
    got, stride = _positions(pos, 1, 12, 8, in_range=6)
    assert got is pos and stride == 0
    with pytest.raises(IndexError, match="sequence length 9 exceeds the rotary table"):
        _positions(pos, 1, 12, 8, in_range=9)
    assert _positions(None, 1, 8, 8) == (None, 0)
    with pytest.raises(IndexError):
        _positions(None, 1, 9, 8)
