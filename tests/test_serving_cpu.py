"""apertis_llm_amd.serving.SlotSchedule, the bookkeeping of generate_many(), driven with made-up token streams: arrival order,
refill only after a slot is freed, the cut at the first eos (inclusive) and at the per-prompt budget, bursts that ran past
either, and the edge cases (no prompt, more slots than prompts, everything finishing in one burst, a budget of 1 or 0).
After every call: live slots + pending + done == n."""
import pytest

from apertis_llm_amd.serving import SlotSchedule

EOS = frozenset({99})


def _stream(i, length=400):
    """Prompt i's made-up tokens: 1000 i + step, never an eos."""
    return [1000 * i + t for t in range(length)]


def _check(s):
    assert len(s.live()) + s.pending + s.done == s.n
    assert sorted(s.live() + s.free()) == list(range(s.slots))
    for b in s.live():
        assert 0 < s.remaining(b) <= s.budgets[s.slot[b]]


def _drive(n, budgets, slots, streams, eos=EOS, cap=16):
    """The loop generate_many() runs, on host lists: returns (schedule, the order in which prompts were placed, bursts)."""
    s = SlotSchedule(n, budgets, slots)
    _check(s)
    placed, at, bursts = [], {}, 0
    while not s.finished():
        for b in s.free():
            while s.head() is not None and s.slot[b] is None:
                i = s.head()
                placed.append(i)
                at[b] = 1
                s.place(b, streams[i][0], eos)
                _check(s)
        if not s.live():
            continue
        k = s.burst(cap)
        assert 1 <= k <= cap
        rows = {}
        for b in s.live():
            i = s.slot[b]
            rows[b] = streams[i][at[b]:at[b] + k]          # the row goes on emitting, past its end too
            at[b] += k
        s.feed(rows, eos)
        _check(s)
        bursts += 1
        assert bursts < 10000
    return s, placed, bursts


def test_arrival_order_budgets_and_refill():
    budgets = [5, 1, 40, 3, 17, 2, 9]
    streams = [_stream(i) for i in range(7)]
    s, placed, _ = _drive(7, budgets, 3, streams)
    assert placed == list(range(7))                         # handed out in arrival order
    assert s.done == 7 and s.pending == 0 and s.live() == []
    for i, m in enumerate(budgets):
        assert s.tokens[i] == streams[i][:m]                # per-prompt budget, nothing beyond it, output in prompt order


def test_a_slot_is_refilled_only_after_it_is_freed():
    s = SlotSchedule(3, [4, 4, 4], 1)
    assert s.head() == 0 and s.place(0, 7, EOS) is True and s.live() == [0] and s.free() == []
    with pytest.raises(ValueError, match="slot 0 holds prompt 0"):
        s.place(0, 8, EOS)
    assert s.head() == 1 and s.pending == 2                 # the refused call took nothing
    assert s.feed({0: [1, 2]}, EOS) == [] and s.live() == [0]
    assert s.feed({0: [3, 4, 5]}, EOS) == [0] and s.free() == [0]
    assert s.tokens[0] == [7, 1, 2, 3] and s.done == 1
    assert s.place(0, 9, EOS) is True and s.slot[0] == 1
    _check(s)


def test_cut_at_the_first_eos_inclusive_and_nothing_after_it():
    streams = [_stream(i) for i in range(4)]
    streams[1][5] = 99                                      # ends at step 5, mid-burst: the row ran 10 more steps
    streams[1][7] = 99
    streams[2][0] = 99                                      # its first token is the eos: never occupies a slot
    s, placed, _ = _drive(4, 30, 2, streams)
    assert placed == [0, 1, 2, 3]
    assert s.tokens[0] == streams[0][:30] and s.tokens[3] == streams[3][:30]
    assert s.tokens[1] == streams[1][:6] and s.tokens[1][-1] == 99
    assert s.tokens[2] == [99]


def test_a_burst_past_the_budget_keeps_nothing_beyond_it():
    s = SlotSchedule(2, [3, 6], 2)
    s.place(0, 1, EOS)
    s.place(1, 2, EOS)
    assert s.burst(16) == 5 and s.burst(4) == 4             # nothing waits: up to the longest row's end
    assert s.feed({0: [10, 11, 12, 13, 14], 1: [20, 21, 22, 99, 24]}, EOS) == [0, 1]
    assert s.tokens == [[1, 10, 11], [2, 20, 21, 22, 99]] and s.fed == 6
    assert s.finished()


def test_burst_stops_at_the_first_budget_while_a_prompt_waits():
    s = SlotSchedule(3, [4, 30, 30], 2)
    s.place(0, 1, EOS)
    s.place(1, 2, EOS)
    assert s.pending == 1 and s.burst(16) == 3              # slot 0 has 3 tokens left and prompt 2 waits for it
    assert s.feed({0: [5, 6, 7], 1: [5, 6, 7]}, EOS) == [0]
    s.place(0, 3, EOS)
    assert s.pending == 0 and s.burst(16) == 16 and s.burst(64) == 29
    _check(s)


def test_zero_prompts_and_more_slots_than_prompts():
    s = SlotSchedule(0, [], 4)
    assert s.finished() and s.head() is None and s.live() == [] and s.tokens == [] and s.burst(16) == 0
    with pytest.raises(ValueError, match="no prompt is pending"):
        s.place(0, 1, EOS)
    streams = [_stream(i) for i in range(2)]
    s, placed, bursts = _drive(2, [20, 3], 8, streams)
    assert placed == [0, 1] and s.tokens == [streams[0][:20], streams[1][:3]]
    assert bursts == 2                                       # 16 steps, then the 3 that are left


def test_every_prompt_finishing_in_the_same_burst():
    streams = [_stream(i) for i in range(6)]
    s, placed, bursts = _drive(6, 9, 3, streams)
    assert placed == list(range(6)) and bursts == 2         # two groups of three, each done in one burst of 8 steps
    assert all(s.tokens[i] == streams[i][:9] for i in range(6))


def test_budget_of_one_and_of_zero():
    streams = [_stream(i) for i in range(5)]
    s, placed, _ = _drive(5, [1, 0, 1, 4, 0], 1, streams)
    assert placed == [0, 2, 3]                              # a budget of 0 asks for no prefill
    assert s.tokens == [streams[0][:1], [], streams[2][:1], streams[3][:4], []] and s.done == 5
    s = SlotSchedule(2, [1, 5], 1)
    assert s.place(0, 7, EOS) is False and s.live() == []   # done with its first token: the slot stays free
    assert s.head() == 1
    _check(s)


def test_complete_runs_a_prompt_outside_the_slots():
    s = SlotSchedule(3, [4, 4, 2], 2)
    s.place(1, 5, EOS)
    s.complete([1, 99, 3, 4, 5], EOS)                       # (as generate() hands them back: cut here the same way)
    s.complete([1, 2, 3, 4, 5], EOS)
    _check(s)
    assert s.tokens[1] == [1, 99] and s.tokens[2] == [1, 2] and s.done == 2 and s.live() == [1] and s.fed == 0


def test_arguments():
    with pytest.raises(ValueError, match="2 budgets for 3 prompts"):
        SlotSchedule(3, [1, 2], 2)
    with pytest.raises(ValueError, match="0 slots"):
        SlotSchedule(3, 5, 0)
    assert SlotSchedule(3, 5, 2).budgets == [5, 5, 5]


def test_module_imports_no_torch_at_module_level():
    import ast
    import inspect

    import apertis_llm_amd.serving as serving
    tree = ast.parse(inspect.getsource(serving))
    names = [a.name for node in tree.body if isinstance(node, ast.Import) for a in node.names]
    names += [node.module for node in tree.body if isinstance(node, ast.ImportFrom)]
    assert not any(n and n.split(".")[0] == "torch" for n in names)
