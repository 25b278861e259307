"""The dispatch plan's overflow select (plan_compact_k + plan_select_keys_k, moe_routing.hip) against the CPU oracle, on key
patterns built bit by bit: every case goes through ops.moe_plan and oracle.ref_cpu.dispatch_plan and compares all four outputs
for equality.  idx and w are built directly (no gate kernel), so the keys of an overflowing slot are exactly the ones named.

Before the GPU is asked anything, each case asserts from the oracle's own output that it reaches the select at all - at
least one (expert, k) slot keeps some but not all of its candidates ("mode 2") - and that the slot has the tie pattern the case
is about; a case cannot pass by never overflowing.

On-chip budget of plan_select_keys_k: one work-group of 1024 threads holds 32 keys per thread, 32768 candidates of a slot, in
registers; a slot with more streams the rest from the compacted array every round.  `over_budget` and `grid_wrap` exceed it.
plan_hist_k / plan_compact_k cover 512 * 1024 (token, k) pairs in one trip of their grid; `grid_wrap` needs a second trip."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEL_BUDGET = 32 * 1024          # candidates of one slot that plan_select_keys_k keeps in registers
HIST_TRIP = 512 * 1024          # (token, k) pairs per trip of plan_hist_k's / plan_compact_k's grid


def _f(bits):
    """float32 array with exactly these bit patterns"""
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def _columns(rng, S, counts):
    """idx [S, K]: column k holds expert e counts[k][e] times (the counts of a column add up to S), in shuffled order"""
    cols = []
    for per_e in counts:
        assert sum(per_e) == S, (sum(per_e), S)
        col = np.repeat(np.arange(len(per_e), dtype=np.int32), per_e)
        cols.append(rng.permutation(col))
    return np.stack(cols, axis=1)


def _distinct_topk(rng, S, E, K, p0=None):
    """idx [S, K] with K distinct experts per token; p0: probability that column 0 is expert 0 (skew)"""
    order = np.argsort(rng.random((S, E)), axis=1).astype(np.int32)
    if p0 is not None:
        hit = rng.random(S) < p0
        pos = np.argmax(order == 0, axis=1)                    # swap expert 0 to the front of the chosen rows
        rows = np.nonzero(hit)[0]
        order[rows, pos[rows]] = order[rows, 0]
        order[rows, 0] = 0
    return np.ascontiguousarray(order[:, :K])


class Case:
    def __init__(self, idx, w, E, cap, active=None, expect=None):
        self.idx, self.w, self.E, self.cap, self.active, self.expect = idx, np.ascontiguousarray(w, dtype=np.float32), E, cap, active, expect


def _two_keys(bit, cap):
    """E = 8, K = 1 (keep == capacity in every overflowing slot).  Every expert's candidates carry one of two keys that differ in
    `bit` only; with C = 40: expert 0 has C + 1 candidates (keep = total - 1), expert 1 more high keys than C (the threshold is
    the high key, some of its ties dropped), expert 2 exactly C high keys, expert 3 fewer (threshold = the low key)."""
    rng = np.random.default_rng(100 + bit + cap)
    lo = 0x3f000000 if bit == 0 else 0x00000001
    hi = lo | (1 << bit)
    C = 40
    totals = [C + 1, 300, 300, 300, 30, 500, 2, 67]
    n_hi = [1, C + 17, C, C - 9, 5, 1, 1, 66]
    S = sum(totals)
    idx = _columns(rng, S, [totals])
    bits = np.full((S, 1), lo, dtype=np.uint32)
    for e in range(8):
        tok = np.nonzero(idx[:, 0] == e)[0]
        bits[rng.permutation(tok)[:n_hi[e]], 0] = hi

    def expect(sit):
        for e in (0, 1, 2, 3, 5, 7) if cap == C else (0, 1, 2, 3, 4, 5, 6, 7):
            tot, kept, keys = sit[e]
            assert 0 < kept < tot and kept == cap and sorted(set(keys.tolist())) == [lo, hi], (e, tot, kept)
        if cap == C:
            assert sit[0][1] == sit[0][0] - 1                       # keep = total - 1
            assert n_hi[1] > cap == n_hi[2] > n_hi[3]               # keep on either side of the split, and on it
        else:
            assert cap == 1
    return Case(idx, _f(bits), 8, cap, expect=expect)


def _all_tie(key_bits):
    rng = np.random.default_rng(21)
    S, E, K, cap = 3000, 4, 2, 500
    idx = _distinct_topk(rng, S, E, K)

    def expect(sit):
        m2 = [v for v in sit.values() if 0 < v[1] < v[0]]
        assert m2 and all(set(v[2].tolist()) == {key_bits} for v in m2)
    return Case(idx, _f(np.full((S, K), key_bits, dtype=np.uint32)), E, cap, expect=expect)


def _random_w(rng, S, K):
    return (rng.random((S, K), dtype=np.float32) * 0.98 + 0.01).astype(np.float32)


def _past_small(E, K, cap):
    rng = np.random.default_rng(65 + E)
    idx = _distinct_topk(rng, 65, E, K, p0=0.4)
    return Case(idx, _random_w(rng, 65, K), E, cap)


def _random_bits():
    rng = np.random.default_rng(7)
    S, E, K = 2000, 8, 2
    bits = rng.integers(0, 0x7f7fffff, size=(S, K), endpoint=True, dtype=np.uint32)

    def expect(sit):
        m2 = [v for v in sit.values() if 0 < v[1] < v[0]]
        spread = np.concatenate([v[2] for v in m2])
        assert all(len(set(((spread >> s) & 255).tolist())) > 100 for s in (0, 8, 16)) and len(set((spread >> 24).tolist())) > 60
    return Case(_distinct_topk(rng, S, E, K), _f(bits), E, 100, expect=expect)


def _neighbours():
    """K = 3, capacity 200.  Expert 0: k = 0 fits (150), k = 1 has one candidate more than what is left (51 for 50), k = 2 finds
    nothing left.  Expert 1: k = 0 uses the capacity up exactly (200), k = 1 and 2 nothing left.  Expert 2: dropped through
    `active`, with enough candidates to overflow.  Expert 3: k = 0 overflows (320), then nothing left.  Expert 4 takes the rest."""
    rng = np.random.default_rng(33)
    S, E, cap = 1200, 5, 200
    counts = [[150, 200, 400, 320, 130], [51, 90, 300, 10, 749], [70, 5, 250, 25, 850]]
    idx = _columns(rng, S, counts)

    def expect(sit):
        modes = {p: (0 if v[1] == 0 else (1 if v[1] == v[0] else 2)) for p, v in sit.items()}
        assert [modes[p] for p in range(15)] == [1, 2, 0, 1, 0, 0, 0, 0, 0, 2, 0, 0, 1, 2, 0], modes
        assert sit[1][:2] == (51, 50) and sit[3][:2] == (200, 200)
    return Case(idx, _random_w(rng, S, 3), E, cap, active=[1, 1, 0, 1, 1], expect=expect)


def _grid_wrap():
    rng = np.random.default_rng(300)
    S, E, K = 300_000, 8, 2
    assert S * K > HIST_TRIP

    def expect(sit):
        assert sit[0][0] > SEL_BUDGET and 0 < sit[0][1] < sit[0][0]     # expert 0, k = 0: overflows, and past the select's budget
        assert sum(1 for v in sit.values() if 0 < v[1] < v[0]) >= 4
    return Case(_distinct_topk(rng, S, E, K, p0=0.45), _random_w(rng, S, K), E, 46_875, expect=expect)


def _over_budget():
    rng = np.random.default_rng(70)
    S = 70_000
    idx = rng.integers(0, 2, size=(S, 1), dtype=np.int32)

    def expect(sit):
        assert all(v[0] > SEL_BUDGET and v[1] == 1000 for v in sit.values())
    return Case(idx, _random_w(rng, S, 1), 2, 1000, expect=expect)


def _many_slots():
    rng = np.random.default_rng(64)
    S, E, K = 5000, 64, 8

    def expect(sit):
        assert len(sit) == 512 and sum(1 for v in sit.values() if 0 < v[1] < v[0]) >= 32
    return Case(_distinct_topk(rng, S, E, K), _random_w(rng, S, K), E, 300, expect=expect)


CASES = {
    "past_small_e8k2": lambda: _past_small(8, 2, 9),
    "past_small_e4k1": lambda: _past_small(4, 1, 1),
    "all_tie_half": lambda: _all_tie(0x3f000000),
    "all_tie_denormal": lambda: _all_tie(0x00000123),
    "two_keys_bit0": lambda: _two_keys(0, 40),
    "two_keys_bit0_keep1": lambda: _two_keys(0, 1),
    "two_keys_bit30": lambda: _two_keys(30, 40),
    "two_keys_bit30_keep1": lambda: _two_keys(30, 1),
    "random_bits": _random_bits,
    "neighbours": _neighbours,
    "grid_wrap": _grid_wrap,
    "over_budget": _over_budget,
    "many_slots": _many_slots,
}


@functools.lru_cache(maxsize=None)
def oracle_side(name):
    """The case, the oracle's plan for it, and the situation per slot p = e * K + k: (candidates, kept, the candidates' keys);
    asserts that the case reaches the select with the pattern it is named for.  Needs no GPU."""
    from oracle import ref_cpu
    c = CASES[name]()
    S, K = c.idx.shape
    assert S > 64 or c.E * K > 16, "the one-launch plan would take this"
    assert (c.w.view(np.uint32) <= 0x7f7fffff).all()
    offs, rt, rk, slot = ref_cpu.dispatch_plan(c.idx, c.w, c.E, c.cap, c.active)
    sit = {}
    for e in range(c.E):
        for k in range(K):
            cand = c.idx[:, k] == e
            sit[e * K + k] = (int(cand.sum()), int((slot[cand, k] >= 0).sum()), c.w.view(np.uint32)[cand, k])
    assert any(0 < v[1] < v[0] for v in sit.values()), "no slot overflows: the select is never reached"
    if c.expect:
        c.expect(sit)
    return c, (offs, rt, rk, slot)


def _plan_outputs(plan, total):
    return (plan.offsets.cpu().numpy(), plan.row_token.cpu().numpy()[:total], plan.row_k.cpu().numpy()[:total],
            plan.slot_of.cpu().numpy())


def _device_inputs(c, dev):
    act = None if c.active is None else torch.tensor(c.active, device=dev)
    return torch.from_numpy(c.idx).to(dev), torch.from_numpy(c.w).to(dev), act


@pytest.mark.parametrize("name", list(CASES))
def test_plan_select(dev, name):
    from apertis_llm_amd import ops
    c, ref = oracle_side(name)
    idx, w, act = _device_inputs(c, dev)
    assert torch.equal(w.cpu().view(torch.int32), torch.from_numpy(c.w).view(torch.int32)), "the keys reach the device bit for bit"
    got = _plan_outputs(ops.moe_plan(idx, w, c.E, c.cap, act), int(ref[0][-1]))
    for g, r, what in zip(got, ref, ("expert_offsets", "row_token", "row_k", "slot_of")):
        assert g.dtype == r.dtype and np.array_equal(g, r), f"{name}: {what} differs in {int((g != r).sum())} places"


def test_plan_select_same_workspace_twice(dev):
    """No state survives a call: three plans through one workspace that starts out as garbage (A, then another input, then A
    again) - both runs of A equal each other and ops.moe_plan's result, on all four outputs."""
    from apertis_llm_amd import _lib, ops
    from apertis_llm_amd._lib import check, ptr, stream_ptr
    lib = _lib.load()
    a, _ = oracle_side("two_keys_bit0")
    b, _ = oracle_side("neighbours")
    nws = max(lib.apertis_moe_plan_workspace_bytes(c.idx.shape[0], c.E, c.idx.shape[1]) for c in (a, b)) // 4 + 1
    ws = torch.randint(-2**31, 2**31 - 1, (nws,), device=dev, dtype=torch.int64).to(torch.int32)

    def run(c):
        idx, w, act = _device_inputs(c, dev)
        S, K = c.idx.shape
        act = None if act is None else act.to(torch.uint8).contiguous()
        out = [torch.full((n,), -7, device=dev, dtype=torch.int32) for n in (c.E + 1, S * K, S * K, S * K)]
        check(lib.apertis_moe_plan(ptr(idx), ptr(w), ptr(act), c.cap, ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), ptr(ws),
                                   S, c.E, K, stream_ptr()), "apertis_moe_plan")
        return out
    first = run(a)
    run(b)
    second = run(a)
    idx, w, act = _device_inputs(a, dev)
    plan = ops.moe_plan(idx, w, a.E, a.cap, act)
    total = int(plan.offsets[-1])
    for x, y in zip(first, second):
        assert torch.equal(x, y)
    assert torch.equal(first[0], plan.offsets) and torch.equal(first[3], plan.slot_of.reshape(-1))
    assert torch.equal(first[1][:total], plan.row_token[:total]) and torch.equal(first[2][:total], plan.row_k[:total])
