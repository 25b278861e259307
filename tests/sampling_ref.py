"""CPU restatement of the reference's next-token selection (core.py:1605-1627) and a numpy copy of the sampling kernel's
counter hash, shared by tests/test_sampling_cpu.py and tests/test_sampling_gpu.py.

Penalty, temperature and top-k run as the reference runs them, in fp32 CPU torch (true divisions, torch.topk).  The top-p cut
is taken in fp64 (softmax, sort with equal values in ascending index order, cumsum), and the final distribution is the fp64
softmax of what is kept: the kernel is held to these within the tolerances of each test."""
import numpy as np
import torch

M32 = 0xFFFFFFFF


def _avalanche32(h):
    h &= M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def sample_bits(seed, row, step):
    """The 32 bits the kernel draws for (seed, row, step) (csrc/sampling.hip sample_bits)."""
    seed &= 0xFFFFFFFFFFFFFFFF
    step &= 0xFFFFFFFFFFFFFFFF
    h = _avalanche32((seed & M32) ^ ((row * 0x9E3779B9) & M32))
    return _avalanche32(h ^ (seed >> 32) ^ ((step * 0x85EBCA6B) & M32) ^ (step >> 32))


def sample_u(seed, row, step):
    return sample_bits(seed, row, step) * 2.0 ** -32


def processed_logits(logits, history=None, penalty=1.0, temperature=1.0):
    """Steps 1-2 on fp32 CPU torch: logits [B, V] (any float dtype, read as fp32), history: list of per-row token lists."""
    x = logits.detach().to("cpu", torch.float32).clone()
    V = x.shape[-1]
    if penalty != 1.0 and history is not None:
        for b, row in enumerate(history):
            for t in row:
                if t < V:                                   # (negative ids index from the end, as in Python)
                    x[b, t] /= penalty
    if temperature != 1.0:
        x = x / temperature
    return x


def topk_keep(x, k):
    """Step 3 exactly as the reference runs it: every value >= the k-th largest (duplicates counted) stays."""
    if k <= 0:
        return torch.ones_like(x, dtype=torch.bool)
    kth = torch.topk(x, k).values[:, -1:]
    return ~(x < kth)


def topp_keep(x, keep, top_p):
    """Step 4 in fp64: sorted descending (equal values: lowest index first), keep up to and including the first position whose
    inclusive cumulative probability exceeds top_p.  Returns (mask, margin): margin = the smallest |cum - top_p| over the
    positions that decide the cut."""
    B, V = x.shape
    out = keep.clone()
    margin = float("inf")
    if top_p >= 1.0:
        return out, margin
    for b in range(B):
        v = x[b].double().numpy().copy()
        v[~keep[b].numpy()] = -np.inf
        order = np.lexsort((np.arange(V), -v))
        s = v[order]
        p = np.exp(s - s.max())
        p /= p.sum()
        cum = np.cumsum(p)
        drop = cum > top_p
        drop[1:] = drop[:-1].copy()
        drop[0] = False
        m = torch.zeros(V, dtype=torch.bool)
        m[torch.from_numpy(order[~drop].copy())] = True
        out[b] &= m
        live = np.isfinite(s)
        if live.any():
            margin = min(margin, float(np.abs(cum[live] - top_p).min()))
    return out, margin


def reference_select(logits, history=None, *, penalty=1.0, do_sample=True, temperature=1.0, top_k=0, top_p=1.0):
    """(processed fp32 logits, kept mask, fp64 probabilities [B, V], top-p margin) of core.py:1605-1627."""
    temp = max(temperature, 1e-6) if do_sample else 1.0
    x = processed_logits(logits, history, penalty, temp)
    if not do_sample:
        return x, None, None, None
    keep = topk_keep(x, top_k)
    keep, margin = topp_keep(x, keep, top_p)
    z = x.double().masked_fill(~keep, float("-inf"))
    probs = torch.softmax(z, dim=-1)
    return x, keep, probs, margin


def inverse_cdf(probs_row, u):
    """(index, distance of u from the nearest CDF step) of an fp64 inverse-CDF pick in vocabulary order."""
    c = np.cumsum(np.asarray(probs_row, dtype=np.float64))
    c /= c[-1]
    i = int(np.searchsorted(c, u, side="right"))
    i = min(i, len(c) - 1)
    steps = c[probs_row > 0] if np.ndim(probs_row) else c
    return i, float(np.abs(steps - u).min())
