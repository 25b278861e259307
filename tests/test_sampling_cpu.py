"""generate()'s fused next-token selection, the parts that need no GPU: the C ABI's argument checks (before any launch), the
binding, and the shared CPU restatement of the reference's selection (tests/sampling_ref.py) against torch's own ops."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import load_golden
from sampling_ref import inverse_cdf, reference_select, sample_bits, topp_keep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from apertis_llm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib, _lib.load()


def _sample(lib, logits=8, rs=64, dtype=0, B=1, V=64, counts=None, pen=1.0, do_sample=1, temp=1.0, top_k=0, top_p=1.0,
            step=8, alive_in=8, alive_out=8, eos=None, n_eos=0, nxt=8, uniforms=None, u_rs=0, u_cols=0, err=8):
    return lib.apertis_sample_next(logits, rs, dtype, B, V, counts, pen, do_sample, temp, top_k, top_p, 1, step, 0, alive_in,
                                   alive_out, eos, n_eos, 0, nxt, uniforms, u_rs, u_cols, None, None, None, err, None)


def test_sampling_entry_points_validate_before_any_launch():
    """Every refusal below returns before a kernel could go out (the pointers are not device memory; a launch would fault)."""
    _lm, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "apertis_hip.h")).read()
    cap = int(re.search(r"#define APERTIS_SAMPLE_MAX_VOCAB (\d+)", hdr).group(1))
    from apertis_llm_amd import ops
    assert cap == ops.SAMPLE_MAX_VOCAB == 262144
    # null pointers, sizes, top_k > V, a bad temperature, bad uniforms: argument errors
    assert _sample(lib, logits=None) == -1
    assert _sample(lib, alive_in=None) == -1 and _sample(lib, alive_out=None) == -1
    assert _sample(lib, nxt=None) == -1 and _sample(lib, err=None) == -1
    assert _sample(lib, B=0) == -1 and _sample(lib, V=0) == -1
    assert _sample(lib, B=2, rs=63) == -1                     # rows would overlap
    assert _sample(lib, top_k=65) == -1 and _sample(lib, top_k=-1) == -1
    assert _sample(lib, temp=0.0) == -1
    assert _sample(lib, n_eos=2) == -1 and _sample(lib, n_eos=-1, eos=8) == -1
    assert _sample(lib, uniforms=8, u_cols=0) == -1 and _sample(lib, B=2, uniforms=8, u_rs=3, u_cols=4) == -1
    # shapes it does not take: unsupported, the caller keeps the stock code
    assert _sample(lib, dtype=2) == -2
    assert _sample(lib, V=cap + 1, rs=cap + 1) == -2
    # the occurrence table
    assert lib.apertis_token_counts(None, 4, 1, 4, 64, 8, 8, None) == -1
    assert lib.apertis_token_counts(8, 4, 1, 4, 64, None, 8, None) == -1
    assert lib.apertis_token_counts(8, 4, 1, 4, 64, 8, None, None) == -1
    assert lib.apertis_token_counts(8, 4, 1, -1, 64, 8, 8, None) == -1 and lib.apertis_token_counts(8, 2, 2, 4, 64, 8, 8, None) == -1
    assert lib.apertis_token_counts(8, 4, 1, 4, cap + 1, 8, 8, None) == -2
    assert lib.apertis_token_counts(8, 4, 1, 0, 64, 8, 8, None) == 0        # nothing to count: no launch


def test_sample_ops_refuse_cpu_tensors_and_fall_back_only_by_shape():
    """ops.sample_next is GPU-only (no CPU fallback); sample_supported is the shape rule generate() keys the stock path on."""
    from apertis_llm_amd import ops
    x = torch.zeros(2, 64)
    assert not ops.sample_supported(x)
    with pytest.raises(ops.ApertisHipError):
        ops.sample_next(x, torch.ones(2, dtype=torch.long), torch.zeros(1, dtype=torch.int32), do_sample=True)
    assert ops.SAMPLE_FUSED is True and ops.SAMPLE_UNIFORMS is None
    ops.SAMPLE_FUSED = False
    try:
        from apertis_llm_amd.ops import sample as S
        assert S.SAMPLE_FUSED is False
    finally:
        ops.SAMPLE_FUSED = True


def test_hash_restatement_is_well_mixed():
    """The numpy copy of the kernel's counter hash: distinct, roughly uniform draws across rows and steps."""
    us = np.array([sample_bits(1234, b, s) for b in range(16) for s in range(256)], dtype=np.float64) / 2.0 ** 32
    assert len(set(us.tolist())) == us.size
    hist = np.histogram(us, bins=16, range=(0, 1))[0]
    assert abs(us.mean() - 0.5) < 0.02 and hist.min() > 0.7 * us.size / 16


def test_restatement_matches_the_reference_ops():
    """sampling_ref's CPU restatement against the reference's own block (core.py:1605-1627, run here with torch's ops): the
    same processed logits bit for bit, the same kept set where the fp32 cumsum is clear of top_p, probabilities within 1e-6."""
    torch.manual_seed(3)
    B, V = 3, 200
    logits = torch.randn(B, V) * 3
    logits[0, 5] = logits[0, 9]                                # a tie
    hist = [torch.randint(0, V + 5, (40,)).tolist() for _ in range(B)]
    for pen, temp, k, p in [(1.3, 0.7, 20, 0.9), (1.0, 1.0, 0, 0.5), (1.1, 0.6, 50, 1.0), (1.0, 2.0, 1, 0.9)]:
        x = logits.clone()
        for b in range(B):
            for t in hist[b]:
                if t < V:
                    x[b, t] /= pen
        if temp != 1.0:
            x = x / temp
        if k > 0:
            kth = torch.topk(x, k).values[:, -1].unsqueeze(-1)
            x.masked_fill_(x < kth, float("-inf"))
        if p < 1.0:
            s, si = torch.sort(x, descending=True)
            cum = torch.cumsum(torch.softmax(s, dim=-1), dim=-1)
            rm = cum > p
            rm[..., 1:] = rm[..., :-1].clone()
            rm[..., 0] = 0
            x.masked_fill_(torch.zeros_like(x, dtype=torch.bool).scatter_(-1, si, rm), float("-inf"))
        ref_probs = torch.softmax(x, dim=-1)
        px, keep, probs, margin = reference_select(logits, hist, penalty=pen, do_sample=True, temperature=temp, top_k=k, top_p=p)
        assert torch.equal(keep, torch.isfinite(x)), (pen, temp, k, p)
        assert torch.allclose(probs.float(), ref_probs, rtol=1e-5, atol=1e-7)
        assert margin > 1e-4


def test_topp_restatement_breaks_ties_by_lowest_index():
    """A tie group straddling the cut keeps its lowest indices first; top_p <= 0 keeps exactly one token."""
    x = torch.tensor([[0.0, 1.0, 1.0, 1.0, 1.0, -1.0]])
    keep, _ = topp_keep(x, torch.ones_like(x, dtype=torch.bool), 0.5)     # 4 x 0.222: the cut falls on the 3rd of the group
    assert keep.tolist() == [[False, True, True, True, False, False]]
    keep, _ = topp_keep(x, torch.ones_like(x, dtype=torch.bool), 0.0)
    assert keep.tolist() == [[False, True, False, False, False, False]]
    i, d = inverse_cdf(np.array([0.25, 0.0, 0.5, 0.25]), 0.3)
    assert i == 2 and abs(d - 0.05) < 1e-12


@pytest.mark.parametrize("name", ["generate_sampled_ssm_dense", "generate_sampled_ssm_moe", "generate_sampled_mha"])
def test_restatement_reproduces_the_reference_capture(name):
    """The shared CPU restatement against the reference itself (tools/gen_golden.py generate_sampled): from the capture's raw
    logits and token history it gives every live step's probs handed to multinomial (same kept set, rtol 1e-5), the recorded
    uniform picks the reference's token by the fp64 inverse CDF, and greedy + penalty gives the reference's greedy tokens."""
    g = load_golden(name)
    P = int(g["prompt"].shape[1])
    kw = dict(penalty=float(g["repetition_penalty"]), do_sample=True, temperature=float(g["temperature"]), top_k=int(g["top_k"]),
              top_p=float(g["top_p"]))
    assert float(g["margin_u"]) >= 1e-3 and float(g["margin_top_p"]) >= 1e-3 and float(g["margin_top_k"]) > 1e-4
    toks, live = g["tokens"], g["live"]
    n = 0
    for s_ in range(live.shape[1]):
        for b in range(2):
            if not live[b, s_]:
                continue
            _, keep, probs, _ = reference_select(g["step_logits"][b:b + 1, s_], [toks[b, :P + s_].tolist()], **kw)
            ref = g["probs"][b, s_].double()
            assert torch.equal(keep[0], ref > 0), (b, s_)
            assert torch.allclose(probs[0][keep[0]], ref[keep[0]], rtol=1e-5, atol=0), (b, s_)
            i, d = inverse_cdf(probs[0].numpy(), float(g["uniforms"][b, s_]))
            assert i == int(toks[b, P + s_]) and d > 5e-4, (b, s_)
            n += 1
    assert n >= 56
    if "pen_tokens" in g:
        pt = g["pen_tokens"]
        for s_ in range(g["pen_live"].shape[1]):
            for b in range(2):
                if g["pen_live"][b, s_]:
                    x, _, _, _ = reference_select(g["pen_step_logits"][b:b + 1, s_], [pt[b, :P + s_].tolist()],
                                                  penalty=kw["penalty"], do_sample=False)
                    assert int(torch.argmax(x[0])) == int(pt[b, P + s_]), (b, s_)
