"""Packed rows through the model on the GPU (`document_ids`): the layers run RoPE at positions within each document and
ops.document_attention; a packed batch gives every document the numbers it gets alone, the gradients of the stock path, the
same dropout mask under gradient checkpointing, and the documents' token-weighted mean loss."""
import pytest
import torch

from conftest import rel_error_report

pytestmark = pytest.mark.gpu

LENS = ([5, 92], [96, 1], [40, 17, 40])          # rows of 97 tokens: boundaries inside a tile, on a tile edge, one-token documents
L = 97


@pytest.fixture
def fused_switch():
    from apertis_llm_amd import ops
    prev = ops.ATTN_FUSED
    yield ops
    ops.ATTN_FUSED = prev


def _model(A, dev, **kw):
    base = dict(vocab_size=512, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                attention_type="standard_mha", position_embedding_type="rotary", max_position_embeddings=128,
                hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    base.update(kw)
    torch.manual_seed(0)
    return A.ApertisForCausalLM(A.ApertisConfig(**base)).to(dev)


def _batch(dev):
    gen = torch.Generator().manual_seed(3)
    ids = torch.randint(4, 512, (len(LENS), L), generator=gen).to(dev)
    docs = torch.stack([torch.repeat_interleave(torch.arange(len(l)), torch.tensor(l)) for l in LENS]).to(dev)
    return ids, docs


def _documents():
    for b, lens in enumerate(LENS):
        at = 0
        for n in lens:
            yield b, slice(at, at + n), n
            at += n


def _launched(ops, fn):
    """The attention forward entry points `fn` launched, by name."""
    names = ("apertis_attention_doc_fwd", "apertis_attention_fwd")
    timer = ops.KernelTimer(names)
    ops.set_kernel_timer(timer)
    try:
        out = fn()
    finally:
        ops.set_kernel_timer(None)
    return out, [r[0] for r in timer.records]


def test_packed_logits_equal_the_documents_alone(dev):
    import apertis_llm_amd as A
    model = _model(A, dev).eval()
    ids, docs = _batch(dev)
    with torch.no_grad():
        logits, names = _launched(A.ops, lambda: model(input_ids=ids, document_ids=docs)[1])
        assert names == ["apertis_attention_doc_fwd"] * 2                    # one per layer, and no plain causal launch
        for b, sl, n in _documents():
            alone = model(input_ids=ids[b:b + 1, sl])[1]
            rel_error_report(f"packed logits row {b} tokens {sl.start}..{sl.stop - 1}", logits[b, sl], alone[0], rtol=1e-4)
        # not the numbers of the rows run as one sequence each
        assert not torch.allclose(logits, model(input_ids=ids)[1], rtol=1e-3, atol=1e-3)


def _grads(model, ids, docs):
    model.zero_grad(set_to_none=True)
    torch.manual_seed(42)                         # (the expert router's training noise and the dropout seeds come from torch's RNG)
    loss = model(input_ids=ids, labels=ids, document_ids=docs)[0]
    loss.backward()
    return float(loss), {n: p.grad.detach().float().clone() for n, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("variant", ["plain", "rmsnorm_swiglu", "experts"])
def test_training_gradients_match_stock_path(dev, fused_switch, variant):
    import apertis_llm_amd as A
    ops = fused_switch
    kw = {"plain": {}, "rmsnorm_swiglu": dict(use_rmsnorm=True, use_swiglu=True),
          "experts": dict(use_expert_system=True, num_experts=4, experts_per_token=2)}[variant]
    model = _model(A, dev, **kw).train()
    ids, docs = _batch(dev)
    ops.ATTN_FUSED = True
    (lf, gf), names = _launched(ops, lambda: _grads(model, ids, docs))
    assert names == ["apertis_attention_doc_fwd"] * 2
    ops.ATTN_FUSED = False
    (ls, gs), names = _launched(ops, lambda: _grads(model, ids, docs))
    assert names == [] and gf.keys() == gs.keys() and len(gs) > 0
    assert abs(lf - ls) <= 1e-5 * abs(ls)
    for n in gs:
        rel_error_report(f"packed train grad fp32 {variant} {n}", gf[n], gs[n], rtol=1e-4)


def test_checkpointed_layer_sees_the_same_dropout_mask(dev):
    import apertis_llm_amd as A
    model = _model(A, dev, attention_probs_dropout_prob=0.1).train()
    ids, docs = _batch(dev)
    grads = []
    for ckpt in (False, True):
        model.model.gradient_checkpointing = ckpt
        grads.append(_grads(model, ids, docs)[1])
    assert grads[0].keys() == grads[1].keys() and len(grads[0]) > 0
    for n in grads[0]:
        torch.testing.assert_close(grads[1][n], grads[0][n], rtol=1e-5, atol=1e-7, msg=n)


@pytest.mark.parametrize("fused_loss", [False, True])
def test_packed_loss_is_the_documents_weighted_mean(dev, fused_loss):
    import apertis_llm_amd as A
    model = _model(A, dev).train()                                       # (no dropout anywhere: train mode only selects the loss path)
    model.fused_lm_head_loss = fused_loss
    ids, docs = _batch(dev)
    labels = ids.clone()
    labels[0, 10:20] = -100                                              # some ignored targets inside a document
    with torch.no_grad():
        out = model(input_ids=ids, labels=labels, document_ids=docs)
        assert (out[1] is None) == fused_loss                            # the fused LM-head loss path keeps no logits
        num, den = 0.0, 0
        for b, sl, n in _documents():
            n_i = int((labels[b, sl][1:] != -100).sum())
            if n_i:
                num += float(model(input_ids=ids[b:b + 1, sl], labels=labels[b:b + 1, sl])[0]) * n_i
                den += n_i
        want = num / den
        assert abs(float(out[0]) - want) <= 1e-4 * abs(want), (float(out[0]), want)
        # the label at a document's first token (t >= 1) is never a target
        changed = labels.clone()
        changed[0, 5], changed[1, 96], changed[2, 40], changed[2, 57] = 7, 8, 9, 10
        assert float(model(input_ids=ids, labels=changed, document_ids=docs)[0]) == float(out[0])
