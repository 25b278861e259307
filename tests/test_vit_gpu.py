"""The vision tower on the project's kernels (ops.VIT_FUSED; multimodal.py: _fused_body) against the fp64 oracle: eval
features, the launches that prove the fused path ran, train-mode gradients of every parameter, bf16 autocast with the tower's
default dropout, a whole multimodal model, and the fallback of a tower that does not qualify.

Geometries: image / patch 32/8 (L = 17: less than one key tile, one work-group) and 72/8 (L = 82: three key tiles, two
work-groups) at (Dv 128, heads 2) and (Dv 256, heads 2) - head dims 64 and 128 - with two layers, so that a boundary between
two layers and the boundary into vision_ln are both there."""
import pytest
import torch

from conftest import rel_error_report

pytestmark = pytest.mark.gpu

GEOMS = [(32, 128), (32, 256), (72, 128), (72, 256)]            # (image size, Dv); patch 8, heads 2, 2 layers
PATCH, HEADS, LAYERS = 8, 2, 2


@pytest.fixture
def vit_switch():
    from apertis_llm_amd import ops
    old = ops.VIT_FUSED
    yield lambda on: setattr(ops, "VIT_FUSED", bool(on))
    ops.VIT_FUSED = old


def _encoder(image, Dv, heads=HEADS, layers=LAYERS):
    import apertis_llm_amd as A
    from oracle import seeded
    cfg = A.ApertisConfig(hidden_size=48, num_attention_heads=3, multimodal=True, image_size=image, vision_embed_dim=Dv,
                          vision_patch_size=PATCH, vision_layers=layers, vision_heads=heads)
    enc = A.UnifiedMultimodalEncoder(cfg)
    sd = seeded.fill_state_dict(enc.state_dict(), gain=2.0)
    enc.load_state_dict(sd)
    return enc, sd


def _pixels(image, B=2, seed=7):
    return torch.randn(B, 3, image, image, generator=torch.Generator().manual_seed(seed))


def _no_dropout(enc):
    for layer in enc.vision_layers:
        layer.dropout.p = layer.dropout1.p = layer.dropout2.p = 0.0
        layer.self_attn.dropout = 0.0


def _launches(fn, name="apertis_attention_full_fwd"):
    from apertis_llm_amd import ops
    timer = ops.KernelTimer([name])
    ops.set_kernel_timer(timer)
    try:
        out = fn()
    finally:
        ops.set_kernel_timer(None)
    return out, timer.summary().get(name, {"launches": 0})["launches"]


@pytest.mark.parametrize("image,Dv", GEOMS)
def test_eval_features_match_fp64_oracle_and_the_fused_path_ran(dev, vit_switch, image, Dv):
    """Switch on: features against the fp64 oracle at the bar test_vision_golden holds the stock path to (rtol 2e-4,
    atol_scale 2e-5), with one apertis_attention_full_fwd launch per layer.  Switch off: no such launch, and the features
    are the bits of a module whose switch was never touched."""
    from oracle import ref_cpu
    enc, sd = _encoder(image, Dv)
    enc = enc.to(dev).eval()
    px = _pixels(image)
    with torch.no_grad():
        untouched = enc(px.to(dev))                                       # (the suite runs with the switch unset: off)
        ref = ref_cpu.vision_encoder({k: v.double() for k, v in sd.items()}, "", px.double(), PATCH, LAYERS, HEADS)
        vit_switch(True)
        assert enc.fused_supported(torch.empty(2, (image // PATCH) ** 2 + 1, Dv, device=dev))
        fused, n_on = _launches(lambda: enc(px.to(dev)))
        vit_switch(False)
        stock, n_off = _launches(lambda: enc(px.to(dev)))
    assert n_on == LAYERS and n_off == 0
    assert fused.shape == ref.shape and fused.dtype == torch.float32
    rel_error_report(f"vit {image}/{PATCH} Dv{Dv} eval features, stock", stock, ref, rtol=2e-4, atol_scale=2e-5, check=False)
    rel_error_report(f"vit {image}/{PATCH} Dv{Dv} eval features, fused", fused, ref, rtol=2e-4, atol_scale=2e-5)
    assert torch.equal(stock, untouched)


def _grads(enc, px, w, dev):
    enc.zero_grad(set_to_none=True)
    pxd = px.to(dev).requires_grad_()
    (enc(pxd) * w.to(dev)).sum().backward()
    g = {n: p.grad.detach().cpu() for n, p in enc.named_parameters()}
    g["pixel_values"] = pxd.grad.detach().cpu()
    return g


@pytest.mark.parametrize("image,Dv", GEOMS)
def test_train_gradients_match_fp64_autograd(dev, vit_switch, image, Dv):
    """Train mode, fp32, every dropout probability of the tower 0: the gradient of every parameter and of pixel_values
    against fp64 autograd through the oracle at rel_error_report's defaults (rtol 1e-4), the stock path's achieved error on
    the same inputs reported beside each.  The stock path meets that bar on every tensor of these geometries (worst_excess
    at most 0.07 on an MI355X; the fused path at most 0.10), so the fused path is held to the bar itself everywhere."""
    from oracle import ref_cpu
    enc, sd = _encoder(image, Dv)
    _no_dropout(enc)
    enc = enc.to(dev).train()
    px = _pixels(image)
    L = (image // PATCH) ** 2 + 1
    w = torch.randn(2, L, Dv, generator=torch.Generator().manual_seed(3))
    sd64 = {k: v.double().requires_grad_() for k, v in sd.items()}
    px64 = px.double().requires_grad_()
    (ref_cpu.vision_encoder(sd64, "", px64, PATCH, LAYERS, HEADS) * w.double()).sum().backward()
    ref = {k: v.grad for k, v in sd64.items()}
    ref["pixel_values"] = px64.grad
    vit_switch(True)
    fused, n_on = _launches(lambda: _grads(enc, px, w, dev), "apertis_attention_full_bwd")
    vit_switch(False)
    stock = _grads(enc, px, w, dev)
    assert n_on == LAYERS and set(fused) == set(ref) == set(stock)
    for n in sorted(ref):
        rel_error_report(f"vit {image}/{PATCH} Dv{Dv} grad {n}, stock", stock[n], ref[n], check=False)
        rel_error_report(f"vit {image}/{PATCH} Dv{Dv} grad {n}, fused", fused[n], ref[n])


def test_bf16_autocast_training_with_default_dropout(dev, vit_switch):
    """The tower's default p = 0.1 under bf16 autocast: finite loss and gradients, the same bits from the same
    torch.manual_seed (every mask is a counter hash seeded from torch's RNG), other features from another seed."""
    enc, _ = _encoder(72, 128)
    enc = enc.to(dev).train()
    px = _pixels(72).to(dev)
    vit_switch(True)

    def run(seed):
        enc.zero_grad(set_to_none=True)
        torch.manual_seed(seed)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            feats = enc(px)
            loss = feats.float().square().mean()
        loss.backward()
        return feats.detach().clone(), loss.detach(), {n: p.grad.detach().clone() for n, p in enc.named_parameters()}

    (f1, l1, g1), n_on = _launches(lambda: run(5))
    f2, l2, g2 = run(5)
    f3, _, _ = run(6)
    assert n_on == LAYERS and f1.dtype == torch.float32
    assert torch.isfinite(l1) and all(torch.isfinite(g).all() for g in g1.values())
    assert len(g1) == len(list(enc.parameters()))
    assert torch.equal(f1, f2) and torch.equal(l1, l2) and all(torch.equal(g1[n], g2[n]) for n in g1)
    assert not torch.equal(f1, f3)


def test_whole_multimodal_model_under_the_switch(dev, vit_switch):
    import apertis_llm_amd as A
    from oracle import seeded
    cfg = A.ApertisConfig(vocab_size=512, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128,
                          attention_type="selective_ssm", multimodal=True, image_size=32, vision_embed_dim=128,
                          vision_patch_size=PATCH, vision_layers=LAYERS, vision_heads=HEADS)
    model = A.ApertisForCausalLM(cfg)
    model.load_state_dict(seeded.fill_state_dict(model.state_dict()))
    model = model.to(dev)
    ids = torch.randint(4, 512, (2, 24), generator=torch.Generator().manual_seed(1)).to(dev)
    px = _pixels(32).to(dev)
    model.eval()
    with torch.no_grad():
        vit_switch(False)
        off = model(input_ids=ids, pixel_values=px, use_cache=False)
        vit_switch(True)
        on, n_on = _launches(lambda: model(input_ids=ids, pixel_values=px, use_cache=False))
    assert n_on == LAYERS
    logits_on, logits_off = on[1], off[1]                                   # (loss, logits, ...)
    assert logits_on.shape[:2] == (2, 24)
    rel_error_report("multimodal model eval logits, fused tower vs stock tower", logits_on, logits_off.double(), rtol=1e-4)
    model.train()
    torch.manual_seed(0)
    loss = model(input_ids=ids, pixel_values=px, labels=ids)[0]
    loss.backward()
    assert torch.isfinite(loss)
    bad = [n for n, p in model.named_parameters() if p.grad is not None and not torch.isfinite(p.grad).all()]
    assert not bad, bad
    tower = [n for n, p in model.named_parameters() if "multimodal_encoder" in n and p.grad is None]
    assert not tower, tower


def test_tower_that_does_not_qualify_runs_the_stock_path(dev, vit_switch):
    """The `vision` fixture's geometry (Dv 32, 2 heads: head dim 16): the switch changes nothing, bit for bit."""
    enc, _ = _encoder(32, 32)
    enc = enc.to(dev).eval()
    px = _pixels(32).to(dev)
    with torch.no_grad():
        vit_switch(False)
        off = enc(px)
        vit_switch(True)
        assert not enc.fused_supported(torch.empty(2, 17, 32, device=dev))
        on, n_on = _launches(lambda: enc(px))
    assert n_on == 0 and torch.equal(on, off)
