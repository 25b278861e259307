"""RMSNorm without a GPU: the three entry points refuse bad arguments before any launch, a use_rmsnorm model has the
reference's state-dict keys and reproduces the reference's forward on the CPU (tests/golden/model_ssm_moe_rms.npz carries a
selective_ssm + MoE model, which has no CPU path here, so the CPU forward is checked norm by norm and on a standard_mha model
built from the fixture's norm scales), and model.RMSNorm off the GPU is the reference formula bit for bit."""
import json

import pytest
import torch

from conftest import load_golden

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -2
F32, BF16 = 0, 1


def _lib():
    from apertis_llm_amd import _lib
    return _lib.load()


# non-null stand-ins: validation happens before any launch, nothing is dereferenced
P = 0x1000


def test_rmsnorm_fwd_validates_before_any_launch():
    lib = _lib()
    good = dict(x=P, scale=P, eps=1e-6, y=P, rms=P, T=3, H=64, dx=F32, dy=BF16, st=None)

    def call(**kw):
        a = {**good, **kw}
        return lib.apertis_rmsnorm_fwd(a["x"], a["scale"], a["eps"], a["y"], a["rms"], a["T"], a["H"], a["dx"], a["dy"], a["st"])
    for name in ("x", "scale", "y", "rms"):
        assert call(**{name: None}) == ERR_ARG, name
    assert call(T=-1) == ERR_ARG
    assert call(dx=2) == ERR_ARG and call(dy=-1) == ERR_ARG and call(dy=7) == ERR_ARG
    for H in (0, -4, 6, 4098, 4100):
        assert call(H=H) == ERR_UNSUPPORTED, H
    assert call(T=0) == OK and call(T=0, H=4096) == OK
    assert call(T=0, H=4100) == ERR_UNSUPPORTED and call(T=0, x=None) == ERR_ARG


def test_rmsnorm_bwd_validates_before_any_launch():
    lib = _lib()
    good = dict(x=P, scale=P, rms=P, eps=1e-6, dy=P, dres=None, dx=P, dblk=None, p=0.0, seed=0, part=P, dscale=P, T=3, H=64,
                tx=F32, tg=BF16, st=None)

    def call(**kw):
        a = {**good, **kw}
        return lib.apertis_rmsnorm_bwd(a["x"], a["scale"], a["rms"], a["eps"], a["dy"], a["dres"], a["dx"], a["dblk"], a["p"],
                                       a["seed"], a["part"], a["dscale"], a["T"], a["H"], a["tx"], a["tg"], a["st"])
    for name in ("x", "scale", "rms", "dy", "dx", "part", "dscale"):
        assert call(**{name: None}) == ERR_ARG, name
    assert call(T=-1) == ERR_ARG
    assert call(tx=2) == ERR_ARG and call(tg=-1) == ERR_ARG
    assert call(p=-0.1) == ERR_ARG and call(p=1.0) == ERR_ARG and call(p=float("nan")) == ERR_ARG
    for H in (0, 6, 4098, 4100):
        assert call(H=H) == ERR_UNSUPPORTED, H
    assert call(T=0) == OK and call(T=0, dres=P, dblk=P, p=0.1, seed=5) == OK          # optional operands, nothing launched
    assert lib.apertis_rmsnorm_bwd_blocks(0, 64) == 1 and lib.apertis_rmsnorm_bwd_blocks(32, 64) == 1
    assert lib.apertis_rmsnorm_bwd_blocks(33, 64) == 2
    # the two-level fold from 256 partial rows on: 32 group rows behind them
    assert lib.apertis_rmsnorm_bwd_blocks(8160, 252) == 255 and lib.apertis_rmsnorm_bwd_blocks(8161, 252) == 256 + 32


def test_dropout_add_rmsnorm_fwd_validates_before_any_launch():
    lib = _lib()
    good = dict(blk=P, slot=None, wk=None, K=0, res=P, scale=P, eps=1e-6, y=P, xn=P, rms=P, T=3, H=64, p=0.1, seed=1, tx=F32,
                ty=BF16, st=None)

    def call(**kw):
        a = {**good, **kw}
        return lib.apertis_dropout_add_rmsnorm_fwd(a["blk"], a["slot"], a["wk"], a["K"], a["res"], a["scale"], a["eps"], a["y"],
                                                   a["xn"], a["rms"], a["T"], a["H"], a["p"], a["seed"], a["tx"], a["ty"], a["st"])
    for name in ("blk", "res", "scale", "y", "xn", "rms"):
        assert call(**{name: None}) == ERR_ARG, name
    assert call(T=-1) == ERR_ARG and call(p=1.0) == ERR_ARG and call(p=-0.5) == ERR_ARG
    assert call(tx=3) == ERR_ARG and call(ty=-2) == ERR_ARG
    # the combine form wants its weights and 1 <= K <= 8
    assert call(slot=P, wk=None, K=2) == ERR_ARG and call(slot=P, wk=P, K=0) == ERR_ARG and call(slot=P, wk=P, K=9) == ERR_ARG
    for H in (0, 6, 4098, 4100):
        assert call(H=H) == ERR_UNSUPPORTED, H
    assert call(T=0) == OK and call(T=0, slot=P, wk=P, K=8) == OK


def _fixture_model():
    import apertis_llm_amd as A
    g = load_golden("model_ssm_moe_rms")
    cfg = A.ApertisConfig.from_dict(json.loads(str(g["config_json"])))
    return g, cfg, A.ApertisForCausalLM(cfg)


def test_use_rmsnorm_state_dict_keys_equal_the_fixture():
    from apertis_llm_amd import model as M
    g, cfg, model = _fixture_model()
    assert cfg.use_rmsnorm is True and cfg.to_dict()["use_rmsnorm"] is True
    sd = model.state_dict()
    assert set(sd) == set(g["sd"]), set(sd) ^ set(g["sd"])
    for k, v in g["sd"].items():
        assert tuple(sd[k].shape) == tuple(v.shape), k
    scales = sorted(k for k in sd if k.endswith(".scale"))
    assert scales == sorted([f"model.layers.{i}.{b}.pre_norm.scale" for i in range(2) for b in ("attention", "feed_forward")] +
                            ["model.final_post_norm.scale"])
    model.load_state_dict(g["sd"])
    norms = [m for m in model.modules() if isinstance(m, M.RMSNorm)]
    assert len(norms) == 5 and all(m.eps == cfg.layer_norm_eps for m in norms)
    assert isinstance(model.model.layers[0].feed_forward.ffn.router_norm, M.HipLayerNorm)       # LayerNorms in the reference too


def _reference_formula(x, scale, eps, hidden_size):
    norm_x = x.norm(p=2, dim=-1, keepdim=True)
    rms_x = norm_x * (hidden_size ** -0.5)
    return scale * (x / (rms_x + eps))


@pytest.mark.parametrize("dt", [torch.float32, torch.float64, torch.bfloat16])
def test_rmsnorm_off_gpu_is_the_reference_formula_bit_for_bit(dt):
    from apertis_llm_amd import model as M
    torch.manual_seed(4)
    for H, eps in ((32, 1e-12), (260, 1e-6), (7, 1e-6)):
        norm = M.RMSNorm(H, eps=eps).to(dt)
        with torch.no_grad():
            norm.scale.add_(0.25 * torch.randn(H).to(dt))
        x = (torch.randn(3, 5, H) * 2).to(dt)
        x[1, 2] = 0
        y = norm(x)
        assert y.dtype == dt and torch.equal(y, _reference_formula(x, norm.scale, eps, H))
        yp, xp = norm.forward_pass(x)
        assert torch.equal(yp, y) and xp is x
        assert torch.equal(y[1, 2], torch.zeros(H, dtype=dt))


def test_cpu_forward_reproduces_the_fixture(monkeypatch):
    """The fixture's model is selective_ssm + MoE, whose blocks run on the GPU only; what runs on the CPU is checked against
    it here: the embedding and the first pre-norm of the fixture's weights feed the reference formula, and a standard_mha model
    (stock torch off the GPU) carrying the fixture's norm scales gives, norm for norm, what the formula gives - so the CPU
    arithmetic of a use_rmsnorm model is the reference's.  tests/test_rmsnorm_model_gpu.py matches the fixture's logits."""
    import apertis_llm_amd as A
    from apertis_llm_amd import model as M
    g, cfg, model = _fixture_model()
    model.load_state_dict(g["sd"])
    model.eval()
    emb = model.model.token_embeddings(g["input_ids"])
    pre = model.model.layers[0].attention.pre_norm
    assert torch.equal(pre(emb), _reference_formula(emb, g["sd"]["model.layers.0.attention.pre_norm.scale"], cfg.layer_norm_eps, 32))
    d = dict(cfg.to_dict(), attention_type="standard_mha", use_expert_system=False)
    d.pop("ssm_d_inner", None)
    mha = A.ApertisForCausalLM(A.ApertisConfig.from_dict(d)).eval()
    sd = mha.state_dict()
    for k in sd:
        if k.endswith(".scale"):
            sd[k] = g["sd"][k].clone()
    mha.load_state_dict(sd)
    seen, stock = [], M.RMSNorm.forward

    def spy(self, x):
        y = stock(self, x)
        seen.append((self, x, y))
        return y
    monkeypatch.setattr(M.RMSNorm, "forward", spy)
    with torch.no_grad():
        out = mha(input_ids=g["input_ids"], labels=g["labels"], use_cache=False)
    assert len(seen) == 5 and torch.isfinite(out[0]) and out[1].shape == g["logits"].shape
    for mod, x, y in seen:
        assert torch.equal(y, _reference_formula(x, mod.scale, mod.eps, 32))
