"""Kernel-level parity of the MoE path (through the C ABI) with the CPU oracle / golden vectors.
Integer outputs (top-k indices, dispatch plan, permutation) are compared bit-exact."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden

pytestmark = pytest.mark.gpu


def _close(got, ref, name, rtol=1e-4, atol_scale=2e-6):
    ref = torch.as_tensor(ref).detach().cpu().to(torch.float64)
    got = got.detach().cpu().to(torch.float64)
    atol = atol_scale * float(ref.abs().max()) + 1e-30
    bad = (got - ref).abs() > atol + rtol * ref.abs()
    assert not bad.any(), f"{name}: {int(bad.sum())}/{bad.numel()} outside rtol {rtol}; max abs diff " \
                          f"{float((got - ref).abs().max()):.3e} (ref max {float(ref.abs().max()):.3e})"


# ------------------------------------------------------------------ gate
@pytest.mark.parametrize("name", ["moe_eval", "moe_train_overflow", "moe_eval_k3"])
def test_gate_topk_golden(dev, name):
    from apertis_llm_amd import ops
    g = load_golden(name)
    K = int(g["K"])
    gates, idx, w = ops.moe_gate_topk(g["logits"].to(dev), K)
    assert torch.equal(idx.cpu().long(), g["idx"].long()), "top-k indices must be bit-exact"
    _close(gates, g["gates"], "gates", rtol=1e-5)
    _close(w, g["w"], "w", rtol=1e-5)


@pytest.mark.parametrize("S,E,K", [(1000, 8, 2), (77, 4, 1), (513, 16, 3), (300, 5, 2), (64, 64, 8)])
def test_gate_topk_backward(dev, S, E, K):
    from apertis_llm_amd import ops
    from oracle import ref_cpu
    torch.manual_seed(S + E)
    logits = torch.randn(S, E) * 2
    lo = logits.clone().requires_grad_(True)
    gates_o = F.softmax(lo, -1)
    p, idx_o = ref_cpu.topk_lowest_index_first(gates_o, K)
    w_o = p / (p.sum(-1, keepdim=True) + 1e-6)
    dw, dg = torch.randn(S, K), torch.randn(S, E)
    (w_o * dw).sum().add((gates_o * dg).sum()).backward()
    ld = logits.to(dev).requires_grad_(True)
    gates, idx, w = ops.moe_gate_topk(ld, K)
    assert torch.equal(idx.cpu().long(), idx_o)
    ((w * dw.to(dev)).sum() + (gates * dg.to(dev)).sum()).backward()
    _close(ld.grad, lo.grad, "dlogits", atol_scale=1e-5)


def test_gate_ties_lowest_index_first(dev):
    from apertis_llm_amd import ops
    logits = torch.zeros(5, 8)
    logits[1, 3] = logits[1, 6] = 1.0
    _, idx, _ = ops.moe_gate_topk(logits.to(dev), 2)
    assert idx.cpu().tolist() == [[0, 1], [3, 6], [0, 1], [0, 1], [0, 1]]


# ------------------------------------------------------------------ plan
def _plan_case(dev, S, E, K, cap, seed, skew=0.0, ties=False, active=None):
    from apertis_llm_amd import ops
    from oracle import ref_cpu
    rng = np.random.default_rng(seed)
    logits = rng.standard_normal((S, E)).astype(np.float32)
    logits[:, 0] += skew
    if ties:
        logits = np.round(logits)       # many equal rows -> equal weights
    gates, idx, w = ops.moe_gate_topk(torch.from_numpy(logits).to(dev), K)
    act_t = None if active is None else torch.tensor(active, device=dev)
    plan = ops.moe_plan(idx, w, E, cap, act_t)
    offs, rt, rk, slot = ref_cpu.dispatch_plan(idx.cpu().numpy(), w.cpu().numpy(), E, cap, active)
    total = int(offs[-1])
    assert plan.offsets.cpu().tolist() == offs.tolist()
    assert plan.row_token.cpu().numpy()[:total].tolist() == rt.tolist()
    assert plan.row_k.cpu().numpy()[:total].tolist() == rk.tolist()
    assert plan.slot_of.cpu().numpy().tolist() == slot.tolist()
    return total


@pytest.mark.parametrize("S,E,K", [(4096, 8, 2), (1000, 8, 2), (63, 4, 2), (64, 4, 1), (65, 16, 3), (5000, 64, 8), (1, 2, 2)])
def test_plan_eval_no_capacity(dev, S, E, K):
    assert _plan_case(dev, S, E, K, None, seed=S) == S * K


@pytest.mark.parametrize("S,E,K,skew", [(4096, 8, 2, 0.0), (4096, 8, 2, 2.0), (1000, 4, 2, 1.0), (777, 8, 3, 3.0), (8192, 8, 2, 0.5),
                                        (24, 4, 2, 0.0), (24, 4, 2, 1.5), (30, 4, 2, 3.0), (7, 2, 2, 1.0), (100, 4, 2, 2.0)])
def test_plan_train_capacity_overflow(dev, S, E, K, skew):
    from oracle import ref_cpu
    cap = ref_cpu.expert_capacity(S, E, 1.25)
    total = _plan_case(dev, S, E, K, cap, seed=S + 1, skew=skew)
    assert total <= E * cap


def test_plan_ties_and_dropped_experts(dev):
    _plan_case(dev, 2000, 8, 2, 100, seed=5, skew=1.0, ties=True)
    _plan_case(dev, 900, 8, 2, 150, seed=6, active=[1, 0, 1, 1, 0, 1, 1, 1])
    _plan_case(dev, 900, 8, 2, None, seed=7, active=[0, 1, 1, 1, 1, 1, 1, 1])
    # a handful of tokens (the decode step's one-launch plan: S <= 64, E * K <= 16): ties at the capacity threshold, dropped
    # experts, a capacity of one row, every token on one expert
    _plan_case(dev, 60, 8, 2, 9, seed=8, skew=1.0, ties=True)
    _plan_case(dev, 64, 8, 2, 5, seed=9, skew=3.0, ties=True)
    _plan_case(dev, 48, 8, 2, 10, seed=10, active=[1, 0, 1, 1, 0, 1, 1, 1])
    _plan_case(dev, 16, 8, 2, None, seed=11, active=[0, 1, 1, 1, 1, 1, 1, 0])
    _plan_case(dev, 33, 4, 2, 1, seed=12, skew=5.0)
    _plan_case(dev, 2, 8, 2, None, seed=13)


def test_plan_golden_kept_rows(dev):
    """kept (token,k,expert) rows captured from the reference's own dispatch loop."""
    from apertis_llm_amd import ops
    for name in ["moe_eval", "moe_train_overflow", "moe_eval_k3"]:
        g = load_golden(name)
        E, K, cap = int(g["E"]), int(g["K"]), int(g["capacity"])
        plan = ops.moe_plan(g["idx"].int().to(dev), g["w"].to(dev), E, cap if cap > 0 else None)
        offs = plan.offsets.cpu().tolist()
        assert offs == g["expert_offsets"].tolist()
        rt, rk = plan.row_token.cpu().tolist(), plan.row_k.cpu().tolist()
        rows = [(rt[r], rk[r], e) for e in range(E) for r in range(offs[e], offs[e + 1])]
        assert rows == [tuple(r) for r in g["kept_rows"].tolist()], name


# ------------------------------------------------------------------ gather+LN, combine
@pytest.mark.parametrize("H,dt", [(32, torch.float32), (704, torch.float32), (256, torch.bfloat16), (1028, torch.float32)])
def test_gather_ln_and_combine(dev, H, dt):
    from apertis_llm_amd import ops
    torch.manual_seed(H)
    S, E, K = 333, 8, 2
    x = torch.randn(S, H) * 2 + 0.5
    gamma, beta = torch.randn(E, H), torch.randn(E, H)
    logits = torch.randn(S, E)
    gates, idx, w = ops.moe_gate_topk(logits.to(dev), K)
    plan = ops.moe_plan(idx, w, E, 70)
    offs = plan.offsets.cpu().tolist()
    total = offs[-1]
    rt = plan.row_token.cpu()[:total].long()
    rk = plan.row_k.cpu()[:total].long()
    eo = torch.repeat_interleave(torch.arange(E), torch.tensor([offs[e + 1] - offs[e] for e in range(E)]))
    xd = x.to(dev).to(dt).requires_grad_(True)
    gd, bd = gamma.to(dev).requires_grad_(True), beta.to(dev).requires_grad_(True)
    wd = w.detach().clone().requires_grad_(True)
    xg = ops.moe_gather_ln(xd, gd, bd, plan, 1e-12)
    out = ops.moe_combine(xg, wd, plan)
    dout = torch.randn(S, H)
    out.backward(dout.to(dev).to(dt))
    # oracle in fp32/fp64 on the same (possibly bf16-rounded) input
    xr = x.to(dt).double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    wr = w.detach().cpu().double().requires_grad_(True)
    xn = F.layer_norm(xr[rt], (H,), None, None, 1e-12) * gr[eo] + br[eo]
    if dt == torch.bfloat16:
        xn_q = xn + (xn.detach().to(torch.bfloat16).double() - xn.detach())   # straight-through rounding
    else:
        xn_q = xn
    o = torch.zeros(S, H, dtype=torch.float64).index_add(0, rt, xn_q * wr[rt, rk].unsqueeze(1))
    o.backward(dout.to(dt).double())
    tol = dict(rtol=1e-4, atol_scale=5e-6) if dt == torch.float32 else dict(rtol=2e-2, atol_scale=2e-2)
    _close(xg[:total], xn, "xg", **tol)
    _close(out, o, "combine", **tol)
    _close(xd.grad, xr.grad, "dx", **(tol if dt == torch.float32 else dict(rtol=5e-2, atol_scale=3e-2)))
    _close(gd.grad, gr.grad, "dgamma", rtol=1e-3 if dt == torch.float32 else 3e-2, atol_scale=1e-4 if dt == torch.float32 else 2e-2)
    _close(bd.grad, br.grad, "dbeta", rtol=1e-3 if dt == torch.float32 else 3e-2, atol_scale=1e-4 if dt == torch.float32 else 2e-2)
    _close(wd.grad, wr.grad, "dw", rtol=1e-3 if dt == torch.float32 else 3e-2, atol_scale=1e-4 if dt == torch.float32 else 2e-2)


# ------------------------------------------------------------------ grouped GEMM
def _grouped_ref(x, W, b, sizes, act):
    outs, r = [], 0
    for e, m in enumerate(sizes):
        u = x[r:r + m] @ W[e].T + (b[e] if b is not None else 0)
        outs.append(u)
        r += m
    u = torch.cat(outs) if outs else x.new_zeros(0, W.shape[1])
    return {"gelu": F.gelu, "relu": F.relu, "silu": F.silu, None: (lambda t: t)}[act](u)


@pytest.mark.parametrize("sizes,N,K,act", [
    ([5, 0, 300, 129, 128, 1, 77, 64], 64, 32, "gelu"),
    ([200, 333], 136, 100, None),
    ([1000], 704, 260, "silu"),
    ([17, 17, 17, 17], 8, 4, "relu"),
])
def test_grouped_linear_fp32_exact_path(dev, sizes, N, K, act):
    """fp32 operands on v_mfma_f32_16x16x4_f32: an exact fp32 FMA chain -> reference tolerance
    1e-4 rtol (measured ~1e-6)."""
    from apertis_llm_amd import ops
    torch.manual_seed(N + K)
    E, R = len(sizes), sum(sizes)
    pad = 7                                   # rows beyond offsets[E] must stay untouched
    x = torch.randn(R + pad, K)
    W, b = torch.randn(E, N, K) / K ** 0.5, torch.randn(E, N)
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32)
    dout = torch.randn(R + pad, N)
    xd = x.to(dev).requires_grad_(True)
    Wd, bd = W.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    out = ops.grouped_linear(xd, Wd, bd, offsets.to(dev), R + pad, act=act)
    (out[:R] * dout[:R].to(dev)).sum().backward()
    xr, Wr, br = x[:R].double().requires_grad_(True), W.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = _grouped_ref(xr, Wr, br, sizes, act)
    (ref * dout[:R].double()).sum().backward()
    _close(out[:R], ref, "out", rtol=1e-4, atol_scale=1e-5)
    _close(xd.grad[:R], xr.grad, "dx", rtol=1e-4, atol_scale=1e-5)
    _close(Wd.grad, Wr.grad, "dW", rtol=1e-4, atol_scale=1e-5)
    _close(bd.grad, br.grad, "db", rtol=1e-4, atol_scale=1e-5)


@pytest.mark.parametrize("sizes,N,K", [([700, 100, 0, 513], 256, 128), ([640] * 8, 1024, 256), ([300, 5], 704, 2816),
                                        ([3000, 0, 1500, 257, 1, 600], 704, 128), ([4100, 90], 512, 704),
                                        # config 3 (H=256, I=1024) at its bench batch: fc1 and fc2 of the expert MLP
                                        ([10240] * 8, 1024, 256), ([10240] * 8, 256, 1024), ([640] * 8, 256, 1024)])
def test_grouped_linear_bf16_mfma(dev, sizes, N, K):
    """bf16 operands / fp32 accumulate: compare with fp64 math on the SAME bf16-rounded operands;
    only the output rounding (bf16, 2^-8) and fp32 accumulation order differ."""
    from apertis_llm_amd import ops
    torch.manual_seed(N)
    E, R = len(sizes), sum(sizes)
    x = torch.randn(R, K).bfloat16()
    W, b = (torch.randn(E, N, K) / K ** 0.5), torch.randn(E, N)
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32)
    dout = torch.randn(R, N).bfloat16()
    xd = x.to(dev).requires_grad_(True)
    Wd, bd = W.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    out = ops.grouped_linear(xd, Wd, bd, offsets.to(dev), R, act="gelu", compute_dtype=torch.bfloat16)
    assert out.dtype == torch.bfloat16
    out.backward(dout.to(dev))
    Wq = W.bfloat16().double()
    xr, Wr, br = x.double().requires_grad_(True), Wq.requires_grad_(True), b.double().requires_grad_(True)
    ref = _grouped_ref(xr, Wr, br, sizes, "gelu")
    ref.backward(dout.double())
    _close(out, ref, "out", rtol=1e-2, atol_scale=6e-3)
    _close(xd.grad, xr.grad, "dx", rtol=2e-2, atol_scale=1e-2)
    _close(Wd.grad, Wr.grad, "dW", rtol=2e-2, atol_scale=1e-2)
    _close(bd.grad, br.grad, "db", rtol=2e-2, atol_scale=1e-2)


def test_grouped_linear_dropout_mask_consistency(dev):
    from apertis_llm_amd import ops
    torch.manual_seed(0)
    R, N, K, p = 1024, 512, 64, 0.1
    x = torch.randn(R, K, device=dev, requires_grad=True)
    W = torch.randn(1, N, K, device=dev) / 8
    offsets = torch.tensor([0, R], dtype=torch.int32, device=dev)
    full = ops.grouped_linear(x, W, None, offsets, R, act="relu")
    y1 = ops.grouped_linear(x, W, None, offsets, R, act="relu", drop_p=p, seed=1234)
    y1b = ops.grouped_linear(x, W, None, offsets, R, act="relu", drop_p=p, seed=1234)
    y2 = ops.grouped_linear(x, W, None, offsets, R, act="relu", drop_p=p, seed=99)
    assert torch.equal(y1, y1b) and not torch.equal(y1, y2)
    pos = full > 0
    kept = (y1 != 0) & pos
    frac = float(kept.sum()) / float(pos.sum())
    assert abs(frac - (1 - p)) < 0.01, frac
    _close(y1[kept], full[kept] / (1 - p), "kept values scaled")
    # backward uses the same mask: d/dx of sum(y1) equals that of sum(full*mask/(1-p))
    mask = kept.float() / (1 - p)
    g1, = torch.autograd.grad(y1.sum(), x, retain_graph=True)
    g2, = torch.autograd.grad((full * mask).sum(), x)
    _close(g1, g2, "dropout backward", rtol=1e-4, atol_scale=1e-5)


def test_linear_mfma_dense(dev):
    from apertis_llm_amd import ops
    torch.manual_seed(1)
    x, W, b = torch.randn(3, 50, 72), torch.randn(40, 72) / 8, torch.randn(40)
    out = ops.linear_mfma(x.to(dev), W.to(dev), b.to(dev))
    _close(out, F.linear(x.double(), W.double(), b.double()), "dense", rtol=1e-4, atol_scale=1e-5)


@pytest.mark.parametrize("rows,N,K,dt", [(5000, 72, 40, torch.float32), (4608, 352, 704, torch.bfloat16),
                                          # the SSM block's projections incl. K % 32 != 0 (two-per-CU NT kernel, ragged variant)
                                          (4700, 400, 176, torch.bfloat16), (4352, 704, 176, torch.bfloat16),
                                          (4101, 704, 352, torch.bfloat16), (4096, 264, 104, torch.bfloat16),
                                          # the H = 256 family's narrow data gradients (N = 64 through the two-per-CU kernel)
                                          (4352, 64, 256, torch.bfloat16), (4200, 256, 64, torch.bfloat16),
                                          (4608, 192, 64, torch.bfloat16)])
def test_linear_mfma_splitk_wgrad(dev, rows, N, K, dt):
    """Dense layer backward: the weight gradient is a deterministic split-K over row chunks."""
    from apertis_llm_amd import ops
    torch.manual_seed(rows)
    x, W, b = torch.randn(rows, K).to(dt), torch.randn(N, K) / K ** 0.5, torch.randn(N)
    dout = torch.randn(rows, N).to(dt)
    xd, Wd, bd = x.to(dev).requires_grad_(True), W.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    out = ops.linear_mfma(xd, Wd, bd, compute_dtype=dt)
    out.backward(dout.to(dev))
    g1 = Wd.grad.clone()
    Wd.grad = None
    xd.grad = None
    bd.grad = None
    ops.linear_mfma(xd, Wd, bd, compute_dtype=dt).backward(dout.to(dev))
    assert torch.equal(g1, Wd.grad), "split-K fold must be bitwise reproducible"
    Wq = W.to(dt).double()
    xr, Wr, br = x.double().requires_grad_(True), Wq.requires_grad_(True), b.double().requires_grad_(True)
    ref = F.linear(xr, Wr, br)
    ref.backward(dout.double())
    tol = dict(rtol=1e-4, atol_scale=1e-5) if dt == torch.float32 else dict(rtol=2e-2, atol_scale=1e-2)
    _close(out, ref, "out", **tol)
    _close(xd.grad, xr.grad, "dx", **tol)
    _close(Wd.grad, Wr.grad, "dW", **tol)
    _close(bd.grad, br.grad, "db", **tol)


@pytest.mark.parametrize("counts,N,K,act,use_bias", [
    ([1], 352, 704, None, False), ([16], 704, 176, None, False), ([3], 448, 176, None, True),
    ([0, 2, 0, 1, 0, 0, 5, 0], 2816, 704, "gelu", True), ([4, 4, 4, 4, 4, 4, 4, 4], 704, 2816, None, True),
    ([17, 0, 33, 1], 104, 104, "gelu", True), ([7, 9], 40, 40, "relu", False)])
def test_grouped_linear_skinny_rows(dev, counts, N, K, act, use_bias):
    """The decode step's shapes: a handful of rows per call (<= 64 in all) go to the skinny NT kernel - a wave per 16 output
    columns, W straight from global memory into the MFMA operand.  Values against fp64 on the bf16 operands (bf16 rounding of
    the pre-activation and of the output as in the tiled kernels), empty groups, groups of more than 16 rows, widths that are
    not multiples of 16 / 32; rows past the last group untouched."""
    from apertis_llm_amd import ops
    torch.manual_seed(sum(counts) + N)
    E, rows = len(counts), sum(counts)
    offs = torch.tensor([0] + list(torch.tensor(counts).cumsum(0).tolist()), dtype=torch.int32, device=dev)
    x = torch.randn(rows + 3, K).bfloat16()
    W = (torch.randn(E, N, K) / K ** 0.5)
    b = torch.randn(E, N) if use_bias else None
    xd = x.to(dev)
    out = ops.grouped_linear(xd, W.to(dev), None if b is None else b.to(dev), offs, rows, act=act, compute_dtype=torch.bfloat16)
    assert out.shape == (rows + 3, N) or out.shape[0] >= rows
    Wq = W.bfloat16().double()
    r0 = 0
    for e, c in enumerate(counts):
        if c == 0:
            continue
        pre = x[r0:r0 + c].double() @ Wq[e].t() + (b[e].double() if b is not None else 0.0)
        pre = pre.float().bfloat16().double()                     # the activation sees the pre-activation as stored
        ref = {None: pre, "gelu": F.gelu(pre), "relu": F.relu(pre)}[act]
        _close(out[r0:r0 + c], ref, f"group {e}", rtol=2e-2, atol_scale=1e-2)
        r0 += c


@pytest.mark.parametrize("rows,N,K", [(8192, 704, 2816), (9000, 1408, 768), (20000, 352, 704), (4200, 768, 768),
                                      (9000, 448, 896)])     # (the last: 256 x 352 tiles with a ragged edge on both sides)
def test_linear_mfma_wide_dense_wgrad(dev, rows, N, K):
    """A bias-free dense layer with enough output (M * N >= 240 000): its weight gradient goes through apertis_grouped_gemm_tn as ONE group -
    the library splits the rows of its 352-wide tiles over the CUs and folds the slices itself (no pseudo-groups, no
    apertis_colsum_f32 from the caller); values against fp64 on the bf16 operands, bits reproducible."""
    from apertis_llm_amd import ops, _lib
    lib = _lib.load()
    assert lib.apertis_grouped_gemm_tn_dense_variant(N, K) >= 0 and lib.apertis_grouped_gemm_tn_dense_variant(704, 176) < 0
    torch.manual_seed(rows)
    x, W = torch.randn(rows, K).bfloat16(), torch.randn(N, K) / K ** 0.5
    dout = torch.randn(rows, N).bfloat16()
    xd, Wd = x.to(dev), W.to(dev).requires_grad_(True)
    folds = {"n": 0}
    real = lib.apertis_colsum_f32

    def counting(*a):
        folds["n"] += 1
        return real(*a)

    lib.apertis_colsum_f32 = counting
    try:
        ops.linear_mfma(xd, Wd, None, compute_dtype=torch.bfloat16).backward(dout.to(dev))
        g1 = Wd.grad.clone()
        Wd.grad = None
        ops.linear_mfma(xd, Wd, None, compute_dtype=torch.bfloat16).backward(dout.to(dev))
    finally:
        lib.apertis_colsum_f32 = real
    assert folds["n"] == 0, "the wide path folds inside the library"
    assert torch.equal(g1, Wd.grad), "slice fold must be bitwise reproducible"
    ref = dout.double().t() @ x.double()
    _close(Wd.grad, ref, "dW", rtol=1e-4, atol_scale=2e-6)


@pytest.mark.parametrize("T,H,dt_in,dt_out", [(1000, 704, torch.float32, torch.float32), (333, 32, torch.float32, torch.float32),
                                              (4100, 256, torch.float32, torch.bfloat16), (77, 1028, torch.float32, torch.float32)])
def test_layer_norm_kernels(dev, T, H, dt_in, dt_out):
    from apertis_llm_amd import ops
    torch.manual_seed(T)
    x = (torch.randn(T, H) * 3 + 1).to(dt_in)
    w, b = torch.randn(H), torch.randn(H)
    dy = torch.randn(T, H)
    xd, wd, bd = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    y = ops.layer_norm(xd, wd, bd, 1e-12, out_dtype=dt_out)
    assert y.dtype == dt_out
    y.backward(dy.to(dev).to(dt_out))
    xr, wr, br = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = F.layer_norm(xr, (H,), wr, br, 1e-12)
    ref.backward(dy.to(dt_out).double())
    tol = dict(rtol=1e-4, atol_scale=1e-5) if dt_out == torch.float32 else dict(rtol=1e-2, atol_scale=8e-3)
    _close(y, ref, "y", **tol)
    _close(xd.grad, xr.grad, "dx", **tol)
    _close(wd.grad, wr.grad, "dgamma", rtol=1e-3, atol_scale=1e-4 if dt_out == torch.float32 else 1e-2)
    _close(bd.grad, br.grad, "dbeta", rtol=1e-3, atol_scale=1e-4 if dt_out == torch.float32 else 1e-2)


@pytest.mark.parametrize("dt,sizes,H,I", [(torch.float32, [100, 0, 333, 64], 32, 64), (torch.bfloat16, [3000, 1200, 0, 500], 256, 512)])
def test_expert_mlp_fused_backward(dev, dt, sizes, H, I):
    """Expert MLP as one node (dgrad of layer 2 applies act'/dropout of layer 1 in its epilogue)
    against the two-node composition and, without dropout, against plain torch autograd."""
    from apertis_llm_amd import ops
    torch.manual_seed(H)
    E, R = len(sizes), sum(sizes)
    x = torch.randn(R, H).to(dt)
    w1, b1 = torch.randn(E, I, H) / H ** 0.5, torch.randn(E, I) * 0.1
    w2, b2 = torch.randn(E, H, I) / I ** 0.5, torch.randn(E, H) * 0.1
    offs = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=dev)
    dout = torch.randn(R, H).to(dt).to(dev)

    def run(fn, p, seed):
        leaves = [t.to(dev).requires_grad_(True) for t in (x, w1, b1, w2, b2)]
        y = fn(leaves, p, seed)
        y.backward(dout)
        return [y] + [t.grad for t in leaves]
    fused = lambda L, p, seed: ops.expert_mlp(L[0], L[1], L[2], L[3], L[4], offs, R, act="gelu", drop_p=p, seed=seed, compute_dtype=dt)
    two = lambda L, p, seed: ops.grouped_linear(ops.grouped_linear(L[0], L[1], L[2], offs, R, act="gelu", drop_p=p, seed=seed,
                                                                    compute_dtype=dt), L[3], L[4], offs, R, compute_dtype=dt)
    tol = dict(rtol=1e-4, atol_scale=1e-5) if dt == torch.float32 else dict(rtol=3e-2, atol_scale=2e-2)
    fuse_default = ops.FUSE_ACT_BWD
    for p_drop, fuse in ((0.0, False), (0.25, False), (0.25, True)):
        ops.FUSE_ACT_BWD = fuse
        try:
            a, b = run(fused, p_drop, 77), run(two, p_drop, 77)
        finally:
            ops.FUSE_ACT_BWD = fuse_default     # (was left False for the rest of the process until round 3)
        for u, v, n in zip(a, b, ["y", "dx", "dw1", "db1", "dw2", "db2"]):
            _close(u, v, f"fused vs two-node {n} (p={p_drop})", **tol)
    # plain torch reference (no dropout)
    xr = x.double().requires_grad_(True)
    W1, B1, W2, B2 = [t.to(dt).double().requires_grad_(True) if t.dim() == 3 else t.double().requires_grad_(True)
                      for t in (w1, b1, w2, b2)]
    hmid = _grouped_ref(xr, W1, B1, sizes, "gelu")
    if dt == torch.bfloat16:
        hmid = hmid + (hmid.detach().to(dt).double() - hmid.detach())
    yref = _grouped_ref(hmid, W2, B2, sizes, None)
    yref.backward(dout.cpu().double())
    a = run(fused, 0.0, 0)
    for u, v, n in zip(a, [yref, xr.grad, W1.grad, B1.grad, W2.grad, B2.grad], ["y", "dx", "dw1", "db1", "dw2", "db2"]):
        _close(u, v, f"fused vs torch {n}", **(tol if dt == torch.float32 else dict(rtol=5e-2, atol_scale=3e-2)))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_dropout_add(dev, dt):
    from apertis_llm_amd import ops
    torch.manual_seed(0)
    x = torch.randn(1000, 704, device=dev).to(dt).requires_grad_(True)
    res = torch.randn(1000, 704, device=dev, requires_grad=True)
    y0 = ops.dropout_add(x, res, 0.1, training=False)
    _close(y0, (res.float() + x.float()).cpu(), "eval = plain add", rtol=1e-6)
    torch.manual_seed(5)
    y = ops.dropout_add(x, res, 0.1, training=True)
    d = (y - res).detach()
    kept = d != 0
    frac = float(kept.float().mean())
    assert abs(frac - 0.9) < 0.01, frac
    _close(d[kept], (x.detach().float() / 0.9)[kept].cpu(), "kept values scaled", rtol=1e-5)
    g = torch.randn_like(y)
    y.backward(g)
    assert torch.equal(res.grad, g)
    _close(x.grad.float(), (g * kept.float() / 0.9).to(dt).float().cpu(), "dx uses the same mask", rtol=1e-5)


@pytest.mark.parametrize("T,K,N,dt", [(1000, 704, 8, torch.bfloat16), (333, 32, 4, torch.float32), (4097, 256, 16, torch.float32),
                                      (50, 1024, 2, torch.float32)])
def test_skinny_linear(dev, T, K, N, dt):
    from apertis_llm_amd import ops
    torch.manual_seed(T)
    x, W, b = torch.randn(T, K).to(dt), torch.randn(N, K) / K ** 0.5, torch.randn(N)
    dy = torch.randn(T, N)
    xd, Wd, bd = x.to(dev).requires_grad_(True), W.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    y = ops.skinny_linear(xd, Wd, bd)
    assert y.dtype == torch.float32
    y.backward(dy.to(dev))
    xr, Wr, br = x.double().requires_grad_(True), W.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = F.linear(xr, Wr, br)
    ref.backward(dy.double())
    _close(y, ref, "y", rtol=1e-4, atol_scale=1e-5)
    _close(xd.grad, xr.grad, "dx", **(dict(rtol=1e-4, atol_scale=1e-5) if dt == torch.float32 else dict(rtol=1e-2, atol_scale=8e-3)))
    _close(Wd.grad, Wr.grad, "dW", rtol=1e-4, atol_scale=1e-5)
    _close(bd.grad, br.grad, "db", rtol=1e-4, atol_scale=1e-5)


# ------------------------------------------------------------------ weight-gradient GEMM (TN) through the C ABI
def _tn_call(dev, A, Bm, offsets, E, with_bias, ws_mode, R=None):
    from apertis_llm_amd import _lib
    lib = _lib.load()
    R, M = A.shape[0] if R is None else R, A.shape[1]
    N = Bm.shape[1]
    dW = torch.full((E, M, N), float("nan"), device=dev)
    db = torch.full((E, M), float("nan"), device=dev) if with_bias else None
    nbytes = lib.apertis_grouped_gemm_tn_workspace_bytes(E, 1)
    ws = torch.empty(max(nbytes, 16), device=dev, dtype=torch.uint8) if ws_mode else None
    # a workspace selects the 256x256-tile kernel, also for groups a caller would normally call too short for it
    # ws_mode == "queue": the same kernel taking its tiles from the per-group item counters (what the data-parallel step uses)
    rc = lib.apertis_grouped_gemm_tn_q(_lib.ptr(A), _lib.ptr(Bm), _lib.ptr(offsets), _lib.ptr(dW), _lib.ptr(db), R, M, N, E,
                                       _lib.ptr(ws), nbytes if ws_mode else 0, _lib.BF16, int(ws_mode == "queue"),
                                       _lib.stream_ptr())
    assert rc == 0, _lib.load().apertis_strerror(rc)
    torch.cuda.synchronize()
    return dW, db


@pytest.mark.parametrize("sizes,M,N", [
    ([700, 100, 0, 513], 256, 128),          # empty group, one tile per group -> every tile is row-split 64 ways
    ([4000, 3000, 5000, 2000, 1, 63, 64, 65], 704, 2816),   # the expert shapes: 33 tiles on 32 CUs, one split 32 ways
    ([9000], 352, 704),                       # dense split-K (E = 1), ragged last m-tile
    ([300, 5], 8, 520),                       # tiny M, N not a multiple of 256
    ([0, 0, 0], 64, 64),                      # nothing to sum: zeros
])
@pytest.mark.parametrize("with_bias", [False, True])
def test_grouped_gemm_tn_bf16(dev, sizes, M, N, with_bias):
    """dW[e] = A[rows_e]^T @ B[rows_e], dbias[e] = column sums of A[rows_e]; the 256x256-tile kernel
    (with workspace) and the 128x128-tile kernel (without) against an fp64 product of the same bf16 values."""
    torch.manual_seed(len(sizes) * 1000 + M + N)
    E, R = len(sizes), sum(sizes)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), device=dev)
    A = torch.randn(R + 7, M, device=dev).bfloat16()      # rows past the last group exist but are never read
    Bm = torch.randn(R + 7, N, device=dev).bfloat16()
    ref_w = torch.zeros(E, M, N, dtype=torch.float64)
    ref_b = torch.zeros(E, M, dtype=torch.float64)
    Ac, Bc = A.double().cpu(), Bm.double().cpu()
    for e in range(E):
        r0, r1 = int(offs[e]), int(offs[e + 1])
        ref_w[e] = Ac[r0:r1].T @ Bc[r0:r1]
        ref_b[e] = Ac[r0:r1].sum(0)
    scale = max(1.0, float(max(sizes)) ** 0.5)
    static = None
    for ws_mode in (True, "queue", False):
        dW, db = _tn_call(dev, A, Bm, offs, E, with_bias, ws_mode, R=R)
        assert torch.isfinite(dW).all(), "every output element must be written"
        if ws_mode is True:
            static = (dW, db)
        elif ws_mode == "queue":     # who computes a tile changes nothing: bit-identical to the static walk
            assert torch.equal(dW, static[0]) and (db is None or torch.equal(db, static[1]))
        err = (dW.double().cpu() - ref_w).abs().max().item()
        assert err <= 2e-5 * scale * 8, f"ws={ws_mode}: max abs err {err:.3e}"   # fp32 accumulation of exact bf16 products
        if with_bias:
            assert torch.isfinite(db).all()
            errb = (db.double().cpu() - ref_b).abs().max().item()
            assert errb <= 2e-5 * scale * 8, f"ws={ws_mode}: bias max abs err {errb:.3e}"


@pytest.mark.parametrize("sizes,N,K", [([9000, 4100, 0, 7000, 12000, 300, 5000, 8000], 704, 2816), ([70000], 704, 352),
                                        ([5000] * 8, 2816, 704)])
def test_grouped_gemm_nt_tile_queue_equals_static_walk(dev, sizes, N, K):
    """apertis_grouped_gemm_nt_q (per-XCD tile counters with stealing, what the data-parallel step uses) against
    apertis_grouped_gemm_nt through the C ABI: which work-group computes a tile changes nothing - bit-identical, every
    tile computed exactly once (NaN-prefilled output), twice in a row on the same queue buffer."""
    from apertis_llm_amd import _lib
    lib = _lib.load()
    torch.manual_seed(N + K)
    E, R = len(sizes), sum(sizes)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), device=dev)
    A = torch.randn(R, K, device=dev).bfloat16()
    W = (torch.randn(E, N, K, device=dev) / K ** 0.5).bfloat16()
    queue = torch.full((512,), 12345, device=dev, dtype=torch.int32)      # dirty on purpose: the entry point zeroes it

    def run(q):
        C = torch.full((R, N), float("nan"), device=dev, dtype=torch.bfloat16)
        if q is None:
            rc = lib.apertis_grouped_gemm_nt(_lib.ptr(A), _lib.ptr(W), None, _lib.ptr(offs), _lib.ptr(C), None, None, R, N, K, K, E,
                                             _lib.ACT_NONE, 0.0, 0, _lib.BF16, _lib.BF16, _lib.stream_ptr())
        else:
            rc = lib.apertis_grouped_gemm_nt_q(_lib.ptr(A), _lib.ptr(W), None, _lib.ptr(offs), _lib.ptr(C), None, None, R, N, K, K, E,
                                               _lib.ACT_NONE, 0.0, 0, _lib.BF16, _lib.BF16, _lib.ptr(q), _lib.stream_ptr())
        assert rc == 0
        torch.cuda.synchronize()
        return C

    ref = run(None)
    assert torch.isfinite(ref.float()).all()
    for _ in range(2):
        got = run(queue)
        assert torch.equal(got, ref)


@pytest.mark.parametrize("sizes,N,K,with_bias", [([9000, 4100, 0, 7000, 300, 257, 1, 5000], 704, 2816, True), ([4000, 3000], 352, 1088, False),
                                                  ([4096], 1056, 2048, True), ([6000, 255, 256], 704, 128, False)])
def test_grouped_gemm_nt_352_wide_tile(dev, sizes, N, K, with_bias):
    """Outputs a multiple of 352 wide with a plain epilogue run on the persistent 256 x 352 tile (grouped_gemm_nt352p_k: fc2 forward
    and the fc1 data gradient of the H = 704 family): against fp64 math on the same bf16 operands, ragged / empty / one-row groups,
    every output element written exactly once (NaN prefill), static walk and tile queue bit-identical."""
    from apertis_llm_amd import _lib
    lib = _lib.load()
    torch.manual_seed(N + K)
    E, R = len(sizes), sum(sizes)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), device=dev)
    A = torch.randn(R, K, device=dev).bfloat16()
    W = (torch.randn(E, N, K, device=dev) / K ** 0.5).bfloat16()
    b = torch.randn(E, N, device=dev) if with_bias else None
    queue = torch.zeros(512, device=dev, dtype=torch.int32)
    outs = []
    for q in (None, queue):
        C = torch.full((R, N), float("nan"), device=dev, dtype=torch.bfloat16)
        args = (_lib.ptr(A), _lib.ptr(W), _lib.ptr(b) if with_bias else None, _lib.ptr(offs), _lib.ptr(C), None, None, R, N, K, K, E,
                _lib.ACT_NONE, 0.0, 0, _lib.BF16, _lib.BF16)
        rc = lib.apertis_grouped_gemm_nt(*args, _lib.stream_ptr()) if q is None else lib.apertis_grouped_gemm_nt_q(*args, _lib.ptr(q), _lib.stream_ptr())
        assert rc == 0
        torch.cuda.synchronize()
        outs.append(C)
    assert torch.equal(outs[0], outs[1])
    ref = torch.empty(R, N, dtype=torch.float64)
    Ad, Wd = A.double().cpu(), W.double().cpu()
    for e in range(E):
        r0, r1 = int(offs[e]), int(offs[e + 1])
        ref[r0:r1] = Ad[r0:r1] @ Wd[e].T + (b[e].double().cpu() if with_bias else 0.0)
    _close(outs[0], ref, "out", rtol=1e-2, atol_scale=6e-3)


def test_grouped_gemm_tn_is_deterministic(dev):
    torch.manual_seed(5)
    sizes = [4000, 3000, 5000, 2000]
    offs = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), device=dev)
    A = torch.randn(sum(sizes), 704, device=dev).bfloat16()
    Bm = torch.randn(sum(sizes), 512, device=dev).bfloat16()
    first = _tn_call(dev, A, Bm, offs, 4, True, True)
    for mode in (True, True, "queue", "queue"):
        again = _tn_call(dev, A, Bm, offs, 4, True, mode)
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


@pytest.mark.parametrize("T,H,dt_in,dt_out", [(1000, 704, torch.float32, torch.bfloat16), (77, 32, torch.float32, torch.float32),
                                               (513, 256, torch.bfloat16, torch.bfloat16)])
def test_layer_norm_pass_folds_residual_gradient(dev, T, H, dt_in, dt_out):
    """(LN(x), x) = ops.layer_norm_pass(x): the gradient arriving on the pass-through is added inside the
    LayerNorm backward kernel; same numbers as autograd's separate add."""
    from apertis_llm_amd import ops
    torch.manual_seed(T + H)
    x = torch.randn(T, H).to(dt_in)
    w, b = torch.randn(H) * 0.2 + 1, torch.randn(H) * 0.1
    gy, gp = torch.randn(T, H).to(dt_out).float(), torch.randn(T, H).to(dt_in).float()   # exactly representable upstream grads
    xr = x.float().clone().requires_grad_(True)
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    (F.layer_norm(xr, (H,), wr, br, 1e-5) * gy).sum().backward()
    ref_dx = xr.grad + gp
    xd = x.to(dev).requires_grad_(True)
    wd, bd = w.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    y, xp = ops.layer_norm_pass(xd, wd, bd, 1e-5, out_dtype=dt_out)
    assert xp.data_ptr() == xd.data_ptr() and y.dtype == dt_out
    ((y.float() * gy.to(dev)).sum() + (xp.float() * gp.to(dev)).sum()).backward()
    tol = 2e-5 if dt_in == torch.float32 else 3e-2
    assert torch.allclose(xd.grad.float().cpu(), ref_dx, rtol=tol, atol=tol * float(ref_dx.abs().max()))
    assert torch.allclose(wd.grad.cpu(), wr.grad, rtol=1e-4, atol=1e-4 * T ** 0.5)
    # only the pass-through used: the gradient is handed on untouched
    xd2 = x.to(dev).requires_grad_(True)
    _, xp2 = ops.layer_norm_pass(xd2, wd, bd, 1e-5, out_dtype=dt_out)
    (xp2.float() * gp.to(dev)).sum().backward()
    assert torch.allclose(xd2.grad.float().cpu(), gp.to(dt_in).float(), rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("T,H,N,dt", [(1000, 704, 8, torch.float32), (333, 32, 4, torch.float32), (4097, 256, 2, torch.bfloat16),
                                       (5000, 704, 8, torch.bfloat16), (1, 1024, 8, torch.float32)])
def test_router_ln_linear(dev, T, H, N, dt):
    """Fused router: logits = Linear(LayerNorm(x)) (core.py:481-482) and its backward with the pass-through
    gradient folded in, against the two stock torch ops in fp32."""
    from apertis_llm_amd import ops
    torch.manual_seed(T + H + N)
    x = (torch.randn(T, H) * 2 + 0.3).to(dt)
    lw, lb = torch.randn(H) * 0.2 + 1, torch.randn(H) * 0.1
    W, b = torch.randn(N, H) * 0.05, torch.randn(N) * 0.1
    gl, gp = torch.randn(T, N), torch.randn(T, H).to(dt).float()
    ref = [t.clone().requires_grad_(True) for t in (x.float(), lw, lb, W, b)]
    ref_logits = F.linear(F.layer_norm(ref[0], (H,), ref[1], ref[2], 1e-5), ref[3], ref[4])
    ((ref_logits * gl).sum() + (ref[0] * gp).sum()).backward()
    dv = [t.to(dev).requires_grad_(True) for t in (x, lw, lb, W, b)]
    assert ops.router_ln_linear_supported(dv[0], H, N)
    logits, xp = ops.router_ln_linear(dv[0], dv[1], dv[2], 1e-5, dv[3], dv[4])
    assert logits.dtype == torch.float32 and xp.data_ptr() == dv[0].data_ptr()
    ((logits * gl.to(dev)).sum() + (xp.float() * gp.to(dev)).sum()).backward()
    _close(logits, ref_logits, "logits", rtol=1e-4, atol_scale=1e-5)
    rt = 1e-4 if dt == torch.float32 else 2e-2
    _close(dv[0].grad.float(), ref[0].grad, "dx", rtol=rt, atol_scale=1e-5 if dt == torch.float32 else 1e-2)
    for i, name in ((1, "dgamma"), (2, "dbeta"), (3, "dW"), (4, "db")):
        _close(dv[i].grad, ref[i].grad, name, rtol=2e-4, atol_scale=2e-5)


@pytest.mark.parametrize("S,E,K", [(1000, 8, 2), (77, 4, 1), (4097, 16, 3), (300, 5, 2)])
def test_gate_topk_aux_losses(dev, S, E, K):
    """Gate + load-balancing + router-z losses in one pass vs the reference formulas (core.py:491-505,524-529)
    written with stock torch ops on the CPU; indices exact, losses and dlogits to fp32 rounding."""
    from apertis_llm_amd import ops
    torch.manual_seed(S * 7 + E)
    logits = torch.randn(S, E) * 2
    lb_coef, rz_coef = 0.01, 0.001
    gw = torch.randn(S, K)
    lo = logits.clone().requires_grad_(True)
    gates = torch.softmax(lo, dim=-1)
    p, idx_ref = torch.topk(gates, K, dim=-1)
    w_ref = p / (p.sum(-1, keepdim=True) + 1e-6)
    frac = torch.zeros(E).index_add_(0, idx_ref.reshape(-1), torch.ones(S * K)) / S
    lb_ref = lb_coef * E * torch.sum(frac * gates.mean(dim=0))
    rz_ref = rz_coef * torch.mean(torch.logsumexp(lo, dim=-1) ** 2)
    ((w_ref * gw).sum() + 3.0 * lb_ref + 0.5 * rz_ref).backward()
    ld = logits.to(dev).requires_grad_(True)
    idx, w, lb, rz = ops.moe_gate_topk_aux(ld, K, lb_coef, rz_coef)
    ((w * gw.to(dev)).sum() + 3.0 * lb + 0.5 * rz).backward()
    assert torch.equal(idx.cpu().long(), idx_ref)
    _close(w, w_ref, "w", rtol=1e-5)
    assert abs(float(lb) - float(lb_ref)) <= 1e-5 * abs(float(lb_ref)) and abs(float(rz) - float(rz_ref)) <= 1e-5 * abs(float(rz_ref))
    # K == 1: w = p / (p + 1e-6) is flat, its two gradient terms cancel to ~1e-4 of their size -> absolute floor
    assert torch.allclose(ld.grad.cpu(), lo.grad, rtol=1e-4, atol=3e-7), float((ld.grad.cpu() - lo.grad).abs().max())


@pytest.mark.parametrize("act,p", [("gelu", 0.1), ("gelu", 0.0)])
def test_expert_mlp_saved_activation_gradient(dev, act, p):
    """Expert MLP whose forward leaves g' = act'(pre) * keep / (1-p) for the backward (APERTIS_ACT_SAVE_GRAD /
    APERTIS_ACT_MUL_SAVED) against the form that keeps the pre-activation: the same output bits (same mask: both forward
    outputs come from one evaluation and one hash), gradients equal to bf16 rounding of g', and both against fp64 math on the same mask."""
    from apertis_llm_amd import _lib, ops
    torch.manual_seed(7)
    sizes = [3000, 2000, 1500, 1692]
    E, R, H, I = len(sizes), sum(sizes), 128, 512
    assert _lib.load().apertis_grouped_gemm_nt_saves_grad(R, I, H, H, E, _lib.ACT_GELU, _lib.BF16, _lib.BF16) == 1
    x = torch.randn(R, H).bfloat16()
    w1, b1 = torch.randn(E, I, H) / H ** 0.5, torch.randn(E, I) * 0.1
    w2, b2 = torch.randn(E, H, I) / I ** 0.5, torch.randn(E, H) * 0.1
    offs = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), device=dev)
    dy = torch.randn(R, H).bfloat16()

    def run(saved):
        ops.SAVE_ACT_GRAD = saved
        try:
            L = [t.to(dev).requires_grad_(True) for t in (x, w1, b1, w2, b2)]
            yr = ops.expert_mlp(L[0], L[1], L[2], L[3], L[4], offs, R, act=act, drop_p=p, seed=4242, compute_dtype=torch.bfloat16)
            yr.backward(dy.to(dev))
            torch.cuda.synchronize()
            return yr.detach(), [t.grad for t in L]
        finally:
            ops.SAVE_ACT_GRAD = True

    y0, g0 = run(False)
    y1, g1 = run(True)
    assert torch.equal(y0, y1)
    for name, a, c in zip(("dx", "dw1", "db1", "dw2", "db2"), g0, g1):
        a, c = a.float(), c.float()
        assert torch.allclose(a, c, rtol=3e-2, atol=1e-2 * float(a.abs().max())), (name, float((a - c).abs().max()), float(a.abs().max()))
    assert torch.equal(g0[3], g1[3]) and torch.equal(g0[4], g1[4])      # layer 2's gradients do not see the difference


@pytest.mark.parametrize("T,H,E,dt_blk,p", [(3001, 704, 8, torch.bfloat16, 0.1), (513, 256, 4, torch.float32, 0.0)])
def test_boundary_with_router_logits_in_one_pass(dev, T, H, E, dt_blk, p):
    """ops.dropout_add_layer_norm_router = dropout_add_layer_norm followed by router_ln_linear on its normalised output, as one
    forward kernel (the backward is the two existing kernels in sequence): outputs bit-identical, gradients equal."""
    from apertis_llm_amd import ops
    torch.manual_seed(T + H)
    blk, res = torch.randn(T, H).to(dt_blk), torch.randn(T, H)
    w, b = torch.randn(H) * 0.2 + 1, torch.randn(H) * 0.1
    rw, rb = torch.randn(H) * 0.2 + 1, torch.randn(H) * 0.1
    W, wb = torch.randn(E, H) / H ** 0.5, torch.randn(E) * 0.1
    gy, gx, gl = torch.randn(T, H), torch.randn(T, H).to(dt_blk), torch.randn(T, E)
    seed_state = torch.get_rng_state()

    def run(fused):
        torch.set_rng_state(seed_state)                # the same dropout seed is drawn on both paths
        L = [t.to(dev).requires_grad_(True) for t in (blk, res, w, b, rw, rb, W, wb)]
        if fused:
            y, xn, logits = ops.dropout_add_layer_norm_router(L[0], L[1], L[2], L[3], 1e-5, p, True, L[4], L[5], 1e-5, L[6], L[7],
                                                              out_dtype=dt_blk)
        else:
            y, xn = ops.dropout_add_layer_norm(L[0], L[1], L[2], L[3], 1e-5, p, True, out_dtype=dt_blk)
            logits, xn = ops.router_ln_linear(xn, L[4], L[5], 1e-5, L[6], L[7])
        ((y * gy.to(dev)).sum() + (xn.float() * gx.to(dev).float()).sum() + (logits * gl.to(dev)).sum()).backward()
        torch.cuda.synchronize()
        return (y, xn, logits), [t.grad for t in L]

    (y0, x0, l0), g0 = run(False)
    (y1, x1, l1), g1 = run(True)
    assert torch.equal(y0, y1) and torch.equal(x0, x1) and torch.equal(l0, l1)
    for name, a, c in zip(("dblk", "dres", "dw", "db", "drw", "drb", "dW", "dwb"), g0, g1):
        assert torch.equal(a, c), (name, float((a.float() - c.float()).abs().max()))


@pytest.mark.parametrize("T,H,E,K,dt,p,with_gather", [(3001, 704, 8, 2, torch.bfloat16, 0.1, True), (2048, 256, 8, 2, torch.bfloat16, 0.0, True),
                                                      (777, 1024, 4, 1, torch.bfloat16, 0.1, True), (513, 256, 4, 2, torch.float32, 0.1, True),
                                                      (1000, 704, 8, 2, torch.bfloat16, 0.1, False)])
def test_boundary_and_router_backward_in_one_pass(dev, T, H, E, K, dt, p, with_gather):
    """apertis_boundary_router_bwd (the router's dx half + the boundary norm's backward in one pass over the rows, xn's
    gradient never in HBM) against the two calls: the residual stream's and the block output's gradients bit-identical, the
    router's dW / db bit-identical (the same second launch), the four norm-affine gradients equal to summation order."""
    from apertis_llm_amd import ops
    torch.manual_seed(T + H)
    blk, res = torch.randn(T, H).to(dt), torch.randn(T, H)
    w, b = torch.randn(H) * 0.2 + 1, torch.randn(H) * 0.1
    rw, rb = torch.randn(H) * 0.2 + 1, torch.randn(H) * 0.1
    W, wb = torch.randn(E, H) / H ** 0.5, torch.randn(E) * 0.1
    eg, eb = torch.randn(E, H) * 0.2 + 1, torch.randn(E, H) * 0.1
    gy, gl, G = torch.randn(T, H), torch.randn(T, E), torch.randn(T * K, H).to(dt)
    seed_state = torch.get_rng_state()

    def run(fused):
        ops.FUSE_ROUTER_BOUNDARY_BWD = fused
        try:
            torch.set_rng_state(seed_state)
            L = [t.to(dev).requires_grad_(True) for t in (blk, res, w, b, rw, rb, W, wb, eg, eb)]
            y, xn, logits = ops.dropout_add_layer_norm_router(L[0], L[1], L[2], L[3], 1e-5, p, True, L[4], L[5], 1e-5, L[6], L[7], out_dtype=dt)
            loss = (y * gy.to(dev)).sum() + (logits * gl.to(dev)).sum()
            if with_gather:
                idx, wk, _, _ = ops.moe_gate_topk_aux(logits.detach(), K, 0.01, 0.001)
                plan = ops.moe_plan(idx, wk, E, capacity=int(T * K / E * 1.25))
                xg = ops.moe_gather_ln(xn, L[8], L[9], plan, 1e-12, out_dtype=dt)
                loss = loss + (xg.float() * G.to(dev)[:xg.shape[0]].float()).sum()
            loss.backward()
            torch.cuda.synchronize()
            return [t.grad.clone() for t in L[:8]]
        finally:
            ops.FUSE_ROUTER_BOUNDARY_BWD = True

    two = run(False)
    n0 = ops.FUSED_ROUTER_BWD_CALLS
    one = run(True)
    assert ops.FUSED_ROUTER_BWD_CALLS == n0 + 1
    for name, a, c in zip(("dblk", "dres", "dw", "db", "drw", "drb", "dW", "dwb"), two, one):
        if name in ("dblk", "dres", "dW", "dwb"):
            assert torch.equal(a, c), (name, float((a.float() - c.float()).abs().max()))
        else:
            assert torch.allclose(a, c, rtol=2e-5, atol=2e-5 * float(a.abs().max())), (name, float((a - c).abs().max()), float(a.abs().max()))


@pytest.mark.parametrize("dt,extra_consumer", [(torch.bfloat16, False), (torch.float32, False), (torch.bfloat16, True)])
def test_gather_gradient_reaches_the_router_as_rows(dev, dt, extra_consumer):
    """The gather-LN backward hands its gradient to the router backward as rows + slot table (ops._RowsGrad) instead of a
    dense [S, H] tensor: every gradient is bit-identical to the dense hand-over, also when the pass-through has a second
    consumer (its gradient then arrives as an ordinary dense term on top of the rows)."""
    from apertis_llm_amd import ops
    torch.manual_seed(11)
    S, H, E, K = 3000, 704, 8, 2
    x0 = torch.randn(S, H).to(dt)
    lnw, lnb = torch.randn(H) * 0.2 + 1, torch.randn(H) * 0.1
    W, b = torch.randn(E, H) / H ** 0.5, torch.randn(E) * 0.1
    eg, eb = torch.randn(E, H) * 0.2 + 1, torch.randn(E, H) * 0.1
    G = torch.randn(S * K, H).to(dt)
    GL, G2 = torch.randn(S, E), torch.randn(S, H).to(dt)

    def run(rows):
        ops.ROWS_GRADIENT = rows
        try:
            L = [t.to(dev).requires_grad_(True) for t in (x0, lnw, lnb, W, b, eg, eb)]
            logits, xp = ops.router_ln_linear(L[0], L[1], L[2], 1e-5, L[3], L[4])
            idx, w, _, _ = ops.moe_gate_topk_aux(logits.detach(), K, 0.01, 0.001)
            plan = ops.moe_plan(idx, w, E, capacity=int(S / E * 1.25))
            xg = ops.moe_gather_ln(xp, L[5], L[6], plan, 1e-12, out_dtype=dt)
            loss = (xg.float() * G.to(dev)[:xg.shape[0]].float()).sum() + (logits * GL.to(dev)).sum()
            if extra_consumer:
                loss = loss + (xp.float() * G2.to(dev).float()).sum()
            loss.backward()
            torch.cuda.synchronize()
            return [t.grad.clone() for t in L]
        finally:
            ops.ROWS_GRADIENT = True

    dense, rows = run(False), run(True)
    for name, a, c in zip(("dx", "dln_w", "dln_b", "dW", "db", "dexp_g", "dexp_b"), dense, rows):
        if name.startswith("dexp"):   # the gather-LN affine gradients use float atomics in the blocks that straddle an expert
            assert torch.allclose(a, c, rtol=1e-5, atol=1e-5 * float(a.abs().max())), name   # boundary: last-bit run-to-run noise
        elif extra_consumer:          # dense: round(round(sum rows) + g2) by autograd's add; rows: both terms added in fp32
            assert torch.allclose(a.float(), c.float(), rtol=2e-2, atol=2e-2 * float(a.float().abs().max())), name
        else:
            assert torch.equal(a, c), (name, float((a.float() - c.float()).abs().max()))


@pytest.mark.parametrize("S,E,K", [(40000, 8, 2), (5001, 5, 1)])
def test_gate_topk_noisy_routing_in_kernel(dev, S, E, K):
    """Noisy top-k routing inside the gate kernels (reference core.py:485-488: logits += randn * softplus(w_noise) * alpha).
    The kernel's normals are recovered from its own outputs (noisy logits = log(gates) + lse), checked for their
    statistics, and then the reference formulas are run on exactly that noise: indices equal, losses 1e-5, dlogits and the
    gradient of w_noise against autograd; same seed -> same draw, the backward regenerates it."""
    from apertis_llm_amd import _lib, ops
    lib = _lib.load()
    torch.manual_seed(S + E)
    logits = (torch.randn(S, E) * 2).to(dev)
    w_noise = (torch.randn(E) * 0.5).to(dev)
    alpha, seed, lb_coef, rz_coef = 0.7, 987654321, 0.01, 0.001
    gates = torch.empty(S, E, device=dev)
    idx = torch.empty(S, K, device=dev, dtype=torch.int32)
    w = torch.empty(S, K, device=dev)
    lse = torch.empty(S, device=dev)
    part = torch.empty(lib.apertis_moe_gate_aux_blocks(S), 2 * E + 1, device=dev)
    stats = torch.empty(2 + E, device=dev)
    rc = lib.apertis_moe_gate_topk_noisy_aux_fwd(_lib.ptr(logits), _lib.ptr(w_noise), alpha, seed, _lib.ptr(gates), _lib.ptr(idx),
                                                 _lib.ptr(w), _lib.ptr(lse), _lib.ptr(part), _lib.ptr(stats), S, E, K, lb_coef,
                                                 rz_coef, _lib.stream_ptr())
    assert rc == 0
    scale = (F.softplus(w_noise) * alpha).double()
    n = ((gates.double().log() + lse.double()[:, None] - logits.double()) / scale).cpu()      # the kernel's draw
    assert abs(float(n.mean())) < 0.02 and abs(float(n.std()) - 1.0) < 0.02, (float(n.mean()), float(n.std()))
    assert abs(float((n.abs() > 2).double().mean()) - 0.0455) < 0.006          # tails of a normal
    c = torch.corrcoef(n.T)
    assert float((c - torch.eye(E, dtype=c.dtype)).abs().max()) < 0.03         # experts (also the two of a Box-Muller pair) uncorrelated
    assert abs(float((n[1:, 0] * n[:-1, 0]).mean())) < 0.03                    # ... and neighbouring tokens

    # the reference formulas on that noise (float64 noise constants, fp32 math as the reference runs it)
    gw = torch.randn(S, K)
    lo = logits.cpu().clone().requires_grad_(True)
    wn = w_noise.cpu().clone().requires_grad_(True)
    noisy = lo + n.float() * (F.softplus(wn) * alpha)
    g_ref = torch.softmax(noisy, dim=-1)
    pr, idx_ref = torch.topk(g_ref, K, dim=-1)
    w_ref = pr / (pr.sum(-1, keepdim=True) + 1e-6)
    frac = torch.zeros(E).index_add_(0, idx_ref.reshape(-1), torch.ones(S * K)) / S
    lb_ref = lb_coef * E * torch.sum(frac * g_ref.mean(dim=0))
    rz_ref = rz_coef * torch.mean(torch.logsumexp(noisy, dim=-1) ** 2)
    ((w_ref * gw).sum() + 3.0 * lb_ref + 0.5 * rz_ref).backward()

    ld, wd = logits.clone().requires_grad_(True), w_noise.clone().requires_grad_(True)
    idx2, w2, lb, rz = ops.moe_gate_topk_aux(ld, K, lb_coef, rz_coef, wd, alpha, seed)
    ((w2 * gw.to(dev)).sum() + 3.0 * lb + 0.5 * rz).backward()
    assert torch.equal(idx2, idx) and torch.equal(w2, w)                       # same seed, same draw
    same = (idx2.cpu().long() == idx_ref).all(dim=-1)
    assert float(same.double().mean()) > 0.9995                                # (ties of the reconstructed noise aside)
    _close(w2[same.to(dev)], w_ref[same], "w", rtol=2e-4, atol_scale=1e-5)
    assert abs(float(lb) - float(lb_ref)) <= 1e-4 * abs(float(lb_ref)) and abs(float(rz) - float(rz_ref)) <= 1e-4 * abs(float(rz_ref))
    dl, dl_ref = ld.grad.cpu()[same], lo.grad[same]
    assert torch.allclose(dl, dl_ref, rtol=2e-3, atol=2e-6), float((dl - dl_ref).abs().max())
    # (K == 1: w = p / (p + 1e-6) is flat, the gradient through it cancels to ~1e-4 of its terms -> absolute floor)
    gerr = (wd.grad.cpu() - wn.grad).abs()
    assert bool((gerr <= 5e-3 * wn.grad.abs() + (5e-6 if K == 1 else 1e-4 * float(wn.grad.abs().max()))).all()), (wd.grad.cpu(), wn.grad)
    idx3, w3, _, _ = ops.moe_gate_topk_aux(logits, K, lb_coef, rz_coef, w_noise, alpha, seed + 1)
    assert not torch.equal(w3, w)                                              # another seed, another draw
    idx0, _, _, _ = ops.moe_gate_topk_aux(logits, K, lb_coef, rz_coef)         # no w_noise: no noise
    assert float((idx0.long() == torch.topk(torch.softmax(logits, dim=-1), K, dim=-1)[1]).double().mean()) > 0.9999


@pytest.mark.parametrize("T,H,dt_res,dt_blk,p", [(1000, 704, torch.float32, torch.bfloat16, 0.1), (333, 32, torch.float32, torch.float32, 0.0),
                                                  (513, 256, torch.float32, torch.float32, 0.25), (77, 64, torch.bfloat16, torch.bfloat16, 0.1)])
def test_dropout_add_layer_norm_boundary(dev, T, H, dt_res, dt_blk, p):
    """(res + dropout(blk), LayerNorm(that)) as one node vs the two ops it fuses (same seed => same mask):
    forward bit-identical, backward to rounding; both gradients (residual path and block output) checked."""
    from apertis_llm_amd import ops
    torch.manual_seed(T + H)
    blk, res = torch.randn(T, H).to(dt_blk), torch.randn(T, H).to(dt_res)
    w, b = torch.randn(H) * 0.2 + 1, torch.randn(H) * 0.1
    gy, gn = torch.randn(T, H).to(dt_res), torch.randn(T, H).to(dt_blk)
    seed = 1234567

    def run(fused):
        L = [t.to(dev).requires_grad_(True) for t in (blk, res, w, b)]
        if fused:
            y, xn = ops._DropoutAddLN.apply(L[0], L[1], L[2], L[3], 1e-5, p, seed, dt_blk)
        else:
            y = ops._DropoutAdd.apply(L[0], L[1], p, seed)
            xn = ops.layer_norm(y, L[2], L[3], 1e-5, out_dtype=dt_blk)
        ((y.float() * gy.to(dev).float()).sum() + (xn.float() * gn.to(dev).float()).sum()).backward()
        return [y, xn] + [t.grad for t in L]
    a, c = run(True), run(False)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]), "forward must match the two-op form bit for bit"
    tol = dict(rtol=1e-5, atol_scale=1e-6) if dt_res == torch.float32 and dt_blk == torch.float32 else dict(rtol=2e-2, atol_scale=1e-2)
    for u, v, n in zip(a[2:], c[2:], ["dblk", "dres", "dgamma", "dbeta"]):
        _close(u.float(), v.float(), n, **tol)


@pytest.mark.parametrize("S,H,E,K,dt,p,cap", [(1000, 704, 8, 2, torch.bfloat16, 0.1, 200), (257, 64, 4, 1, torch.float32, 0.0, None),
                                               (512, 256, 8, 3, torch.float32, 0.2, 100)])
def test_boundary_with_moe_combine(dev, S, H, E, K, dt, p, cap):
    """MoE combine formed inside the boundary kernel vs moe_combine -> dropout_add -> layer_norm: forward
    bit-identical (incl. capacity-dropped tokens = exact zero rows), all five gradients to rounding."""
    from apertis_llm_amd import ops
    torch.manual_seed(S + H + K)
    logits = torch.randn(S, E, device=dev)
    _, idx, w0 = ops.moe_gate_topk(logits, K)
    plan = ops.moe_plan(idx, w0, E, cap, None)
    rows = int(plan.max_rows)
    yr0, res0 = torch.randn(rows, H).to(dt), torch.randn(S, H)
    g0, b0 = torch.randn(H) * 0.2 + 1, torch.randn(H) * 0.1
    gy, gn = torch.randn(S, H, device=dev), torch.randn(S, H, device=dev).to(dt)
    seed = 424242

    def run(fused):
        L = [t.detach().clone().to(dev).requires_grad_(True) for t in (yr0, w0, res0, g0, b0)]
        if fused:
            y, xn = ops._DropoutAddLN.apply(L[0], L[2], L[3], L[4], 1e-5, p, seed, dt, L[1], plan)
        else:
            out = ops.moe_combine(L[0], L[1], plan, out_dtype=dt)
            y = ops._DropoutAdd.apply(out, L[2], p, seed)
            xn = ops.layer_norm(y, L[3], L[4], 1e-5, out_dtype=dt)
        ((y * gy).sum() + (xn.float() * gn.float()).sum()).backward()
        return [y, xn] + [t.grad for t in L]
    a, c = run(True), run(False)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]), "forward must match the three-op form bit for bit"
    tol = dict(rtol=1e-5, atol_scale=1e-6) if dt == torch.float32 else dict(rtol=2e-2, atol_scale=1e-2)
    for u, v, n in zip(a[2:], c[2:], ["dyr", "dw", "dres", "dgamma", "dbeta"]):
        _close(u.float(), v.float(), n, **tol)


@pytest.mark.parametrize("S,H,E,K,dt,p,cap", [(1000, 704, 8, 2, torch.bfloat16, 0.1, 200), (257, 64, 4, 1, torch.float32, 0.0, None),
                                               (777, 1024, 8, 2, torch.bfloat16, 0.25, 150), (530, 704, 8, 2, torch.float32, 0.1, 90),
                                               (300, 320, 4, 2, torch.bfloat16, 0.0, None)])
def test_combine_backward_inside_the_layernorm_backward_is_bit_identical(dev, monkeypatch, S, H, E, K, dt, p, cap):
    """apertis_layernorm_combine_bwd (round 6: the MoE combine's backward on the row that the boundary's LayerNorm backward
    holds in registers - the masked gradient rows [T, H] never reach HBM) against apertis_layernorm_bwd followed by
    apertis_moe_combine_bwd: all five gradients (expert rows, combine weights, residual, gamma, beta) bit for bit, with
    capacity-dropped slots (their weight gradient stays zero), K = 1 and 2, every row-chunk count, fp32 and bf16 rows; and the
    fused path is the one that ran (no [T, H] gradient row tensor is allocated: the two-launch entry point is not called)."""
    from apertis_llm_amd import ops, _lib
    torch.manual_seed(S + H + K)
    logits = torch.randn(S, E, device=dev)
    _, idx, w0 = ops.moe_gate_topk(logits, K)
    plan = ops.moe_plan(idx, w0, E, cap, None)
    rows = int(plan.max_rows)
    yr0, res0 = torch.randn(rows, H).to(dt), torch.randn(S, H)
    g0, b0 = torch.randn(H) * 0.2 + 1, torch.randn(H) * 0.1
    gy, gn = torch.randn(S, H, device=dev), torch.randn(S, H, device=dev).to(dt)
    lib = _lib.load()
    calls = {"two": 0}
    real = lib.apertis_moe_combine_bwd

    def run(fused):
        monkeypatch.setattr(ops.norm, "FUSE_COMBINE_BWD", fused)
        L = [t.detach().clone().to(dev).requires_grad_(True) for t in (yr0, w0, res0, g0, b0)]
        y, xn = ops._DropoutAddLN.apply(L[0], L[2], L[3], L[4], 1e-5, p, 424242, dt, L[1], plan)
        ((y * gy).sum() + (xn.float() * gn.float()).sum()).backward()
        return [t.grad for t in L]

    class _Spy:
        def __call__(self, *a):
            calls["two"] += 1
            return real(*a)
    monkeypatch.setattr(lib, "apertis_moe_combine_bwd", _Spy(), raising=False)
    a = run(True)
    assert calls["two"] == 0, "the fused entry point must have been taken"
    c = run(False)
    assert calls["two"] == 1
    n_rows = int(plan.offsets[-1])
    for u, v, n in zip(a, c, ["dyr", "dw", "dres", "dgamma", "dbeta"]):
        if n == "dyr":          # (rows past the last kept one are never written by either form)
            u, v = u[:n_rows], v[:n_rows]
        assert torch.equal(u, v), n
    if cap is not None:
        assert int((plan.slot_of < 0).sum()) > 0 and float(a[1][plan.slot_of < 0].abs().max()) == 0.0


@pytest.mark.parametrize("sizes,N,K", [([4100, 0, 90, 513], 576, 96), ([2000, 2300], 512, 160), ([5000, 300, 0, 1], 1024, 704)])
def test_grouped_gemm_nt_two_per_cu_kernel(dev, sizes, N, K):
    """The 256x128 two-work-groups-per-CU NT kernel (taken for an activation / second-output epilogue on a short K)
    against the plain-epilogue path on the same operands: the pre-activation output is bit-identical (same K order),
    the activated output is gelu of it, and dropout only zeroes / rescales it.  Ragged groups, an empty group, a
    partial n-tile, odd and minimal numbers of 32-deep K steps."""
    from apertis_llm_amd import _lib
    lib, P, S = _lib.load(), _lib.ptr, _lib.stream_ptr
    torch.manual_seed(N + K)
    E, R = len(sizes), sum(sizes)
    x = torch.randn(R, K, device=dev).bfloat16()
    W = (torch.randn(E, N, K, device=dev) / K ** 0.5).bfloat16()
    b = torch.randn(E, N, device=dev)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=dev)
    plain, pre, act, drop = (torch.full((R, N), float("nan"), device=dev, dtype=torch.bfloat16) for _ in range(4))
    pre2 = torch.empty_like(pre)

    def nt(out, pre_out, a, p):
        rc = lib.apertis_grouped_gemm_nt(P(x), P(W), P(b), P(offs), P(out), P(pre_out), None, R, N, K, K, E, a, p, 77, 1, 1, S())
        assert rc == 0
    nt(plain, None, 0, 0.0)
    nt(act, pre, 1, 0.0)
    nt(drop, pre2, 1, 0.25)
    torch.cuda.synchronize()
    assert torch.equal(plain, pre) and torch.equal(pre, pre2), "pre-activation output must match the plain path bit for bit"
    ref = torch.nn.functional.gelu(pre.float())
    _close(act.float(), ref, "gelu(pre)", rtol=8e-3, atol_scale=1e-5)
    kept = drop != 0
    frac = float((kept & (act != 0)).sum()) / max(1.0, float((act != 0).sum()))
    assert abs(frac - 0.75) < 0.01, frac
    _close(drop.float()[kept], (act.float() / 0.75)[kept], "kept values rescaled", rtol=8e-3, atol_scale=1e-5)


@pytest.mark.parametrize("batch", [32, 44])
def test_moe_full_size_properties(dev, batch):
    """BASELINE sizes (1.5B MoE: 44 x 4096 tokens - the bench's batch, 225 280 routed rows - and the earlier 32 x 4096;
    H=704, I=2816, 8 experts, top-2, capacity 1.25): the kernels the
    launch heuristics pick at THIS size (two-per-CU and persistent NT, TN v3 pair, radix select, fused activation backward)
    checked through size-independent properties - the plan is a bijection onto the kept assignments in canonical order
    under the capacity, and sampled rows / one expert's weight gradient of the expert MLP equal dense fp64 / fp32 math on
    the same bf16-rounded operands."""
    from apertis_llm_amd import ops
    torch.manual_seed(0)
    S, H, I, E, K = batch * 4096, 704, 2816, 8, 2
    logits = torch.randn(S, E, device=dev)
    logits[:, 0] += 0.7                                    # skew: experts 0 overflows, others vary
    _, idx, w = ops.moe_gate_topk(logits, K)
    cap = max(1, int((S / E) * 1.25))
    plan = ops.moe_plan(idx, w, E, cap, None)
    offs = plan.offsets.cpu().numpy().astype(np.int64)
    total = int(offs[-1])
    counts = np.diff(offs)
    assert (counts >= 0).all() and (counts <= cap).all() and total <= E * cap
    want = np.minimum(np.bincount(idx.cpu().numpy().reshape(-1), minlength=E), cap)
    assert counts.tolist() == want.tolist(), "every expert keeps min(assigned, capacity) rows"
    rt, rk = plan.row_token.cpu().numpy()[:total].astype(np.int64), plan.row_k.cpu().numpy()[:total].astype(np.int64)
    slot = plan.slot_of.cpu().numpy()
    assert len(np.unique(rt * K + rk)) == total, "an assignment is kept at most once"
    assert (slot[rt, rk] == np.arange(total)).all() and int((slot >= 0).sum()) == total, "slot_of inverts the row lists"
    idx_c = idx.cpu().numpy()
    for e in range(E):
        a, b = offs[e], offs[e + 1]
        assert (idx_c[rt[a:b], rk[a:b]] == e).all(), "rows of an expert's range were routed to it"
        key = rk[a:b] * S + rt[a:b]
        assert (np.diff(key) > 0).all(), "canonical order inside an expert: k, then token"
    # overflow keeps the largest weights of each (expert, k) slot
    w_c = w.cpu().numpy()
    e0k0 = (idx_c[:, 0] == 0)
    kept0 = np.zeros(S, bool)
    sel = rt[offs[0]:offs[1]][rk[offs[0]:offs[1]] == 0]
    kept0[sel] = True
    if e0k0.sum() > len(sel) > 0:
        assert w_c[e0k0 & kept0, 0].min() >= w_c[e0k0 & ~kept0, 0].max()

    # expert MLP at the planned row counts
    rows = int(plan.max_rows)
    xg = torch.randn(rows, H, device=dev).bfloat16().requires_grad_(True)
    w1 = (torch.randn(E, I, H, device=dev) * 0.03).requires_grad_(True)
    b1 = (torch.randn(E, I, device=dev) * 0.1).requires_grad_(True)
    w2 = (torch.randn(E, H, I, device=dev) * 0.03).requires_grad_(True)
    b2 = (torch.randn(E, H, device=dev) * 0.1).requires_grad_(True)
    y = ops.expert_mlp(xg, w1, b1, w2, b2, plan.offsets, rows, act="gelu", drop_p=0.0, seed=0, compute_dtype=torch.bfloat16)
    dy = torch.randn(rows, H, device=dev).bfloat16()
    y.backward(dy)
    sample = torch.from_numpy(np.random.default_rng(1).choice(total, 384, replace=False)).to(dev)
    exp_of = torch.bucketize(sample, plan.offsets[1:].long(), right=True)
    w1q, w2q = w1.detach().bfloat16().double(), w2.detach().bfloat16().double()
    xs = xg.detach()[sample].double().requires_grad_(True)
    pre = torch.einsum("rh,rih->ri", xs, w1q[exp_of]) + b1.detach().double()[exp_of]
    hmid = torch.nn.functional.gelu(pre.bfloat16().double())          # the kernel rounds pre and h to bf16 between the GEMMs
    ref = torch.einsum("ri,rhi->rh", hmid.bfloat16().double(), w2q[exp_of]) + b2.detach().double()[exp_of]
    _close(y.detach()[sample].double(), ref, "expert MLP rows (sampled)", rtol=2e-2, atol_scale=1e-2)
    # input gradient of the sampled rows (through both data-gradient GEMMs and the fused act' epilogue)
    dh = torch.einsum("rh,rhi->ri", dy[sample].double(), w2q[exp_of]).bfloat16().double()
    gp = torch.autograd.grad(torch.nn.functional.gelu(pre), pre, dh)[0].bfloat16().double()
    dx_ref = torch.einsum("ri,rih->rh", gp, w1q[exp_of])
    _close(xg.grad[sample].double(), dx_ref, "dx rows (sampled)", rtol=3e-2, atol_scale=2e-2)
    # one expert's weight and bias gradients (TN v3 pair) against fp32 dense math on the same rows
    e = 3
    a, b = int(offs[e]), int(offs[e + 1])
    xe = xg.detach()[a:b].float()
    pre_e = (xe @ w1.detach()[e].bfloat16().float().T + b1.detach()[e]).bfloat16().float()
    h_e = torch.nn.functional.gelu(pre_e).bfloat16().float()
    _close(w2.grad[e], dy[a:b].float().T @ h_e, "dW2[e]", rtol=2e-2, atol_scale=1e-2)
    _close(b2.grad[e], dy[a:b].float().sum(0), "db2[e]", rtol=2e-2, atol_scale=1e-2)
    dh_e = (dy[a:b].float() @ w2.detach()[e].bfloat16().float()).bfloat16().float()
    pre_g = pre_e.clone().requires_grad_(True)
    dpre_e = torch.autograd.grad(torch.nn.functional.gelu(pre_g), pre_g, dh_e)[0].bfloat16().float()
    _close(w1.grad[e], dpre_e.T @ xe, "dW1[e]", rtol=2e-2, atol_scale=1e-2)
    _close(b1.grad[e], dpre_e.sum(0), "db1[e]", rtol=2e-2, atol_scale=1e-2)


@pytest.mark.parametrize("batch", [44])
def test_expert_mlp_full_size_dropout_mask_recovered(dev, batch):
    """Dropout ON (p = 0.1, the reference default core.py:439) at the bench's full size: 225 280 capacity-filled rows, the
    two-per-CU kernel's saved-gradient epilogue.  The mask is recovered from the tensors the forward leaves for the
    backward (h = gelu(pre) * keep / (1-p), g' = gelu'(pre) * keep / (1-p): an element is dropped iff both are exactly 0),
    its statistics are checked (rate, per-column and per-row rates inside binomial bounds, no correlation between
    neighbours), and on sampled rows the KEPT elements equal dense fp64 math on the same bf16-rounded operands, the dropped
    ones are exact zeros; the layer output and the input gradient are then checked against dense math that uses the
    recovered mask."""
    from apertis_llm_amd import ops
    torch.manual_seed(1)
    H, I, E, p = 704, 2816, 8, 0.1
    per = int((batch * 4096 / E) * 1.25)
    rows = per * E
    offs = torch.arange(E + 1, device=dev, dtype=torch.int32) * per
    xg = torch.randn(rows, H, device=dev).bfloat16().requires_grad_(True)
    w1 = (torch.randn(E, I, H, device=dev) * 0.03).requires_grad_(True)
    b1 = (torch.randn(E, I, device=dev) * 0.1).requires_grad_(True)
    w2 = (torch.randn(E, H, I, device=dev) * 0.03).requires_grad_(True)
    b2 = (torch.randn(E, H, device=dev) * 0.1).requires_grad_(True)
    y = ops.expert_mlp(xg, w1, b1, w2, b2, offs, rows, act="gelu", drop_p=p, seed=12345, compute_dtype=torch.bfloat16)
    assert y.grad_fn.saved_grad, "the saved-gradient epilogue is the form the bench runs at this size"
    _xg, gsv, h = y.grad_fn.saved_tensors[:3]
    keep = (h != 0) | (gsv != 0)
    # ---- statistics of the mask
    rate = float(keep.float().mean())
    assert abs(rate - (1 - p)) < 5e-4, rate
    col = keep.float().mean(0)
    row = keep[:: max(1, rows // 65536)].float().mean(1)
    sd_c, sd_r = (p * (1 - p) / rows) ** 0.5, (p * (1 - p) / I) ** 0.5
    assert float((col - (1 - p)).abs().max()) < 6 * sd_c, float((col - (1 - p)).abs().max()) / sd_c
    assert float((row - (1 - p)).abs().max()) < 6.5 * sd_r, float((row - (1 - p)).abs().max()) / sd_r
    kf = keep[: 1 << 15].float() - (1 - p)
    for shifted in (kf[:, 1:] * kf[:, :-1], kf[1:] * kf[:-1], kf[:, 4:] * kf[:, :-4]):   # neighbours in a row, a column, a hash group
        assert abs(float(shifted.mean())) < 6 * p * (1 - p) / shifted.numel() ** 0.5
    # the mask hash is FACTORISED (round 5: fin(rowmix(row) ^ colmix(column pair)), grouped_gemm.hip gd_pair): rows and columns at the
    # distances its structure repeats on (a lane's rows are 16 apart, its pieces 8 columns wide, a tile 256 x 128) must be as
    # uncorrelated as neighbours, and so must the four corners of a rectangle - the bare xor of a row half and a column half
    # would make h(r1,c1) ^ h(r1,c2) ^ h(r2,c1) ^ h(r2,c2) vanish, the multiply behind it is what has to break that
    for dr in (16, 64, 256, 1024):
        sh = kf[dr:] * kf[:-dr]
        assert abs(float(sh.mean())) < 6 * p * (1 - p) / sh.numel() ** 0.5, ("rows", dr)
    for dc in (2, 8, 128, 1408):
        sh = kf[:, dc:] * kf[:, :-dc]
        assert abs(float(sh.mean())) < 6 * p * (1 - p) / sh.numel() ** 0.5, ("columns", dc)
    for dr, dc in ((1, 1), (1, 2), (16, 2), (4, 8), (64, 352), (256, 128)):
        quad = kf[:-dr, :-dc] * kf[:-dr, dc:] * kf[dr:, :-dc] * kf[dr:, dc:]
        assert abs(float(quad.mean())) < 6 * (p * (1 - p)) ** 2 / quad.numel() ** 0.5, ("rectangle", dr, dc)
    # (and between the two 16-bit halves of one hash word: elements 2c and 2c + 1 of a row are kf[:, 1:] * kf[:, :-1] above)
    # ---- kept elements = dense math, dropped = exact zeros (sampled rows)
    sample = torch.from_numpy(np.random.default_rng(2).choice(rows, 320, replace=False)).to(dev)
    exp_of = (sample // per).long()
    w1q, w2q = w1.detach().bfloat16().double(), w2.detach().bfloat16().double()
    xs = xg.detach()[sample].double()
    pre = (torch.einsum("rh,rih->ri", xs, w1q[exp_of]) + b1.detach().double()[exp_of]).bfloat16().double().requires_grad_(True)
    act = torch.nn.functional.gelu(pre)
    dact = torch.autograd.grad(act.sum(), pre)[0]
    ks = keep[sample]
    assert bool((h[sample][~ks] == 0).all()) and bool((gsv[sample][~ks] == 0).all())
    _close(h[sample].double()[ks], (act.detach() / (1 - p))[ks], "kept h = gelu(pre)/(1-p)", rtol=1.2e-2, atol_scale=2e-3)
    _close(gsv[sample].double()[ks], (dact / (1 - p))[ks], "kept g' = gelu'(pre)/(1-p)", rtol=1.2e-2, atol_scale=2e-3)
    # ---- the layer output and the input gradient with the recovered mask
    ref = torch.einsum("ri,rhi->rh", h[sample].double(), w2q[exp_of]) + b2.detach().double()[exp_of]
    _close(y.detach()[sample].double(), ref, "y rows (sampled, dropout on)", rtol=2e-2, atol_scale=1e-2)
    dy = torch.randn(rows, H, device=dev).bfloat16()
    y.backward(dy)
    dh = torch.einsum("rh,rhi->ri", dy[sample].double(), w2q[exp_of]).bfloat16().double()
    dpre = (dh * gsv[sample].double()).bfloat16().double()
    _close(xg.grad[sample].double(), torch.einsum("ri,rih->rh", dpre, w1q[exp_of]), "dx rows (sampled, dropout on)",
           rtol=3e-2, atol_scale=2e-2)
    e = 5
    a, b = e * per, (e + 1) * per
    _close(w2.grad[e], dy[a:b].float().T @ h[a:b].float(), "dW2[e] (dropout on)", rtol=2e-2, atol_scale=1e-2)


@pytest.mark.parametrize("E,R,C", [(1, 704, 704), (8, 2816, 704), (8, 704, 2816), (1, 448, 176), (3, 70, 36), (2, 65, 130), (1, 7, 5)])
def test_cast_transpose_plain_and_transposed(dev, E, R, C):
    """apertis_cast_transpose (the GEMM operands' preparation, reference: the autocast of core.py's nn.Linear weights): the
    bf16 copy with its K padded to 64 and the transposed copy, bit-exact against torch's rounding, pads exactly zero - both the
    four-column kernel (C % 4 == 0) and the scalar one, partial 64 x 64 tiles, more than one group."""
    from apertis_llm_amd import ops
    torch.manual_seed(E * 1000 + R + C)
    w = torch.randn(E, R, C, device=dev)
    plain, tr = ops.cast_transpose(w, torch.bfloat16)
    Cp, Rp = -(-C // 64) * 64, -(-R // 64) * 64
    assert plain.shape == (E, R, Cp) and tr.shape == (E, C, Rp)
    ref = w.to(torch.bfloat16)
    assert torch.equal(plain[:, :, :C], ref) and (Cp == C or bool((plain[:, :, C:] == 0).all()))
    assert torch.equal(tr[:, :, :R], ref.transpose(1, 2)) and (Rp == R or bool((tr[:, :, R:] == 0).all()))
    p32, t32 = ops.cast_transpose(w, torch.float32)
    assert torch.equal(p32, w) and torch.equal(t32, w.transpose(1, 2))


@pytest.mark.parametrize("S,E,K,H,dt", [(1, 8, 2, 704, torch.bfloat16), (16, 8, 2, 704, torch.bfloat16), (64, 8, 2, 704, torch.bfloat16),
                                        (7, 4, 1, 256, torch.float32), (33, 16, 1, 1024, torch.bfloat16), (5, 4, 4, 128, torch.float32)])
def test_route_small_equals_gate_plan_gather(dev, S, E, K, H, dt):
    """apertis_moe_route_small (gate + plan + gather-LN of a handful of rows in one launch: the decode step) against the three
    ops it replaces: every output bit-identical, also with ties in the logits and with experts nobody chose."""
    from apertis_llm_amd import ops
    torch.manual_seed(S * 131 + E)
    logits = torch.randn(S, E)
    if S > 2:
        logits[1] = logits[0]                       # identical rows
        logits[2, :] = 0.25                         # an all-tie row: lowest expert indices win
    x = torch.randn(S, H).to(dt)
    g, b = torch.randn(E, H) * 0.2 + 1, torch.randn(E, H) * 0.1
    with torch.no_grad():
        lg, xd, gd, bd = logits.to(dev), x.to(dev), g.to(dev), b.to(dev)
        assert ops.moe_route_small_supported(lg, xd, K) == (S <= 16)
        gates0, idx0, w0 = ops.moe_gate_topk(lg, K)
        plan0 = ops.moe_plan(idx0, w0, E)
        xg0 = ops.moe_gather_ln(xd, gd, bd, plan0, 1e-5, out_dtype=dt)
        gates1, idx1, w1, plan1, xg1 = ops.moe_route_small(lg, xd, gd, bd, 1e-5, K, out_dtype=dt)
        torch.cuda.synchronize()
    assert torch.equal(gates0, gates1) and torch.equal(idx0.to(torch.int32), idx1) and torch.equal(w0, w1)
    rows = int(plan0.offsets[-1])
    assert rows == S * K and torch.equal(plan0.offsets, plan1.offsets) and torch.equal(plan0.slot_of, plan1.slot_of)
    assert torch.equal(plan0.row_token[:rows], plan1.row_token[:rows]) and torch.equal(plan0.row_k[:rows], plan1.row_k[:rows])
    assert torch.equal(xg0[:rows], xg1[:rows])


@pytest.mark.parametrize("S,E,K,H,dt", [(1, 8, 2, 704, torch.bfloat16), (16, 8, 2, 704, torch.bfloat16), (5, 4, 2, 256, torch.float32),
                                        (3, 8, 1, 1024, torch.bfloat16)])
def test_moe_entrance_of_a_handful_of_rows_in_one_launch(dev, S, E, K, H, dt):
    """apertis_moe_enter_small (block boundary + router + gate + plan + gather-LN for <= 16 rows: the decode step) against
    dropout_add_layer_norm_router followed by the gate / plan / gather-LN ops: every output bit-identical."""
    from apertis_llm_amd import ops
    torch.manual_seed(S * 7 + H)
    blk, res = torch.randn(S, H).to(dt), torch.randn(S, H)
    w, b = torch.randn(H) * 0.2 + 1, torch.randn(H) * 0.1
    rw, rb = torch.randn(H) * 0.2 + 1, torch.randn(H) * 0.1
    W, wb = torch.randn(E, H) / H ** 0.5, torch.randn(E) * 0.1
    eg, eb = torch.randn(E, H) * 0.2 + 1, torch.randn(E, H) * 0.1
    with torch.no_grad():
        d = [t.to(dev) for t in (blk, res, w, b, rw, rb, W, wb, eg, eb)]
        assert ops.moe_enter_small_supported(d[0], d[1], E, K)
        y0, xn0, lg0 = ops.dropout_add_layer_norm_router(d[0], d[1], d[2], d[3], 1e-5, 0.1, False, d[4], d[5], 1e-5, d[6], d[7],
                                                         out_dtype=dt)
        _g, idx0, w0 = ops.moe_gate_topk(lg0, K)
        plan0 = ops.moe_plan(idx0, w0, E)
        xg0 = ops.moe_gather_ln(xn0, d[8], d[9], plan0, 1e-12, out_dtype=dt)
        y1, lg1, w1, plan1, xg1 = ops.moe_enter_small(d[0], d[1], d[2], d[3], 1e-5, d[4], d[5], 1e-5, d[6], d[7], d[8], d[9], 1e-12, K)
        torch.cuda.synchronize()
    assert torch.equal(y0, y1) and torch.equal(lg0, lg1) and torch.equal(w0, w1)
    assert torch.equal(plan0.offsets, plan1.offsets) and torch.equal(plan0.slot_of, plan1.slot_of)
    assert torch.equal(plan0.row_token[:S * K], plan1.row_token[:S * K]) and torch.equal(xg0[:S * K], xg1[:S * K])


@pytest.mark.parametrize("S,H,dt,ok", [(16, 904, torch.float32, True), (16, 908, torch.float32, False), (13, 1000, torch.float32, False),
                                       (16, 1024, torch.bfloat16, True), (16, 1024, torch.float32, False)])
def test_moe_entrance_predicate_mirrors_the_kernels_lds_bound(dev, S, H, dt, ok):
    """moe_enter_small_supported must decline exactly the shapes apertis_moe_enter_small declines on its 160 KiB of
    LDS ((3E+4)*H*4 + S*H*sizeof(blk) + 4 KiB of static tables) - generate() has advanced every layer's SSM state by the time the launch would return -2."""
    from apertis_llm_amd import ops
    E, K = 8, 2
    torch.manual_seed(H + S)
    with torch.no_grad():
        blk, res = torch.randn(S, H, device=dev).to(dt), torch.randn(S, H, device=dev)
        assert ops.moe_enter_small_supported(blk, res, E, K) == ok
        if ok:   # and an accepted shape at the edge really launches
            v = lambda *s: torch.randn(*s, device=dev)
            y, lg, w, plan, xg = ops.moe_enter_small(blk, res, v(H), v(H), 1e-5, v(H), v(H), 1e-5, v(E, H) / H ** 0.5, v(E), v(E, H),
                                                     v(E, H), 1e-12, K)
            torch.cuda.synchronize()
            assert torch.isfinite(y).all() and int(plan.offsets[-1]) == S * K


@pytest.mark.parametrize("rows,H,I,ragged", [(16384, 704, 1408, False), (12000, 704, 1408, True), (33024, 384, 1024, True)])
def test_ring_kernel_under_the_tile_queue_is_bit_identical(dev, rows, H, I, ragged):
    """Round 6: grouped_gemm_nt4r_k takes a dynamic tile queue (data-parallel steps; one counter per XCD, the ticket fetched by
    a hand-issued atomic one tile ahead).  The saved-gradient forward and the fused data gradient of the expert MLP under the
    queue must equal the static walk bit for bit - a lost or doubled ticket shows as a missing tile - with even groups, with
    ragged groups incl. an EMPTY expert (padding tiles: the slow path) and on a grid only a little larger than the chip (the
    steal from other XCDs' counters).  K = H >= 352 and (rows / 256 + E) * ceil(I / 256) >= 256 tiles: the queue form's conditions."""
    from apertis_llm_amd import ops
    E = 8
    torch.manual_seed(rows + H)
    if ragged:
        cuts = torch.sort(torch.randint(0, rows, (E - 2,))).values.tolist()
        offs = [0] + cuts[:3] + [cuts[3]] + cuts[3:] + [rows]            # one expert with no rows
        offs = sorted(offs)[:E + 1]
        offs[-1] = rows
    else:
        offs = [rows // E * i for i in range(E)] + [rows]
    offsets = torch.tensor(offs, dtype=torch.int32, device=dev)
    xg = torch.randn(rows, H, device=dev).bfloat16()
    w1, b1 = torch.randn(E, I, H, device=dev) * 0.03, torch.randn(E, I, device=dev) * 0.1
    w2, b2 = torch.randn(E, H, I, device=dev) * 0.03, torch.randn(E, H, device=dev) * 0.1
    dy = torch.randn(rows, H, device=dev).bfloat16()

    def run(queue):
        old = ops.GEMM_DYNAMIC_QUEUE
        ops.GEMM_DYNAMIC_QUEUE = queue
        try:
            x = xg.clone().requires_grad_(True)
            ws = [t.clone().requires_grad_(True) for t in (w1, b1, w2, b2)]
            outs = []
            for rep in range(2):       # (twice: the queue's counters are re-zeroed by every launch)
                y = ops.expert_mlp(x, *ws, offsets, rows, act="gelu", drop_p=0.1, seed=99, compute_dtype=torch.bfloat16)
                y.backward(dy)
                outs.append([y.detach().clone(), x.grad.clone()] + [w.grad.clone() for w in ws])
                x.grad = None
                for w in ws:
                    w.grad = None
            torch.cuda.synchronize()
            return outs
        finally:
            ops.GEMM_DYNAMIC_QUEUE = old
    a, b = run(False), run(True)
    for rep in range(2):
        for i, (p, q) in enumerate(zip(a[rep], b[rep])):
            assert torch.equal(p, q), f"rep {rep}, tensor {i}: the queue-driven ring kernel differs from the static walk"
