"""The optimizer kernels of csrc/optimizer.hip - apertis_grad_sumsq, apertis_clip_coef, apertis_adamw_step - against the update
rule in float64, through ApertisAdamW and through the C ABI.

Reference, per element and step t, in float64 with the constants the entry point forms in double and rounds once to fp32:
decay = 1 - lr wd, step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t);
    g' = g coef;  p *= decay;  m += (g' - m) (1 - beta1);  v = v beta2 + (1 - beta2) g'^2;  p -= step_size m / (sqrt(v) / bc2_sqrt + eps)
with coef = min(1, max_norm / (||g|| + 1e-6)) over all gradients of the step (1 without a clip), a NaN coefficient handed
through.  The fp32 state is carried from step to step by the kernels; the reference carries its own in float64.

A work-group takes a chunk of 16384 elements of one tensor and reads it 16 bytes at a time when the chunk's gradient
(grad_sumsq_k) or all four of its arrays (adamw_step_k) start on a 16-byte boundary, element by element otherwise; a chunk
whose length is no multiple of 4 ends element by element.  ApertisAdamW accepts a contiguous tensor that is an offset view of
a larger buffer, so the parameters, or the gradients, are buf[1:] - one float past a boundary - in two of the three layouts.

Bounds: p, exp_avg, exp_avg_sq rtol 2e-6 with an absolute floor of 1e-6 of the tensor's largest entry, the norm 1e-5 relative
(those of test_adamw_kernels_match_torch, here against float64); apertis_clip_coef alone 2e-7 relative on norm and
coefficient: its sum is accumulated in double, so only the final roundings to fp32 count (one for the norm, three for the
coefficient: 3 x 2^-24 = 1.8e-7)."""
import math

import numpy as np
import pytest
import torch

from test_row_kernels_gpu import NAN, OK, _close, _lib

gpu = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------------------------------
# mirror of csrc/optimizer.hip: a change there must be made here too
OPT_CHUNK, OPT_NT, CLIP_NT = 16384, 256, 1024
SIZES = [1, 3, 5, 16383, 16384, 16385, 2 * 16384 + 7]
LAYOUTS = ["aligned", "offset-params", "offset-grads"]
CLIP_NS = [0, 1, 1023, 1024, 1025, 5000]


def _chunk_paths(numel, p_off, g_off):
    """The (kernel, load form) pairs the chunks of one tensor take; *_off: floats between a 16-byte boundary and element 0."""
    out = set()
    for c in range(-(-numel // OPT_CHUNK)):
        n = min(OPT_CHUNK, numel - c * OPT_CHUNK)
        g_vec, all_vec = g_off % 4 == 0, g_off % 4 == 0 and p_off % 4 == 0        # (a chunk starts 65536 bytes after the last)
        for kernel, vec in (("sumsq", g_vec), ("adamw", all_vec)):
            if vec and n >= 4:
                out.add((kernel, "vector"))
            if not vec or n % 4:
                out.add((kernel, "element" if not vec else "tail"))
    return out


def _clip_passes(n):
    return -(-n // CLIP_NT)


def test_case_tables_cover_every_dispatch_path():
    """From the mirror: the sizes give chunks that are shorter than a vector, end in a tail, fill a chunk exactly, spill one
    element into a second chunk and span three; the layouts take both kernels through their 16-byte and element forms; the
    partial counts of apertis_clip_coef sit at none, one, both sides of one pass of its 1024 threads, and five passes."""
    seen = {lay: set() for lay in LAYOUTS}
    for lay in LAYOUTS:
        for n in SIZES:
            seen[lay] |= _chunk_paths(n, int(lay == "offset-params"), int(lay == "offset-grads"))
    assert seen["aligned"] == {("sumsq", "vector"), ("sumsq", "tail"), ("adamw", "vector"), ("adamw", "tail")}
    assert seen["offset-params"] == {("sumsq", "vector"), ("sumsq", "tail"), ("adamw", "element")}
    assert seen["offset-grads"] == {("sumsq", "element"), ("adamw", "element")}
    assert _chunk_paths(3, 0, 0) == {("sumsq", "tail"), ("adamw", "tail")} and ("adamw", "tail") not in _chunk_paths(16384, 0, 0)
    assert [-(-n // OPT_CHUNK) for n in SIZES] == [1, 1, 1, 1, 1, 2, 3]
    assert [_clip_passes(n) for n in CLIP_NS] == [0, 1, 1, 1, 2, 5]


# ---------------------------------------------------------------------------------------------------------------------------
# float64 reference
def _f32(x):
    return float(np.float32(x))


def _adam_args(lr, b1, b2, eps, wd, step):
    """AdamArgs as apertis_adamw_step forms them: in double, rounded once to fp32."""
    return dict(decay=_f32(1.0 - lr * wd), omb1=_f32(1.0 - b1), b2=_f32(b2), omb2=_f32(1.0 - b2), eps=_f32(eps),
                step_size=_f32(lr / (1.0 - b1 ** step)), bc2=_f32(math.sqrt(1.0 - b2 ** step)))


def _adam64(p, g, m, v, a, coef):
    """One step on float64 tensors, in place."""
    g = g * coef
    p.mul_(a["decay"])
    m.add_((g - m) * a["omb1"])
    v.mul_(a["b2"]).add_(a["omb2"] * g * g)
    p.sub_(a["step_size"] * (m / (v.sqrt() / a["bc2"] + a["eps"])))


def _coef64(grads, max_norm):
    norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))
    c = max_norm / (norm + 1e-6)
    return norm, (c if c != c else min(c, 1.0))


def _offset_view(t, dev):
    """t on the device as a contiguous view one float past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, device=dev)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


# ---------------------------------------------------------------------------------------------------------------------------
# 1. through ApertisAdamW
@gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_adamw_five_steps_against_fp64(dev, layout):
    """Five steps over two parameter groups (weight decay 0.01 / 0) with a changing learning rate; the clip active (coef 0.1),
    inactive, exactly at the boundary (max_grad_norm = the norm), max_grad_norm = 0 (the gradient counts for nothing: only the
    decay and the moments' own decay act) and no clip at all."""
    from apertis_llm_amd.training import ApertisAdamW
    gen = torch.Generator().manual_seed(3 + len(layout))
    p0 = [torch.randn(n, generator=gen) for n in SIZES]
    if layout == "offset-params":
        mine = [_offset_view(p, dev).requires_grad_(True) for p in p0]
    else:
        mine = [p.to(dev).requires_grad_(True) for p in p0]
    assert all((p.data_ptr() % 16 == 4) == (layout == "offset-params") for p in mine)
    cut, wds = 4, (0.01, 0.0)
    opt = ApertisAdamW([{"params": mine[:cut], "weight_decay": wds[0]}, {"params": mine[cut:], "weight_decay": wds[1]}], lr=1e-2)
    P64, M64, V64 = [p.double() for p in p0], [torch.zeros(n, dtype=torch.float64) for n in SIZES], \
        [torch.zeros(n, dtype=torch.float64) for n in SIZES]
    b1, b2, eps = 0.9, 0.999, 1e-8
    for it, mode in enumerate(["active", "inactive", "boundary", "zero", "none"]):
        scale = 1e-3 if mode == "inactive" else 1.0
        grads = [torch.randn(n, generator=gen) * scale for n in SIZES]
        norm, _ = _coef64(grads, 1.0)
        max_norm = {"active": 0.1 * norm, "inactive": 1.0, "boundary": _f32(norm), "zero": 0.0, "none": None}[mode]
        for p, g in zip(mine, grads):
            p.grad = _offset_view(g, dev) if layout == "offset-grads" else g.to(dev)
            assert (p.grad.data_ptr() % 16 == 4) == (layout == "offset-grads")
        lr = 1e-2 / (it + 1)
        for gr in opt.param_groups:
            gr["lr"] = lr
        opt.step(max_grad_norm=max_norm)
        coef = 1.0
        if max_norm is not None:
            _, coef = _coef64(grads, max_norm)
            got = float(opt.last_grad_norm)
            assert abs(got - norm) <= 1e-5 * norm, (mode, got, norm)
            assert {"active": coef < 0.11, "inactive": coef == 1.0, "boundary": abs(coef - 1) < 1e-6, "zero": coef == 0.0}[mode]
        for i in range(len(SIZES)):
            _adam64(P64[i], grads[i].double(), M64[i], V64[i], _adam_args(lr, b1, b2, eps, wds[i >= cut], it + 1), coef)
        for i, (p, n) in enumerate(zip(mine, SIZES)):
            st = opt.state[p]
            _close(p.detach(), P64[i], f"{mode}: param {n}", rtol=2e-6, atol_scale=1e-6)
            _close(st["exp_avg"], M64[i], f"{mode}: exp_avg {n}", rtol=2e-6, atol_scale=1e-6)
            _close(st["exp_avg_sq"], V64[i], f"{mode}: exp_avg_sq {n}", rtol=2e-6, atol_scale=1e-6)
            assert float(st["step"]) == it + 1


@gpu
@pytest.mark.parametrize("layout", ["aligned", "offset-params"])
def test_adamw_zero_infinite_and_late_steps(dev, layout):
    """Through ApertisAdamW.step, one after the other on the same optimizer: all-zero gradients (norm 0, coefficient 1: p becomes
    p * decay exactly, the moments stay 0), one infinite gradient (last_grad_norm is inf, the coefficient 0, and 0 * inf = NaN
    lands in that element's p, exp_avg and exp_avg_sq and nowhere else), and, on a second optimizer, a host step count of
    10^6 - 1 before the step, so that the kernel is handed step = 10^6 and both bias corrections round to 1."""
    from apertis_llm_amd.training import ApertisAdamW
    gen = torch.Generator().manual_seed(29 + len(layout))
    sizes, lr, wd = [5, 16385], 1e-2, 0.05
    p0 = [torch.randn(n, generator=gen) for n in sizes]
    put = (lambda t: _offset_view(t, dev)) if layout == "offset-params" else (lambda t: t.to(dev))
    mine = [put(p).requires_grad_(True) for p in p0]
    opt = ApertisAdamW(mine, lr=lr, weight_decay=wd)
    for p in mine:
        p.grad = torch.zeros_like(p)
    opt.step(max_grad_norm=1.0)
    assert float(opt.last_grad_norm) == 0.0
    decay = torch.tensor(_adam_args(lr, 0.9, 0.999, 1e-8, wd, 1)["decay"], dtype=torch.float32)
    for p, q in zip(mine, p0):
        assert torch.equal(p.detach().cpu(), q * decay), "p is not p * (1 - lr wd) bit for bit"
        assert not opt.state[p]["exp_avg"].any() and not opt.state[p]["exp_avg_sq"].any() and float(opt.state[p]["step"]) == 1.0
    hit = (1, 16384)                                   # the one element of the second chunk of tensor 1
    for p in mine:
        p.grad = torch.zeros_like(p)
    mine[hit[0]].grad[hit[1]] = float("inf")
    before = [p.detach().cpu().clone() for p in mine]
    opt.step(max_grad_norm=1.0)
    assert float(opt.last_grad_norm) == float("inf")
    for ti, (p, pb) in enumerate(zip(mine, before)):
        nan = torch.zeros(p.numel(), dtype=torch.bool)
        if ti == hit[0]:
            nan[hit[1]] = True
        st = opt.state[p]
        for name, t in (("p", p.detach()), ("exp_avg", st["exp_avg"]), ("exp_avg_sq", st["exp_avg_sq"])):
            assert torch.equal(torch.isnan(t).cpu(), nan), f"tensor {ti}: NaN in {name} elsewhere than at the infinite gradient"
        assert torch.equal(p.detach().cpu()[~nan], pb[~nan] * decay)
        assert not st["exp_avg"].cpu()[~nan].any() and not st["exp_avg_sq"].cpu()[~nan].any()
    # a late step: one ordinary step makes the moments, then the host step counts are set to 10^6 - 1
    mine = [put(p).requires_grad_(True) for p in p0]
    opt = ApertisAdamW(mine, lr=lr, weight_decay=wd)
    for p in mine:
        p.grad = torch.randn(p.numel(), generator=gen).to(dev)
    opt.step()
    P64 = [p.detach().cpu().double() for p in mine]
    M64 = [opt.state[p]["exp_avg"].cpu().double() for p in mine]
    V64 = [opt.state[p]["exp_avg_sq"].cpu().double() for p in mine]
    for p in mine:
        opt.state[p]["step"] = torch.tensor(1e6 - 1)
    grads = [torch.randn(n, generator=gen) for n in sizes]
    for p, g in zip(mine, grads):
        p.grad = g.to(dev)
    opt.step(max_grad_norm=1.0)
    norm, coef = _coef64(grads, 1.0)
    assert abs(float(opt.last_grad_norm) - norm) <= 1e-5 * norm
    a = _adam_args(lr, 0.9, 0.999, 1e-8, wd, 10 ** 6)
    assert a["step_size"] == _f32(lr) and a["bc2"] == 1.0
    for i, (p, n) in enumerate(zip(mine, sizes)):
        _adam64(P64[i], grads[i].double(), M64[i], V64[i], a, coef)
        st = opt.state[p]
        assert float(st["step"]) == 1e6
        _close(p.detach(), P64[i], f"param {n}", rtol=2e-6, atol_scale=1e-6)
        _close(st["exp_avg"], M64[i], f"exp_avg {n}", rtol=2e-6, atol_scale=1e-6)
        _close(st["exp_avg_sq"], V64[i], f"exp_avg_sq {n}", rtol=2e-6, atol_scale=1e-6)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. through the C ABI: the same edges on the bare kernels, with NaN sentinels around every output and bit checks
def _tables(dev, tensors):
    """Device tables of one launch over [(p, g, m, v)]: records, chunk -> tensor, chunk -> index, number of chunks."""
    rec = np.array([[p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()] for p, g, m, v in tensors], dtype=np.int64)
    ct = np.concatenate([np.full(-(-p.numel() // OPT_CHUNK), i, dtype=np.int32) for i, (p, *_) in enumerate(tensors)])
    ci = np.concatenate([np.arange(-(-p.numel() // OPT_CHUNK), dtype=np.int32) for p, *_ in tensors])
    return torch.from_numpy(rec).to(dev), torch.from_numpy(ct).to(dev), torch.from_numpy(ci).to(dev), len(ct)


def _state(dev, sizes, gen, offset=False):
    """[(p, g, m, v)] on the device with non-trivial moments, and their float64 copies."""
    host = [(torch.randn(n, generator=gen), torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.1,
             torch.rand(n, generator=gen) * 0.01) for n in sizes]
    put = (lambda t: _offset_view(t, dev)) if offset else (lambda t: t.to(dev))
    return [tuple(put(t) for t in quad) for quad in host], [tuple(t.double() for t in quad) for quad in host]


def _sumsq_and_clip(lib, P, S, dev, tabs, max_norm, poison=None):
    rec, ct, ci, n = tabs
    partials = torch.full((n + 2,), NAN, device=dev)
    nc = torch.full((4,), NAN, device=dev)
    assert lib.apertis_grad_sumsq(P(rec), P(ct), P(ci), n, P(partials[1:]), S()) == OK
    assert lib.apertis_clip_coef(P(partials[1:]), n, max_norm, P(nc[1:]), P(poison), S()) == OK
    torch.cuda.synchronize()
    assert math.isnan(float(partials[0])) and math.isnan(float(partials[-1])) and math.isnan(float(nc[0])) and math.isnan(float(nc[3]))
    return partials[1:-1], nc[1:3]


@gpu
@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset"])
def test_step_one_million_and_the_chunk_sums(dev, offset):
    """apertis_grad_sumsq's per-chunk sums against float64 within 5e-6 relative - every term is positive and passes through at
    most 73 fp32 roundings (the square, a thread's 64 sequential additions in the element form, six shuffle steps, two final
    additions): 73 x 2^-24 = 4.4e-6 -, then apertis_adamw_step at step = 10^6, where both bias corrections round to 1
    (step_size = lr, bc2_sqrt = 1), from non-zero moments; all four arrays of every tensor one float past a 16-byte boundary in
    the second case."""
    lib, P, S = _lib()
    gen = torch.Generator().manual_seed(17)
    dev_t, ref = _state(dev, SIZES, gen, offset)
    tabs = _tables(dev, dev_t)
    partials, nc = _sumsq_and_clip(lib, P, S, dev, tabs, 1.0)
    want = torch.cat([torch.stack([c.sum() for c in (g.double() ** 2).split(OPT_CHUNK)]) for _, g, _, _ in ref])
    _close(partials, want, "chunk sums", rtol=5e-6, atol_scale=0.0)
    norm, coef = _coef64([g for _, g, _, _ in ref], 1.0)
    assert abs(float(nc[0]) - norm) <= 3e-6 * norm and abs(float(nc[1]) - coef) <= 3e-6 * coef     # (the square root halves it)
    lr, b1, b2, eps, wd, step = 3e-3, 0.9, 0.999, 1e-8, 0.1, 10 ** 6
    a = _adam_args(lr, b1, b2, eps, wd, step)
    assert a["step_size"] == _f32(lr) and a["bc2"] == 1.0
    rec, ct, ci, n = tabs
    g_before = [g.clone() for _, g, _, _ in dev_t]
    assert lib.apertis_adamw_step(P(rec), P(ct), P(ci), n, lr, b1, b2, eps, wd, step, P(nc), S()) == OK
    torch.cuda.synchronize()
    for (p, g, m, v), (p64, g64, m64, v64), gb, sz in zip(dev_t, ref, g_before, SIZES):
        _adam64(p64, g64, m64, v64, a, coef)
        _close(p, p64, f"param {sz}", rtol=2e-6, atol_scale=1e-6)
        _close(m, m64, f"exp_avg {sz}", rtol=2e-6, atol_scale=1e-6)
        _close(v, v64, f"exp_avg_sq {sz}", rtol=2e-6, atol_scale=1e-6)
        assert torch.equal(g, gb), "the gradients are not written back"


@gpu
@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset"])
def test_zero_and_infinite_gradients(dev, offset):
    """All-zero gradients from zero moments: the norm is 0, the coefficient 1, and p becomes p * decay exactly - nothing else
    moves.  One infinite gradient: the norm is inf, the coefficient 0, 0 * inf = NaN lands in that element's p, m and v and
    nowhere else - every other element sees a zero gradient."""
    lib, P, S = _lib()
    gen = torch.Generator().manual_seed(23)
    sizes = [5, 16385]
    put = (lambda t: _offset_view(t, dev)) if offset else (lambda t: t.to(dev))
    p0 = [torch.randn(n, generator=gen) for n in sizes]
    quad = [(put(p), put(torch.zeros_like(p)), put(torch.zeros_like(p)), put(torch.zeros_like(p))) for p in p0]
    tabs = _tables(dev, quad)
    rec, ct, ci, n = tabs
    lr, b1, b2, eps, wd = 1e-2, 0.9, 0.999, 1e-8, 0.05
    _, nc = _sumsq_and_clip(lib, P, S, dev, tabs, 1.0)
    assert nc.tolist() == [0.0, 1.0]
    assert lib.apertis_adamw_step(P(rec), P(ct), P(ci), n, lr, b1, b2, eps, wd, 1, P(nc), S()) == OK
    torch.cuda.synchronize()
    decay = torch.tensor(_adam_args(lr, b1, b2, eps, wd, 1)["decay"], dtype=torch.float32)
    for (p, g, m, v), q in zip(quad, p0):
        assert torch.equal(p.cpu(), q * decay), "p is not p * (1 - lr wd) bit for bit"
        assert not m.any() and not v.any() and not g.any()
    hit = (1, 16384)                                   # the one element of the second chunk of tensor 1
    quad[hit[0]][1][hit[1]] = float("inf")
    before = [tuple(t.clone() for t in q) for q in quad]
    _, nc = _sumsq_and_clip(lib, P, S, dev, tabs, 1.0)
    assert nc.tolist() == [float("inf"), 0.0]
    assert lib.apertis_adamw_step(P(rec), P(ct), P(ci), n, lr, b1, b2, eps, wd, 2, P(nc), S()) == OK
    torch.cuda.synchronize()
    for ti, ((p, g, m, v), (pb, gb, mb, vb)) in enumerate(zip(quad, before)):
        nan = torch.zeros(p.numel(), dtype=torch.bool, device=dev)
        if ti == hit[0]:
            nan[hit[1]] = True
        for name, t in (("p", p), ("m", m), ("v", v)):
            assert torch.equal(torch.isnan(t), nan), f"tensor {ti}: NaN in {name} elsewhere than at the infinite gradient"
        assert torch.equal(p[~nan].cpu(), (pb[~nan].cpu() * decay)) and not m[~nan].any() and not v[~nan].any()
        assert torch.equal(g, gb)


@gpu
@pytest.mark.parametrize("n", CLIP_NS)
def test_clip_coef_alone(dev, n):
    """apertis_clip_coef on synthetic partials: norm = sqrt(sum) against a float64 sum and coef = min(1, max_norm / (norm +
    1e-6)) within 2e-7 relative, clipping (max_norm = norm / 3) and not (max_norm = 2 norm + 1); n = 0 is the norm of nothing
    (0: the coefficient is min(1, max_norm / 1e-6)); a non-zero poison word makes them (NaN, -1), and apertis_adamw_step
    then leaves p, m, v bit-unchanged."""
    lib, P, S = _lib()
    gen = torch.Generator().manual_seed(n + 1)
    part = torch.rand(max(n, 1), generator=gen) * 10 + 0.1
    buf = torch.full((n + 2,), NAN, device=dev)
    buf[1:n + 1] = part[:n].to(dev)
    norm = math.sqrt(float(part[:n].double().sum()))
    zero = torch.zeros(1, dtype=torch.int32, device=dev)
    for max_norm in ((norm / 3, 2 * norm + 1) if n else (1.0, 1e-7)):
        for poison in (None, zero):
            out = torch.full((4,), NAN, device=dev)
            assert lib.apertis_clip_coef(P(buf[1:]) if n else None, n, max_norm, P(out[1:]), P(poison), S()) == OK
            torch.cuda.synchronize()
            assert math.isnan(float(out[0])) and math.isnan(float(out[3]))
            want = min(1.0, _f32(max_norm) / (norm + 1e-6))
            assert abs(float(out[1]) - norm) <= 2e-7 * norm, (float(out[1]), norm)
            assert abs(float(out[2]) - want) <= 2e-7 * want, (float(out[2]), want)
            assert (float(out[2]) == 1.0) == (want == 1.0)
    # the poison word
    word = torch.tensor([7], dtype=torch.int32, device=dev)
    out = torch.full((2,), 5.0, device=dev)
    assert lib.apertis_clip_coef(P(buf[1:]) if n else None, n, 1.0, P(out), P(word), S()) == OK
    quad, _ = _state(dev, [5, 16385], gen)
    before = [tuple(t.clone() for t in q) for q in quad]
    rec, ct, ci, nch = _tables(dev, quad)
    assert lib.apertis_adamw_step(P(rec), P(ct), P(ci), nch, 1e-2, 0.9, 0.999, 1e-8, 0.01, 3, P(out), S()) == OK
    torch.cuda.synchronize()
    assert math.isnan(float(out[0])) and float(out[1]) == -1.0
    for q, b in zip(quad, before):
        for t, tb in zip(q, b):
            assert torch.equal(t.view(torch.int32), tb.view(torch.int32)), "a poisoned step wrote"
