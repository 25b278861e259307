"""The shifted cross entropy kernels of csrc/loss.hip through the C ABI - apertis_cross_entropy_fwd, _bwd and the one-pass
_fwd_bwd - and the two-kernel in-place path of ops.linear_cross_entropy, against float64 references on the stored logits.

Reference: row loss = logsumexp(x) - x[target] and dlogits = (softmax(x) - onehot(target)) * gscale in float64 on the logits as
stored (bf16 or fp32), for the rows that have a target; 0 for ignored rows, rows whose label is outside [0, V) and rows at
l >= n_pos.  The target of row (b, l) is labels[b, l + 1] at row pitch label_stride.

A work-group of 256 threads walks a row in 16-byte chunks (VN = 8 bf16 or 4 fp32 logits), thread t taking chunks t, t + 256,
...; the one-pass form keeps at most 16 chunks per thread and declines wider rows (-2).  The widths below sit at one chunk,
exactly one chunk per thread, one more (thread 0 alone walks a second), 32000, the one-pass form's last width and the first it
declines; the targets at column 0, V - 1, both ends of a chunk and in a thread's second chunk.  All three kernels run on every
case; the one-pass form must equal forward + backward bit for bit, out of place and in place (dlogits = logits).

Logits of -inf (a masked vocabulary): exp(-inf - lse) is an exact 0 and the loss stays finite, also where a 16-byte chunk
holds nothing but -inf behind a finite one of the same thread: such a chunk's exponents are taken against 0, not against its
maximum, so it contributes (-inf, 0) instead of -inf - (-inf) = NaN (test_chunk_loop_on_the_cpu replays a thread's loop in
numpy with and without that guard).

lse[row] leaves the forward as ONE fp32, spaced 2^-20 or finer only while |lse| < 16 (CE_PAIR_FROM).  Below, loss and softmax
are taken from it (lse - x[t], exp(x - lse)); from 16 on - next to 1e4 its spacing is 9.8e-4 - they are taken from the pair
(M, log S): (M - x[t]) + log S and exp((x - M) - log S), which the backward kernel sums again for such a row.  Rows of equal
logits put lse on both sides of 16; test_fp32_logits_offset_by_1e4 puts it next to +-1e4, in the one-pass form and past its
last width.

Tolerances, for every case (those of the loss tests in tests/test_model_gpu.py, here against float64): row losses rtol 2e-6 +
atol 2e-6, fp32 gradient 1e-6 |ref| + 1e-7, bf16 gradient 2^-8 |ref| + 1e-7.  No case needed a measured allowance;
test_fp32_logits_offset_by_1e4 prints the error of stock fp32 F.cross_entropy on its inputs next to the kernels' for
comparison only."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_row_kernels_gpu import BF16, F32, NAN, OK, ERR_UNSUPPORTED, _close, _code, _lib, _tag

gpu = pytest.mark.gpu
NEG_INF = float("-inf")

# ---------------------------------------------------------------------------------------------------------------------------
# mirror of csrc/loss.hip: a change there must be made here too
CE_NT, CE_KEEP = 256, 16
CE_PAIR_FROM = 16.0       # |lse| from which loss and softmax come from the pair (M, log S)


def _vn(dt):
    return 8 if dt == BF16 else 4


def _one_pass_ok(V, dt):
    return V % _vn(dt) == 0 and V // _vn(dt) <= CE_KEEP * CE_NT


def _chunks_of_thread(V, dt, t):
    """How many chunks thread t of a row's work-group walks."""
    n = V // _vn(dt)
    return len(range(t, n, CE_NT))


def _widths(dt):
    vn = _vn(dt)
    return [vn, CE_NT * vn, CE_NT * vn + vn, 32000, CE_KEEP * CE_NT * vn, CE_KEEP * CE_NT * vn + vn]


B_, L_, NPOS, LSTRIDE = 2, 8, 6, 11        # rows 6 and 7 of each sequence are beyond n_pos; label_stride > n_pos + 1


def _labels(V, dt, ignore_index, gen, hi=None):
    """int64 [B_, LSTRIDE]: the targets of rows 0..5 of sequence 0 are column 0, V - 1, the last column of chunk 0, the first
    of chunk 1, a column of thread 0's second chunk and ignore_index; those of sequence 1 a label past V, a negative label
    that is not ignore_index, random columns and the two edges again.  hi: live targets stay below it (masked tails)."""
    vn = _vn(dt)
    top = (V if hi is None else hi) - 1
    second = CE_NT * vn + 3 if V > CE_NT * vn + 3 else V // 2
    rnd = [int(torch.randint(0, top + 1, (1,), generator=gen)) for _ in range(2)]
    rows = [[0, top, vn - 1, min(vn, top), min(second, top), ignore_index],
            [V + 5, -3 if ignore_index != -3 else -4, rnd[0], rnd[1], top, 0]]
    lab = torch.randint(0, top + 1, (B_, LSTRIDE), generator=gen)          # (what no row may read is a valid label too)
    for b in range(B_):
        for l, t in enumerate(rows[b]):
            lab[b, l + 1] = t
    return lab


def _logits(kind, V, dt, gen):
    """float64 [B_, L_, V] holding values of dt."""
    vn = _vn(dt)
    if kind == "equal":
        x = (torch.arange(B_ * L_, dtype=torch.float64).reshape(B_, L_, 1) - 4).expand(B_, L_, V).clone()
    elif kind == "saturated":
        x = torch.randn(B_, L_, V, generator=gen, dtype=torch.float64)
        hot = torch.randint(0, V, (B_, L_), generator=gen)
        hot[0, 0], hot[0, 1] = 0, V - 1                   # ... on the row's own target, twice
        x.scatter_(2, hot[..., None], 80.0)
    else:
        x = torch.randn(B_, L_, V, generator=gen, dtype=torch.float64) * 3
    x = x.to(dt).double()
    col = torch.arange(V)
    if kind == "inf-scattered":                           # about one logit in five, never a whole chunk
        m = (torch.rand(B_, L_, V, generator=gen) < 0.2) & (col % vn != 1)
        x[m] = NEG_INF
    elif kind == "inf-chunk":                             # thread 0's second chunk, whole
        assert V >= 2 * CE_NT * vn
        x[..., CE_NT * vn:CE_NT * vn + vn] = NEG_INF
    elif kind == "inf-tail":
        x[..., _tail_from(V):] = NEG_INF
    return x


def _tail_from(V):
    return 4000 if V == 4096 else V - 100


# (kind, V, dtype, ignore_index)
def _ce_cases():
    out = []
    for dt in (BF16, F32):
        vn = _vn(dt)
        for V in _widths(dt):
            out.append(("normal", V, dt, -100))
            out.append(("normal", V, dt, 0))
        for V in (vn, CE_NT * vn + vn, 32000):
            out += [("equal", V, dt, -100), ("saturated", V, dt, -100)]
        out += [("inf-scattered", CE_NT * vn + vn, dt, -100), ("inf-scattered", 32000, dt, -100),
                ("inf-chunk", 2 * CE_NT * vn, dt, -100), ("inf-chunk", CE_KEEP * CE_NT * vn + vn, dt, -100),
                ("inf-tail", 4096, dt, -100), ("inf-tail", 32000, dt, -100), ("inf-tail", CE_KEEP * CE_NT * vn + vn, dt, -100)]
    return out


CE_CASES = _ce_cases()


def test_case_tables_cover_every_dispatch_path():
    """From the mirror: both dtypes meet the six widths (one chunk; one chunk per thread; thread 0 alone with a second; 32000; the
    one-pass form's last width and the first it declines) with both ignore_index values; the -inf cases put a whole chunk of
    -inf behind a finite one in some thread, in the one-pass form and in the two-pass form alone."""
    seen = set()
    for kind, V, dt, ign in CE_CASES:
        vn = _vn(dt)
        assert V % vn == 0
        seen.add(("width", dt, V, ign) if kind == "normal" else ("kind", dt, kind))
        seen.add(("one-pass", dt, _one_pass_ok(V, dt)))
        if kind == "inf-chunk":
            assert _chunks_of_thread(V, dt, 0) >= 2
            seen.add(("inf-after-finite", dt, _one_pass_ok(V, dt)))
        if kind == "inf-tail":
            c0 = -(-_tail_from(V) // vn)                  # first chunk that is -inf only
            assert c0 < V // vn and c0 >= CE_NT, "the thread that holds it has walked a finite chunk before"
            seen.add(("inf-after-finite", dt, _one_pass_ok(V, dt)))
    for dt in (BF16, F32):
        vn = _vn(dt)
        w = _widths(dt)
        assert [_chunks_of_thread(V, dt, 0) for V in w] == [1, 1, 2, -(-32000 // vn // CE_NT), CE_KEEP, CE_KEEP + 1]
        assert [_chunks_of_thread(V, dt, 1) for V in w[:3]] == [0, 1, 1]
        assert [_one_pass_ok(V, dt) for V in w] == [True] * 3 + [dt == BF16, True, False]     # (32000 fp32 logits: two-pass only)
        assert {("width", dt, V, ign) for V in w for ign in (-100, 0)} <= seen
        assert {("kind", dt, k) for k in ("equal", "saturated", "inf-scattered", "inf-chunk", "inf-tail")} <= seen
        assert {("one-pass", dt, True), ("one-pass", dt, False)} <= seen
        assert {("inf-after-finite", dt, True), ("inf-after-finite", dt, False)} <= seen
    assert ("inf-chunk", 4096, BF16, -100) in CE_CASES and ("inf-tail", 4096, BF16, -100) in CE_CASES
    # both regimes of lse: the rows of equal logits at V = 32000 have lse = x + ln V on both sides of CE_PAIR_FROM
    for dt in (BF16, F32):
        assert ("equal", 32000, dt, -100) in CE_CASES
    eq = _logits("equal", 8, F32, None)[..., 0] + math.log(32000)
    live = torch.zeros(B_, L_, dtype=torch.bool)
    live[0, :5], live[1, 2:6] = True, True                      # (the rows of _labels that carry a target at ignore_index -100)
    assert (eq[live] < CE_PAIR_FROM - 1).sum() >= 3 and (eq[live] > CE_PAIR_FROM + 0.5).sum() >= 2, eq
    # the targets of _labels: column 0, V - 1, ti = VN - 1, ti = 0 of the next chunk, a thread's second chunk
    lab = _labels(32000, BF16, -100, torch.Generator().manual_seed(0))
    assert lab[0, 1:7].tolist() == [0, 31999, 7, 8, 2051, -100] and lab[1, 1:3].tolist() == [32005, -3]
    assert 2051 // 8 == CE_NT and LSTRIDE > NPOS + 1 and NPOS < L_


# ---------------------------------------------------------------------------------------------------------------------------
# the per-thread chunk loop on the CPU: why the -inf cases failed before the fix
def _thread_loop(chunks, guarded):
    """ce_fwd_k's loop of one thread over its chunks in fp32 numpy: (m, s).  guarded: the exponents of a chunk are taken
    against 0 where its maximum is -inf (ce_chunk_base); unguarded is the kernel before the fix."""
    f = np.float32
    m, s = f(-np.inf), f(0)
    with np.errstate(invalid="ignore"):
        for v in chunks:
            v = np.asarray(v, dtype=np.float32)
            cm = v.max()
            cb = f(0) if (guarded and cm == -np.inf) else cm
            cs = np.exp2((v - cb) * f(1.4426950408889634)).astype(np.float32).sum(dtype=np.float32)
            mn = max(m, cm)                                # ce_merge
            if mn == -np.inf:
                m, s = mn, f(0)
                continue
            s = f(s * np.exp2((m - mn) * f(1.4426950408889634)) + cs * np.exp2((cm - mn) * f(1.4426950408889634)))
            m = mn
    return m, s


def test_chunk_loop_on_the_cpu():
    """A chunk of -inf only behind a finite one made the thread's sum NaN before the fix and adds nothing after it; in front of
    the first finite chunk it was harmless (ce_merge's own guard); chunks with a finite maximum give the same bits either way."""
    fin1, fin2, ninf = [0.5, -1.0, 2.0, 0.25], [1.5, 0.0, -2.0, 3.0], [-np.inf] * 4
    mixed = [-np.inf, 1.0, -np.inf, 0.5]
    for order, nan_before in (([fin1, ninf], True), ([fin1, ninf, fin2], True), ([ninf, fin1], False), ([ninf, ninf, fin1], False),
                              ([fin1, mixed, fin2], False), ([ninf], False)):
        m0, s0 = _thread_loop(order, guarded=False)
        m1, s1 = _thread_loop(order, guarded=True)
        assert bool(np.isnan(s0)) == nan_before, (order, s0)
        flat = np.array([x for c in order for x in c], dtype=np.float64)
        if np.isfinite(flat).any():
            ref = np.log(np.exp(flat[np.isfinite(flat)]).sum())
            assert abs(float(m1) + math.log(float(s1)) - ref) < 1e-6, (order, m1, s1, ref)
        else:
            assert m1 == -np.inf and s1 == 0
        if not nan_before:
            assert m0 == m1 and s0.tobytes() == s1.tobytes(), "a result that was right must keep its bits"


# ---------------------------------------------------------------------------------------------------------------------------
# float64 reference and the three kernels
def _ref64(x, lab, V, ignore_index, g):
    """(row losses [B, L], dlogits [B, L, V], live [B, L]) in float64."""
    B, L, _ = x.shape
    tgt = torch.full((B, L), -1, dtype=torch.int64)
    tgt[:, :NPOS] = lab[:, 1:NPOS + 1]
    live = (tgt != ignore_index) & (tgt >= 0) & (tgt < V)
    live[:, NPOS:] = False
    t = torch.where(live, tgt, torch.zeros_like(tgt))
    lse = torch.logsumexp(x, -1)
    loss = torch.where(live, lse - x.gather(2, t[..., None])[..., 0], torch.zeros_like(lse))
    p = torch.exp(x - lse[..., None])
    p.scatter_add_(2, t[..., None], -torch.ones(B, L, 1, dtype=torch.float64))
    return loss, torch.where(live[..., None], p * g, torch.zeros_like(p)), live


def _run_kernels(dev, x, lab, V, dt, ignore_index, g):
    """fwd + bwd into NaN-filled outputs, then the one-pass form out of place and in place: its outputs must be the two
    kernels' bit for bit where it accepts the width, and it must decline (-2) where it does not.  (lse, loss, dlogits)."""
    lib, P, S = _lib()
    B, L, _ = x.shape
    X, LAB, G = x.to(dt).to(dev), lab.to(dev), torch.tensor([g], device=dev)
    code = _code(dt)
    args = (B, L, V, lab.shape[1], NPOS, ignore_index, code, S())
    lse, loss = torch.full((B * L,), NAN, device=dev), torch.full((B * L,), NAN, device=dev)
    d = torch.full((B * L * V + 128,), NAN, dtype=dt, device=dev)
    assert lib.apertis_cross_entropy_fwd(P(X), P(LAB), P(lse), P(loss), *args) == OK
    assert lib.apertis_cross_entropy_bwd(P(X), P(LAB), P(lse), P(G), P(d[64:]), *args) == OK
    torch.cuda.synchronize()
    assert torch.isnan(d[:64].float()).all() and torch.isnan(d[-64:].float()).all(), "dlogits written outside its rows"
    d = d[64:-64].view(B, L, V)
    lse1, loss1 = torch.full((B * L,), NAN, device=dev), torch.full((B * L,), NAN, device=dev)
    d1 = torch.full_like(X, NAN)
    rc = lib.apertis_cross_entropy_fwd_bwd(P(X), P(LAB), P(lse1), P(loss1), P(G), P(d1), *args)
    if not _one_pass_ok(V, dt):
        assert rc == ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert torch.isnan(d1.float()).all() and torch.isnan(lse1).all(), "the declined call wrote"
        # ... and the in-place form of the two kernels, as ops.linear_cross_entropy then calls them
        inpl = X.clone()
        assert lib.apertis_cross_entropy_bwd(P(inpl), P(LAB), P(lse), P(G), P(inpl), *args) == OK
        torch.cuda.synchronize()
        assert torch.equal(inpl.view(torch.int16 if dt == BF16 else torch.int32), d.view(torch.int16 if dt == BF16 else torch.int32))
        return lse, loss, d
    assert rc == OK
    inpl = X.clone()
    lse2, loss2 = torch.full((B * L,), NAN, device=dev), torch.full((B * L,), NAN, device=dev)
    assert lib.apertis_cross_entropy_fwd_bwd(P(inpl), P(LAB), P(lse2), P(loss2), P(G), P(inpl), *args) == OK
    torch.cuda.synchronize()
    bits = torch.int16 if dt == BF16 else torch.int32
    for name, a, b_, c in (("lse", lse, lse1, lse2), ("loss", loss, loss1, loss2)):
        assert torch.equal(a.view(torch.int32), b_.view(torch.int32)), f"{name}: the one-pass form differs from the forward"
        assert torch.equal(a.view(torch.int32), c.view(torch.int32)), f"{name}: the in-place one-pass form differs"
    assert torch.equal(d.view(bits), d1.view(bits)), "dlogits: the one-pass form differs from the backward"
    assert torch.equal(d.view(bits), inpl.view(bits)), "dlogits: the in-place one-pass form differs"
    return lse, loss, d


def _check(lse, loss, d, x, lab, V, dt, ignore_index, g):
    """The issue's bounds against float64.  Returns the largest errors (loss, gradient)."""
    B, L, _ = x.shape
    loss_ref, d_ref, live = _ref64(x, lab, V, ignore_index, g)
    assert live.sum() >= 7 and (~live[:, :NPOS]).sum() >= 3
    loss, lse, d = loss.cpu().double().view(B, L), lse.cpu().double().view(B, L), d.cpu().double()
    assert torch.isfinite(loss).all() and torch.isfinite(d).all() and torch.isfinite(lse).all()
    assert torch.equal(loss[~live], torch.zeros_like(loss[~live])) and torch.equal(lse[~live], torch.zeros_like(lse[~live]))
    assert float(d[~live].abs().max()) == 0.0, "a row without a target has a gradient"
    le = (loss - loss_ref).abs()
    lb = 2e-6 * loss_ref.abs() + 2e-6
    ge = (d - d_ref).abs()
    gb = (2.0 ** -8 if dt == BF16 else 1e-6) * d_ref.abs() + 1e-7
    print(f"CE {_tag(dt)} V={V}: max loss err {float(le.max()):.3e} (worst excess {float((le / lb).max()):.3f}), "
          f"max grad err {float(ge.max()):.3e} (worst excess {float((ge / gb).max()):.3f})")
    assert (le <= lb).all(), f"row losses: max err {float(le.max()):.3e}, {int((le > lb).sum())} rows outside the bound"
    assert (ge <= gb).all(), f"dlogits: max err {float(ge.max()):.3e}, {int((ge > gb).sum())} elements outside the bound"
    masked = torch.isinf(x) & live[..., None]
    assert float(d[masked].abs().max() if masked.any() else 0.0) == 0.0, "a masked (-inf) logit has a gradient"
    _close(lse[live], torch.logsumexp(x, -1)[live], "lse", 2e-6, 2e-6)
    return float(le.max()), float(ge.max())


@gpu
@pytest.mark.parametrize("kind,V,dt,ignore_index", CE_CASES, ids=[f"{c[0]}-V{c[1]}-{_tag(c[2])}-ign{c[3]}" for c in CE_CASES])
def test_cross_entropy_kernels_against_fp64(dev, kind, V, dt, ignore_index):
    """All three kernels on [2, 8, V] logits with n_pos = 6 and label_stride = 11: live rows with the targets of _labels,
    ignored rows, rows with a label outside [0, V), rows beyond n_pos."""
    gen = torch.Generator().manual_seed(V * 7 + (3 if dt == BF16 else 5) + len(kind))
    hi = None
    if kind == "inf-tail":
        hi = _tail_from(V)
    elif kind == "inf-chunk":
        hi = CE_NT * _vn(dt)
    lab = _labels(V, dt, ignore_index, gen, hi)
    x = _logits(kind, V, dt, gen)
    if kind == "inf-scattered":                             # the targets themselves stay finite
        t = lab[:, 1:L_ + 1].clamp(0, V - 1)
        x.scatter_(2, t[..., None], x.gather(2, t[..., None]).clamp_min(-9.0))
    g = 0.37
    lse, loss, d = _run_kernels(dev, x, lab, V, dt, ignore_index, g)
    _check(lse, loss, d, x, lab, V, dt, ignore_index, g)
    if kind == "equal":                                     # lse = x + ln V
        _, _, live = _ref64(x, lab, V, ignore_index, g)
        _close(lse.cpu().view(B_, L_)[live], (x[..., 0] + math.log(V))[live], "lse of equal logits", 2e-6, 2e-6)


@gpu
@pytest.mark.parametrize("V", [1028, 16388], ids=["V1028", "V16388-two-pass"])
@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["plus", "minus"])
def test_fp32_logits_offset_by_1e4(dev, sign, V):
    """fp32 rows of N(0, 3) offset by +1e4 and by -1e4, in the one-pass form (V = 1028) and past its last width (V = 16388: the
    two kernels, out of place and in place), within the bounds of every other case.  Every such row is in the pair regime:
    one fp32 lse[row] next to 1e4 is spaced 9.8e-4, which as the base of loss and softmax would be 4.6e-4 on a row loss and
    up to 1.2e-4 on the gradient.  The error of stock fp32 F.cross_entropy on the same inputs against the same reference is
    printed next to the kernels' for comparison (row loss 6.0e-7 ... 1.3e-6, gradient 2.7e-8 ... 4.7e-7 over the four cases;
    the kernels: 8.7e-7 and 3.8e-8 at most); it is a sanity check of the reference and enters no bound."""
    dt, g = F32, 0.37
    gen = torch.Generator().manual_seed(11 + int(sign) + V)
    lab = _labels(V, dt, -100, gen)
    x = (_logits("normal", V, dt, gen) + sign * 1e4).float().double()
    loss_ref, d_ref, live = _ref64(x, lab, V, -100, g)
    assert (torch.logsumexp(x, -1).abs() > 9e3).all()
    xs = x.float().requires_grad_(True)
    tgt = torch.where(live, torch.cat([lab[:, 1:NPOS + 1], lab[:, :L_ - NPOS]], 1), torch.full((B_, L_), -100))
    stock = F.cross_entropy(xs.view(-1, V), tgt.view(-1), ignore_index=-100, reduction="none")
    (stock.sum() * g).backward()
    stock_le = float((stock.detach().double().view(B_, L_) - loss_ref).abs().max())
    stock_ge = float((xs.grad.double() - d_ref).abs().max())
    print(f"stock fp32 F.cross_entropy against float64: loss {stock_le:.3e}, gradient {stock_ge:.3e}")
    assert stock_le < 4e-6 and stock_ge < 1e-6
    lse, loss, d = _run_kernels(dev, x, lab, V, dt, -100, g)
    _check(lse, loss, d, x, lab, V, dt, -100, g)


# ---------------------------------------------------------------------------------------------------------------------------
# the ops
@gpu
@pytest.mark.parametrize("dt,V", [(BF16, 520), (F32, 1028)], ids=["bf16", "f32"])
def test_ops_shifted_cross_entropy_ignore_index_0(dev, dt, V):
    """ops.shifted_cross_entropy(ignore_index=0): rows whose target is column 0 carry no loss and no gradient, -100 is then
    a label outside [0, V) and skipped as such; mean loss and gradient against float64."""
    from apertis_llm_amd import ops
    gen = torch.Generator().manual_seed(V)
    B, L = 3, 9
    x = (torch.randn(B, L, V, generator=gen, dtype=torch.float64) * 3).to(dt).double()
    lab = torch.randint(0, V, (B, L), generator=gen)
    lab[0, 2], lab[1, 4], lab[2, 1], lab[2, 8] = 0, 0, 0, -100
    tgt = lab[:, 1:]
    live = (tgt > 0)
    xr = x[:, :L - 1].clone().requires_grad_(True)
    lse = torch.logsumexp(xr, -1)
    ref = ((lse - xr.gather(2, tgt.clamp_min(0)[..., None])[..., 0]) * live).sum() / live.sum()
    (ref * 1.7).backward()
    xd = x.to(dt).to(dev).requires_grad_(True)
    loss = ops.shifted_cross_entropy(xd, lab.to(dev), ignore_index=0)
    (loss * 1.7).backward()
    got_loss, ref = float(loss.detach()), float(ref.detach())
    assert abs(got_loss - ref) <= 2e-6 * abs(ref) + 2e-6, (got_loss, ref)
    got = xd.grad.double().cpu()
    bound = (2.0 ** -8 if dt == BF16 else 1e-6) * xr.grad.abs() + 1e-7
    assert ((got[:, :L - 1] - xr.grad).abs() <= bound).all(), float((got[:, :L - 1] - xr.grad).abs().max())
    assert float(got[:, L - 1].abs().max()) == 0.0 and float(got[:, :L - 1][~live].abs().max()) == 0.0


def _lce_ref(h, W, lab, dt, scale):
    V = W.shape[0]
    n = min(h.shape[1], lab.shape[1]) - 1
    hr, Wr = h.double().clone().requires_grad_(True), W.to(dt).double().clone().requires_grad_(True)
    ref = F.cross_entropy(F.linear(hr, Wr)[:, :n].reshape(-1, V), lab[:, 1:n + 1].reshape(-1), ignore_index=-100)
    (ref * scale).backward()
    return ref.detach(), hr.grad, Wr.grad


def _spy(monkeypatch, lib, names):
    calls = []
    for name in names:
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, (lambda real, name: lambda *a: (calls.append((name, a)), real(*a))[1])(real, name))
    return calls


CE_ENTRIES = ("apertis_cross_entropy_fwd", "apertis_cross_entropy_bwd", "apertis_cross_entropy_fwd_bwd")


@gpu
@pytest.mark.parametrize("dt,V,how", [(BF16, 512, "switch"), (F32, 512, "switch"), (BF16, 32776, "declines"), (F32, 16388, "declines")],
                         ids=["bf16-V512-switched-off", "f32-V512-switched-off", "bf16-V32776-declined", "f32-V16388-declined"])
def test_linear_cross_entropy_two_kernel_path(dev, monkeypatch, dt, V, how):
    """ops.linear_cross_entropy on apertis_cross_entropy_fwd + apertis_cross_entropy_bwd IN PLACE on the chunk's logits - with
    LCE_FUSED_CE switched off, and at the first widths the one-pass entry point declines by itself (H = 32): loss, d hidden
    and d W against float64 within the bounds of test_linear_cross_entropy_matches_lm_head_then_loss; at V = 512 the
    switched-off path equals the one-pass path bit for bit; under torch.no_grad() only the forward kernel runs and gives
    the same loss."""
    from apertis_llm_amd import ops
    lib, _, _ = _lib()
    B, L, H, scale = 2, 9, 32, 1.3
    gen = torch.Generator().manual_seed(V + 1)
    h = (torch.randn(B, L, H, generator=gen) * 0.7).to(dt)
    W = torch.randn(V, H, generator=gen) * 0.1
    lab = torch.randint(0, V, (B, L + 2), generator=gen)
    lab[0, 3], lab[1, 1] = -100, V - 1
    ref, dh_ref, dW_ref = _lce_ref(h, W, lab, dt, scale)

    def run(grad=True):
        hd, Wd = h.to(dev).requires_grad_(grad), W.to(dev).requires_grad_(grad)
        loss = ops.linear_cross_entropy(hd, Wd, lab.to(dev), compute_dtype=dt)
        if grad:
            (loss * scale).backward()
        return loss.detach(), hd.grad, Wd.grad
    calls = _spy(monkeypatch, lib, CE_ENTRIES)
    fused = run() if how == "switch" else None
    if how == "switch":
        assert [c[0] for c in calls] == ["apertis_cross_entropy_fwd_bwd"]
        monkeypatch.setattr(ops.loss, "LCE_FUSED_CE", False)
    del calls[:]
    loss, dh, dW = run()
    names = [c[0] for c in calls]
    assert names == (["apertis_cross_entropy_fwd_bwd"] if how == "declines" else []) + ["apertis_cross_entropy_fwd", "apertis_cross_entropy_bwd"]
    bwd = calls[-1][1]
    assert bwd[0] == bwd[4], "the backward of the chunk runs in place on its logits"
    ltol = 1e-5 if dt == F32 else 2e-3
    assert abs(float(loss) - float(ref)) <= ltol * max(1.0, abs(float(ref))), (float(loss), float(ref))
    rtol, asc = (1e-4, 1e-5) if dt == F32 else (3e-2, 2e-2)
    _close(dh, dh_ref, "d hidden", rtol=rtol, atol_scale=asc)
    _close(dW, dW_ref, "d W", rtol=rtol, atol_scale=asc)
    assert dh.dtype == dt and dW.dtype == F32 and float(dh[:, L - 1:].abs().max()) == 0.0
    if fused is not None:
        assert torch.equal(loss, fused[0]) and torch.equal(dh, fused[1]) and torch.equal(dW, fused[2]), \
            "the two-kernel path differs from the one-pass path"
    del calls[:]
    with torch.no_grad():
        loss_ng, _, _ = run(grad=False)
    assert [c[0] for c in calls] == ["apertis_cross_entropy_fwd"]
    assert torch.equal(loss_ng, loss)
