"""The grouped GEMM kernels of csrc/grouped_gemm.hip against the float64 references of tests/gemm_ref.py, at every
path of launch_nt and of the TN entry points, through the C ABI (so that pre_act, act_bwd_pre, ldw, dtype_out, the tile queue and
the workspace are in the test's hands).  The tables and the mirror that says which kernel a row runs live in gemm_ref.py;
test_gemm_paths_cpu.py holds the mirror to hand-computed points, and test_profiler_sees_the_kernels_the_mirror_names holds it to
the library.

Operands lie on the dyadic grid of gemm_ref.py: nothing is rounded in any accumulation order, so
  - every fp32 output (dW, dbias, the fp32-output NT form, the fp32 kernel) equals the float64 reference,
  - every bf16 output of a linear epilogue (no activation or ReLU; dropout at p = 0.5, scale exactly 2; a saved gradient from
    {0, +-1/2, +-1, +-2}; the plain pre_act output; the data-gradient form with ReLU) equals ITS SINGLE bf16 ROUNDING,
and those assertions are torch.equal.  The dropout mask is gemm_ref.keep_mask (gd_keep), the same for every kernel and for
apertis_act_dropout_bwd.

GELU and SiLU outputs and the SAVE_GRAD derivative are compared with a tolerance.  What the activation is fed: EVERY bf16-output
epilogue rounds the pre-activation to bf16 first (`to_f32(from_f32<TO>(v))` in grouped_gemm_nt_k, the skinny kernel, nt256p_out_round
and nt2x_epilogue - EPI_BOTH packs it with pack_bf16x2), so the reference is
float64 on round_bf16(pre); with an fp32 output (TO = float) that rounding is the identity and the reference is float64 on the
exact pre-activation.  Tolerance of a bf16 output: ONE bf16 rounding, rtol 8e-3 with the floor 1e-5 of the tensor's maximum
(tests/test_decode_step_gpu.py's figure); fp32 outputs: rtol 1e-4, same floor.  The bf16-operand kernels evaluate GELU in a
three-term Abramowitz-Stegun form (gelu_terms); gemm_ref.gelu_fast_form evaluates that form in fp32 ON THE CPU at the case's
pre-activations and its distance from float64 is added as an absolute term.  Measured over the tables' rows (CPU, float64
against the fp32 form, per unit of output scale): at most 2.55e-5 for gelu and 1.10e-5 for gelu'; the per-case figure is what is
added, and it must stay below GELU_FORM_ABS / GELU_GRAD_FORM_ABS (2.8e-5 / 1.2e-5: a libm's last bits above the measurement).
No figure comes from a kernel's output.  Elements the mask drops are exactly 0.

Every output is prefilled with NaN below offsets[E] (each element must be written) and with a sentinel from there to max_rows (none
may be); operands are compared with their originals after the call."""
import functools

import pytest
import torch

import gemm_ref as R
from gemm_ref import BF16, F32, NT_CASES, NT_REFUSED, NT_TWINS, TN_CASES, TN_PAIR_CASES, TN_REFUSED

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT = -768.0                   # exact in bf16
GELU_FORM_ABS, GELU_GRAD_FORM_ABS = 2.8e-5, 1.2e-5


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def test_case_tables_cover_every_dispatch_path_at_this_cu_count():
    """The tables reach every path at THIS device's CU count (the mirror's queue4_ok, cpg and fold depend on it): a machine
    with another count fails here rather than testing less."""
    R.check_case_tables_cover_every_dispatch_path(_ncu())


# ---------------------------------------------------------------------------------------------------------------------------
def _api():
    from apertis_llm_amd import _lib
    return _lib.load(), _lib.ptr, _lib.stream_ptr


def _dtc(dt):
    from apertis_llm_amd import _lib
    return _lib.BF16 if dt == BF16 else _lib.F32


def _close(got, ref, name, rtol, extra_abs=0.0):
    ref = ref.detach().cpu().double()
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), f"{name}: {int((~torch.isfinite(got)).sum())} non-finite values"
    if ref.numel() == 0:
        return
    bound = rtol * ref.abs() + 1e-5 * float(ref.abs().max()) + extra_abs + 1e-30
    err = (got - ref).abs()
    print(f"FIGURE {name}: max abs err {float(err.max()):.3e}, worst excess {float((err / bound).max()):.3f} (rtol {rtol}, "
          f"extra abs {extra_abs:.2e}, ref max {float(ref.abs().max()):.3e})")
    bad = err > bound
    assert not bad.any(), f"{name}: {int(bad.sum())} / {bad.numel()} outside rtol {rtol}; max abs diff {float(err.max()):.3e}"


def _exact(got, ref, name):
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.shape == ref.shape and got.dtype == ref.dtype, (name, got.shape, ref.shape, got.dtype, ref.dtype)
    if not torch.equal(got, ref):
        bad = ~((got == ref) | (got.isnan() & ref.isnan()))
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f"{name}: {int(bad.sum())} / {bad.numel()} elements differ ({int(got.isnan().sum())} NaN); first at {idx}: "
                             f"got {float(got[tuple(idx)])}, expected {float(ref[tuple(idx)])}")


def _round_out(x, dt):
    return R.round_bf16(x) if dt == BF16 else x.float()


# ---------------------------------------------------------------------------------------------------------------------------
# NT
@functools.lru_cache(maxsize=None)
def _nt_problem(key):
    c = dict(key)
    i = R.nt_inputs(c)
    i["pre"] = R.nt_pre_ref(i["A"], i["W"], i["b"], i["offs"], c["K"])
    return i


def _nt_prepared(cid):
    """A case's inputs and float64 pre-activation, computed once per PROBLEM and shared (twins differ in id and queue only; the
    profiler test); never modified."""
    c = {c["id"]: c for c in NT_CASES}[cid]
    return c, _nt_problem(tuple(sorted((k, v) for k, v in c.items() if k not in ("id", "queue"))))


def _nt_call(c, i, dev):
    """One call through the C ABI; returns (rc, C, pre_act or None) with the operands checked unchanged."""
    lib, ptr, sp = _api()
    R_, N, rows = c["max_rows"], c["N"], int(i["offs"][-1])
    A, W, offs = i["A"].to(dev), i["W"].to(dev), i["offs"].to(dev)
    b = i["b"].to(dev) if i["b"] is not None else None
    mul = i["mul"].to(dev) if i["mul"] is not None else None

    def out():
        t = torch.full((R_, N), SENT, dtype=c["out"], device=dev)
        t[:rows] = NAN
        return t
    C, P = out(), (out() if c["pre"] else None)
    queue = torch.full((512,), 0x5a5a5a5a, dtype=torch.int32, device=dev) if c["queue"] else None   # (the entry point zeroes it)
    rc = lib.apertis_grouped_gemm_nt_q(ptr(A), ptr(W), ptr(b) if b is not None else None, ptr(offs), ptr(C),
                                       ptr(P) if P is not None else None, ptr(mul) if mul is not None else None, R_, N, c["K"],
                                       c["ldw"], len(c["sizes"]), c["act"] | c["flags"], c["p"], i["seed"], _dtc(c["dtype"]),
                                       _dtc(c["out"]), ptr(queue) if queue is not None else None, sp())
    torch.cuda.synchronize()
    assert torch.equal(A.cpu(), i["A"]) and torch.equal(W.cpu(), i["W"]) and torch.equal(offs.cpu(), i["offs"]), "operands changed"
    assert (b is None or torch.equal(b.cpu(), i["b"])) and (mul is None or torch.equal(mul.cpu(), i["mul"])), "operands changed"
    return rc, C, P


def _nt_check(c, i, C, P):
    cid, rows, act, p, out = c["id"], int(i["offs"][-1]), c["act"], c["p"], c["out"]
    for name, t in (("C", C), ("pre_act", P)):
        if t is not None:
            assert bool((t[rows:] == SENT).all()), f"{cid} {name}: rows at or past offsets[E] were written"
    C = C[:rows].cpu()
    pre = i["pre"]
    epi = R.nt_epilogue(act | c["flags"], p, c["pre"], c["mul"] is not None)
    scale = 1.0 / (1.0 - p) if p > 0 else 1.0
    keep = torch.from_numpy(R.keep_mask(i["seed"], rows, c["N"], p)) if p > 0 else torch.ones(rows, c["N"], dtype=torch.bool)
    if epi == "mul_saved":
        return _exact(C, _round_out(pre * i["mul"][:rows].double(), out), f"{cid} C (saved gradient)")
    if epi == "mul_act":
        assert act == R.ACT_RELU
        ref = pre * R.act_grad_ref(i["mul"][:rows], act) * keep.double() * scale
        return _exact(C, _round_out(ref, out), f"{cid} C (data gradient)")
    # the activation's argument (module doc): the pre-activation as a bf16 output stores it
    x = R.round_bf16(pre).double() if out == BF16 else pre
    if epi == "save_grad":
        form = [float((f.double() - scale * r).abs().max()) for f, r in
                zip(R.gelu_fast_form(x, scale), (R.act_ref(x, act), R.act_grad_ref(x, act)))]
        assert form[0] <= GELU_FORM_ABS * scale and form[1] <= GELU_GRAD_FORM_ABS * scale, form
        assert bool((C[~keep] == 0).all()) and bool((P[:rows].cpu()[~keep] == 0).all()), f"{cid}: dropped elements are not 0"
        _close(C, R.act_ref(x, act) * keep * scale, f"{cid} C (gelu)", 8e-3, form[0])
        return _close(P[:rows], R.act_grad_ref(x, act) * keep * scale, f"{cid} pre_act (gelu')", 8e-3, form[1])
    if P is not None:
        _exact(P[:rows].cpu(), _round_out(pre, out), f"{cid} pre_act")
    if act in (R.ACT_NONE, R.ACT_RELU) and p in (0.0, 0.5):
        return _exact(C, _round_out(R.act_ref(pre, act) * keep.double() * scale, out), f"{cid} C")
    if act in (R.ACT_NONE, R.ACT_RELU):                      # p = 0.3: the scale is no power of two - the MASK is still exact
        zero = ~keep | (R.act_ref(pre, act) == 0)
        probe = R.thresh_probe(c, i) & ~zero
        assert int(probe.sum()) >= 2 and bool((C[probe] != 0).all()), f"{cid}: the threshold is not uint32(p * 65536), truncated"
        assert torch.equal(C == 0, zero), f"{cid}: {int(((C == 0) != zero).sum())} elements kept / dropped against keep_mask"
        return _close(C, R.act_ref(pre, act) * keep * scale, f"{cid} C (p = {p})", 8e-3 if out == BF16 else 1e-4)
    assert bool((C[~keep] == 0).all()), f"{cid}: dropped elements are not 0"
    extra = 0.0
    if act == R.ACT_GELU and c["dtype"] == BF16:
        extra = float((R.gelu_fast_form(x, scale)[0].double() - scale * R.act_ref(x, act)).abs().max())
        assert extra <= GELU_FORM_ABS * scale, extra
    _close(C, R.act_ref(x, act) * keep * scale, f"{cid} C (act {act})", 8e-3 if out == BF16 else 1e-4, extra)


@pytest.mark.parametrize("cid", [c["id"] for c in NT_CASES])
def test_nt_case(dev, cid):
    """One row of NT_CASES on the kernel the mirror names for it: exact where the epilogue is linear, one bf16 rounding (plus the
    CPU-measured distance of the kernel's GELU form) otherwise; sentinel rows untouched, every live element written, operands
    unchanged (module doc)."""
    c, i = _nt_prepared(cid)
    assert isinstance(R.nt_case_path(c, _ncu()), dict)
    rc, C, P = _nt_call(c, i, dev)
    assert rc == 0, rc
    _nt_check(c, i, C, P)


@pytest.mark.parametrize("a,b", NT_TWINS)
def test_nt_same_problem_on_two_kernels(dev, a, b):
    """Where the mirror sends one problem to two kernels (a tile queue on a grid too small for queue4_ok moves nt4r's calls to
    nt2x) or to two walks of one (static and queue), the results are equal bit for bit - GELU outputs included."""
    (ca, ia), (cb, ib) = _nt_prepared(a), _nt_prepared(b)
    assert torch.equal(ia["A"], ib["A"]) and torch.equal(ia["W"], ib["W"]) and ia["seed"] == ib["seed"]
    pa, pb = R.nt_case_path(ca, _ncu()), R.nt_case_path(cb, _ncu())
    assert (pa["path"], ca["queue"]) != (pb["path"], cb["queue"])
    rca, Ca, Pa = _nt_call(ca, ia, dev)
    rcb, Cb, Pb = _nt_call(cb, ib, dev)
    assert rca == 0 and rcb == 0
    _exact(Ca, Cb, f"{a} / {b} C")
    if Pa is not None:
        _exact(Pa, Pb, f"{a} / {b} pre_act")


@pytest.mark.parametrize("name", [n for n, _, _ in NT_REFUSED])
def test_nt_refused(dev, name):
    """A call the entry point must decline returns its exact code and leaves the outputs untouched."""
    _, c, rc = next(r for r in NT_REFUSED if r[0] == name)
    assert R.nt_case_path(c, _ncu()) == rc
    c = dict(c)
    ldw = c["ldw"]
    i = R.nt_inputs(dict(c, ldw=max(ldw, c["K"])))          # (W as wide as K at least: the call is refused before it is read)
    got, C, P = _nt_call(c, i, dev)
    assert got == rc, (name, got, rc)
    rows = int(i["offs"][-1])
    assert bool(C[:rows].isnan().all()) and bool((C[rows:] == SENT).all()), f"{name}: C was written"
    assert P is None or (bool(P[:rows].isnan().all()) and bool((P[rows:] == SENT).all())), f"{name}: pre_act was written"


# ---------------------------------------------------------------------------------------------------------------------------
# TN
@functools.lru_cache(maxsize=None)
def _tn_prepared(cid):
    c = {c["id"]: c for c in TN_CASES + TN_PAIR_CASES}[cid]
    ops, offs = R.tn_inputs(c)
    return c, ops, offs, [R.tn_ref(A, B, offs) for A, B in ops]


def _tn_call(c, ops, offs, dev, form, ws=None):
    """One call of apertis_grouped_gemm_tn_q / _tn_pair_q; returns (rc, [(dW, dbias or None)], ws)."""
    lib, ptr, sp = _api()
    E, rows = len(c["sizes"]), max(sum(c["sizes"]), 1)
    dops = [(A.to(dev), B.to(dev)) for A, B in ops]
    outs = [(torch.full((E, A.shape[1], B.shape[1]), NAN, device=dev), torch.full((E, A.shape[1]), NAN, device=dev) if c["dbias"] else None)
            for A, B in ops]
    offs_d = offs.to(dev)
    if form != "nows" and ws is None:
        nbytes = max(int(lib.apertis_grouped_gemm_tn_workspace_bytes(E, len(ops))), 1024)
        ws = torch.full((nbytes // 4,), NAN, device=dev)               # contents don't care: NaN would show in a sum
    wsp, wsb = (ptr(ws), ws.numel() * 4) if form != "nows" else (None, 0)
    q = 1 if form == "queue" else 0
    (A0, B0), (W0, b0) = dops[0], outs[0]
    if c["pair"]:
        (A1, B1), (W1, b1) = dops[1], outs[1]
        rc = lib.apertis_grouped_gemm_tn_pair_q(ptr(A0), ptr(B0), ptr(W0), ptr(b0) if b0 is not None else None, A0.shape[1], B0.shape[1],
                                                ptr(A1), ptr(B1), ptr(W1), ptr(b1) if b1 is not None else None, A1.shape[1], B1.shape[1],
                                                ptr(offs_d), rows, E, wsp, wsb, _dtc(c["dtype"]), q, sp())
    else:
        rc = lib.apertis_grouped_gemm_tn_q(ptr(A0), ptr(B0), ptr(offs_d), ptr(W0), ptr(b0) if b0 is not None else None, rows,
                                           A0.shape[1], B0.shape[1], E, wsp, wsb, _dtc(c["dtype"]), q, sp())
    torch.cuda.synchronize()
    for (A, B), (Ad, Bd) in zip(ops, dops):
        assert torch.equal(Ad.cpu(), A) and torch.equal(Bd.cpu(), B), "operands changed"
    return rc, outs, ws


def _tn_check(c, outs, refs, name):
    for k, ((dW, db), (rW, rb)) in enumerate(zip(outs, refs)):
        _exact(dW, rW.float(), f"{name} dW{k}")
        if db is not None:
            _exact(db, rb.float(), f"{name} dbias{k}")


@pytest.mark.parametrize("cid", [c["id"] for c in TN_CASES + TN_PAIR_CASES])
def test_tn_case(dev, cid):
    """dW and dbias equal the float64 reference EXACTLY in every form the row names (workspace, workspace with the item queue, no
    workspace - hence equal to each other), NaN-prefilled outputs are fully written (groups without rows: zeros), and a second
    call on the same, now dirty, workspace gives the same."""
    c, ops, offs, refs = _tn_prepared(cid)
    for form in c["forms"]:
        assert isinstance(R.tn_case_path(c, form, _ncu()), dict)
        rc, outs, ws = _tn_call(c, ops, offs, dev, form)
        assert rc == 0, (form, rc)
        _tn_check(c, outs, refs, f"{cid} {form}")
        if form != "nows":
            rc, outs, _ = _tn_call(c, ops, offs, dev, form, ws)
            assert rc == 0
            _tn_check(c, outs, refs, f"{cid} {form} (dirty workspace)")


@pytest.mark.parametrize("name", [n for n, _, _ in TN_REFUSED])
def test_tn_refused(dev, name):
    _, c, rc = next(r for r in TN_REFUSED if r[0] == name)
    ops, offs = R.tn_inputs(dict(c, M=max(c["M"], 8)))
    if c["M"] <= 0:
        lib, ptr, sp = _api()
        A, B, W = ops[0][0].to(dev), ops[0][1].to(dev), torch.full((8,), NAN, device=dev)
        got = lib.apertis_grouped_gemm_tn_q(ptr(A), ptr(B), ptr(offs.to(dev)), ptr(W), None, sum(c["sizes"]), c["M"], c["N"],
                                            len(c["sizes"]), None, 0, _dtc(c["dtype"]), 0, sp())
        torch.cuda.synchronize()
        assert got == rc and bool(W.isnan().all())
        return
    for form in ("nows", "ws"):
        got, outs, _ = _tn_call(c, ops, offs, dev, form)
        assert got == rc, (name, form, got, rc)
        assert all(bool(dW.isnan().all()) and (db is None or bool(db.isnan().all())) for dW, db in outs), f"{name}: outputs written"


# ---------------------------------------------------------------------------------------------------------------------------
# the elementwise backward
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("act,p", [(R.ACT_RELU, 0.5), (R.ACT_GELU, 0.5), (R.ACT_RELU, 0.3)])
def test_act_dropout_bwd(dev, dt, act, p):
    """apertis_act_dropout_bwd regenerates the forward's mask: with ReLU and p = 0.5 dpre is exactly 0 or 2 dh, by keep_mask and
    the sign of pre; with p = 0.3 the kept / dropped pattern is exact (the threshold truncated, module doc of gemm_ref) and the
    values are within one rounding; with GELU within one rounding of float64 (fp32: 1e-4) plus the CPU-measured distance of the
    bf16 path's form.  Rows at and past offsets[E] keep their sentinel.  3 000 rows of 132 in three groups (one empty): a grid-stride
    loop of several blocks with a ragged tail, and enough elements for a handful to sit exactly on the threshold."""
    lib, ptr, sp = _api()
    g = torch.Generator().manual_seed(77 + act)
    sizes, N, max_rows, seed = (5, 0, 2995), 132, 3040, 0x9E3779B97F4A7C15
    rows, scale = sum(sizes), 1.0 / (1.0 - p)
    offs = torch.tensor([0, 5, 5, 3000], dtype=torch.int32)
    dh, pre = R.dyadic((max_rows, N), 16, g).to(dt), R.dyadic((max_rows, N), 16, g, bound=40).to(dt)
    out = torch.full((max_rows, N), SENT, dtype=dt, device=dev)
    out[:rows] = NAN
    dh_d, pre_d = dh.to(dev), pre.to(dev)
    rc = lib.apertis_act_dropout_bwd(ptr(dh_d), ptr(pre_d), ptr(out), ptr(offs.to(dev)), max_rows, N, len(sizes), act, p, seed,
                                     _dtc(dt), sp())
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(dh_d.cpu(), dh) and torch.equal(pre_d.cpu(), pre)
    assert bool((out[rows:] == SENT).all()), "rows at or past offsets[E] were written"
    keep = torch.from_numpy(R.keep_mask(seed, rows, N, p))
    got = out[:rows].cpu()
    x = pre[:rows].double()
    ref = dh[:rows].double() * R.act_grad_ref(x, act) * keep * scale
    if act == R.ACT_RELU and p == 0.5:
        return _exact(got, _round_out(ref, dt), "dpre")
    if act == R.ACT_RELU:
        probe = torch.from_numpy(R.keep_mask(seed, rows, N, p) != R.keep_mask(seed, rows, N, p, thresh=R.thresh16(p) + 1)) & (ref != 0)
        assert int(probe.sum()) >= 2 and bool((got[probe] != 0).all()), "the threshold is not uint32(p * 65536), truncated"
        assert torch.equal(got == 0, ref == 0), f"{int(((got == 0) != (ref == 0)).sum())} elements kept / dropped against keep_mask"
        return _close(got, ref, "dpre", 8e-3 if dt == BF16 else 1e-4)
    assert bool((got[~keep] == 0).all())
    extra = 0.0
    if dt == BF16:
        form = float((R.gelu_fast_form(x)[1].double() - R.act_grad_ref(x, act)).abs().max())
        assert form <= GELU_GRAD_FORM_ABS
        extra = scale * form * float(dh.abs().max())
    _close(got, ref, "dpre", 8e-3 if dt == BF16 else 1e-4, extra)


# ---------------------------------------------------------------------------------------------------------------------------
# the mirror held to the library
def test_profiler_sees_the_kernels_the_mirror_names(dev):
    """Every accepted row of the tables, run once inside ONE profiler session: the device kernels whose names contain
    grouped_gemm_, tn3_fold_k or tn5_fold_k, in start order, are exactly the sequence the mirror predicts, template arguments
    included where the name shows them.  A stock torch kernel launched first tells a blind profiler (skip) from one that sees
    torch's kernel but not ours (failure).
    How the names come back depends on the profiler's demangler (gemm_ref.kernel_name_targs).  Seen on an MI355X with torch 2.10
    / ROCm 7.0, over all 169 launches: fp32 and non-template kernels demangled in full; a bf16 kernel whose first value argument is
    0 / false / 4 / 16 still MANGLED (every argument legible: nt4r<*, false, *>, nt2x<false>, nt256p<false>, nt352p,
    nt_k<bf16, *>, nt_skinny<4 | 16>); a bf16 kernel whose first value argument is 1 / true GARBLED ("<bool _Accum, bool, E, false>":
    the demangler, not knowing the type code DF16b, swallows the literal behind it) with only later booleans intact - nt4r<*, true, *>,
    nt2x<true>, nt256p<true>, nt_skinny<1>, 21 launches.  So a garbled name is held to a mirror's prediction whose first
    value argument is true / 1 and whose later booleans are the legible ones: together with the mangled and demangled names
    that pins every template argument on this build.  The FIGURE lines say, per kernel, how many launches came back in which form.
    """
    from torch.profiler import ProfilerActivity, profile
    ncu, expected = _ncu(), []
    jobs = []
    for c in NT_CASES:
        jobs.append(("nt", _nt_prepared(c["id"]), None))
        expected += [(c["id"],) + l for l in R.nt_case_path(c, ncu)["launches"]]
    for c in TN_CASES + TN_PAIR_CASES:
        for form in c["forms"]:
            jobs.append(("tn", _tn_prepared(c["id"]), form))
            expected += [(f"{c['id']} {form}",) + l for l in R.tn_case_path(c, form, ncu)["launches"]]
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        probe = torch.arange(4096, device=dev, dtype=torch.float32).cos().sum()
        torch.cuda.synchronize()
        for kind, prep, form in jobs:
            if kind == "nt":
                assert _nt_call(prep[0], prep[1], dev)[0] == 0
            else:
                assert _tn_call(prep[0], prep[1], prep[2], dev, form)[0] == 0
        torch.cuda.synchronize()
    assert float(probe) == float(probe)
    device = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    if not device:
        pytest.skip("torch.profiler returned no device event at all, not even for torch's own kernel")
    ours = sorted((e for e in device if any(s in e.name for s in ("grouped_gemm_", "tn3_fold_k", "tn5_fold_k"))),
                  key=lambda e: e.time_range.start)
    assert ours, f"the profiler sees {len(device)} device events of torch's but none of the library's kernels"
    got = []
    for e in ours:
        kernel = next(k for k in sorted(R.ALL_KERNELS, key=len, reverse=True) if k in e.name)
        got.append((kernel,) + R.kernel_name_targs(e.name, kernel) + (e.name,))
    for n in sorted({g[3] for g in got}):
        print(f"FIGURE profiler name: {n[:200]}")
    forms = {}
    for kernel, args, complete, name in got:
        form = "garbled" if not complete else "mangled" if name.startswith("_Z") else "demangled"
        forms.setdefault(kernel, {}).setdefault(form, 0)
        forms[kernel][form] += 1
    for kernel in sorted(forms):
        print(f"FIGURE profiler {kernel}: " + ", ".join(f"{n} {form}" for form, n in sorted(forms[kernel].items())) +
              ("  (garbled: first value argument 1 / true, later booleans legible)" if "garbled" in forms[kernel] else ""))
    print(f"FIGURE profiler: {len(device)} device events, {len(got)} of the grouped GEMM's, {len(expected)} expected")
    for k, (exp, g) in enumerate(zip(expected, got)):
        shown = tuple(exp[2]) if g[2] else tuple(exp[2])[len(exp[2]) - len(g[1]):]
        assert g[2] or (len(exp[2]) > 1 and exp[2][1] in (True, 1) and len(g[1]) <= len(exp[2]) - 2), \
            f"launch {k} ({exp[0]}): a garbled name ({g[3][:120]}) where the mirror expects {exp[1:]}"
        assert exp[1] == g[0] and shown == g[1], f"launch {k} ({exp[0]}): expected {exp[1:]}, the device ran {g[:2]}: {g[3][:200]}"
    assert len(got) == len(expected), (len(got), len(expected), got[len(expected):][:3], expected[len(got):][:3])
