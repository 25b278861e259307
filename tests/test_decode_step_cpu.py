"""tests/decode_step_ref.py without a device: its float64 references against torch's own functions in float64, its dyadic grid
against exact integer arithmetic, and its case tables against its mirror of the entry points' dispatch."""
import copy

import pytest
import torch
import torch.nn.functional as F

import decode_step_ref as R


def _eq(a, b, tol=1e-12):
    assert a.shape == b.shape and float((a.double() - b.double()).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def test_elementwise_references_against_torch():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1000, generator=g, dtype=torch.float64) * 6
    _eq(R.silu(x), F.silu(x))
    _eq(R.softplus(x), F.softplus(x, threshold=1e9))
    _eq(R.softplus(x), F.softplus(x), tol=3e-9)               # torch's default threshold 20 (the kernel's form)
    big = torch.tensor([-800.0, 800.0], dtype=torch.float64)
    assert torch.equal(R.softplus(big), torch.tensor([0.0, 800.0], dtype=torch.float64))


def test_conv_reference_is_the_first_output_of_the_padded_conv():
    """The front-slice quirk: conv1d over [window | xp] with padding k - 1, FIRST output kept - only window[0] meets a tap."""
    g = torch.Generator().manual_seed(2)
    for k in (2, 3, 4, 16):
        NL, B, Dn = 3, 2, 5
        win = torch.randn(NL, B, Dn, k - 1, generator=g, dtype=torch.float64)
        xp = torch.randn(NL, B, Dn, generator=g, dtype=torch.float64)
        w, b = torch.randn(NL, Dn, k, generator=g, dtype=torch.float64), torch.randn(NL, Dn, generator=g, dtype=torch.float64)
        full = torch.cat([win, xp.unsqueeze(-1)], dim=-1)
        for l in range(NL):
            y = F.conv1d(full[l], w[l].unsqueeze(1), b[l], padding=k - 1, groups=Dn)[..., 0]
            _eq(R.conv_ref(win, w, b)[l], F.silu(y))
        new = R.push_ref(win, xp)
        assert new.shape == win.shape and torch.equal(new, full[..., 1:])


def test_state_reference_against_a_plain_loop():
    g = torch.Generator().manual_seed(3)
    NL, B, h, N, Rk = 3, 2, 3, 4, 5
    Dn = h * N
    x = torch.randn(NL, B, Rk, generator=g, dtype=torch.float64)
    W, bd = torch.randn(NL, h, Rk, generator=g, dtype=torch.float64), torch.randn(NL, h, generator=g, dtype=torch.float64)
    A, D = torch.randn(NL, h, N, generator=g, dtype=torch.float64), torch.randn(NL, Dn, generator=g, dtype=torch.float64)
    Bt, C, xc, s0 = (torch.randn(NL, B, Dn, generator=g, dtype=torch.float64) for _ in range(4))
    for sp in (True, False):
        for bias in (bd, None):
            s, pre = R.state_ref(x, W, bias, A, Bt, C, D, xc, s0, sp)
            for l in range(NL):
                dl = F.linear(x[l], W[l], None if bias is None else bias[l])
                dl = F.softplus(dl, threshold=1e9) if sp else dl
                for b in range(B):
                    for c in range(Dn):
                        a = torch.exp(-torch.exp(A[l].reshape(-1)[c]) * dl[b, c // N])
                        sv = a * s0[l, b, c] + Bt[l, b, c]
                        assert abs(float(s[l, b, c] - sv)) <= 1e-12 * max(1.0, abs(float(sv)))
                        pv = C[l, b, c] * sv + D[l, c] * xc[l, b, c]
                        assert abs(float(pre[l, b, c] - pv)) <= 1e-12 * max(1.0, abs(float(pv)))
    _eq(R.gate_ref(pre, xc), pre * F.silu(xc))


def test_gemv_and_boundary_references_against_torch():
    g = torch.Generator().manual_seed(4)
    x, W, b = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((5, 24), (12, 32), (12,)))
    _eq(R.gemv_ref(x, W, b, 24), F.linear(x, W[:, :24], b))
    _eq(R.gemv_ref(x, W, None, 24), F.linear(x, W[:, :24]))
    H = 40
    res, blk = torch.randn(3, 1, H, generator=g), torch.randn(3, H, generator=g).bfloat16()
    ga, be = torch.randn(H, generator=g), torch.randn(H, generator=g)
    y, xn = R.boundary_ref(res, blk, ga, be, 1e-5)
    assert y.dtype == torch.float32 and torch.equal(y, res.reshape(3, H) + blk.float())
    _eq(xn, F.layer_norm(y.double(), (H,), ga.double(), be.double(), 1e-5))
    yr, wk = R.dyadic((4, H), 16, g).bfloat16(), R.dyadic((3, 2), 8, g, bound=7)
    slot = torch.tensor([[0, -1], [3, 1], [-1, -1]], dtype=torch.int32)
    comb = R.combine_ref(yr, wk, slot)
    _eq(comb[0], wk[0, 0].double() * yr[0].double())
    _eq(comb[1], wk[1, 0].double() * yr[3].double() + wk[1, 1].double() * yr[1].double())
    assert float(comb[2].abs().max()) == 0.0
    y2, _ = R.boundary_ref(res, yr, ga, be, 1e-5, (wk, slot))
    assert torch.equal(y2, res.reshape(3, H) + comb.float().bfloat16().float())


def test_dyadic_grid_sums_are_exact_in_fp32_in_any_order():
    """The claim the bit-for-bit assertions rest on: on the grid a K <= 1024 dot product plus bias fits an fp32 significand at
    every partial sum, so fp32 accumulation in any order equals the integer sum; checked with int64 arithmetic, forwards,
    backwards and in four K quarters (the in_proj kernel's grouping)."""
    assert R.dyadic_sum_bits(1024) <= 24 and R.dyadic_sum_bits(504) <= 24
    x, W, b = R.dyadic_gemv_inputs(16, 1024, 20, True, seed=5)
    assert torch.equal(x.bfloat16().float(), x) and torch.equal(W.bfloat16().float(), W)
    xi, Wi, bi = (x * 16).long(), (W * 32).long(), (b * 64).long()
    exact = (xi @ Wi.t() + 8 * bi).double() / 512
    assert torch.equal(R.gemv_ref(x, W, b, 1024), exact)
    f = torch.zeros(16, 20)
    for k in range(1024):
        f += x[:, k:k + 1] * W[:, k].unsqueeze(0)
    r = torch.zeros(16, 20)
    for k in reversed(range(1024)):
        r += x[:, k:k + 1] * W[:, k].unsqueeze(0)
    q = sum((x[:, i:i + 256] @ W[:, i:i + 256].t()) for i in (768, 512, 256, 0))
    for v in (f, r, q):
        assert torch.equal((v + b).double(), exact)
    assert torch.equal(R.round_bf16(exact), (f + b).bfloat16())
    # worst case: every product at its bound
    assert float(torch.tensor(961.0 * 1024 + 248)) == 961 * 1024 + 248


def test_dispatch_mirror():
    assert R.gemv_rc(1, 64, 64, 56) == R.ERR_ARG and R.gemv_rc(16, 504, 4, 504) == 0 and R.gemv_rc(1, 8, 4, 8) == 0
    assert [R.gemv_path(1, K, 16, K)["k_batches"] for K in (8, 256, 264, 504)] == [1, 1, 2, 2]
    assert [R.inproj_path(1, H, 64)["IT"] for H in (512, 520, 768, 776, 1024)] == [2, 3, 3, 4, 4]
    assert R.inproj_path(1, 520, 64)["kq"] == 160 and R.inproj_path(1, 520, 64)["last_ragged"]
    assert not R.inproj_path(1, 704, 64)["last_ragged"] and R.inproj_path(1, 704, 64)["last_short"]
    assert R.inproj_path(1, 512, 130)["straddle"] and R.inproj_path(1, 512, 130)["n_partial"]
    assert [R.shift_path(k) for k in (2, 3, 4, 15, 16)] == ["none", "one", "some", "some", "all"]
    assert R.elem_path(256) == (1, False) and R.elem_path(257) == (2, True)
    assert R.inproj_rc(16, 1024, 4, 1024, 16) == 0 and R.inproj_rc(1, 512, 128, 504) == R.ERR_UNSUPPORTED


def test_case_tables_cover_every_dispatch_path():
    R.check_case_tables_cover_every_dispatch_path()


@pytest.mark.parametrize("table", ["ELEM_CASES", "STATE_CASES", "GEMV_CASES", "INPROJ_CASES", "BOUNDARY_CASES", "XZ_CASES",
                                   "CHAIN_CASES", "GEMV_REFUSED", "INPROJ_REFUSED"])
def test_coverage_check_fails_when_a_row_is_removed(table, monkeypatch):
    """Every row of every table is needed: the coverage check fails without any one of them."""
    rows = copy.copy(getattr(R, table))
    for i in range(len(rows)):
        monkeypatch.setattr(R, table, rows[:i] + rows[i + 1:])
        with pytest.raises(AssertionError):
            R.check_case_tables_cover_every_dispatch_path()
    monkeypatch.setattr(R, table, rows)
    R.check_case_tables_cover_every_dispatch_path()
