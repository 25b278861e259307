"""tests/gemm_ref.py without a device: its float64 references against torch's own functions in float64, its dyadic grid against
exact integer arithmetic, its dropout masks against scalar transcriptions of csrc/grouped_gemm.hip's gd_keep / gd_keep4 and
csrc/common.h's drop_keep / drop_keep4, its mirror of launch_nt and of the TN entry points on hand-computed points, and its case
tables against the mirror."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gemm_ref as R
from gemm_ref import ACT_GELU, ACT_NONE, ACT_RELU, ACT_SILU, BF16, ERR_ARG, ERR_UNSUPPORTED, F32, MUL_SAVED, SAVE_GRAD


def _eq(a, b, tol=1e-12):
    assert a.shape == b.shape
    assert a.numel() == 0 or float((a.double() - b.double()).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def test_references_against_torch():
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(2000, generator=g, dtype=torch.float64) * 4).requires_grad_(True)
    for act, fn in ((ACT_GELU, F.gelu), (ACT_RELU, F.relu), (ACT_SILU, F.silu), (ACT_NONE, lambda v: v * 1.0)):
        y = fn(x)
        _eq(R.act_ref(x.detach(), act), y.detach())
        (gr,) = torch.autograd.grad(y.sum(), x)
        _eq(R.act_grad_ref(x.detach(), act), gr)
    sizes = (0, 3, 1, 0, 5)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32))
    A = torch.randn(12, 10, generator=g, dtype=torch.float64)              # three rows past offsets[E]
    W, b = torch.randn(5, 6, 16, generator=g, dtype=torch.float64), torch.randn(5, 6, generator=g, dtype=torch.float64)
    pre = R.nt_pre_ref(A, W, b, offs, 10)
    assert pre.shape == (9, 6)
    for e in range(5):
        r0, r1 = int(offs[e]), int(offs[e + 1])
        _eq(pre[r0:r1], F.linear(A[r0:r1], W[e][:, :10], b[e]))
    _eq(R.nt_pre_ref(A, W, None, offs, 10)[4:9], F.linear(A[4:9], W[4][:, :10]))
    keep = torch.from_numpy(R.keep_mask(7, 9, 6, 0.5))
    _eq(R.nt_ref(A, W, b, offs, 10, ACT_GELU, 0.5, 7), F.gelu(pre) * keep * 2.0)
    _eq(R.nt_ref(A, W, b, offs, 10, ACT_SILU, 0.0, 7, round_pre=True), F.silu(pre.float().bfloat16().double()))
    B = torch.randn(9, 4, generator=g, dtype=torch.float64)
    dW, db = R.tn_ref(A[:9], B, offs)
    assert dW.shape == (5, 10, 4) and db.shape == (5, 10)
    for e in range(5):
        r0, r1 = int(offs[e]), int(offs[e + 1])
        _eq(dW[e], A[r0:r1].t() @ B[r0:r1])
        _eq(db[e], A[r0:r1].sum(0))
    assert float(dW[0].abs().max()) == 0.0 and float(db[3].abs().max()) == 0.0


def test_gelu_fast_form_is_close_to_gelu():
    """The fp32 transcription of the bf16 kernels' GELU form (gelu_terms): within the 2.8e-5 / 1.2e-5 per unit of scale that the
    GPU test caps it at, over the range the tables' pre-activations cover (|x| <= 3), and with the scale folded in."""
    x = torch.linspace(-3, 3, 6001, dtype=torch.float64)
    for s in (1.0, 2.0):
        g, dg = R.gelu_fast_form(x, s)
        assert g.dtype == F32
        assert float((g.double() - s * R.act_ref(x, ACT_GELU)).abs().max()) <= 2.8e-5 * s
        assert float((dg.double() - s * R.act_grad_ref(x, ACT_GELU)).abs().max()) <= 1.2e-5 * s


def test_dyadic_grid_sums_are_exact_in_fp32_in_any_order():
    """The claim the bit-for-bit assertions rest on: on the grid a dot product of depth D <= 17 457 plus a bias fits an fp32
    significand at every partial sum, so fp32 accumulation forwards, backwards and in slices folded afterwards equals the int64
    sum; and the single bf16 rounding of that value is the reference's."""
    assert R.MAX_DEPTH == 17457 and R.dyadic_sum_bits(R.MAX_DEPTH) == 24 and R.dyadic_sum_bits(R.MAX_DEPTH + 1) == 25
    assert 961 * R.MAX_DEPTH + 248 < 2 ** 24 <= 961 * (R.MAX_DEPTH + 1) + 248
    assert float(torch.tensor(961.0 * R.MAX_DEPTH + 248)) == 961 * R.MAX_DEPTH + 248         # the worst case is itself an fp32 number
    D = 2824                                                                                 # the deepest K of the tables
    assert max(c["K"] for c in R.NT_CASES) == D
    g = torch.Generator().manual_seed(5)
    x, W, b = R.dyadic((9, D), 16, g), R.dyadic((20, D), 32, g), R.dyadic((20,), 64, g)
    x[0], W[0] = 31 / 16, 31 / 32                                                            # one sum at the bound
    assert torch.equal(x.bfloat16().float(), x) and torch.equal(W.bfloat16().float(), W)
    xi, Wi, bi = (x * 16).long(), (W * 32).long(), (b * 64).long()
    exact = (xi @ Wi.t() + 8 * bi).double() / 512
    assert int((xi @ Wi.t() + 8 * bi).abs().max()) == 961 * D + 8 * int(bi[0]) < 2 ** 24
    offs = torch.tensor([0, 9], dtype=torch.int32)
    assert torch.equal(R.nt_pre_ref(x, W.unsqueeze(0), b.unsqueeze(0), offs, D), exact)
    fwd, rev = torch.zeros(9, 20), torch.zeros(9, 20)
    for k in range(D):
        fwd += x[:, k:k + 1] * W[:, k].unsqueeze(0)
    for k in reversed(range(D)):
        rev += x[:, k:k + 1] * W[:, k].unsqueeze(0)
    parts = [x[:, i:i + 192] @ W[:, i:i + 192].t() for i in range(0, D, 192)]                # 15 slices, the last one short
    fold = parts[0].clone()
    for q in parts[1:]:
        fold += q
    for v in (fwd, rev, fold):
        assert torch.equal((v + b).double(), exact)
    assert torch.equal(R.round_bf16(exact), (fwd + b).bfloat16())
    # the TN direction: depth = a group's rows; dbias sums n/16 alone
    A, B = R.dyadic((1300, 24), 16, g), R.dyadic((1300, 16), 32, g)
    dW, db = R.tn_ref(A, B, torch.tensor([0, 1300], dtype=torch.int32))
    assert torch.equal(dW[0], ((A * 16).long().t() @ (B * 32).long()).double() / 512)
    assert torch.equal(db[0], (A * 16).long().sum(0).double() / 16)
    assert torch.equal(dW.float().double(), dW) and torch.equal(db.float().double(), db)
    assert max(max(c["sizes"] + (0,)) for c in R.TN_CASES + R.TN_PAIR_CASES) <= R.MAX_DEPTH


# ---------------------------------------------------------------------------------------------------------------------------
# scalar transcriptions of the device functions (Python integers, masked to 32 bits)
M32 = 0xFFFFFFFF


def _fmix(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def _gd_pair(seed, row, cpair):
    rowmix = _fmix(((row & M32) * 0x9E3779B9 + (row >> 32) * 0x7F4A7C15 + (seed & M32)) & M32)
    colmix = _fmix(((cpair * 0x85EBCA77) & M32) ^ (seed >> 32))
    x = ((rowmix ^ colmix) * 0x2C1B3C6D) & M32
    return x ^ (x >> 15)


def gd_keep(seed, row, col, thresh):
    h = _gd_pair(seed, row, col >> 1)
    return ((h >> 16) if col & 1 else (h & 0xFFFF)) >= thresh


def gd_keep4(seed, row, col0, thresh):
    h0, h1 = _gd_pair(seed, row, col0 >> 1), _gd_pair(seed, row, (col0 >> 1) + 1)
    return [(h0 & 0xFFFF) >= thresh, (h0 >> 16) >= thresh, (h1 & 0xFFFF) >= thresh, (h1 >> 16) >= thresh]


def drop_keep(seed, row, col, ncols, thresh):
    lin = row * ncols + col
    h = ((lin >> 1) & M32) ^ (seed & M32)
    h = (h + ((lin >> 33) & M32) * 0x9E3779B9 + (seed >> 32)) & M32
    h = _fmix(h)
    return ((h >> 16) if lin & 1 else (h & 0xFFFF)) >= thresh


def drop_keep4(seed, lin0, thresh):
    def pair(p):
        h = ((p & M32) ^ (seed & M32)) + (seed >> 32) + (p >> 32) * 0x9E3779B9
        return _fmix(h & M32)
    h0, h1 = pair(lin0 >> 1), pair((lin0 >> 1) + 1)
    return [(h0 & 0xFFFF) >= thresh, (h0 >> 16) >= thresh, (h1 & 0xFFFF) >= thresh, (h1 >> 16) >= thresh]


@pytest.mark.parametrize("seed", [0, 0x9E3779B97F4A7C15, 12345 << 32 | 99])
def test_keep_masks_against_scalar_transcriptions(seed):
    """keep_mask is gd_keep element by element and gd_keep4 four at a time; keep_mask_linear is drop_keep / drop_keep4.  The
    threshold is truncated: p = 0.3 gives 19660, not 19661."""
    assert R.thresh16(0.5) == 32768 and R.thresh16(0.3) == 19660 and R.thresh16(0.1) == 6553 and R.thresh16(0.0) == 0
    for p in (0.5, 0.3):
        t = R.thresh16(p)
        rows, N, row0 = 7, 20, 3
        m = R.keep_mask(seed, rows, N, p, row0=row0)
        assert m.shape == (rows, N) and m.dtype == np.bool_
        for r in range(rows):
            for c in range(N):
                assert m[r, c] == gd_keep(seed, row0 + r, c, t)
            for c0 in range(0, N, 4):
                assert list(m[r, c0:c0 + 4]) == gd_keep4(seed, row0 + r, c0, t)
        lin = R.keep_mask_linear(seed, rows, N, p)
        for r in range(rows):
            for c in range(N):
                assert lin[r, c] == drop_keep(seed, r, c, N, t)
            for c0 in range(0, N, 4):
                assert list(lin[r, c0:c0 + 4]) == drop_keep4(seed, r * N + c0, t)
    big = R.keep_mask(seed, 512, 512, 0.5)
    assert abs(float(big.mean()) - 0.5) < 0.01                        # a mask, not a constant
    assert np.array_equal(R.keep_mask(seed, 512, 514, 0.5)[:, :512], big)      # N does not enter gd_keep
    assert gd_keep(seed, 2 ** 33 + 5, 7, 32768) == bool(R.keep_mask(seed, 1, 8, 0.5, row0=2 ** 33 + 5)[0, 7])


# ---------------------------------------------------------------------------------------------------------------------------
def _nt(max_rows, N, K, E=8, act=ACT_NONE, p=0.0, pre=False, mul=False, bias=True, queue=False, ldw=0, dt=BF16, out=BF16, ncu=256):
    r = R.nt_path(dt, out, max_rows, N, K, ldw, E, act, p, pre, mul, bias, queue, ncu)
    return r if not isinstance(r, dict) else r["path"]


def test_nt_mirror_on_hand_computed_points():
    """launch_nt at the shapes its own comments quote, and at each side of every threshold."""
    big = 225280
    # the skinny kernel: <= 64 rows; K < 512 one wave, < 2048 four, else sixteen
    assert [_nt(16, 704, K) for K in (176, 504, 512, 2040, 2048, 2816)] == \
        ["nt_skinny<bf16,1>"] * 2 + ["nt_skinny<bf16,4>"] * 2 + ["nt_skinny<bf16,16>"] * 2
    assert _nt(64, 704, 176) == "nt_skinny<bf16,1>" and _nt(65, 704, 176) == "nt<bf16,bf16>"
    assert _nt(16, 704, 176, act=ACT_GELU) == "nt_skinny<bf16,1>" and _nt(16, 704, 176, p=0.5) == "nt<bf16,bf16>"
    assert R.nt_path(BF16, BF16, 16, 704, 2816, 0, 8, 0, 0.0, False, False, True, False, 256)["k_share"] == 192   # six 32-deep steps
    # the SSM block's dense projections (E = 1): N = 352, K = 704 on the 352-wide tile, the others on the ring kernel
    assert _nt(big, 352, 704, E=1) == "nt352p<bf16>"
    # (K = 176 is ragged against the 32-deep step: the weights' compute copies carry a pitch of 192)
    assert [_nt(big, N, K, E=1, ldw=-(-K // 64) * 64) for N, K in ((704, 176), (704, 352), (448, 176), (400, 176), (176, 448), (176, 704))] == \
        ["nt4r<bf16,True,False>", "nt4r<bf16,False,False>", "nt4r<bf16,True,False>", "nt4r<bf16,True,False>"] + ["nt4r<bf16,False,False>"] * 2
    assert _nt(big, 704, 176, E=1) == "nt<bf16,bf16>"                            # ... and without it no persistent kernel takes them
    assert _nt(big, 352, 704, E=1, ldw=768) == "nt4r<bf16,False,False>"          # a pitch of its own: not the 352-wide tile
    assert _nt(big, 64, 256, E=1) == "nt2x<bf16,False>" and _nt(big, 56, 256, E=1) == "nt<bf16,bf16>"
    assert _nt(big, 128, 128, E=1) == "nt256p<bf16,False>"                       # K > 128 for the ring kernel, N >= 256 for use2x
    # the experts: fc2 forward / fc1 data gradient at N = 704 on the 352-wide tile; fc1 forward (GELU, saved gradient) and the
    # fused fc2 data gradient (N = 2816, K = 704) on the ring kernel; plain N = 2816 on the 256 x 256 kernel
    assert _nt(big, 704, 2816) == "nt352p<bf16>" and _nt(big, 704, 2816, queue=True) == "nt352p<bf16>"
    assert _nt(big, 2816, 704, act=ACT_GELU | SAVE_GRAD, p=0.1, pre=True) == "nt4r<bf16,False,False>"
    assert _nt(big, 2816, 704, act=MUL_SAVED, mul=True, bias=False) == "nt4r<bf16,False,False>"
    assert _nt(big, 2816, 704) == "nt352p<bf16>" and _nt(big, 1024, 256) == "nt256p<bf16,False>"      # (2816 = 8 x 352)
    assert _nt(big, 3584, 896) == "nt256p<bf16,False>"
    assert _nt(big, 256, 1024) == "nt2x<bf16,False>"                             # the H = 256 family's narrow expert outputs
    assert _nt(big, 3584, 896, act=ACT_GELU) == "nt4r<bf16,False,False>" and _nt(big, 3584, 1088, act=ACT_GELU) == "nt256p<bf16,False>"
    # the tile queue: taken by the ring kernel from K >= 352 on a grid of at least #CUs, else the two-per-CU kernel
    assert _nt(4096, 2816, 352, act=ACT_RELU, queue=True) == "nt4r<bf16,False,True>"       # (16 + 8) * 11 = 264 >= 256
    assert _nt(4096, 2560, 352, act=ACT_RELU, queue=True) == "nt2x<bf16,False>"            # 24 * 10 = 240
    assert _nt(4096, 2816, 320, act=ACT_RELU, queue=True) == "nt2x<bf16,False>"            # ten 32-deep steps
    assert _nt(4096, 2816, 328, act=ACT_RELU, queue=True, ldw=352) == "nt4r<bf16,True,True>"
    assert _nt(4096, 2816, 352, act=ACT_RELU, queue=True, ncu=304) == "nt2x<bf16,False>" and \
        _nt(4096, 2816, 352, act=ACT_RELU, queue=True, ncu=260) == "nt2x<bf16,False>"      # 260 % 8 != 0
    # ragged K: the 32-deep kernels want ldw padded to 32, the 64-deep one to 64; unpadded falls to the 128 x 128 kernel
    assert _nt(4096, 520, 168, act=ACT_RELU, ldw=192) == "nt4r<bf16,True,False>" and _nt(4096, 520, 168, act=ACT_RELU) == "nt<bf16,bf16>"
    assert _nt(4096, 520, 168, ldw=192) == "nt256p<bf16,True>" and _nt(4096, 520, 168, ldw=176) == "nt<bf16,bf16>"
    assert _nt(4096, 520, 192, ldw=200) == "nt256p<bf16,True>" and _nt(4096, 520, 192) == "nt256p<bf16,False>"
    assert _nt(4095, 520, 192) == "nt<bf16,bf16>" and _nt(4096, 504, 192) == "nt2x<bf16,False>" and _nt(4096, 248, 192) == "nt<bf16,bf16>"
    assert _nt(4096, 520, 128, act=ACT_RELU) == "nt2x<bf16,False>" and _nt(4096, 520, 136, act=ACT_RELU, ldw=160) == "nt4r<bf16,True,False>"
    assert _nt(4096, 520, 88, act=ACT_RELU, ldw=96) == "nt<bf16,bf16>" and _nt(4096, 520, 96, act=ACT_RELU) == "nt2x<bf16,False>"
    # the tile walk
    p = R.nt_path(BF16, BF16, 4096, 1280, 160, 0, 8, ACT_RELU, 0.0, False, False, True, False, 256)
    assert (p["walk_g"], p["n_tiles"], p["m_tiles"], p["tile"]) == (8, 5, 24, (256, 256))
    assert R.nt_path(BF16, BF16, 4096, 1024, 160, 0, 8, ACT_RELU, 0.0, False, False, True, False, 256)["walk_g"] == 0
    p = R.nt_path(BF16, BF16, 4096, 1160, 96, 0, 8, ACT_RELU, 0.0, False, False, True, False, 256)
    assert (p["path"], p["walk_g"], p["n_tiles"], p["n_partial"]) == ("nt2x<bf16,False>", 8, 10, True)
    assert R.nt_path(BF16, BF16, 4096, 1024, 96, 0, 8, ACT_RELU, 0.0, False, False, True, False, 256)["walk_g"] == 0
    # other types
    assert _nt(big, 2816, 704, out=F32) == "nt<bf16,f32>" and _nt(big, 2816, 704, dt=F32, out=F32) == "nt<f32,f32>"
    assert _nt(big, 2816, 704, dt=F32, out=BF16) == ERR_UNSUPPORTED and _nt(big, 2820, 704, out=F32) == "nt<bf16,f32>"
    # refusals and the empty call
    assert _nt(0, 704, 176) == "none" and _nt(-1, 704, 176) == ERR_ARG and _nt(16, 704, 176, ldw=168) == ERR_ARG
    assert _nt(big, 2816, 704, p=1.0) == ERR_ARG and _nt(big, 2816, 704, mul=True, bias=True) == ERR_ARG
    assert _nt(big, 2816, 704, act=ACT_GELU | SAVE_GRAD) == ERR_ARG and _nt(big, 2816, 704, act=MUL_SAVED, bias=False) == ERR_ARG
    assert _nt(big, 2816, 704, act=ACT_SILU | SAVE_GRAD, pre=True) == ERR_UNSUPPORTED
    assert _nt(2 ** 21, 2048, 704, act=ACT_GELU | SAVE_GRAD, pre=True) == ERR_UNSUPPORTED      # (rows + 256) * N >= 2^32: the mask's index
    assert _nt(big, 2816, 1056, act=ACT_GELU | SAVE_GRAD, pre=True) == ERR_UNSUPPORTED and _nt(big, 2816, 700) == ERR_UNSUPPORTED
    assert _nt(big, 2816, 704, ldw=708) == ERR_UNSUPPORTED and _nt(big, 2816, 704, E=4097) == ERR_UNSUPPORTED
    # apertis_grouped_gemm_nt_saves_grad promises no more than launch_nt takes (it is narrower at 256 <= N < 512, E > 1, which the
    # two-per-CU kernel would take)
    points = ((big, 2816, 704, 0, 8), (4095, 2816, 704, 0, 8), (big, 504, 704, 0, 8), (big, 2816, 1056, 0, 8), (big, 2816, 168, 0, 8),
              (big, 2816, 168, 192, 8), (big, 2816, 88, 0, 8), (big, 2816, 96, 0, 1025))
    assert [R.nt_saves_grad(*a, ACT_GELU, BF16, BF16) for a in points] == [1, 0, 0, 0, 0, 1, 0, 0]
    taken = [isinstance(R.nt_path(BF16, BF16, a[0], a[1], a[2], a[3], a[4], ACT_GELU | SAVE_GRAD, 0.1, True, False, True, False, 256), dict)
             for a in points]
    assert taken == [True, False, True, False, False, True, False, False]
    assert R.nt_saves_grad(big, 2816, 704, 0, 8, ACT_RELU, BF16, BF16) == 0 and R.nt_saves_grad(big, 2816, 704, 0, 8, ACT_GELU, F32, F32) == 0


def _tn(M, N, E, ws=True, q=False, ncu=256, pair=None, dt=BF16):
    return R.tn_path(dt, M, N, E, ws, q, ncu, pair=pair)


def test_tn_mirror_on_hand_computed_points():
    """apertis_grouped_gemm_tn_dense_variant at the shapes its comment quotes, the pair's tile choice, and the schedules."""
    assert [R.tn_dense_variant(M, N) for M, N in ((704, 2816), (768, 768), (352, 704), (896, 224), (704, 176))] == [1, 1, 1, -1, -1]
    assert R.tn_dense_variant(2816, 704) == 0 and R.tn_dense_variant(256, 1056) == 0 and R.tn_dense_variant(200, 1240) == 0
    assert R.tn_dense_variant(264, 1000) == 1 and R.tn_dense_variant(488, 488) == -1 and R.tn_dense_variant(496, 496) == 1
    assert R.tn_dense_variant(120, 4000) == -1 and R.tn_dense_variant(260, 1000) == -1 and R.tn_dense_variant(136, 1800) == -1   # 45 % fill
    assert R.tn5_variant(2816, 704) == 0 and R.tn5_variant(704, 2816) == 1 and R.tn5_variant(512, 512) == -1
    assert R.tn5_variant(704, 256) == 1 and R.tn5_variant(256, 704) == 0 and R.tn5_variant(248, 704) == -1 and R.tn5_variant(768, 768) == -1
    assert R.tn3_sched(11, 3, 32) == {"T": 33, "full": 1, "rem": 1, "s": 32} and R.tn3_sched(2, 2, 4)["s"] == 0
    # the experts' pair (E = 8: 16 CUs per group, 22 tiles = one round and 6 tiles cut in two), and the dense layer's single group
    p = _tn(2816, 704, 8, pair=(704, 2816))
    assert p["kernel"] == "grouped_gemm_tn5_k" and p["cpg"] == 16 and p["fold"] and [q["wide_m"] for q in p["problems"]] == [0, 1]
    assert [(q["T"], q["full"], q["rem"], q["s"]) for q in p["problems"]] == [(22, 1, 6, 2)] * 2
    assert [k for k, _ in p["launches"]] == ["grouped_gemm_tn5_k", "tn5_fold_k"]
    p = _tn(704, 2816, 1)
    assert p["cpg"] == 256 and p["problems"][0]["wide_m"] == 1 and (p["problems"][0]["T"], p["problems"][0]["s"]) == (22, 11)
    p = _tn(2816, 704, 8)                                            # E > 1 as a single problem: the 256 x 256 kernel
    assert p["kernel"] == "grouped_gemm_tn3_k" and p["cpg"] == 32 and (p["problems"][0]["T"], p["problems"][0]["full"], p["problems"][0]["s"]) == (33, 1, 32)
    assert _tn(896, 224, 1)["kernel"] == "grouped_gemm_tn3_k" and _tn(512, 512, 8, pair=(512, 512))["kernel"] == "grouped_gemm_tn3_k"
    assert not _tn(512, 512, 64)["fold"] and not _tn(768, 256, 64)["fold"] and _tn(520, 264, 64)["fold"]
    assert _tn(512, 512, 256)["kernel"] == "grouped_gemm_tn3_k" and _tn(512, 512, 257)["kernel"] == "grouped_gemm_tn2_k"
    assert _tn(512, 512, 129, pair=(512, 512))["kernel"] == "grouped_gemm_tn2_k" and _tn(512, 512, 8, ws=False)["kernel"] == "grouped_gemm_tn2_k"
    assert _tn(512, 512, 76, ncu=304)["cpg"] == 4 and _tn(512, 512, 8, q=True)["item_queue"]
    assert _tn(132, 136, 3, dt=F32)["path"] == "tn<f32>" and len(_tn(132, 136, 3, dt=F32, pair=(136, 132))["launches"]) == 2
    assert _tn(132, 136, 3) == ERR_UNSUPPORTED and _tn(130, 136, 3, dt=F32) == ERR_UNSUPPORTED and _tn(0, 136, 3) == ERR_ARG
    assert _tn(136, 136, 3, pair=(136, 132)) == ERR_UNSUPPORTED and _tn(136, 136, 0) == ERR_ARG


# ---------------------------------------------------------------------------------------------------------------------------
def test_case_tables_cover_every_dispatch_path():
    R.check_case_tables_cover_every_dispatch_path()


@pytest.mark.parametrize("path", R.NT_PATHS)
def test_coverage_check_fails_without_an_nt_path(path, monkeypatch):
    """With the rows of any one kernel instantiation taken out of NT_CASES the coverage check fails."""
    rows = [c for c in R.NT_CASES if R.nt_case_path(c, 256)["path"] != path]
    assert 0 < len(rows) < len(R.NT_CASES)
    monkeypatch.setattr(R, "NT_CASES", rows)
    monkeypatch.setattr(R, "NT_TWINS", [t for t in R.NT_TWINS if {t[0], t[1]} <= {c["id"] for c in rows}])
    with pytest.raises(AssertionError):
        R.check_case_tables_cover_every_dispatch_path()


def _tn_paths():
    out = set()
    for c in R.TN_CASES + R.TN_PAIR_CASES:
        for form in c["forms"]:
            p = R.tn_case_path(c, form, 256)
            out.add((p["kernel"], p["pair"], p["fold"]))
    return sorted(out)


@pytest.mark.parametrize("kernel,pair,fold", _tn_paths())
def test_coverage_check_fails_without_a_tn_path(kernel, pair, fold, monkeypatch):
    """... and with the rows of any one TN path (kernel, single or pair, with or without its fold) taken out of the TN tables."""
    def keeps(c):
        return all((p["kernel"], p["pair"], p["fold"]) != (kernel, pair, fold)
                   for p in (R.tn_case_path(c, f, 256) for f in c["forms"]))
    monkeypatch.setattr(R, "TN_CASES", [c for c in R.TN_CASES if keeps(c)])
    monkeypatch.setattr(R, "TN_PAIR_CASES", [c for c in R.TN_PAIR_CASES if keeps(c)])
    with pytest.raises(AssertionError):
        R.check_case_tables_cover_every_dispatch_path()


@pytest.mark.parametrize("table", ["NT_REFUSED", "TN_REFUSED"])
def test_refused_tables_hold_both_codes(table, monkeypatch):
    rows = getattr(R, table)
    for code in (ERR_ARG, ERR_UNSUPPORTED):
        monkeypatch.setattr(R, table, [r for r in rows if r[2] != code])
        with pytest.raises(AssertionError):
            R.check_case_tables_cover_every_dispatch_path()
    monkeypatch.setattr(R, table, rows)
    R.check_case_tables_cover_every_dispatch_path()


def test_inputs_are_on_the_grid_and_twins_share_them():
    for c in R.NT_CASES[:6] + [c for c in R.NT_CASES if c["mul"]][:2]:
        i = R.nt_inputs(c)
        assert i["A"].shape == (c["max_rows"], c["K"]) and i["W"].shape == (len(c["sizes"]), c["N"], c["ldw"])
        assert float(i["W"][:, :, c["K"]:].abs().sum()) == 0.0                        # the pad columns are zero
        assert torch.equal((i["A"].double() * 16).round() / 16, i["A"].double()) and float(i["A"].abs().max()) <= c["bound"] / 16
        assert torch.equal((i["W"].double() * 32).round() / 32, i["W"].double()) and int(i["offs"][-1]) == sum(c["sizes"])
        if c["mul"] == "saved":
            assert set(i["mul"].double().unique().tolist()) <= {0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0}
    by_id = {c["id"]: c for c in R.NT_CASES}
    for a, b in R.NT_TWINS:
        ia, ib = R.nt_inputs(by_id[a]), R.nt_inputs(by_id[b])
        assert torch.equal(ia["A"], ib["A"]) and torch.equal(ia["W"], ib["W"]) and ia["seed"] == ib["seed"] and ia["seed"] >> 32


def test_truncated_threshold_cases_can_tell_truncation_from_rounding():
    """Each p = 0.3 row has live, non-zero elements whose 16 mask bits equal the truncated threshold 19 660 exactly: kept by the
    definition, dropped by a kernel that rounds p * 65536 = 19 660.8 up."""
    rows = [c for c in R.NT_CASES if c["p"] == 0.3]
    assert len(rows) == 4 and R.thresh16(0.3) == 19660
    for c in rows:
        i = R.nt_inputs(c)
        probe = R.thresh_probe(c, i)
        pre = R.nt_pre_ref(i["A"], i["W"], i["b"], i["offs"], c["K"])
        assert int((probe & (pre != 0)).sum()) >= 2, (c["id"], int(probe.sum()))


def test_kernel_name_template_arguments():
    """The forms in which the profiler names this library's kernels (seen on an MI355X with torch 2.10 / ROCm 7.0): demangled,
    still mangled, and garbled where its demangler meets the bf16 type code."""
    f = R.kernel_name_targs
    assert f("_ZN12_GLOBAL__N_124grouped_gemm_nt_skinny_kIDF16bLi16EEEvPKDF16bS2_PKfPKiPT_iiiii", "grouped_gemm_nt_skinny_k") == (("bf16", 16), True)
    assert f("_ZN12_GLOBAL__N_119grouped_gemm_nt4r_kIDF16bLb1ELb0EEEvPKDF16b", "grouped_gemm_nt4r_k") == (("bf16", True, False), True)
    assert f("void (anonymous namespace)::grouped_gemm_nt4r_k<bool _Accum, bool, E, false>(bool _Accum const*, _P", "grouped_gemm_nt4r_k") == ((False,), False)
    assert f("void (anonymous namespace)::grouped_gemm_nt2x_k<bool _Accum, bool, E>(bool _Accum const*", "grouped_gemm_nt2x_k") == ((), False)
    assert f("void (anonymous namespace)::grouped_gemm_nt_k<float, float>(float const*, float const*)", "grouped_gemm_nt_k") == (("f32", "f32"), True)
    assert f("void (anonymous namespace)::grouped_gemm_tn3_k<true, true>((anonymous namespace)::Tn3Args, int const*)", "grouped_gemm_tn3_k") == ((True, True), True)
    assert f("(anonymous namespace)::tn5_fold_k((anonymous namespace)::Tn5Args, int)", "tn5_fold_k") == ((), True)
