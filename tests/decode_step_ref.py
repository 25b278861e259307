"""float64 CPU references, a mirror of the host-side dispatch and the case tables of the single-token decode-step kernels
(csrc/decode_step.hip, decode_ln_inproj_k in csrc/layernorm.hip, decode_conv_k / decode_state_k in csrc/scan_gate.hip), shared by
tests/test_decode_step_cpu.py (no device: the references against torch's own functions, the tables against the mirror) and
tests/test_decode_step_gpu.py (the kernels against the references).

Every reference takes the inputs AS STORED (bf16 tensors are read as the values they hold) and works in float64:
  conv      xc = silu(w[l, c, k-1] * window[l, b, c, 0] + bias[l, c])       (the front-slice quirk: decode_step.hip's header)
  state     dlt = b_dt + sum_r x_r W_dt[l, hd, r] (, softplus);  a = exp(-exp(A_log) dlt);  s' = a s + Bt;  pre = C s' + D xc
  gate      gated = pre * silu(z)
  push      new window = [w1 .. w_{k-2}, xp]
  gemv      x @ W[:, :K].T + bias
  boundary  y = res + blk   or   res + bf16(sum_k wk * yr[slot]) (slots < 0 skipped);   xn = LayerNorm(y)

The dyadic grid (the two GEMV kernels): x = n/16, W = m/32, bias = j/64 with |n|, |m|, |j| <= 31.  A product is n m / 512 with
|n m| <= 961 < 2^10, a sum of K <= 1024 of them is an integer below 961 * 1024 < 2^20 over 512, the bias adds 8 j / 512: every
partial sum, in any order and any grouping (MFMA blocks, K quarters met in LDS), is an integer of fewer than 21 bits over
2^9 - inside the 24 bits of an fp32 significand, so nothing is ever rounded before the single bf16 rounding of the result, and
that rounding (to nearest even, of an exactly known value) is the reference's `.float().bfloat16()`.
"""
import torch

F32, BF16 = torch.float32, torch.bfloat16
ERR_ARG, ERR_UNSUPPORTED = -1, -2


# ---------------------------------------------------------------------------------------------------------------------------
# references
def silu(x):
    x = x.double()
    return x / (1.0 + torch.exp(-x))


def softplus(x):
    """log(1 + e^x), stable on both sides (torch's threshold-20 form differs from it by less than 3e-9)."""
    x = x.double()
    return torch.clamp(x, min=0.0) + torch.log1p(torch.exp(-x.abs()))


def round_bf16(x):
    """A float64 tensor rounded once to bf16 (through fp32: exact for every value on the dyadic grid)."""
    return x.float().bfloat16()


def conv_ref(window, w, bias):
    """window [NL,B,Dn,k-1], w [NL,Dn,k], bias [NL,Dn] -> xc [NL,B,Dn]: only window[..., 0] and the last tap are used."""
    return silu(w.double()[:, None, :, -1] * window.double()[..., 0] + bias.double()[:, None, :])


def push_ref(window, xp):
    """window [..., k-1] and xp [...] (one dtype) -> the window after the push, [w1 .. w_{k-2}, xp]."""
    return torch.cat([window[..., 1:], xp.unsqueeze(-1)], dim=-1)


def state_ref(x_dt, W_dt, b_dt, A_log, Bt, C, D, xc, state, use_softplus):
    """x_dt [NL,B,R], W_dt [NL,h,R], b_dt [NL,h] or None, A_log [NL,h,N], Bt / C / xc / state [NL,B,Dn], D [NL,Dn] ->
    (new state, pre = C s' + D xc), float64 [NL,B,Dn]."""
    NL, h, N = A_log.shape
    dlt = torch.einsum("lbr,lhr->lbh", x_dt.double(), W_dt.double())
    if b_dt is not None:
        dlt = dlt + b_dt.double()[:, None, :]
    if use_softplus:
        dlt = softplus(dlt)
    dlt = dlt.repeat_interleave(N, dim=-1)                                     # [NL,B,Dn]: channel c belongs to head c // N
    a = torch.exp(-torch.exp(A_log.double().reshape(NL, 1, h * N)) * dlt)
    s = a * state.double() + Bt.double()
    return s, C.double() * s + D.double()[:, None, :] * xc.double()


def gate_ref(pre, z):
    return pre.double() * silu(z)


def gemv_ref(x, W, bias, K):
    out = x.double() @ W.double()[:, :K].t()
    return out if bias is None else out + bias.double()


def layer_norm_ref(y, gamma, beta, eps):
    y = y.double()
    mean = y.mean(-1, keepdim=True)
    var = ((y - mean) ** 2).mean(-1, keepdim=True)
    return (y - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()


def combine_ref(yr, wk, slot_of):
    """sum_k wk[s, k] * yr[slot_of[s, k]] with slots < 0 skipped, float64 [S, H]."""
    S, KK = slot_of.shape
    out = torch.zeros(S, yr.shape[1], dtype=torch.float64)
    for s in range(S):
        for k in range(KK):
            if int(slot_of[s, k]) >= 0:
                out[s] += float(wk[s, k]) * yr[int(slot_of[s, k])].double()
    return out


def boundary_ref(res, blk, gamma, beta, eps, combine=None):
    """(y fp32 as the kernel stores it, xn float64): y = res + blk in ONE fp32 addition of the stored values (correctly
    rounded on both sides: the same bits), blk being the bf16-rounded combine when `combine` = (wk, slot_of) is given."""
    a = round_bf16(combine_ref(blk, *combine)) if combine is not None else blk
    y = res.float().reshape(-1, res.shape[-1]) + a.float()
    return y, layer_norm_ref(y, gamma, beta, eps)


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
def dyadic(shape, den, gen, bound=31):
    """Integers in [-bound, bound] over `den`, fp32."""
    return torch.randint(-bound, bound + 1, shape, generator=gen).float() / den


def dyadic_gemv_inputs(B, K, N, use_bias, seed):
    g = torch.Generator().manual_seed(seed)
    return dyadic((B, K), 16, g), dyadic((N, K), 32, g), (dyadic((N,), 64, g) if use_bias else None)


def dyadic_sum_bits(K):
    """Bits an exact sum of K grid products plus a bias needs, in units of 1/512 (module doc)."""
    return (961 * K + 8 * 31).bit_length()


# ---------------------------------------------------------------------------------------------------------------------------
# mirror of the host-side dispatch: a change in the entry points must be made here too, and then
# check_case_tables_cover_every_dispatch_path says whether the tables below still reach every path
BLOCK = 256                 # threads of an elementwise block (decode_pre_conv_k, decode_pre_state_k, decode_post_k, decode_*_k)
KBATCH = 256                # one batch of eight 32-deep MFMA steps
KEEP = 14                   # window entries a thread holds while it shifts (k <= 16)


def elem_path(total):
    """(blocks, the last block ragged) of an elementwise launch over `total` elements."""
    return -(-total // BLOCK), total % BLOCK != 0


def shift_path(k):
    """Entries the window push moves: 'none' (k = 2), 'one' (k = 3), 'all' (k = 16: KEEP of them) or 'some'."""
    n = k - 2
    return "none" if n == 0 else "one" if n == 1 else "all" if n == KEEP else "some"


def gemv_rc(B, K, N, ldw):
    """apertis_decode_dense_gemv's answer to a shape (0 = launched)."""
    if ldw < K:
        return ERR_ARG
    if B < 1 or B > 16 or K < 8 or K % 8 or K >= 512 or N < 4 or N % 4 or ldw % 8:
        return ERR_UNSUPPORTED
    return 0


def gemv_path(B, K, N, ldw):
    """What decode_dense_gemv_k does at a shape: K batches (1 or 2), whether the last one is ragged (steps past K masked),
    whether the last work-group's 16 columns are partly past N, whether W's rows are padded.  (The kernel's scalar tail
    `nq + 3 >= N` cannot be reached: N % 4 == 0 is required and nq is a multiple of 4, so nq < N implies nq + 3 < N.)"""
    assert gemv_rc(B, K, N, ldw) == 0
    return {"k_batches": -(-K // KBATCH), "k_ragged": K % KBATCH != 0, "n_partial": N % 16 != 0, "padded": ldw > K,
            "rows": "one" if B == 1 else "full" if B == 16 else "some"}


def inproj_rc(S, H, N, ldw, kconv=None):
    """apertis_decode_inproj's answer (kconv given: the epilogue form)."""
    if S < 1 or S > 16 or H < 512 or H % 8 or H > 1024 or N < 4 or N % 4 or ldw < H or ldw % 8:
        return ERR_UNSUPPORTED
    if kconv is not None and (kconv < 2 or kconv > 16):
        return ERR_UNSUPPORTED
    return 0


def inproj_path(S, H, Dn, N=None):
    """decode_ln_inproj_k at a shape: IT = ceil(H / 256) (the template's row chunks and its __builtin_assume), the K quarter
    of a wave kq = 32 ceil(H / 128), whether the last wave's quarter ends inside a 32-deep step (H % 32 != 0) or is merely
    shorter than the others, whether the last work-group is partial (N % 16), whether one 4-column group holds xp AND z columns
    (Dn % 4 != 0: window entries and gated values from one lane)."""
    N = 2 * Dn if N is None else N
    kq = -(-H // 128) * 32
    return {"IT": -(-H // 256), "kq": kq, "last_ragged": H % 32 != 0, "last_short": H - 3 * kq < kq, "n_partial": N % 16 != 0,
            "straddle": Dn % 4 != 0, "rows": "one" if S == 1 else "full" if S == 16 else "some"}


# ---------------------------------------------------------------------------------------------------------------------------
# case tables
# conv / post / per-layer conv: (id, dtype, k, NL, B, Dn, xz_pad).  NL * B * Dn is the stacked launch's size, B * Dn the
# per-layer one (decode_post, ssm_decode_step); xz_pad: columns of xz past 2 Dn (NaN) for decode_post.
ELEM_CASES = [
    ("f32-k2-nl1-60", F32, 2, 1, 3, 20, 0),               # one ragged block
    ("bf16-k3-nl3-312", BF16, 3, 3, 2, 52, 8),            # two blocks stacked, one per layer
    ("f32-k4-nl3-1200", F32, 4, 3, 5, 80, 0),             # five blocks stacked, two per layer
    ("bf16-k16-nl1-390", BF16, 16, 1, 3, 130, 4),         # every KEEP entry shifted
    ("f32-k16-nl3-72", F32, 16, 3, 1, 24, 8),
    ("bf16-k2-nl3-960", BF16, 2, 3, 16, 20, 0),           # nothing shifted
    ("bf16-k4-nl1-176", BF16, 4, 1, 1, 176, 0),
    ("f32-k3-nl1-308", F32, 3, 1, 7, 44, 4),
]

# state: (id, dtype, NL, B, h, N, R, bias, softplus, lead).  p rows are the model's: [lead | Bt (Wb) | C (Wb) | dt (Wr)] with
# Wb, Wr = Dn, R rounded up to 64-column blocks and `lead` more columns in front; every column outside Bt / C / dt is NaN.
STATE_CASES = [
    ("f32-n16-h11-r20", F32, 3, 5, 11, 16, 20, True, True, 0),
    ("bf16-n8-h16-r64", BF16, 3, 1, 16, 8, 64, False, True, 64),
    ("f32-n64-h1-r1", F32, 1, 16, 1, 64, 1, True, False, 64),
    ("bf16-n16-h11-r20-raw", BF16, 1, 5, 11, 16, 20, True, False, 0),
    ("f32-n8-h1-r64-nobias", F32, 3, 1, 1, 8, 64, False, False, 64),      # 24 elements: below one block
    ("bf16-n64-h16-r1", BF16, 3, 16, 16, 64, 1, False, True, 0),
]

# chain equality: (k, dtype) at NL 3, B 5, h 10, N 8 (Dn 80), R 20
CHAIN_CASES = [(2, BF16), (16, BF16)]
CHAIN_SHAPE = dict(NL=3, B=5, h=10, N=8, R=20)

# dense GEMV: (id, B, K, N, ldw - K, bias, grid)
GEMV_CASES = [
    ("b1-k8-n4", 1, 8, 4, 0, False, "dyadic"),
    ("b7-k64-n20-pad", 7, 64, 20, 8, True, "dyadic"),
    ("b16-k176-n704", 16, 176, 704, 0, True, "dyadic"),
    ("b7-k256-n20", 7, 256, 20, 0, False, "dyadic"),            # one batch, full
    ("b1-k264-n704-pad", 1, 264, 704, 56, True, "dyadic"),      # the second batch: one live chunk
    ("b16-k504-n20-pad", 16, 504, 20, 8, True, "dyadic"),       # the second batch, ragged at its end
    ("b7-k504-n704", 7, 504, 704, 0, False, "dyadic"),
    ("b16-k264-n4", 16, 264, 4, 0, True, "dyadic"),
    ("b7-k504-n704-random", 7, 504, 704, 8, True, "random"),
    ("b16-k176-n20-random", 16, 176, 20, 0, False, "random"),
]
GEMV_REFUSED = [(17, 64, 64, 64), (1, 512, 64, 512), (1, 12, 64, 16), (1, 64, 6, 64), (1, 64, 64, 68)]   # (B, K, N, ldw) -> -2

# in_proj with epilogue, xn given: (id, S, H, Dn, kconv, ldw - H)
INPROJ_CASES = [
    ("s1-h512-dn64-k2", 1, 512, 64, 2, 0),
    ("s5-h520-dn130-k4", 5, 520, 130, 4, 56),
    ("s16-h704-dn176-k16", 16, 704, 176, 16, 0),
    ("s5-h1024-dn130-k16", 5, 1024, 130, 16, 0),
    ("s16-h1024-dn64-k4", 16, 1024, 64, 4, 8),
    ("s1-h704-dn130-k2", 1, 704, 130, 2, 64),
]

# boundary form: (id, S, H, Dn, kconv, form)
BOUNDARY_CASES = [
    ("s1-h512-dense", 1, 512, 64, 4, "dense"),
    ("s4-h704-combine", 4, 704, 130, 4, "combine"),
    ("s4-h1024-dense", 4, 1024, 64, 2, "dense"),
    ("s1-h1024-combine", 1, 1024, 64, 16, "combine"),
    ("s4-h512-combine", 4, 512, 176, 3, "combine"),
    ("s1-h704-dense", 1, 704, 130, 16, "dense"),
]

# xz output form (pre == NULL): (id, S, H, N)
XZ_CASES = [("s5-h520-n20", 5, 520, 20), ("s16-h704-n260", 16, 704, 260), ("s1-h1024-n20", 1, 1024, 20)]
INPROJ_REFUSED = [(17, 512, 128, 512, 4), (1, 504, 128, 504, 4), (1, 1032, 128, 1032, 4), (1, 512, 128, 512, 17)]  # (S,H,N,ldw,k)


def check_case_tables_cover_every_dispatch_path():
    """Every path the mirror above knows is reached by a row of a table; a row taken out of a table fails an assertion here."""
    # elementwise kernels: both dtypes at every window-shift edge, one and several blocks (stacked and per layer), ragged, NL
    seen = set()
    for _, dt, k, NL, B, Dn, pad in ELEM_CASES:
        nb, ragged = elem_path(NL * B * Dn)
        assert ragged, "the stacked size must not be a multiple of the block"
        seen |= {("shift", shift_path(k), dt), ("k", k, dt), ("stacked", "one" if nb == 1 else "many"), ("NL", NL),
                 ("layer", "one" if elem_path(B * Dn)[0] == 1 else "many"), ("xz_pad", pad > 0)}
    for dt in (F32, BF16):
        for k in (2, 3, 4, 16):
            assert ("k", k, dt) in seen, (k, dt)
        assert {("shift", s, dt) for s in ("none", "one", "some", "all")} <= seen, dt
    assert {("stacked", "one"), ("stacked", "many"), ("layer", "one"), ("layer", "many"), ("NL", 1), ("NL", 3),
            ("xz_pad", True), ("xz_pad", False)} <= seen

    # state kernels
    seen = set()
    for _, dt, NL, B, h, N, R, bias, sp, lead in STATE_CASES:
        nb, _ = elem_path(NL * B * h * N)
        seen |= {("dt", dt), ("N", N), ("h", h), ("R", R), ("B", B), ("bias", bias), ("softplus", sp), ("NL", NL), ("lead", lead > 0),
                 ("blocks", "one" if nb == 1 else "many"), ("NL3", dt) if NL == 3 else ("NL1", dt),
                 ("pitch>cols", 2 * (-(-h * N // 64) * 64) + -(-R // 64) * 64 + lead > 2 * h * N + R)}
    for key, vals in (("N", (8, 16, 64)), ("h", (1, 11, 16)), ("R", (1, 20, 64)), ("B", (1, 5, 16)), ("bias", (True, False)),
                      ("softplus", (True, False)), ("NL", (1, 3)), ("lead", (True, False)), ("dt", (F32, BF16)),
                      ("blocks", ("one", "many"))):
        for v in vals:
            assert (key, v) in seen, (key, v)
    assert ("NL3", F32) in seen and ("NL3", BF16) in seen and ("pitch>cols", True) in seen
    pairs = {(dt, key, v) for _, dt, NL, B, h, N, R, bias, sp, lead in STATE_CASES
             for key, v in (("bias", bias), ("softplus", sp), ("lead", lead > 0), ("NL", NL), ("wide heads", N == 64 and h > 1))}
    for dt in (F32, BF16):
        for key in ("bias", "softplus", "lead"):
            assert (dt, key, True) in pairs and (dt, key, False) in pairs, (dt, key)
        assert (dt, "NL", 1) in pairs and (dt, "NL", 3) in pairs
    assert (BF16, "wide heads", True) in pairs          # the head index c / N with several 64-channel heads
    assert {k for k, _ in CHAIN_CASES} == {2, 16}

    # dense GEMV
    seen = set()
    for _, B, K, N, pad, bias, grid in GEMV_CASES:
        p = gemv_path(B, K, N, K + pad)
        assert dyadic_sum_bits(K) <= 24
        if grid == "dyadic":
            seen |= {("B", B), ("K", K), ("N", N), ("bias", bias), ("padded", p["padded"]),
                     ("kb", p["k_batches"], p["k_ragged"]), ("n_partial", p["n_partial"]), ("rows", p["rows"])}
            if p["k_batches"] == 2:
                seen.add(("kb2", K, "padded" if p["padded"] else "tight"))
        else:
            seen.add(("random", p["k_batches"]))
    for key, vals in (("B", (1, 7, 16)), ("K", (8, 64, 176, 256, 264, 504)), ("N", (4, 20, 704)), ("bias", (True, False)),
                      ("padded", (True, False)), ("n_partial", (True, False)), ("rows", ("one", "some", "full"))):
        for v in vals:
            assert (key, v) in seen, (key, v)
    assert {("kb", 1, True), ("kb", 1, False), ("kb", 2, True), ("random", 1), ("random", 2)} <= seen
    # the second K batch with one live chunk (264) and ragged at its end (504), each with and without padding behind the row
    assert {("kb2", K, p) for K in (264, 504) for p in ("padded", "tight")} <= seen
    assert all(gemv_rc(*c) == ERR_UNSUPPORTED for c in GEMV_REFUSED) and gemv_rc(1, 64, 64, 56) == ERR_ARG
    assert len(GEMV_REFUSED) == 5 and len(INPROJ_REFUSED) == 4          # one row per refusal the entry points make

    # in_proj, xn form with epilogue
    seen = set()
    for _, S, H, Dn, k, pad in INPROJ_CASES:
        assert inproj_rc(S, H, 2 * Dn, H + pad, k) == 0 and dyadic_sum_bits(H) <= 24
        p = inproj_path(S, H, Dn)
        seen |= {("S", S), ("H", H), ("Dn", Dn), ("k", k), ("IT", p["IT"]), ("ragged", p["last_ragged"]), ("short", p["last_short"]),
                 ("straddle", p["straddle"]), ("n_partial", p["n_partial"]), ("padded", pad > 0), ("shift", shift_path(k)),
                 ("straddle-shift", shift_path(k)) if p["straddle"] else ("aligned-shift", shift_path(k)), ("IT-rows", p["IT"], p["rows"])}
    for key, vals in (("S", (1, 5, 16)), ("H", (512, 520, 704, 1024)), ("Dn", (64, 130, 176)), ("k", (2, 4, 16)), ("IT", (2, 3, 4)),
                      ("ragged", (True, False)), ("short", (True, False)), ("straddle", (True, False)),
                      ("n_partial", (True, False)), ("padded", (True, False)), ("shift", ("none", "some", "all"))):
        for v in vals:
            assert (key, v) in seen, (key, v)
    assert {("straddle-shift", s) for s in ("none", "some", "all")} <= seen
    assert {("IT-rows", 3, "full"), ("IT-rows", 4, "full"), ("IT-rows", 4, "some")} <= seen       # all 16 rows at the longest K

    # boundary form
    seen = set()
    for _, S, H, Dn, k, form in BOUNDARY_CASES:
        assert S <= 4 and inproj_rc(S, H, 2 * Dn, H, k) == 0
        seen |= {("S", S, form), ("IT", inproj_path(S, H, Dn)["IT"], form), ("shift", shift_path(k))}
    for form in ("dense", "combine"):
        assert {("S", 1, form), ("S", 4, form), ("IT", 2, form), ("IT", 3, form), ("IT", 4, form)} <= seen, form
    assert {("shift", s) for s in ("none", "one", "some", "all")} <= seen

    # xz output form
    assert {N for _, _, _, N in XZ_CASES} == {20, 260}
    assert {inproj_path(S, H, 0, N)["IT"] for _, S, H, N in XZ_CASES} == {3, 4}
    assert any(inproj_path(S, H, 0, N)["last_ragged"] for _, S, H, N in XZ_CASES)
    assert all(inproj_rc(S, H, N, H) == 0 and N % 16 != 0 for _, S, H, N in XZ_CASES)
    assert all(inproj_rc(*c) == ERR_UNSUPPORTED for c in INPROJ_REFUSED)
