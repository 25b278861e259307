"""float64 CPU references, a mirror of the host-side dispatch and the case tables of the grouped GEMM kernels
(csrc/grouped_gemm.hip), shared by tests/test_gemm_paths_cpu.py (no device: the references against torch in
float64, the grid against int64 arithmetic, the mask against a scalar transcription, the tables against the mirror) and
tests/test_gemm_paths_gpu.py (the kernels, through the C ABI, against the references).

References (inputs AS STORED, float64):
  nt_ref        per group  x @ W[e][:, :K].T + b[e]  (the pre-activation), then the activation, then the dropout scale
  tn_ref        per group  A^T B  and the column sums of A
  act_ref / act_grad_ref   the activation codes of include/apertis_hip.h and their derivatives
  keep_mask     the dropout mask of csrc/grouped_gemm.hip (gd_keep / gd_keep4: the factorised hash every kernel of that file,
                forward and backward, draws from) - a pure function of (seed, row, column) and thresh16 = uint32(p * 65536);
                N does not enter it.  (csrc/common.h's drop_keep is the linear-index mask of the OTHER files - attention, LayerNorm,
                SSM elementwise; keep_mask_linear mirrors it and test_gemm_paths_cpu.py pins both transcriptions.)

The dyadic grid.  Operands are n/16 and m/32 with |n|, |m| <= 31 - both exact in bf16 (5 significant bits) - and the bias is
j/64 in fp32.  A product is n m / 512, an integer of at most 961 in units of 1/512; the bias adds 8 j.  A sum of D such products
plus a bias stays below 2^24 in those units while 961 D + 248 < 2^24, i.e. for a reduction depth D <= 17 457 (D = K for the NT
kernels, the rows of ONE group for the TN kernels; dbias sums n/16: far smaller).  Under that bound every partial sum in every
order and grouping - MFMA blocks, the skinny kernel's K shares met in LDS, the row slices of a split TN tile and the tn3 / tn5
folds - is an integer of at most 24 bits over 2^9: inside an fp32 significand, so NOTHING is rounded in the accumulation.  Every
fp32 output (dW, dbias, the fp32-output NT form, the fp32 kernel) is therefore known exactly, every bf16 output is the single
round-to-nearest-even of a known value, and the float64 reference is exact, not merely precise.  Scaling by a power of two (the
dropout's 1 / (1 - 0.5) = 2, a saved gradient drawn from {0, +-1/2, +-1, +-2}) commutes with the bf16 rounding, so those
epilogues are exact too, whichever order they round and scale in.  `dyadic_sum_bits(D)` gives the bits a case needs.
"""
import re

import numpy as np
import torch

from decode_step_ref import dyadic, dyadic_sum_bits, round_bf16  # noqa: F401  (re-exported: grid, bits and rounding are the decode tests')

F32, BF16 = torch.float32, torch.bfloat16
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -2
ACT_NONE, ACT_GELU, ACT_RELU, ACT_SILU = 0, 1, 2, 3
SAVE_GRAD, MUL_SAVED = 0x100, 0x200
MAX_DEPTH = (2 ** 24 - 1 - 248) // 961          # 17 457


# ---------------------------------------------------------------------------------------------------------------------------
# references
def act_ref(x, act):
    x = x.double()
    if act == ACT_GELU:
        return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))
    if act == ACT_RELU:
        return torch.clamp(x, min=0.0)
    if act == ACT_SILU:
        return x / (1.0 + torch.exp(-x))
    return x


def act_grad_ref(x, act):
    x = x.double()
    if act == ACT_GELU:
        return 0.5 * (1.0 + torch.erf(x * 0.7071067811865476)) + x * 0.3989422804014327 * torch.exp(-0.5 * x * x)
    if act == ACT_RELU:
        return (x > 0).double()
    if act == ACT_SILU:
        s = 1.0 / (1.0 + torch.exp(-x))
        return s * (1.0 + x * (1.0 - s))
    return torch.ones_like(x)


def gelu_fast_form(x, scale=1.0):
    """(gelu, gelu') as the bf16 kernels form them (gelu_terms in csrc/grouped_gemm.hip: Abramowitz-Stegun 7.1.25, three terms,
    the output scale folded into the coefficients), evaluated in fp32 on the CPU.  What it differs from float64 by at a case's
    pre-activations is the part of a GELU tolerance that is the FORM's and not a rounding's."""
    x = x.float()
    s = torch.tensor(scale, dtype=F32)
    c1, c2, c3 = s * (0.5 * 0.3480242), s * (0.5 * -0.0958798), s * (0.5 * 0.7478556)
    t = 1.0 / (torch.tensor(0.47047 * 0.70710678118654752, dtype=F32) * x.abs() + 1.0)
    p = (c3 * t + c2) * t + c1
    e = torch.exp2((x * x) * torch.tensor(-0.5 * 1.4426950408889634, dtype=F32))
    q = (p * t) * e
    P = torch.where(x >= 0, s - q, q)
    return x * P, (x * (s * 0.3989422804014327)) * e + P


def nt_pre_ref(x, W, b, offsets, K):
    """The pre-activation of every row below offsets[E], float64 [offsets[E], N]."""
    E, N = W.shape[0], W.shape[1]
    out = torch.zeros(int(offsets[-1]), N, dtype=torch.float64)
    xd = x.double()
    for e in range(E):
        r0, r1 = int(offsets[e]), int(offsets[e + 1])
        if r1 > r0:
            out[r0:r1] = xd[r0:r1, :K] @ W[e].double()[:, :K].t()
            if b is not None:
                out[r0:r1] += b[e].double()
    return out


def nt_ref(x, W, b, offsets, K, act=ACT_NONE, drop_p=0.0, seed=0, round_pre=False):
    """act(pre) * keep / (1 - p), float64.  round_pre: the activation sees the pre-activation rounded to bf16 (what every bf16
    epilogue feeds it)."""
    pre = nt_pre_ref(x, W, b, offsets, K)
    h = act_ref(round_bf16(pre).double() if round_pre else pre, act)
    if drop_p > 0.0:
        h = h * torch.from_numpy(keep_mask(seed, pre.shape[0], pre.shape[1], drop_p)).double() / (1.0 - drop_p)
    return h


def tn_ref(A, B, offsets):
    """(dW [E, M, N], dbias [E, M]) in float64: per group A^T B and the column sums of A."""
    E = len(offsets) - 1
    dW = torch.zeros(E, A.shape[1], B.shape[1], dtype=torch.float64)
    db = torch.zeros(E, A.shape[1], dtype=torch.float64)
    Ad, Bd = A.double(), B.double()
    for e in range(E):
        r0, r1 = int(offsets[e]), int(offsets[e + 1])
        if r1 > r0:
            dW[e] = Ad[r0:r1].t() @ Bd[r0:r1]
            db[e] = Ad[r0:r1].sum(0)
    return dW, db


# ---------------------------------------------------------------------------------------------------------------------------
# the dropout masks
_M32 = np.uint64(0xFFFFFFFF)


def _u32(a):
    return np.asarray(a, dtype=np.uint64) & _M32


def _fmix(h):
    h = _u32(h)
    h ^= h >> np.uint64(16)
    h = _u32(h * np.uint64(0x85EBCA6B))
    h ^= h >> np.uint64(13)
    h = _u32(h * np.uint64(0xC2B2AE35))
    h ^= h >> np.uint64(16)
    return h


def thresh16(p):
    """uint32(p * 65536) in fp32, truncated (not rounded)."""
    return int(np.float32(p) * np.float32(65536.0))


def keep_mask(seed, rows, N, p, row0=0, thresh=None):
    """bool [rows, N]: gd_keep(seed, row0 + r, c, thresh16(p)) of csrc/grouped_gemm.hip, vectorised (uint32 arithmetic held in
    uint64 lanes and masked).  thresh: another threshold than thresh16(p)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    r = np.arange(row0, row0 + rows, dtype=np.uint64)
    rowmix = _fmix(_u32(_u32(r) * np.uint64(0x9E3779B9)) + _u32((r >> np.uint64(32)) * np.uint64(0x7F4A7C15)) + np.uint64(seed & 0xFFFFFFFF))
    cp = np.arange((N + 1) // 2, dtype=np.uint64)
    colmix = _fmix(_u32(cp * np.uint64(0x85EBCA77)) ^ np.uint64(seed >> 32))
    x = _u32((rowmix[:, None] ^ colmix[None, :]) * np.uint64(0x2C1B3C6D))
    x ^= x >> np.uint64(15)
    r16 = np.stack([x & np.uint64(0xFFFF), x >> np.uint64(16)], axis=-1).reshape(rows, -1)[:, :N]
    return r16 >= np.uint64(thresh16(p) if thresh is None else thresh)


def keep_mask_linear(seed, rows, N, p):
    """bool [rows, N]: drop_keep(seed, r, c, N, thresh16(p)) of csrc/common.h (the linear-index mask of the other files)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    lin = np.arange(rows * N, dtype=np.uint64)
    h = _u32(lin >> np.uint64(1)) ^ np.uint64(seed & 0xFFFFFFFF)
    h = _u32(h + _u32((lin >> np.uint64(33)) * np.uint64(0x9E3779B9)) + np.uint64(seed >> 32))
    h = _fmix(h)
    r16 = np.where(lin & np.uint64(1), h >> np.uint64(16), h & np.uint64(0xFFFF))
    return (r16 >= np.uint64(thresh16(p))).reshape(rows, N)


# ---------------------------------------------------------------------------------------------------------------------------
# mirror of the host-side dispatch: a change in launch_nt or the TN entry points must be made here too, and then
# check_case_tables_cover_every_dispatch_path says whether the tables below still reach every path
def _cdiv(a, b):
    return -(-a // b)


# kernel -> (tile height, tile width, K step)
NT_TILES = {"nt_skinny": (16, 16, 32), "nt352p": (256, 352, 64), "nt4r": (256, 256, 32),
            "nt2x": (256, 128, 32), "nt256p": (256, 256, 64), "nt": (128, 128, 64)}


def _nt_hit(kernel, targs, max_rows, N, K, ldw, E, epi, **extra):
    h, w, kstep = NT_TILES[kernel]
    if kernel == "nt" and targs[0] == "f32":
        kstep = 32
    d = {"kernel": f"grouped_gemm_{kernel}_k", "targs": targs, "path": f"{kernel}<{','.join(str(t) for t in targs)}>",
         "tile": (h, w), "m_tiles": _cdiv(max_rows, h) + E, "n_tiles": _cdiv(N, w), "m_partial": max_rows % h != 0,
         "n_partial": N % w != 0, "k_step": kstep, "k_ragged": K % kstep != 0, "k_padded": ldw > K, "walk_g": 0, "epi": epi,
         "launches": [(f"grouped_gemm_{kernel}_k", targs)]}
    d.update(extra)
    return d


def nt_epilogue(act_flags, drop_p, has_pre, has_mul):
    """The epilogue form a call asks for: raw | act | pre+act (both outputs) | save_grad | mul_saved | mul_act."""
    if act_flags & SAVE_GRAD:
        return "save_grad"
    if has_mul:
        return "mul_saved" if act_flags & MUL_SAVED else "mul_act"
    if has_pre:
        return "pre+act"
    return "raw" if (act_flags & 0xff) == ACT_NONE and drop_p <= 0.0 else "act"


def nt_path(dtype, dtype_out, max_rows, N, K, ldw, E, act_flags, drop_p, has_pre, has_mul, has_bias, has_queue, ncu):
    """apertis_grouped_gemm_nt_q's answer to a call (pointers non-null and 16-byte aligned): a negative return code, "none"
    (max_rows = 0: nothing launched), or the facts of the launch."""
    if max_rows < 0 or N <= 0 or K <= 0 or E <= 0 or (ldw != 0 and ldw < K):
        return ERR_ARG
    if ldw == 0:
        ldw = K
    if drop_p < 0.0 or drop_p >= 1.0 or (has_mul and (has_pre or has_bias)):
        return ERR_ARG
    if max_rows == 0:
        return "none"
    if max_rows > 0x7fffffff or N > 0x3fffffff or K > 0x3fffffff or ldw > 0x3fffffff or E > 4096:
        return ERR_UNSUPPORTED
    both16 = dtype == BF16 and dtype_out == BF16
    if both16:
        if K % 8 or N % 8:
            return ERR_UNSUPPORTED
    elif dtype == BF16 and dtype_out == F32:
        if K % 8 or N % 4:
            return ERR_UNSUPPORTED
    elif dtype == F32 and dtype_out == F32:
        if K % 4 or N % 4:
            return ERR_UNSUPPORTED
    else:
        return ERR_UNSUPPORTED
    # launch_nt
    if ldw % (8 if dtype == BF16 else 4):                      # aligned16 of W's rows (A's and C's follow from K and N above)
        return ERR_UNSUPPORTED
    flagged = (act_flags & (SAVE_GRAD | MUL_SAVED)) != 0
    act = act_flags & 0xff
    if flagged and (not has_pre if act_flags & SAVE_GRAD else not has_mul):
        return ERR_ARG
    if (act_flags & SAVE_GRAD) and (act != ACT_GELU or (max_rows + 256) * N >= 0x100000000):
        return ERR_UNSUPPORTED
    if (_cdiv(max_rows, 128) + E) * _cdiv(N, 128) > 0x7fffffff:
        return ERR_UNSUPPORTED
    epi = nt_epilogue(act_flags, drop_p, has_pre, has_mul)
    tn = lambda dt: "bf16" if dt == BF16 else "f32"
    if both16:
        heavy = act != ACT_NONE or drop_p > 0.0 or has_pre or has_mul
        if (max_rows <= 64 and not flagged and not has_pre and not has_mul and drop_p <= 0.0 and K % 8 == 0 and N % 4 == 0 and
                ldw % 8 == 0 and E <= 65535):
            ks = 16 if K >= 2048 else 4 if K >= 512 else 1
            return _nt_hit("nt_skinny", ("bf16", ks), max_rows, N, K, ldw, E, epi, k_share=_cdiv(K, ks * 32) * 32 if ks > 1 else K)
        kpad_ok = K % 64 == 0 or ldw >= _cdiv(K, 64) * 64
        plain352 = N == 352 and K % 64 == 0 and ldw == K
        use2x = ((heavy and K <= 1024 and N >= 512) or (E == 1 and K <= 1024 and N >= 256 and not plain352) or
                 (E > 1 and K <= 1024 and 256 <= N < 512) or (E == 1 and K <= 1024 and 64 <= N < 128))
        big = max_rows >= 4096 and E <= 1024
        if (not use2x and not heavy and N % 352 == 0 and K % 64 == 0 and ldw == K and K >= 128 and big):
            return _nt_hit("nt352p", ("bf16",), max_rows, N, K, ldw, E, epi, queue=has_queue)
        ragged2x = K % 32 != 0
        pad32_ok = not ragged2x or ldw >= _cdiv(K, 32) * 32
        use4r = (heavy and K <= 1024 and N >= 512) or (E == 1 and K <= 1024 and N >= 128 and not plain352)
        queue4_ok = has_queue and _cdiv(K, 32) >= 11 and (_cdiv(max_rows, 256) + E) * _cdiv(N, 256) >= ncu and ncu % 8 == 0
        if (use4r and not (has_mul and has_bias) and (not has_queue or queue4_ok) and pad32_ok and K > 128 and K % 8 == 0 and
                N % 8 == 0 and N >= 128 and big):
            nt4 = _cdiv(N, 256)
            return _nt_hit("nt4r", ("bf16", ragged2x, has_queue), max_rows, N, K, ldw, E, epi, walk_g=8 if nt4 > 4 else 0,
                           walk_nb=2, queue=has_queue)
        if use2x and pad32_ok and K >= 96 and K % 8 == 0 and N % 8 == 0 and N >= 64 and big:
            nt3 = _cdiv(N, 128)
            return _nt_hit("nt2x", ("bf16", ragged2x), max_rows, N, K, ldw, E, epi, walk_g=8 if nt3 > 8 else 0, walk_nb=4)
        if flagged:
            return ERR_UNSUPPORTED
        if kpad_ok and (N >= 512 or (E == 1 and N >= 128)) and big:
            return _nt_hit("nt256p", ("bf16", not (K % 64 == 0 and ldw == K)), max_rows, N, K, ldw, E, epi, queue=has_queue)
    if flagged:
        return ERR_UNSUPPORTED
    return _nt_hit("nt", (tn(dtype), tn(dtype_out)), max_rows, N, K, ldw, E, epi)


def nt_saves_grad(max_rows, N, K, ldw, E, act, dtype, dtype_out):
    """apertis_grouped_gemm_nt_saves_grad."""
    if dtype != BF16 or dtype_out != BF16 or N <= 0 or K <= 0 or E <= 0 or act != ACT_GELU:
        return 0
    ldw = ldw or K
    return int(K <= 1024 and N >= 512 and (K % 32 == 0 or ldw >= _cdiv(K, 32) * 32) and K >= 96 and K % 8 == 0 and N % 8 == 0 and
               max_rows >= 4096 and E <= 1024 and (max_rows + 256) * N < 0x100000000)


def tn3_sched(m_tiles, n_tiles, cpg):
    T = m_tiles * n_tiles
    full = T // cpg
    rem = T - full * cpg
    return {"T": T, "full": full, "rem": rem, "s": cpg // rem if rem else 0}


def tn5_variant(M, N):
    """Which v5 tile suits an [M, N] problem of a PAIR: 1 = 352 x 256, 0 = 256 x 352, -1 = neither."""
    area = lambda tm, tn: _cdiv(M, tm) * _cdiv(N, tn) * tm * tn
    a3, aw, an = area(256, 256), area(352, 256), area(256, 352)
    if M < 256 or N < 256 or min(aw, an) * 100 > a3 * 95:
        return -1
    return 1 if aw < an else 0


def tn_dense_variant(M, N):
    """apertis_grouped_gemm_tn_dense_variant: the v5 tile of a ONE-group weight gradient, or -1."""
    if M < 128 or N < 128 or M % 8 or N % 8 or M * N < 240000:
        return -1
    area = lambda tm, tn: _cdiv(M, tm) * _cdiv(N, tn) * tm * tn
    aw, an = area(352, 256), area(256, 352)
    if M * N * 100 < min(aw, an) * 60:
        return -1
    return 1 if aw <= an else 0


def _tn_ws_launch(kind, probs, variants, E, max_rows, item_queue, ncu):
    """launch_tn3 / launch_tn5 with a sufficient workspace: None where they return APERTIS_ERR_UNSUPPORTED."""
    groups = len(probs) * E
    if groups > ncu or (kind == "tn5" and min(variants) < 0):
        return None
    if (max_rows + 256) * max(max(p) for p in probs) * 2 >= 0xffffffff:
        return None
    cpg = ncu // groups
    facts = []
    for (M, N), v in zip(probs, variants):
        tm, tn = (256, 256) if kind == "tn3" else ((352, 256) if v else (256, 352))
        mt, nt = _cdiv(M, tm), _cdiv(N, tn)
        sc = tn3_sched(mt, nt, cpg)
        facts.append(dict(sc, tile=(tm, tn), m_tiles=mt, n_tiles=nt, m_partial=M % tm != 0, n_partial=N % tn != 0,
                          wide_m=v if kind == "tn5" else None))
    fold = any(f["rem"] and f["s"] > 1 for f in facts)
    kname = "grouped_gemm_tn3_k" if kind == "tn3" else "grouped_gemm_tn5_k"
    targs = ()                                                 # neither kernel is a template
    launches = [(kname, targs)] + ([(f"{kind}_fold_k", ())] if fold else [])
    return {"kernel": kname, "targs": targs, "cpg": cpg, "grid": groups * cpg, "problems": facts, "fold": fold, "pair": len(probs) == 2,
            "item_queue": bool(item_queue), "launches": launches,
            "path": f"{kind}<{'pair' if len(probs) == 2 else 'single'},{'fold' if fold else 'nofold'},{'queue' if item_queue else 'static'}>"}


def tn_path(dtype, M, N, E, has_ws, item_queue, ncu, pair=None, max_rows=4096):
    """apertis_grouped_gemm_tn_q's answer ([M, N] per group), or apertis_grouped_gemm_tn_pair_q's with pair = (M1, N1): a
    negative return code or the facts of the launch(es).  has_ws: a 16-byte aligned workspace of
    apertis_grouped_gemm_tn_workspace_bytes bytes is passed."""
    probs = [(M, N)] + ([tuple(pair)] if pair else [])
    if max_rows < 0 or E <= 0 or (not pair and (M <= 0 or N <= 0)):
        return ERR_ARG
    if pair and dtype != BF16:                                  # fp32 parity path: two ordinary launches
        a, b = tn_path(dtype, M, N, E, False, 0, ncu), tn_path(dtype, pair[0], pair[1], E, False, 0, ncu)
        if isinstance(a, int) or isinstance(b, int):
            return a if isinstance(a, int) else b
        return dict(a, pair=True, launches=a["launches"] + b["launches"], path="tn<f32,pair>")
    if pair and (min(M, N, *pair) <= 0 or (M | N | pair[0] | pair[1]) % 8):
        return ERR_UNSUPPORTED
    if max(max(p) for p in probs) > 0x3fffffff or max_rows > 0x7fffffff:
        return ERR_UNSUPPORTED
    if sum(E * _cdiv(m, 128) * _cdiv(n, 128) for m, n in probs) > 0x7fffffff:
        return ERR_UNSUPPORTED
    if dtype == F32:
        if M % 4 or N % 4:
            return ERR_UNSUPPORTED
        return {"kernel": "grouped_gemm_tn_k", "targs": ("f32",), "path": "tn<f32>", "launches": [("grouped_gemm_tn_k", ("f32",))],
                "tile": (128, 128), "m_partial": M % 128 != 0, "n_partial": N % 128 != 0, "fold": False, "pair": False}
    if dtype != BF16:
        return ERR_ARG
    if M % 8 or N % 8:
        return ERR_UNSUPPORTED
    if has_ws:
        if pair:
            hit = _tn_ws_launch("tn5", probs, [tn5_variant(*p) for p in probs], E, max_rows, item_queue, ncu)
        else:
            dv = tn_dense_variant(M, N)
            hit = _tn_ws_launch("tn5", probs, [dv], E, max_rows, item_queue, ncu) if E == 1 and dv >= 0 else None
        hit = hit or _tn_ws_launch("tn3", probs, [None] * len(probs), E, max_rows, item_queue, ncu)
        if hit:
            return hit
    return {"kernel": "grouped_gemm_tn2_k", "targs": (), "path": f"tn2<{'pair' if pair else 'single'}>",
            "launches": [("grouped_gemm_tn2_k", ())], "tile": (128, 128), "pair": bool(pair), "fold": False,
            "m_partial": any(m % 128 for m, _ in probs), "n_partial": any(n % 128 for _, n in probs)}


def kernel_name_targs(name, kernel):
    """(template arguments, complete) as a device kernel's name shows them, written as the mirror writes them: 'f32' / 'bf16',
    True / False, integers.  The profiler's demangler does not know the bf16 type code (DF16b): such a name comes back either
    still mangled - then every argument is legible - or, where the literal behind the type code is 1 / true, garbled
    ("<bool _Accum, bool, E, false>") with only the booleans after it intact - then those are returned and `complete` is False."""
    rest = name[name.index(kernel) + len(kernel):]
    m = re.match(r"I((?:DF16b|f|Lb[01]E|Li\d+E)+)E", rest)
    if m:                                                      # Itanium mangling: I <args> E
        return tuple("bf16" if t == "DF16b" else "f32" if t == "f" else t == "Lb1E" if t[1] == "b" else int(t[2:-1])
                     for t in re.findall(r"DF16b|f|Lb[01]E|Li\d+E", m.group(1))), True
    if not rest.startswith("<"):
        return (), True
    depth, end = 0, 0
    for k, ch in enumerate(rest):
        depth += ch == "<"
        depth -= ch == ">"
        if depth == 0:
            end = k
            break
    toks = [t.strip() for t in rest[1:end].split(",")]
    if "_Accum" in rest[1:end]:
        tail = []
        while toks and toks[-1] in ("true", "false"):
            tail.insert(0, toks.pop() == "true")
        return tuple(tail), False
    return tuple(True if t == "true" else False if t == "false" else int(t) if t.lstrip("-").isdigit() else
                 "f32" if t == "float" else "bf16" for t in toks), True



# ---------------------------------------------------------------------------------------------------------------------------
# case tables
def edges(h):
    """Group sizes with an empty group first, in the middle and last, a group of one row and boundaries at a tile height minus
    one, exactly a tile height and plus one: 3 h + 1 rows in 7 groups."""
    return (0, h - 1, 1, 0, h, h + 1, 0)


def nt(cid, sizes, N, K, pad=0, act=ACT_NONE, p=0.0, bias=True, pre=False, mul=None, queue=False, flags=0, dtype=BF16, out=BF16,
       max_rows=4096, bound=31):
    """One NT call.  sizes: rows per group; pad: ldw - K (W's pad columns are zero); mul: None | "saved" (MUL_SAVED, act_bwd_pre
    drawn from {0, +-1/2, +-1, +-2}) | "act" (act_bwd_pre = a pre-activation); bound: |n|, |m| of the operands' grid (smaller
    where the activation should see |pre| of a few units at most)."""
    return dict(id=cid, sizes=tuple(sizes), N=N, K=K, ldw=K + pad, act=act, flags=flags | (MUL_SAVED if mul == "saved" else 0),
                p=p, bias=bias, pre=pre, mul=mul, queue=queue, dtype=dtype, out=out, max_rows=max_rows, bound=bound)


def nt_case_path(c, ncu):
    return nt_path(c["dtype"], c["out"], c["max_rows"], c["N"], c["K"], c["ldw"], len(c["sizes"]), c["act"] | c["flags"], c["p"],
                   c["pre"], c["mul"] is not None, c["bias"], c["queue"], ncu)


E7, E3 = edges(256), edges(128)
QROWS = (0, 255, 1, 0, 256, 257, 1300, 0)                 # 2 069 rows in 8 groups: 11 real m-tiles of 256
BIG = (0, 2047, 1, 2048, 2049, 0, 3000, 0)                # 9 145 rows in 8 groups: 38 real m-tiles of 256 - with 8 n-tiles or more
BIG_ROWS = 10240                                          # there are more valid tiles than CUs: a persistent work-group walks on
WALK = (300, 0, 257, 511, 1, 256, 255, 700)           # 2 280 rows: 12 real m-tiles of 256 - the grouped tile walk runs
NT_CASES = [
    # --- the skinny kernel (max_rows <= 64): one wave, four waves, sixteen waves splitting K; rows <= 16 and several row blocks
    nt("skinny1-k8", (1,), 8, 8, max_rows=1, bias=False),
    nt("skinny1-k504-pad-relu", (0, 15, 1, 0, 16, 17, 0), 40, 504, pad=8, act=ACT_RELU, max_rows=64),
    nt("skinny1-k264-gelu", (5, 0, 11), 24, 264, act=ACT_GELU, max_rows=16, bound=7),
    nt("skinny4-k512", (0, 15, 1, 0, 16, 17, 0), 24, 512, max_rows=64, bias=False),
    nt("skinny4-k2040-pad-silu", (7, 0, 9), 40, 2040, pad=8, act=ACT_SILU, max_rows=16, bound=3),
    nt("skinny16-k2048", (0, 15, 1, 0, 16, 17, 0), 40, 2048, max_rows=64),
    nt("skinny16-k2824-pad-relu", (3, 0, 13), 24, 2824, pad=56, act=ACT_RELU, bias=False, max_rows=16),
    # --- nt352p: N % 352 == 0 by its launcher (no partial n-tile), K % 64 == 0, ldw == K, plain epilogue
    nt("352p-e1-n352-k704", (769,), 352, 704, bias=False),                    # launch_nt's quoted shape (the SSM input projection)
    nt("352p-e7-n704-k128", E7, 704, 128),
    nt("352p-e7-n704-k128-queue", E7, 704, 128, queue=True),
    nt("352p-big", BIG, 2816, 128, max_rows=BIG_ROWS),                        # 304 valid tiles: second tiles, the ring carried over
    nt("352p-big-queue", BIG, 2816, 128, max_rows=BIG_ROWS, queue=True),      # ... and tickets drawn from the queue
    # --- nt4r<ragged, queue>
    nt("4r-relu-drop", E7, 520, 160, act=ACT_RELU, p=0.5),
    nt("4r-none-drop-nobias", E7, 512, 352, p=0.5, bias=False),
    nt("4r-pre-relu", E7, 776, 192, act=ACT_RELU, pre=True),
    nt("4r-e1-dense-raw", (769,), 136, 192),                                  # one group, plain epilogue, one half-empty n-tile
    nt("4r-gelu", E7, 520, 160, act=ACT_GELU, bound=7),
    nt("4r-silu-drop", E7, 520, 160, act=ACT_SILU, p=0.5, bound=7),
    nt("4r-save-grad-drop", E7, 520, 160, act=ACT_GELU, p=0.5, pre=True, flags=SAVE_GRAD, bound=7),
    nt("4r-save-grad", E7, 640, 352, act=ACT_GELU, pre=True, flags=SAVE_GRAD, bias=False, bound=5),
    nt("4r-mul-saved", E7, 520, 160, mul="saved", bias=False),
    nt("4r-mul-act-relu-drop", E7, 520, 160, act=ACT_RELU, p=0.5, mul="act", bias=False),
    nt("4r-none-drop03", E7, 520, 160, p=0.3),                                # p * 65536 = 19660.8: the threshold is TRUNCATED
    nt("4r-big-relu", BIG, 2816, 352, act=ACT_RELU, max_rows=BIG_ROWS),       # 418 valid tiles on the ring kernel, static ...
    nt("4r-big-relu-queue", BIG, 2816, 352, act=ACT_RELU, max_rows=BIG_ROWS, queue=True),   # ... and from the queue
    nt("4r-walk-relu", WALK, 1288, 160, act=ACT_RELU),                        # 6 n-tiles, 12 m-tiles: walk_g = 8
    nt("4r-ragged-relu-drop", E7, 520, 168, pad=24, act=ACT_RELU, p=0.5),
    nt("4r-ragged-mul-saved", E7, 640, 328, pad=24, mul="saved", bias=False),
    nt("4r-ragged-e1-raw-nobias", (769,), 264, 136, pad=24, bias=False),
    nt("4r-ragged-walk-pre", WALK, 1288, 136, pad=24, act=ACT_RELU, pre=True),
    nt("4r-ragged-gelu", E7, 520, 168, pad=24, act=ACT_GELU, bound=7),
    nt("4r-queue-relu-drop", QROWS, 2816, 352, act=ACT_RELU, p=0.5, queue=True),
    nt("4r-queue-mul-saved", QROWS, 2816, 352, mul="saved", bias=False, queue=True),
    nt("4r-queue-save-grad", QROWS, 2824, 352, act=ACT_GELU, pre=True, flags=SAVE_GRAD, queue=True, bound=5),
    nt("4r-ragged-queue-relu", QROWS, 2824, 328, pad=24, act=ACT_RELU, queue=True),
    nt("4r-ragged-queue-none-drop", QROWS, 2816, 328, pad=24, p=0.5, bias=False, queue=True),
    # --- nt2x<ragged>
    nt("2x-narrow-raw", E7, 264, 160),                                        # E > 1, 256 <= N < 512, plain epilogue
    nt("2x-narrow-raw-nobias", E7, 384, 96, bias=False),
    nt("2x-shortk-relu-drop", E7, 520, 128, act=ACT_RELU, p=0.5),             # K <= 128: below the ring kernel
    nt("2x-shortk-pre-none", E7, 520, 96, pre=True),
    nt("2x-shortk-none-drop03", E7, 520, 128, p=0.3),
    nt("2x-e1-n64-raw", (769,), 72, 160),
    nt("2x-queue-relu", E7, 520, 160, act=ACT_RELU, queue=True),              # a queue on a grid too small for queue4_ok
    nt("2x-queue-mul-saved", E7, 520, 160, mul="saved", bias=False, queue=True),
    nt("2x-queue-mul-act-relu-drop", E7, 520, 160, act=ACT_RELU, p=0.5, mul="act", bias=False, queue=True),
    nt("2x-shortk-gelu-drop", E7, 520, 128, act=ACT_GELU, p=0.5, bound=7),
    nt("2x-shortk-silu", E7, 520, 96, act=ACT_SILU, bound=7),
    nt("2x-shortk-save-grad-drop", E7, 520, 128, act=ACT_GELU, p=0.5, pre=True, flags=SAVE_GRAD, bound=7),
    nt("2x-walk-queue-relu", WALK, 1160, 160, act=ACT_RELU, queue=True),      # 10 n-tiles of 128, 12 m-tiles: walk_g = 8
    nt("2x-ragged-narrow-raw", E7, 264, 168, pad=24),
    nt("2x-ragged-shortk-relu-drop", E7, 520, 104, pad=24, act=ACT_RELU, p=0.5, bias=False),
    nt("2x-ragged-queue-mul-saved", E7, 520, 168, pad=24, mul="saved", bias=False, queue=True),
    nt("2x-ragged-shortk-gelu", E7, 520, 104, pad=24, act=ACT_GELU, bound=7),
    nt("2x-ragged-walk-relu", WALK, 1160, 104, pad=24, act=ACT_RELU),
    # --- nt256p<kpad>
    nt("256p-raw", E7, 520, 192),
    nt("256p-raw-nobias-queue", E7, 520, 192, bias=False, queue=True),
    nt("256p-longk-relu-drop", E7, 520, 1088, act=ACT_RELU, p=0.5),           # K > 1024: heavy epilogues stay here
    nt("256p-longk-pre-none-drop", E7, 512, 1088, p=0.5, pre=True, bias=False),
    nt("256p-longk-mul-act-relu-drop", E7, 520, 1088, act=ACT_RELU, p=0.5, mul="act", bias=False),
    nt("256p-longk-none-drop03", E7, 520, 1088, p=0.3),
    nt("256p-longk-gelu-drop", E7, 520, 1088, act=ACT_GELU, p=0.5, bound=3),
    nt("256p-longk-silu", E7, 520, 1088, act=ACT_SILU, bound=3),
    nt("256p-big-raw", BIG, 2824, 192, max_rows=BIG_ROWS),                    # 456 valid tiles
    nt("256p-big-raw-queue", BIG, 2824, 192, max_rows=BIG_ROWS, queue=True),
    nt("256p-kpad-big-queue", BIG, 2824, 72, pad=56, bias=False, max_rows=BIG_ROWS, queue=True),
    nt("256p-kpad-raw", E7, 520, 72, pad=56),
    nt("256p-kpad-k%64-pitch", E7, 512, 128, pad=64, bias=False),             # K % 64 == 0 with a pitch of its own
    nt("256p-kpad-longk-relu-drop-queue", E7, 520, 1096, pad=56, act=ACT_RELU, p=0.5, queue=True),
    nt("256p-kpad-longk-gelu", E7, 520, 1096, pad=56, act=ACT_GELU, bound=3),
    nt("256p-kpad-e1-longk", (769,), 136, 1096, pad=56, bias=False),
    # --- the 128 x 128 kernel: bf16 (too few rows, too narrow, K not padded), bf16 -> fp32, fp32
    nt("128-bf16-raw", E3, 136, 72, max_rows=400),
    nt("128-bf16-relu-drop-nobias", E3, 128, 200, pad=8, act=ACT_RELU, p=0.5, bias=False, max_rows=400),
    nt("128-bf16-pre-relu", E3, 136, 64, act=ACT_RELU, pre=True, max_rows=400),
    nt("128-bf16-mul-act-relu-drop", E3, 136, 72, act=ACT_RELU, p=0.5, mul="act", bias=False, max_rows=400),
    nt("128-bf16-none-drop03", (1500, 1400), 248, 72, p=0.3),
    nt("128-bf16-gelu", E3, 136, 72, act=ACT_GELU, max_rows=400, bound=7),
    nt("128-bf16-silu-drop", E3, 136, 72, act=ACT_SILU, p=0.5, max_rows=400, bound=7),
    nt("128-bf16-big-narrow", E7, 136, 72),                                   # max_rows 4096, E > 1 and N < 256
    nt("128-bf16-big-unpadded-k", E7, 520, 72, bias=False),                   # K % 64 != 0 without the pad: no persistent kernel
    nt("128-mixed-raw", E3, 132, 72, out=F32, max_rows=400),
    nt("128-mixed-relu-drop-pre", E3, 132, 200, pad=8, act=ACT_RELU, p=0.5, pre=True, bias=False, out=F32, max_rows=4096),
    nt("128-mixed-gelu", E3, 132, 72, act=ACT_GELU, out=F32, max_rows=400, bound=7),
    nt("128-mixed-silu", E3, 132, 72, act=ACT_SILU, out=F32, max_rows=400, bound=7),
    nt("128-f32-raw", E3, 132, 68, dtype=F32, out=F32, max_rows=400),
    nt("128-f32-relu-drop-pre", E3, 132, 100, pad=4, act=ACT_RELU, p=0.5, pre=True, bias=False, dtype=F32, out=F32, max_rows=4096),
    nt("128-f32-mul-act-relu-drop", E3, 128, 68, act=ACT_RELU, p=0.5, mul="act", bias=False, dtype=F32, out=F32, max_rows=400),
    nt("128-f32-gelu-drop", E3, 132, 68, act=ACT_GELU, p=0.5, dtype=F32, out=F32, max_rows=400, bound=7),
    nt("128-f32-silu", E3, 132, 68, act=ACT_SILU, dtype=F32, out=F32, max_rows=400, bound=7),
]

# the same problem on two kernels (or two walks of one): (id a, id b) - C (and pre_act) must be equal bit for bit
NT_TWINS = [
    ("352p-big", "352p-big-queue"),                                           # static walk and tile queue of one kernel, with
    ("256p-big-raw", "256p-big-raw-queue"),                                   # more valid tiles than CUs: tickets are drawn
    ("4r-big-relu", "4r-big-relu-queue"),
    ("4r-relu-drop", "2x-queue-relu-drop-twin"),                              # a queue too small for queue4_ok: nt4r -> nt2x
    ("4r-mul-saved", "2x-queue-mul-saved"),
    ("4r-save-grad-drop", "2x-queue-save-grad-drop-twin"),
]
NT_CASES += [
    nt("2x-queue-relu-drop-twin", E7, 520, 160, act=ACT_RELU, p=0.5, queue=True),
    nt("2x-queue-save-grad-drop-twin", E7, 520, 160, act=ACT_GELU, p=0.5, pre=True, flags=SAVE_GRAD, queue=True, bound=7),
]

# refused calls: (id, case, return code).  Every refusal launch_nt and apertis_grouped_gemm_nt_q make on a shape or a flag.
NT_REFUSED = [
    ("ldw-below-k", nt("r", E7, 520, 160, pad=-8), ERR_ARG),
    ("drop-p-one", nt("r", E7, 520, 160, p=1.0), ERR_ARG),
    ("act-bwd-pre-with-bias", nt("r", E7, 520, 160, act=ACT_RELU, mul="act", bias=True), ERR_ARG),
    ("act-bwd-pre-with-pre-act", nt("r", E7, 520, 160, act=ACT_RELU, mul="act", pre=True, bias=False), ERR_ARG),
    ("save-grad-without-pre-act", nt("r", E7, 520, 160, act=ACT_GELU, flags=SAVE_GRAD), ERR_ARG),
    ("mul-saved-without-act-bwd-pre", nt("r", E7, 520, 160, flags=MUL_SAVED, bias=False), ERR_ARG),
    ("k-not-8", nt("r", E7, 520, 164), ERR_UNSUPPORTED),
    ("n-not-8", nt("r", E7, 516, 160), ERR_UNSUPPORTED),
    ("ldw-unaligned", nt("r", E7, 520, 160, pad=4), ERR_UNSUPPORTED),
    ("f32-in-bf16-out", nt("r", E3, 136, 72, dtype=F32, out=BF16, max_rows=400), ERR_UNSUPPORTED),
    ("f32-k-not-4", nt("r", E3, 132, 70, dtype=F32, out=F32, max_rows=400), ERR_UNSUPPORTED),
    ("save-grad-relu", nt("r", E7, 520, 160, act=ACT_RELU, pre=True, flags=SAVE_GRAD), ERR_UNSUPPORTED),
    ("save-grad-few-rows", nt("r", E3, 520, 160, act=ACT_GELU, pre=True, flags=SAVE_GRAD, max_rows=400), ERR_UNSUPPORTED),
    ("save-grad-narrow", nt("r", E7, 136, 160, act=ACT_GELU, pre=True, flags=SAVE_GRAD), ERR_UNSUPPORTED),
    ("save-grad-long-k", nt("r", E7, 520, 1088, act=ACT_GELU, pre=True, flags=SAVE_GRAD), ERR_UNSUPPORTED),
    ("save-grad-unpadded-k", nt("r", E7, 520, 168, act=ACT_GELU, pre=True, flags=SAVE_GRAD), ERR_UNSUPPORTED),
    ("save-grad-fp32", nt("r", E3, 132, 68, act=ACT_GELU, pre=True, flags=SAVE_GRAD, dtype=F32, out=F32, max_rows=400), ERR_UNSUPPORTED),
    ("mul-saved-short-k", nt("r", E7, 520, 88, mul="saved", bias=False), ERR_UNSUPPORTED),
]


def tn(cid, sizes, M, N, dbias=True, dtype=BF16, forms=("ws", "queue", "nows"), pair=None):
    """One TN problem (or a pair over the same grouping) and the forms it is run in: with a workspace, with the workspace and the
    item queue, without a workspace."""
    return dict(id=cid, sizes=tuple(sizes), M=M, N=N, dbias=dbias, dtype=dtype, forms=tuple(forms), pair=pair)


def tn_case_path(c, form, ncu):
    return tn_path(c["dtype"], c["M"], c["N"], len(c["sizes"]), form in ("ws", "queue"), form == "queue", ncu, pair=c["pair"],
                   max_rows=max(sum(c["sizes"]), 1))


def spread(E, rows, empty=()):
    """E group sizes that sum to about `rows`, uneven (1, 2, 3 ... shares), with the groups in `empty` left without rows."""
    w = [0 if e in empty else 1 + (e * 7) % 5 for e in range(E)]
    return tuple(rows * x // max(sum(w), 1) for x in w)


TN_CASES = [
    # tn5 as a single group (E = 1, the dense variant): both tile shapes, partial tiles on both sides, 85 / 64 slices of 32-row
    # blocks over a few hundred rows (most slices get no rows)
    tn("tn5-wide-264x1000", (777,), 264, 1000),
    tn("tn5-narrow-200x1240", (1500,), 200, 1240, dbias=False),
    tn("tn5-narrow-256x1056-empty", (0,), 256, 1056),                          # all groups empty: zeros
    # tn3 single: a fold (s > 1), full rounds only (rem == 0), one CU per remainder tile (s == 1), full + fold
    tn("tn3-e8-fold", spread(8, 2400, empty=(0, 4, 7)), 512, 520),
    tn("tn3-e64-rem0", spread(64, 3000, empty=(5,)), 512, 512, dbias=False),
    tn("tn3-e64-s1", spread(64, 3000, empty=(63,)), 768, 256),
    tn("tn3-e64-full+fold", spread(64, 3000), 520, 264),
    tn("tn3-e1-small", (1300,), 136, 264),                                     # one group the dense variant declines
    tn("tn3-e8-all-empty", (0,) * 8, 264, 136),
    # no workspace can apply: more groups than CUs
    tn("tn2-e300", spread(300, 2000, empty=(0, 150, 299)), 136, 200, forms=("ws", "nows")),
    tn("tn2-e3-edges", E3, 264, 136, dbias=False, forms=("nows",)),
    # fp32
    tn("tn-f32-edges", E3, 132, 260, dtype=F32, forms=("nows",)),
    tn("tn-f32-empty", (0, 0), 128, 128, dbias=False, dtype=F32, forms=("nows",)),
]
TN_PAIR_CASES = [
    tn("pair-tn5-e64-rem0", spread(64, 3000, empty=(0, 33)), 704, 256, pair=(256, 704)),
    tn("pair-tn5-e16-fold", spread(16, 3000, empty=(15,)), 704, 264, pair=(264, 704), dbias=False),
    tn("pair-tn5-e32-s1", spread(32, 2500), 1056, 256, pair=(256, 1056)),
    tn("pair-tn3-e32-nofold", spread(32, 3000, empty=(7,)), 512, 512, pair=(512, 512)),
    tn("pair-tn3-e8-fold", spread(8, 2400, empty=(3,)), 520, 136, pair=(136, 520), dbias=False),
    tn("pair-tn5-all-empty", (0,) * 32, 704, 256, pair=(256, 704)),
    tn("pair-tn3-all-empty", (0,) * 8, 520, 136, pair=(136, 520)),
    tn("pair-tn2-e200", spread(200, 2000), 136, 200, pair=(200, 136), forms=("ws", "nows")),
    tn("pair-f32", E3, 132, 68, pair=(68, 132), dtype=F32, forms=("nows",)),
]
TN_REFUSED = [
    ("bf16-m-not-8", tn("r", E3, 132, 136), ERR_UNSUPPORTED),
    ("bf16-n-not-8", tn("r", E3, 136, 132), ERR_UNSUPPORTED),
    ("f32-m-not-4", tn("r", E3, 130, 136, dtype=F32), ERR_UNSUPPORTED),
    ("zero-m", tn("r", E3, 0, 136), ERR_ARG),
    ("pair-n1-not-8", tn("r", E3, 136, 136, pair=(136, 132)), ERR_UNSUPPORTED),
]

# ---------------------------------------------------------------------------------------------------------------------------
# inputs of a case, on the grid (CPU tensors; generated from the case's own fields, so twins share them)
def _case_seed(c):
    import zlib
    return zlib.crc32(repr(sorted((k, str(v)) for k, v in c.items() if k not in ("id", "queue", "forms"))).encode())


def nt_inputs(c):
    """A [max_rows, K], W [E, N, ldw] (pad columns zero), bias [E, N] fp32 or None, offsets int32 [E + 1], act_bwd_pre
    [max_rows, N] or None, and the dropout seed (both 32-bit halves in use)."""
    s = _case_seed(c)
    g = torch.Generator().manual_seed(s)
    E, N, K, ldw, R = len(c["sizes"]), c["N"], c["K"], c["ldw"], c["max_rows"]
    A = dyadic((R, K), 16, g, c["bound"]).to(c["dtype"])
    W = torch.zeros(E, N, ldw)
    W[:, :, :K] = dyadic((E, N, K), 32, g, c["bound"])
    b = dyadic((E, N), 64, g) if c["bias"] else None
    offs = torch.tensor(np.concatenate([[0], np.cumsum(c["sizes"])]).astype(np.int32))
    mul = None
    if c["mul"] == "saved":
        mul = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0])[torch.randint(0, 7, (R, N), generator=g)].to(c["out"])
    elif c["mul"] == "act":
        mul = dyadic((R, N), 16, g).to(c["out"])
    return dict(A=A, W=W.to(c["dtype"]), b=b, offs=offs, mul=mul, seed=(s * 0x9E3779B97F4A7C15 + 12345) & 0xFFFFFFFFFFFFFFFF)


def tn_inputs(c):
    """Per problem (A [rows, M], B [rows, N]) on the grid, and the offsets."""
    g = torch.Generator().manual_seed(_case_seed(c))
    R = sum(c["sizes"])
    probs = [(c["M"], c["N"])] + ([tuple(c["pair"])] if c["pair"] else [])
    ops = [(dyadic((max(R, 1), m), 16, g).to(c["dtype"]), dyadic((max(R, 1), n), 32, g).to(c["dtype"])) for m, n in probs]
    return ops, torch.tensor(np.concatenate([[0], np.cumsum(c["sizes"])]).astype(np.int32))


# every instantiation a launch can name (launch_nt; launch_tn2 / launch_tn3 / launch_tn5 and the fp32 kernel; both fold kernels)
NT_PATHS = (["nt_skinny<bf16,1>", "nt_skinny<bf16,4>", "nt_skinny<bf16,16>", "nt352p<bf16>"] +
            [f"nt4r<bf16,{r},{q}>" for r in (False, True) for q in (False, True)] + ["nt2x<bf16,False>", "nt2x<bf16,True>",
             "nt256p<bf16,False>", "nt256p<bf16,True>", "nt<bf16,bf16>", "nt<bf16,f32>", "nt<f32,f32>"])
TN_KERNELS = ["grouped_gemm_tn_k", "grouped_gemm_tn2_k", "grouped_gemm_tn3_k", "grouped_gemm_tn5_k", "tn3_fold_k", "tn5_fold_k"]
ALL_KERNELS = [f"grouped_gemm_{k}_k" for k in NT_TILES] + TN_KERNELS


def thresh_probe(c, i):
    """bool [offsets[E], N]: the live elements of a p = 0.3 case that a ROUNDED threshold (19 661) would treat differently from
    the truncated one (19 660) - those whose 16 random bits are exactly 19 660."""
    rows = int(i["offs"][-1])
    t = thresh16(c["p"])
    return torch.from_numpy(keep_mask(i["seed"], rows, c["N"], c["p"], thresh=t) != keep_mask(i["seed"], rows, c["N"], c["p"], thresh=t + 1))


def nt_valid_tiles(c, p):
    """The tiles of a launch that hold rows: the real m-tiles of every group times the n-tiles."""
    return sum(_cdiv(n, p["tile"][0]) for n in c["sizes"]) * p["n_tiles"]


def nt_row_edges(sizes, h, max_rows):
    """The row edges a case's grouping has against a tile height h."""
    E, s = len(sizes), set()
    for e, n in enumerate(sizes):
        if n == 0:
            s.add("empty-first" if e == 0 else "empty-last" if e == E - 1 else "empty-middle")
        for name, v in (("one-row", 1), ("h-1", h - 1), ("h", h), ("h+1", h + 1)):
            if n == v:
                s.add(name)
    if sum(sizes) < max_rows:
        s.add("rows-below-max")
    return s


def check_case_tables_cover_every_dispatch_path(ncu=256):
    """Every kernel instantiation the mirror can name is reached by a row of a table, with the edges the kernel admits; taking
    all rows of any one path out of a table fails an assertion here."""
    ids = [c["id"] for c in NT_CASES]
    assert len(set(ids)) == len(ids)
    seen = {}
    for c in NT_CASES:
        p = nt_case_path(c, ncu)
        assert isinstance(p, dict), (c["id"], p)
        assert dyadic_sum_bits(c["K"]) <= 24 and sum(c["sizes"]) <= c["max_rows"], c["id"]
        f = seen.setdefault(p["path"], set())
        h = p["tile"][0]
        f |= nt_row_edges(c["sizes"], h, c["max_rows"])
        f |= {("bias", c["bias"]), ("act", c["act"]), ("drop", c["p"] > 0.0), ("p", c["p"]), ("epi", p["epi"]), ("n_partial", p["n_partial"]),
              ("k_ragged", p["k_ragged"]), ("k_padded", p["k_padded"]), ("walk_g", p["walk_g"]), ("queue", c["queue"])}
        if p["k_padded"]:
            assert p["k_ragged"] or "nt256p" in p["path"] or "nt<" in p["path"] or "skinny" in p["path"], c["id"]
        if p["walk_g"]:                                            # (the kernel takes walk_g from N alone: it RUNS with > 8 m-tiles)
            assert p["n_tiles"] > (4 if "nt4r" in p["path"] else 8), c["id"]
            if sum(_cdiv(n, h) for n in c["sizes"]) > 8:
                f.add("walk-runs")
        if c["queue"] and "nt4r" in p["path"]:
            assert p["m_tiles"] * p["n_tiles"] >= ncu, c["id"]
        if nt_valid_tiles(c, p) > ncu:                             # a persistent work-group goes on to a second tile
            f |= {"walks-on", ("walks-on", "queue" if c["queue"] else "static")}
    assert set(seen) == set(NT_PATHS), (set(NT_PATHS) - set(seen), set(seen) - set(NT_PATHS))
    rows = {"empty-first", "empty-middle", "empty-last", "one-row", "h-1", "h", "h+1"}
    fam = {}                                                       # the epilogue's run-time switches: per kernel, not per instantiation
    for path, f in seen.items():
        fam.setdefault(path if path.startswith("nt<") else path.split("<")[0], set()).update(f)
    for path, f in seen.items():
        g = fam[path if path.startswith("nt<") else path.split("<")[0]]
        assert rows <= f, (path, rows - f)
        assert "rows-below-max" in f, path
        # more valid tiles than CUs: the pass of a persistent kernel that prefetches tile i + 1 under tile i's epilogue, the ring
        # carried across tiles, tickets drawn from the queue
        if path in ("nt352p<bf16>", "nt256p<bf16,False>", "nt4r<bf16,False,False>"):
            assert ("walks-on", "static") in f, path
        if path in ("nt352p<bf16>", "nt256p<bf16,False>", "nt256p<bf16,True>", "nt4r<bf16,False,True>"):
            assert ("walks-on", "queue") in f, path
        assert ("bias", True) in f and ("bias", False) in f, path
        if path.startswith("nt352p"):                              # plain epilogue, N % 352 == 0, K % 64 == 0, ldw == K by its launcher
            assert ("queue", True) in f and ("queue", False) in f
            continue
        assert ("n_partial", True) in f, path
        assert {("act", a) for a in (ACT_NONE, ACT_GELU, ACT_RELU, ACT_SILU)} <= g, (path, g)
        if path.startswith("nt_skinny"):                           # no dropout / second output in the skinny kernel
            assert ("k_padded", True) in f and ("k_padded", False) in f, path
            continue
        assert ("drop", True) in f and ("drop", False) in f and ("p", 0.5) in f, path
        if path.startswith(("nt4r", "nt2x", "nt256p", "nt<bf16,bf16>")):       # each computes thresh16 itself: truncated (p = 0.3)
            assert ("p", 0.3) in g, path
        assert ("epi", "raw") in g and ("epi", "act") in f and ("epi", "pre+act") in g, (path, g)
        if path != "nt<bf16,f32>":                                 # (the data-gradient form: bf16 or fp32 throughout)
            assert ("epi", "mul_act") in g, path
        if path.startswith(("nt4r", "nt2x")):
            assert ("epi", "mul_saved") in g and ("epi", "save_grad") in g, path
            assert ("walk_g", 8) in f and "walk-runs" in f and ("walk_g", 0) in g, path
            assert (("k_ragged", True) in f and ("k_padded", True) in f) if path.split(",")[1].startswith("True") else ("k_ragged", False) in f, path
        if path in ("nt256p<bf16,True>", "nt<bf16,bf16>", "nt<f32,f32>", "nt<bf16,f32>"):
            assert ("k_ragged", True) in f and ("k_padded", True) in f, path
        if path.startswith("nt256p"):
            assert ("queue", True) in f and ("queue", False) in f, path
    # the twins name rows of the table, on different paths or walks
    by_id = {c["id"]: c for c in NT_CASES}
    twin_kinds = set()
    for a, b in NT_TWINS:
        ca, cb = by_id[a], by_id[b]
        same = {k: v for k, v in ca.items() if k not in ("id", "queue")}
        assert same == {k: v for k, v in cb.items() if k not in ("id", "queue")} and ca["queue"] != cb["queue"], (a, b)
        pa, pb = nt_case_path(ca, ncu), nt_case_path(cb, ncu)
        if pa["kernel"] == pb["kernel"]:                           # two walks of one kernel differ only where tiles are drawn from the queue
            assert nt_valid_tiles(ca, pa) > ncu, (a, b)
        twin_kinds.add((pa["path"].split("<")[0], pb["path"].split("<")[0]))
    assert {("nt352p", "nt352p"), ("nt256p", "nt256p"), ("nt4r", "nt2x"), ("nt4r", "nt4r")} <= twin_kinds, twin_kinds
    # refusals
    for name, c, rc in NT_REFUSED:
        assert nt_case_path(c, ncu) == rc, (name, nt_case_path(c, ncu), rc)
    assert {rc for _, _, rc in NT_REFUSED} == {ERR_ARG, ERR_UNSUPPORTED}
    need = {"ldw-unaligned", "save-grad-without-pre-act", "save-grad-narrow", "act-bwd-pre-with-bias", "k-not-8"}
    assert need <= {n for n, _, _ in NT_REFUSED}

    # TN
    kernels, facts = set(), set()
    for table, is_pair in ((TN_CASES, False), (TN_PAIR_CASES, True)):
        for c in table:
            assert (c["pair"] is not None) == is_pair and max(c["sizes"] + (1,)) <= MAX_DEPTH, c["id"]
            for form in c["forms"]:
                p = tn_case_path(c, form, ncu)
                assert isinstance(p, dict), (c["id"], form, p)
                kernels |= {k for k, _ in p["launches"]}
                kind = p["path"].split("<")[0]
                facts |= {(kind, is_pair, "fold" if p["fold"] else "nofold"), (kind, is_pair, "dbias", c["dbias"]), (kind, is_pair, form)}
                if sum(c["sizes"]) == 0:
                    facts.add((kind, is_pair, "all-empty"))
                if any(n == 0 for n in c["sizes"]) and sum(c["sizes"]):
                    facts.add((kind, is_pair, "some-empty"))
                for q in p.get("problems", ()):
                    facts |= {(kind, is_pair, "rem0") if q["rem"] == 0 else (kind, is_pair, "s1") if q["s"] == 1 else (kind, is_pair, "s>1"),
                              (kind, is_pair, "wide_m", q["wide_m"]), (kind, is_pair, "m_partial", q["m_partial"]),
                              (kind, is_pair, "n_partial", q["n_partial"])}
                    if q["full"] and q["rem"] and q["s"] > 1:
                        facts.add((kind, is_pair, "full+fold"))
                if "problems" not in p:
                    facts |= {(kind, is_pair, "m_partial", p["m_partial"]), (kind, is_pair, "n_partial", p["n_partial"])}
    assert kernels == set(TN_KERNELS), (kernels, TN_KERNELS)
    need = []
    for kind, is_pair in (("tn5", False), ("tn5", True), ("tn3", False), ("tn3", True)):
        need += [(kind, is_pair, "fold"), (kind, is_pair, "s>1"), (kind, is_pair, "dbias", True), (kind, is_pair, "dbias", False),
                 (kind, is_pair, "ws"), (kind, is_pair, "queue"), (kind, is_pair, "all-empty"),
                 (kind, is_pair, "m_partial", True), (kind, is_pair, "n_partial", True)]
        if (kind, is_pair) != ("tn5", False):                      # one group on 256 CUs: T < cpg always - every tile is split
            need += [(kind, is_pair, "nofold"), (kind, is_pair, "rem0")]
    need += [("tn5", False, "wide_m", 0), ("tn5", False, "wide_m", 1), ("tn5", True, "wide_m", 0), ("tn5", True, "wide_m", 1),
             ("tn5", True, "s1"), ("tn3", False, "s1"), ("tn3", False, "full+fold"), ("tn3", False, "some-empty"), ("tn5", True, "some-empty"),
             ("tn2", False, "nows"), ("tn2", False, "ws"), ("tn2", True, "nows"), ("tn2", True, "ws"), ("tn2", False, "some-empty"),
             ("tn2", False, "m_partial", True), ("tn2", False, "n_partial", True), ("tn2", False, "dbias", False), ("tn2", False, "dbias", True),
             ("tn", False, "nows"), ("tn", True, "nows"), ("tn", False, "all-empty"), ("tn", False, "m_partial", True),
             ("tn", False, "n_partial", True), ("tn", False, "dbias", False), ("tn", False, "dbias", True)]
    for n in need:
        assert n is None or n in facts, n
    for name, c, rc in TN_REFUSED:
        assert tn_case_path(c, "nows", ncu) == rc and tn_case_path(c, "ws", ncu) == rc, (name, rc)
    assert {rc for _, _, rc in TN_REFUSED} == {ERR_ARG, ERR_UNSUPPORTED}
