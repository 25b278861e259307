"""The two ends of a training step without a GPU: the entry points of csrc/small_linear.hip (the router's skinny linear, the
SSM's tiny linear), csrc/loss.hip (shifted cross entropy) and csrc/optimizer.hip (clip + AdamW) refuse bad arguments before any
launch.  A call that passes validation is made only where the entry point returns before launching (B = 0, T = 0 on the
forwards, n_chunks = 0): apertis_skinny_linear_bwd, apertis_tiny_linear_bwd / _bwd_pad and apertis_clip_coef launch even at
size zero (they leave zeros, or the norm of nothing) and are therefore never called here with valid arguments."""
import pytest

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -2
F32, BF16 = 0, 1
NAN = float("nan")

# non-null stand-ins: validation happens before any launch, nothing is dereferenced
P = 0x1000          # 16-byte aligned
P_ODD = 0x1004      # not 16-byte aligned


def _lib():
    from apertis_llm_amd import _lib
    return _lib.load()


def test_the_codes_are_the_headers():
    from apertis_llm_amd import _lib
    assert (_lib.OK, _lib.ERR_ARG, _lib.ERR_UNSUPPORTED, _lib.F32, _lib.BF16) == (OK, ERR_ARG, ERR_UNSUPPORTED, F32, BF16)


# ---------------------------------------------------------------------------------------------------------------------------
# small_linear.hip
SKINNY_BAD_SHAPES = [(0, 4), (-4, 4), (6, 4), (1028, 4), (2048, 2), (64, 0), (64, -2), (64, 17), (64, 32),
                     (260, 16), (1024, 16)] + [(64, N) for N in (1, 3, 5, 6, 7, 9, 12, 15)]


def test_skinny_linear_fwd_validates_before_any_launch():
    lib = _lib()
    good = dict(x=P, W=P, b=P, y=P, T=3, K=64, N=4, dt=F32, st=None)

    def call(**kw):
        a = {**good, **kw}
        return lib.apertis_skinny_linear_fwd(a["x"], a["W"], a["b"], a["y"], a["T"], a["K"], a["N"], a["dt"], a["st"])
    for name in ("x", "W", "y"):
        assert call(**{name: None}) == ERR_ARG, name
    assert call(T=-1) == ERR_ARG
    for K, N in SKINNY_BAD_SHAPES:
        assert call(K=K, N=N) == ERR_UNSUPPORTED, (K, N)
    assert call(dt=2) == ERR_ARG and call(dt=-1) == ERR_ARG
    # nothing to do: returned before the launch, with and without a bias, at both ends of the accepted shapes
    assert call(T=0) == OK and call(T=0, b=None) == OK and call(T=0, K=1024, N=8, dt=BF16) == OK and call(T=0, K=256, N=16) == OK
    assert call(T=0, K=260, N=16) == ERR_UNSUPPORTED and call(T=0, x=None) == ERR_ARG


def test_skinny_linear_bwd_validates_before_any_launch():
    lib = _lib()
    good = dict(x=P, W=P, dy=P, dx=P, part=P, out=P, T=3, K=64, N=4, dt=F32, st=None)

    def call(**kw):
        a = {**good, **kw}
        return lib.apertis_skinny_linear_bwd(a["x"], a["W"], a["dy"], a["dx"], a["part"], a["out"], a["T"], a["K"], a["N"], a["dt"],
                                             a["st"])
    for name in ("x", "W", "dy", "dx", "part", "out"):
        assert call(**{name: None}) == ERR_ARG, name
    assert call(T=-1) == ERR_ARG
    for K, N in SKINNY_BAD_SHAPES:
        assert call(K=K, N=N) == ERR_UNSUPPORTED, (K, N)
        assert call(K=K, N=N, T=0) == ERR_UNSUPPORTED, (K, N)
    assert call(dt=2) == ERR_ARG and call(dt=-1) == ERR_ARG
    # the workspace rows: one block per 32 rows (four waves of RPW = 8), one block for nothing
    assert [lib.apertis_skinny_linear_bwd_blocks(T) for T in (-5, 0, 1, 32, 33, 32777)] == [1, 1, 1, 1, 2, 1025]


TINY_BAD_SHAPES = [(0, 4), (-1, 4), (65, 4), (128, 4), (8, 0), (8, -1), (8, 17), (8, 64)]


def test_tiny_linear_fwd_validates_before_any_launch():
    lib = _lib()
    good = dict(x=P, ldx=48, W=P, b=P, y=P, T=3, K=22, N=11, dt=BF16, st=None)

    def call(**kw):
        a = {**good, **kw}
        return lib.apertis_tiny_linear_fwd(a["x"], a["ldx"], a["W"], a["b"], a["y"], a["T"], a["K"], a["N"], a["dt"], a["st"])
    for name in ("x", "W", "y"):
        assert call(**{name: None}) == ERR_ARG, name
    assert call(T=-1) == ERR_ARG and call(ldx=21) == ERR_ARG and call(ldx=0) == ERR_ARG and call(ldx=-48) == ERR_ARG
    for K, N in TINY_BAD_SHAPES:
        assert call(K=K, N=N, ldx=128) == ERR_UNSUPPORTED, (K, N)
    assert call(dt=2) == ERR_ARG and call(dt=-1) == ERR_ARG
    assert call(T=0) == OK and call(T=0, b=None) == OK and call(T=0, K=64, N=16, ldx=64, dt=F32) == OK and call(T=0, K=1, N=1, ldx=1) == OK
    assert call(T=0, K=65, ldx=65) == ERR_UNSUPPORTED and call(T=0, ldx=21) == ERR_ARG


def test_tiny_linear_doc_fwd_validates_before_any_launch():
    lib = _lib()
    good = dict(x=P, ldx=48, W=P, b=P, start=P, reset=-30.0, y=P, T=6, L=3, K=22, N=11, dt=BF16, st=None)

    def call(**kw):
        a = {**good, **kw}
        return lib.apertis_tiny_linear_doc_fwd(a["x"], a["ldx"], a["W"], a["b"], a["start"], a["reset"], a["y"], a["T"], a["L"],
                                               a["K"], a["N"], a["dt"], a["st"])
    for form in (dict(), dict(x=None)):           # the projection form and the overwrite-only form share these
        assert call(start=None, **form) == ERR_ARG and call(y=None, **form) == ERR_ARG
        assert call(T=-3, **form) == ERR_ARG and call(L=0, **form) == ERR_ARG and call(L=-3, **form) == ERR_ARG
        assert call(T=7, **form) == ERR_ARG, "T must be whole sequences of L"
        assert call(reset=NAN, **form) == ERR_ARG and call(N=0, **form) == ERR_ARG
    assert call(W=None) == ERR_ARG and call(ldx=21) == ERR_ARG
    for K, N in TINY_BAD_SHAPES:
        if N >= 1:
            assert call(K=K, N=N, ldx=128) == ERR_UNSUPPORTED, (K, N)
    assert call(dt=2) == ERR_ARG and call(dt=-1) == ERR_ARG
    assert call(T=0) == OK and call(T=0, b=None) == OK
    # overwrite only: W, b, K and the dtype are unused and N is free
    assert call(T=0, x=None, W=None, b=None, K=0, N=20, dt=7) == OK


def test_tiny_linear_bwd_validates_before_any_launch():
    lib = _lib()
    good = dict(x=P, ldx=48, W=P, dy=P, dx=P, lddx=48, part=P, out=P, T=3, K=22, N=11, zero_to=24, dt=BF16, st=None)

    def pad(**kw):
        a = {**good, **kw}
        return lib.apertis_tiny_linear_bwd_pad(a["x"], a["ldx"], a["W"], a["dy"], a["dx"], a["lddx"], a["part"], a["out"], a["T"],
                                               a["K"], a["N"], a["zero_to"], a["dt"], a["st"])

    def plain(**kw):
        a = {**good, **kw}
        return lib.apertis_tiny_linear_bwd(a["x"], a["ldx"], a["W"], a["dy"], a["dx"], a["lddx"], a["part"], a["out"], a["T"],
                                           a["K"], a["N"], a["dt"], a["st"])
    for call in (pad, plain):
        for name in ("x", "W", "dy", "dx", "part", "out"):
            assert call(**{name: None}) == ERR_ARG, name
        assert call(T=-1) == ERR_ARG and call(ldx=21) == ERR_ARG and call(lddx=21) == ERR_ARG
        for K, N in TINY_BAD_SHAPES:
            assert call(K=K, N=N, ldx=128, lddx=128) == ERR_UNSUPPORTED, (K, N)
            assert call(K=K, N=N, ldx=128, lddx=128, T=0) == ERR_UNSUPPORTED, (K, N)
        assert call(dt=2) == ERR_ARG and call(dt=-1) == ERR_ARG
    assert pad(zero_to=49) == ERR_ARG and pad(zero_to=1 << 40) == ERR_ARG
    # the workspace rows: one block per 128 rows, at most 1024
    assert [lib.apertis_tiny_linear_bwd_blocks(T) for T in (-1, 0, 1, 128, 129, 131072, 131073, 10 ** 7)] == \
        [1, 1, 1, 1, 2, 1024, 1024, 1024]


# ---------------------------------------------------------------------------------------------------------------------------
# loss.hip
def _ce_calls(lib):
    good = dict(logits=P, labels=P, lse=P, loss=P, gscale=P, dlogits=P, B=2, L=5, V=64, ls=5, n_pos=4, ign=-100, dt=BF16, st=None)

    def fwd(**kw):
        a = {**good, **kw}
        return lib.apertis_cross_entropy_fwd(a["logits"], a["labels"], a["lse"], a["loss"], a["B"], a["L"], a["V"], a["ls"],
                                             a["n_pos"], a["ign"], a["dt"], a["st"])

    def bwd(**kw):
        a = {**good, **kw}
        return lib.apertis_cross_entropy_bwd(a["logits"], a["labels"], a["lse"], a["gscale"], a["dlogits"], a["B"], a["L"], a["V"],
                                             a["ls"], a["n_pos"], a["ign"], a["dt"], a["st"])

    def one(**kw):
        a = {**good, **kw}
        return lib.apertis_cross_entropy_fwd_bwd(a["logits"], a["labels"], a["lse"], a["loss"], a["gscale"], a["dlogits"], a["B"],
                                                 a["L"], a["V"], a["ls"], a["n_pos"], a["ign"], a["dt"], a["st"])
    return {"fwd": (fwd, ("logits", "labels", "lse", "loss")),
            "bwd": (bwd, ("logits", "labels", "lse", "gscale", "dlogits")),
            "one": (one, ("logits", "labels", "lse", "loss", "gscale", "dlogits"))}


@pytest.mark.parametrize("ep", ["fwd", "bwd", "one"])
def test_cross_entropy_validates_before_any_launch(ep):
    call, operands = _ce_calls(_lib())[ep]
    for name in operands:
        assert call(**{name: None}) == ERR_ARG, name
    assert call(B=-1) == ERR_ARG and call(L=0) == ERR_ARG and call(L=-5) == ERR_ARG
    assert call(V=0) == ERR_ARG and call(V=-8) == ERR_ARG and call(n_pos=-1) == ERR_ARG
    assert call(n_pos=6, ls=9) == ERR_ARG, "n_pos > L"
    assert call(n_pos=5, ls=5) == ERR_ARG and call(n_pos=4, ls=4) == ERR_ARG, "n_pos + 1 > label_stride"
    assert call(B=1 << 31, L=1, n_pos=1, ls=2) == ERR_ARG and call(B=1 << 16, L=1 << 15, ls=1 << 15, n_pos=4) == ERR_ARG, "B L >= 2^31"
    assert call(V=1 << 31) == ERR_ARG
    assert call(dt=2) == ERR_ARG and call(dt=-1) == ERR_ARG
    # whole 16-byte chunks of aligned rows: 8 bf16 or 4 fp32 logits
    for V in (4, 12, 63, 100):
        assert call(V=V, dt=BF16) == ERR_UNSUPPORTED, V
    for V in (2, 6, 63, 101):
        assert call(V=V, dt=F32) == ERR_UNSUPPORTED, V
    for dt in (BF16, F32):
        assert call(logits=P_ODD, dt=dt) == ERR_UNSUPPORTED
        if "dlogits" in operands:
            assert call(dlogits=P_ODD, dt=dt) == ERR_UNSUPPORTED
    # nothing to do: returned before the launch
    assert call(B=0) == OK and call(B=0, n_pos=0, ls=1) == OK and call(B=0, L=1 << 40, ls=1 << 41, n_pos=0) == OK


def test_cross_entropy_one_pass_width_bound():
    """A row of the one-pass form waits in 16 sixteen-byte registers of each of 256 threads: 32768 bf16 or 16384 fp32 logits."""
    one, _ = _ce_calls(_lib())["one"]
    assert one(V=32768 + 8, dt=BF16) == ERR_UNSUPPORTED and one(V=16384 + 4, dt=F32) == ERR_UNSUPPORTED
    assert one(V=32768 + 8, dt=BF16, B=0) == OK, "B = 0 returns before the width is looked at"
    fwd, _ = _ce_calls(_lib())["fwd"]
    assert fwd(V=32768 + 8, dt=BF16, B=0) == OK and fwd(V=32768 + 4, dt=BF16) == ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------------------
# optimizer.hip
def test_grad_sumsq_validates_before_any_launch():
    lib = _lib()
    assert lib.apertis_opt_chunk_elems() == 16384
    assert lib.apertis_grad_sumsq(P, P, P, -1, P, None) == ERR_ARG
    assert lib.apertis_grad_sumsq(P, P, P, 1 << 31, P, None) == ERR_ARG
    for i in range(4):
        a = [P, P, P, P]
        a[i] = None
        assert lib.apertis_grad_sumsq(a[0], a[1], a[2], 3, a[3], None) == ERR_ARG, i
    assert lib.apertis_grad_sumsq(P, P, P, 0, P, None) == OK and lib.apertis_grad_sumsq(None, None, None, 0, None, None) == OK


def test_clip_coef_validates_before_any_launch():
    lib = _lib()
    assert lib.apertis_clip_coef(P, 3, 1.0, None, None, None) == ERR_ARG
    assert lib.apertis_clip_coef(P, -1, 1.0, P, None, None) == ERR_ARG
    assert lib.apertis_clip_coef(None, 3, 1.0, P, None, None) == ERR_ARG
    for bad in (-1.0, -1e-30, NAN, float("-inf")):
        assert lib.apertis_clip_coef(P, 3, bad, P, None, None) == ERR_ARG, bad
        assert lib.apertis_clip_coef(None, 0, bad, P, P, None) == ERR_ARG, bad


def test_adamw_step_validates_before_any_launch():
    lib = _lib()
    hp = (1e-3, 0.9, 0.999, 1e-8, 0.01)
    assert lib.apertis_adamw_step(P, P, P, -1, *hp, 1, P, None) == ERR_ARG
    assert lib.apertis_adamw_step(P, P, P, 1 << 31, *hp, 1, P, None) == ERR_ARG
    for step in (0, -1, -(1 << 40)):
        assert lib.apertis_adamw_step(P, P, P, 3, *hp, step, P, None) == ERR_ARG, step
        assert lib.apertis_adamw_step(P, P, P, 0, *hp, step, P, None) == ERR_ARG, step
    for i in range(3):
        a = [P, P, P]
        a[i] = None
        assert lib.apertis_adamw_step(*a, 3, *hp, 1, P, None) == ERR_ARG, i
    assert lib.apertis_adamw_step(P, P, P, 0, *hp, 1, P, None) == OK
    assert lib.apertis_adamw_step(None, None, None, 0, *hp, 10 ** 6, None, None) == OK
