"""generate()'s next-token selection: repetition penalty, temperature, top-k, top-p and the draw (or the argmax), then the pad /
eos / occurrence-count bookkeeping, in ONE launch per token step (csrc/sampling.hip; reference core.py:1605-1633).

Part of apertis_llm_amd.ops.  torch is used for device memory and streams only.  Nothing in the per-step call reads a device
value on the host: it runs inside the decode graph's capture.  Errors the kernel finds (a row with no finite weight, a step
outside SAMPLE_UNIFORMS) land in a device word that the caller reads at a sync it already has (Sampler.check).
"""
import torch

from .. import _lib
from .._lib import ApertisHipError, dtype_code, ptr, stream_ptr
from ._base import _launch, _require_gpu

# generate() selects its tokens with the kernel below when this is on and the call qualifies (sampling or a repetition
# penalty, CUDA logits, a supported vocabulary); off: the stock torch block everywhere (A/B and tests)
SAMPLE_FUSED = True
# test hook: a [B, steps] tensor of uniforms in [0, 1) that replaces the counter hash, u = SAMPLE_UNIFORMS[b, step]
SAMPLE_UNIFORMS = None
SAMPLE_MAX_VOCAB = _lib.CONSTANTS["APERTIS_SAMPLE_MAX_VOCAB"]
SAMPLE_MAX_ROWS = _lib.CONSTANTS["APERTIS_SAMPLE_MAX_ROWS"]          # (the occurrence table's launch)
ERR_NOT_FINITE, ERR_UNIFORMS, ERR_TOKEN_ID = 1, 2, 4


def sample_supported(logits):
    """Whether sample_next and token_counts take these last-position logits [B, V] (fp32 or bf16 on a ROCm device,
    1 <= V <= 262 144, 1 <= B <= 65 535)."""
    return (logits.is_cuda and logits.dim() == 2 and logits.dtype in (torch.float32, torch.bfloat16)
            and 1 <= logits.shape[-1] <= SAMPLE_MAX_VOCAB and 1 <= logits.shape[0] <= SAMPLE_MAX_ROWS)


def token_counts(tokens, vocab_size, err):
    """int32 [B, V] occurrence table of the rows of `tokens` (int64 [B, L]): what the repetition penalty divides by.  Ids >= V
    are skipped and ids in [-V, 0) wrap, as the reference's loop and indexing do; an id below -V sets ERR_TOKEN_ID in `err`."""
    _require_gpu(tokens, err)
    if tokens.dim() != 2:
        raise ApertisHipError(f"token_counts: tokens of shape {tuple(tokens.shape)}, expected [B, L]")
    if tokens.dtype != torch.int64 or tokens.stride(-1) != 1:
        tokens = tokens.to(torch.int64).contiguous()
    B, L = tokens.shape
    counts = torch.zeros(B, vocab_size, dtype=torch.int32, device=tokens.device)
    _launch("apertis_token_counts", _lib.load().apertis_token_counts,
            (ptr(tokens), tokens.stride(0), B, L, vocab_size, ptr(counts), ptr(err), stream_ptr()))
    return counts


def sample_next(logits, alive, err, *, do_sample, temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0, counts=None,
                eos=None, pad=0, seed=0, step=None, step_off=0, alive_out=None, out=None, uniforms=None, probs_out=None,
                x_out=None, u_out=None):
    """The next token of every row from its logits [B, V] (fp32 or bf16, unit column stride): int64 [B] (`out` if given).
    alive int64 [B]: finished rows get `pad`; alive_out (default: alive, in place) is cleared where the token is in `eos`
    (int64 device tensor); counts (int32 [B, V] or None) is what the penalty reads, incremented at the token.  temperature is
    used as given (generate() passes max(temperature, 1e-6)).  step: int64 device tensor [1] (read only) + step_off, the
    counter of the draw and the column of `uniforms` (fp64 [B, cols]).  probs_out fp32 [B, V] (final distribution), x_out fp32
    [B, V] (the row after penalty and temperature), u_out fp64 [B]: test outputs."""
    _require_gpu(logits, alive, err, counts, eos, step, alive_out, out, uniforms, probs_out, x_out, u_out)
    if not sample_supported(logits):
        raise ApertisHipError(f"sample_next: logits {tuple(logits.shape)} {logits.dtype} (fp32 or bf16 [B, V], V <= {SAMPLE_MAX_VOCAB})")
    B, V = logits.shape
    if logits.stride(-1) != 1:
        logits = logits.contiguous()
    top_k = int(top_k) if top_k and top_k > 0 else 0
    if do_sample and top_k > V:
        raise RuntimeError(f"selected index k out of range: top_k = {top_k} > vocabulary size {V}")   # (torch.topk's error)
    for name, t, dt, shape in (("alive", alive, torch.int64, (B,)), ("err", err, torch.int32, (1,)),
                               ("counts", counts, torch.int32, (B, V)), ("alive_out", alive_out, torch.int64, (B,)),
                               ("out", out, torch.int64, (B,)), ("probs_out", probs_out, torch.float32, (B, V)),
                               ("x_out", x_out, torch.float32, (B, V)),
                               ("u_out", u_out, torch.float64, (B,)), ("step", step, torch.int64, (1,))):
        if t is not None and (t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous()):
            raise ApertisHipError(f"sample_next: {name} must be a contiguous {dt} tensor of shape {shape}")
    if eos is not None and (eos.dtype != torch.int64 or eos.dim() != 1 or not eos.is_contiguous()):
        raise ApertisHipError("sample_next: eos must be a contiguous int64 vector")
    if uniforms is not None and (uniforms.dtype != torch.float64 or uniforms.dim() != 2 or uniforms.shape[0] != B
                                 or uniforms.stride(-1) != 1):
        raise ApertisHipError(f"sample_next: uniforms must be fp64 [{B}, steps] with unit column stride")
    if out is None:
        out = torch.empty(B, dtype=torch.int64, device=logits.device)
    if alive_out is None:
        alive_out = alive
    n_eos = 0 if eos is None else eos.numel()
    _launch("apertis_sample_next", _lib.load().apertis_sample_next,
            (ptr(logits), logits.stride(0), dtype_code(logits), B, V, ptr(counts), float(repetition_penalty), int(bool(do_sample)),
             float(temperature), top_k, float(top_p), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(step), int(step_off), ptr(alive),
             ptr(alive_out), ptr(eos) if n_eos else None, n_eos, int(pad), ptr(out), ptr(uniforms),
             0 if uniforms is None else uniforms.stride(0), 0 if uniforms is None else uniforms.shape[1], ptr(probs_out),
             ptr(x_out), ptr(u_out), ptr(err), stream_ptr()))
    return out


def raise_sample_error(code):
    if code & ERR_NOT_FINITE:
        raise ApertisHipError("probability tensor contains either `inf`, `nan` or element < 0 (a sampled row had no finite "
                              "logits after penalty / temperature)")
    if code & ERR_UNIFORMS:
        raise ApertisHipError("SAMPLE_UNIFORMS has no column for a decoded step")
    if code & ERR_TOKEN_ID:
        raise IndexError("a token id below -vocab_size in the sequence the repetition penalty reads")
    if code:
        raise ApertisHipError(f"sampling error word {code}")


class Sampler:
    """generate()'s per-call sampling state: the settings, the seed (drawn once per call from torch's CPU generator, as the
    dropout seeds are, so torch.manual_seed reproduces a sampled run), the occurrence table built from the prompt, the eos
    list on the device, the error word and a zero step counter for the eager steps.  The decode graph's tail reuses the same
    tensors (counts and error word as static buffers) and draws with the same (seed, row, step) counter."""

    def __init__(self, logits, tokens, *, do_sample, temperature, top_k, top_p, repetition_penalty, eos, pad):
        B, V = logits.shape
        dev = logits.device
        self.do_sample = bool(do_sample)
        self.temp = max(temperature, 1e-6) if do_sample else 1.0
        self.top_k = int(top_k) if (do_sample and top_k is not None and top_k > 0) else 0
        if self.top_k > V:
            raise RuntimeError(f"selected index k out of range: top_k = {self.top_k} > vocabulary size {V}")
        self.top_p = float(top_p) if do_sample else 1.0
        self.penalty = float(repetition_penalty)
        self.pad = int(pad)
        self.seed = int(torch.empty((), dtype=torch.int64).random_().item()) if do_sample else 0
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)
        self.counts = token_counts(tokens, V, self.err) if self.penalty != 1.0 else None
        ids = [int(e) for e in eos if e is not None]
        self.eos = torch.tensor(ids, dtype=torch.int64, device=dev) if ids else None
        self.zero_step = torch.zeros(1, dtype=torch.int64, device=dev)
        u = SAMPLE_UNIFORMS
        self.uniforms = None if u is None else u.to(device=dev, dtype=torch.float64).contiguous()

    def step(self, logits, alive, step_off, step=None, alive_out=None, out=None):
        """The tokens of one step (int64 [B]); alive_out (default: a new tensor) gets the alive flags after it."""
        if alive_out is None:
            alive_out = torch.empty_like(alive)
        return sample_next(logits, alive, self.err, do_sample=self.do_sample, temperature=self.temp, top_k=self.top_k,
                           top_p=self.top_p, repetition_penalty=self.penalty, counts=self.counts, eos=self.eos, pad=self.pad,
                           seed=self.seed, step=self.zero_step if step is None else step, step_off=step_off,
                           alive_out=alive_out, out=out, uniforms=self.uniforms), alive_out

    def check(self, code=None):
        """Raise what the kernel reported (reads the error word: a host sync, unless the caller hands its value over)."""
        raise_sample_error(int(self.err[0]) if code is None else int(code))
