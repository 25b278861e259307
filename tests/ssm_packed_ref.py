"""Packed selective_ssm rows restated in fp64 (torch, CPU): the depthwise causal conv + SiLU that stops at document starts, and
the recurrence + skip + gate whose state is reset there - with their gradients through torch autograd.  The kernels under test
(csrc/ssm_elementwise.hip's doc pair, the scan forms behind ops.scan_gate(layout=...)) are compared with these, and so are the
existing plain kernels run on every document alone: the tests hold the packed error to a multiple of that one.

A batch of packed rows is described by `lens`: per batch row the list of its documents' lengths (summing to L)."""
import torch
import torch.nn.functional as F


def documents(lens):
    """(b, start, stop) of every document, row by row."""
    for b, row in enumerate(lens):
        at = 0
        for n in row:
            yield b, at, at + n
            at += n


def document_ids(lens):
    """int64 [B, L]: the document index of every token (what the model's `document_ids` takes)."""
    return torch.stack([torch.repeat_interleave(torch.arange(len(row)), torch.tensor(row)) for row in lens])


def starts_ends(lens):
    """(start, end) int64 [B, L]: token t of row b belongs to the document [start[b, t], end[b, t])."""
    L = sum(lens[0])
    start = torch.zeros(len(lens), L, dtype=torch.int64)
    end = torch.zeros(len(lens), L, dtype=torch.int64)
    for b, s, e in documents(lens):
        start[b, s:e], end[b, s:e] = s, e
    return start, end


def lens_from_boundaries(L, boundaries):
    """Document lengths of one row of L tokens with a document starting at 0 and at every boundary in (0, L)."""
    cuts = sorted({c for c in boundaries if 0 < c < L})
    edges = [0] + cuts + [L]
    return [b - a for a, b in zip(edges[:-1], edges[1:])]


def conv_silu(x, w, b, start):
    """silu(bias + sum_q w[c, q] * x[t - (k-1) + q, c]) with the taps in front of start[b, t] (and of the row) read as zero.
    x [B, L, Dn], w [Dn, k], b [Dn] fp64 (autograd leaves or not), start int64 [B, L]."""
    B, L, Dn = x.shape
    k = w.shape[1]
    t = torch.arange(L)
    pre = b.view(1, 1, Dn).expand(B, L, Dn)
    for q in range(k):
        back = k - 1 - q                                       # the tap reads token t - back
        shifted = F.pad(x, (0, 0, back, 0))[:, :L]
        inside = ((t.view(1, L) - back) >= start).to(x.dtype).unsqueeze(-1)
        pre = pre + w[:, q].view(1, 1, Dn) * shifted * inside
    return F.silu(pre)


def scan_gate(logits, A_log, Bt, C, xc, z, D, start):
    """(C * s + D * xc) * silu(z) with s_t = exp(softplus(logit_t) * A) * s_{t-1} + Bt_t, A = -exp(A_log), and the state taken
    as zero in front of every document: s_t = Bt_t where start[b, t] == t.  logits [B, L, h], A_log [h, N], Bt / C / xc / z
    [B, L, h*N], D [h*N] fp64, start int64 [B, L]."""
    B, L, h = logits.shape
    N = A_log.shape[1]
    a = torch.exp(F.softplus(logits).unsqueeze(-1) * (-torch.exp(A_log)).view(1, 1, h, N)).reshape(B, L, h * N)
    first = (start == torch.arange(L).view(1, L)).unsqueeze(-1)
    a = torch.where(first, torch.zeros_like(a), a)
    s = torch.zeros(B, h * N, dtype=logits.dtype)
    ys = []
    for t in range(L):
        s = a[:, t] * s + Bt[:, t]
        ys.append(C[:, t] * s)
    y = torch.stack(ys, dim=1)
    return (y + D.view(1, 1, -1) * xc) * F.silu(z)


def leaves(tensors):
    """fp64 autograd leaves of a dict of tensors."""
    return {k: v.detach().to(torch.float64).clone().requires_grad_(True) for k, v in tensors.items()}
