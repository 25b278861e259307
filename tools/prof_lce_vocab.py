"""What an odd vocabulary costs at the LM head + loss (ops/loss.py, LCE_PAD_VOCAB): forward + backward of the head and the loss
alone, as the tail of ApertisForCausalLM.forward runs them in training under fused_lm_head_loss, bf16 autocast, fp32 weight:
    stock    V (odd), switch off: logits tensor, shifted fp32 copy, F.cross_entropy   - what such a model gets by default
    padded   V (odd), switch on:  the fused path on Vp-wide chunks with -inf pads
    aligned  Vp,      today's fused path                                              - the yardstick for what the padding costs
The legs alternate in one process; after a warm-up of every leg each round times `iters` calls of each between two HIP events
and takes the leg's peak allocation (torch.cuda.max_memory_allocated, reset before the leg).  Every round is written out as
one JSON line, then a summary line with the medians and the two ratios.
    python tools/prof_lce_vocab.py [--B 16] [--L 1024] [--H 768] [--V 50257] [--rounds 5] [--iters 10] [--out FILE]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from apertis_llm_amd import ops
from apertis_llm_amd.ops._base import _compute_dtype

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=16)
ap.add_argument("--L", type=int, default=1024)
ap.add_argument("--H", type=int, default=768)
ap.add_argument("--V", type=int, default=50257)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU: a CPU run says nothing about this"
dev = torch.device("cuda:0")
B, L, H, V = args.B, args.L, args.H, args.V
Vp = ops.loss._lce_padded_vocab(V, torch.bfloat16)
assert V < Vp, "give an odd vocabulary"
torch.manual_seed(0)
hs = (torch.randn(B, L, H, device=dev) * 0.7).requires_grad_(True)
w_full = torch.randn(Vp, H, device=dev) * 0.02
weights = {V: w_full[:V].clone().requires_grad_(True), Vp: w_full.clone().requires_grad_(True)}
labels = torch.randint(0, V, (B, L), device=dev)
labels[1, :5] = -100


def head_and_loss(weight):
    """The tail of ApertisForCausalLM.forward (training, fused_lm_head_loss) on `hs`."""
    if ops.linear_cross_entropy_supported(hs, weight, labels):
        return ops.linear_cross_entropy(hs, weight, labels, ignore_index=-100, compute_dtype=_compute_dtype(hs)), "fused"
    logits = F.linear(hs, weight)
    assert not ops.shifted_cross_entropy_supported(logits, labels)
    sl, tl = logits[..., :-1, :], labels[..., 1:]
    return F.cross_entropy(sl.reshape(-1, sl.shape[-1]).float(), tl.reshape(-1), ignore_index=-100), "stock"


LEGS = [("stock", V, False), ("padded", V, True), ("aligned", Vp, False)]


def call(leg):
    name, v, pad = leg
    ops.loss.LCE_PAD_VOCAB = pad
    hs.grad = weights[v].grad = None
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss, path = head_and_loss(weights[v])
    loss.backward()
    assert path == ("stock" if name == "stock" else "fused"), (name, path)
    return loss.detach()


records = []


def emit(rec):
    records.append(rec)
    print(json.dumps(rec), flush=True)


# warm-up of every shape, and what the legs compute on the same operands
got = {}
for leg in LEGS:
    for _ in range(3):
        got[leg[0]] = (float(call(leg)), hs.grad.clone(), weights[leg[1]].grad[:V].clone())
torch.cuda.synchronize()
s, p = got["stock"], got["padded"]
emit({"check": "padded against stock on the same operands", "loss_stock": s[0], "loss_padded": p[0], "loss_aligned": got["aligned"][0],
      "dh_max_abs_diff": float((s[1] - p[1]).abs().max()), "dh_max_abs": float(s[1].abs().max()),
      "dw_max_abs_diff": float((s[2] - p[2]).abs().max()), "dw_max_abs": float(s[2].abs().max())})
del got, s, p
for rnd in range(args.rounds):
    for leg in LEGS:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            call(leg)
        b.record()
        b.synchronize()
        emit({"round": rnd, "leg": leg[0], "V": leg[1], "pad_vocab": leg[2], "B": B, "L": L, "H": H, "iters": args.iters,
              "ms_per_call": a.elapsed_time(b) / args.iters, "peak_bytes": torch.cuda.max_memory_allocated()})


def med(name, key):
    xs = sorted(r[key] for r in records if r.get("leg") == name)
    return xs[len(xs) // 2]


ms = {n: med(n, "ms_per_call") for n, _, _ in LEGS}
emit({"summary": "medians over the rounds", "ms": ms, "peak_gib": {n: med(n, "peak_bytes") / 2 ** 30 for n, _, _ in LEGS},
      "padded_over_aligned": ms["padded"] / ms["aligned"], "padded_over_stock": ms["padded"] / ms["stock"],
      "spread_ms": {n: [min(r["ms_per_call"] for r in records if r.get("leg") == n),
                        max(r["ms_per_call"] for r in records if r.get("leg") == n)] for n, _, _ in LEGS}})
if args.out:
    with open(args.out, "w") as f:
        f.writelines(json.dumps(r) + "\n" for r in records)
