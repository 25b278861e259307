"""Packed selective_ssm rows (ops.ssm.SSM_PACKED): what packing does to a training step of the 125M selective_ssm model on short
items, and what the conv kernels that stop at document starts cost against the plain conv kernels.

    python tools/prof_packed_ssm.py [--out DIR] [--reps N] [--train-steps N]

One process, HIP-event / synchronised host-clock timing after a warm-up, the legs of a comparison alternating call by call, and
EVERY round listed next to the medians.  Appends nothing: DIR/packed_ssm_mi355x.jsonl (DIR defaults to profiles/) is rewritten,
one JSON record per line:
  kind "step"    (a) a training step (bf16 autocast, fused LM-head loss, AdamW with the norm clip) on items of uniform 32..512
                 tokens at max_length 512, 16 rows per batch, padded against packed: real (non-pad) tokens per second and peak
                 memory of each leg, the time of every step
  kind "conv"    (b) the doc conv forward and backward (both consumer gradients, as in the model) at 44 x 4096 x 176 bf16, k = 4,
                 with one document per row and with 8 x 512 documents per row, against the plain conv kernels: median ms, every
                 round, the ratio to the plain kernels, and whether the one-document outputs have the plain kernels' bits."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                              # noqa: E402
import torch                                    # noqa: E402

import apertis_llm_amd as A                     # noqa: E402
from apertis_llm_amd import ops                 # noqa: E402
from apertis_llm_amd.data import PackedDataset  # noqa: E402
from apertis_llm_amd.training import build_optimizer, clip_and_step     # noqa: E402


def ab_rounds(fns, reps, warm=3):
    """ms of every round of every function; the functions alternate call by call so drift hits all alike."""
    times = [[] for _ in fns]
    for r in range(warm + reps):
        for j, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= warm:
                times[j].append(a.elapsed_time(b))
    return times


def median(t):
    return sorted(t)[len(t) // 2]


def conv_record(B, L, Dn, k, docs_per_row, reps, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, L, Dn, device=dev, generator=g, dtype=torch.bfloat16)
    g1, g2 = (torch.randn(B, L, Dn, device=dev, generator=g, dtype=torch.bfloat16) for _ in range(2))
    w = (0.5 * torch.randn(Dn, 1, k, device=dev, generator=g)).requires_grad_()
    b = (0.5 * torch.randn(Dn, device=dev, generator=g)).requires_grad_()
    xg = x.clone().requires_grad_()
    layouts = {n: ops.document_layout((torch.arange(L, device=dev) // (L // n)).expand(B, L).contiguous()) for n in docs_per_row}
    legs = [("plain", None)] + [(f"doc_{n}x{L // n}", layouts[n]) for n in docs_per_row]

    def fwd(lay):
        def run():
            with torch.no_grad():
                ops.dwconv_silu(x, w, b, layout=lay)
        return run

    def pair(lay):
        return ops.dwconv_silu_pair(xg, w, b, layout=lay)

    def bwd(lay):
        """The backward alone: the forward's node is built outside the timed call, its graph kept."""
        a, c = pair(lay)

        def run():
            torch.autograd.grad([a, c], (xg, w, b), [g1, g2], retain_graph=True)
        return run
    f_rounds = ab_rounds([fwd(lay) for _, lay in legs], reps)
    b_rounds = ab_rounds([bwd(lay) for _, lay in legs], reps)
    e = x.element_size()
    rec = {"kind": "conv", "device": torch.cuda.get_device_name(0), "dtype": "bf16", "B": B, "L": L, "Dn": Dn, "k": k, "reps": reps,
           "algorithmic_bytes": {"fwd": 2 * B * L * Dn * e, "bwd": 4 * B * L * Dn * e}, "legs": {}}
    with torch.no_grad():
        plain_out = ops.dwconv_silu(x, w, b)
    plain_dx = torch.autograd.grad(list(pair(None)), (xg,), [g1, g2])[0]
    for j, (name, lay) in enumerate(legs):
        fm, bm = median(f_rounds[j]), median(b_rounds[j])
        leg = {"fwd_ms": fm, "bwd_ms": bm, "fwd_rounds_ms": f_rounds[j], "bwd_rounds_ms": b_rounds[j],
               "fwd_TBps": rec["algorithmic_bytes"]["fwd"] / fm / 1e9, "bwd_TBps": rec["algorithmic_bytes"]["bwd"] / bm / 1e9,
               "fwd_vs_plain": fm / median(f_rounds[0]), "bwd_vs_plain": bm / median(b_rounds[0])}
        if lay is not None:
            with torch.no_grad():
                out = ops.dwconv_silu(x, w, b, layout=lay)
            dx = torch.autograd.grad(list(pair(lay)), (xg,), [g1, g2])[0]
            n = docs_per_row[j - 1]
            if n == 1:
                leg["bits_of_plain"] = {"out": bool(torch.equal(out, plain_out)), "dx": bool(torch.equal(dx, plain_dx))}
            else:       # every document alone is a row of the reshaped batch
                xr = x.reshape(B * n, L // n, Dn).clone().requires_grad_()
                with torch.no_grad():
                    want = ops.dwconv_silu(xr, w, b)
                want_dx = torch.autograd.grad(list(ops.dwconv_silu_pair(xr, w, b)), (xr,),
                                              [g1.reshape(xr.shape), g2.reshape(xr.shape)])[0]
                leg["bits_of_plain_per_document"] = {"out": bool(torch.equal(out.reshape(xr.shape), want)),
                                                     "dx": bool(torch.equal(dx.reshape(xr.shape), want_dx))}
        rec["legs"][name] = leg
    return rec


class _Items(torch.utils.data.Dataset):
    """Synthetic items in the datasets' format: `n` random tokens, right-padded to max_length."""

    def __init__(self, lengths, max_length, vocab, seed):
        g = torch.Generator().manual_seed(seed)
        self.max_length, self.rows = max_length, []
        for n in lengths:
            ids = torch.zeros(max_length, dtype=torch.int64)
            ids[:n] = torch.randint(4, vocab, (int(n),), generator=g)
            self.rows.append(ids)

    def __len__(self):
        return len(self.rows)

    def __getitem__(self, i):
        ids = self.rows[i]
        return {"input_ids": ids, "attention_mask": (ids != 0).long(), "labels": ids.masked_fill(ids == 0, -100)}


def step_record(steps, dev, rows_per_batch=16, max_length=512, n_items=512, seed=0, vocab=32000):
    lengths = np.random.RandomState(seed).randint(32, max_length + 1, size=n_items)
    items = _Items(lengths, max_length, vocab, seed)
    packed = PackedDataset(items, max_length, 0)
    torch.manual_seed(0)
    model = A.create_apertis_model("125M", vocab_size_override=vocab, attention_type_override="selective_ssm").to(dev).train()
    model.fused_lm_head_loss = True
    ops.doc_reset_check(model)
    opt = build_optimizer(model, 1e-4, 0.01)
    params = [p for p in model.parameters() if p.requires_grad]

    def batches(ds):
        out = []
        for at in range(0, len(ds) - rows_per_batch + 1, rows_per_batch):
            rows = [ds[i] for i in range(at, at + rows_per_batch)]
            out.append({k_: torch.stack([r[k_] for r in rows]).to(dev) for k_ in rows[0]})
        return out
    legs = {"padded": batches(items), "packed": batches(packed)}
    losses = {name: [] for name in legs}

    def step(name, batch):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = model(**batch)[0]
        loss.backward()
        clip_and_step(opt, params, 1.0)
        opt.zero_grad(set_to_none=True)
        losses[name].append(loss.detach())

    for name in legs:                                     # warm-up both
        for i in range(3):
            step(name, legs[name][i % len(legs[name])])
    torch.cuda.synchronize()
    per = {name: {"s": [], "tokens": [], "peak": 0} for name in legs}
    for r in range(steps):                                # alternate single steps
        for name, bs in legs.items():
            batch = bs[r % len(bs)]
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            step(name, batch)
            torch.cuda.synchronize()
            per[name]["s"].append(time.perf_counter() - t0)
            per[name]["tokens"].append(int((batch["labels"] != -100).sum()))
            per[name]["peak"] = max(per[name]["peak"], torch.cuda.max_memory_allocated())
    if ops.scan_gate_error():
        raise RuntimeError("a single-pass scan launch timed out in its look-back")
    rec = {"kind": "step", "device": torch.cuda.get_device_name(0), "model": "125M selective_ssm", "autocast": "bf16",
           "optimizer": "AdamW (clip 1.0)", "lengths": f"uniform {32}..{max_length}, numpy RandomState({seed}), {n_items} items",
           "max_length": max_length, "rows_per_batch": rows_per_batch, "items": n_items, "packed_rows": len(packed),
           "mean_length": float(lengths.mean()), "steps_timed": steps, "legs": {}}
    for name, p in per.items():
        total_s, total_tok = sum(p["s"]), sum(p["tokens"])
        ls = torch.stack(losses[name]).float()
        if not bool(torch.isfinite(ls).all()):
            raise RuntimeError(f"{name}: a loss is not finite")
        rec["legs"][name] = {"step_ms_median": median(p["s"]) * 1e3, "step_ms_rounds": [s * 1e3 for s in p["s"]],
                             "real_tokens_per_step": total_tok / steps, "real_tokens_per_s": total_tok / total_s,
                             "peak_memory_MiB": p["peak"] / 2 ** 20, "first_loss": float(ls[0]), "last_loss": float(ls[-1])}
    rec["packed_vs_padded_real_tokens_per_s"] = (rec["legs"]["packed"]["real_tokens_per_s"]
                                                  / rec["legs"]["padded"]["real_tokens_per_s"])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--train-steps", type=int, default=12)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prof_packed_ssm.py measures on a ROCm GPU; none is visible")
    dev = torch.device("cuda:0")
    ops.SSM_PACKED = True
    recs = [step_record(args.train_steps, dev), conv_record(44, 4096, 176, 4, (1, 8), args.reps, dev)]
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "packed_ssm_mi355x.jsonl"), "w") as f:
        for r in recs:
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
