"""Packed-sequence training (document_ids): what the document-masked attention kernels cost and save against the plain causal
kernels, and what packing does to a training step of the 125M standard_mha model on short sequences.

    python tools/prof_packed.py [--out DIR] [--reps N] [--train-steps N]

One process, HIP-event / synchronised host-clock timing after a warm-up, the legs of a comparison alternating call by call.
Appends nothing: DIR/packed_mi355x.jsonl (DIR defaults to profiles/) is rewritten, one JSON record per line:
  kind "kernel"  one shape, bf16: the causal kernels and the document kernels under three layouts (one document per row, 8 and 64
                 equal documents per row), forward and forward + backward, median ms; the ratio to the causal kernels; the ratio of
                 32-wide tiles the kernels walk (counted on the host from the layout, the loops' own bounds); and whether the
                 outputs at THIS shape have the bits of the causal kernels run on every document alone
  kind "step"    a training step (bf16 autocast, fused LM-head loss, AdamW with the norm clip) on items of a seeded length
                 distribution, padded to max_length against packed, the same number of rows per batch: real (non-pad) tokens
                 per second and peak memory of each leg."""
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

ROWS, TILE = 16, 32                              # attn_tile.h: rows per wave, columns per loop step


def ab_time(fns, reps, warm=3):
    """Median ms per function; the functions alternate call by call so drift hits all alike."""
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
    return [sorted(t)[len(t) // 2] for t in times], [(min(t), max(t)) for t in times]


def tiles_walked(start, end):
    """(forward / dQ tiles, dK/dV tiles) of one row's layout, by the kernels' loop bounds: a wave of 16 queries walks key tiles
    from the tile of its smallest start to the diagonal; a wave of 16 keys walks query tiles from its own to its largest end."""
    L = len(start)
    fwd = bwd = 0
    for r0 in range(0, L, ROWS):
        r1 = min(r0 + ROWS, L)
        fwd += (r1 - 1) // TILE - (min(int(start[r0:r1].min()), r0) // TILE) + 1
        bwd += -(-(min(int(end[r0:r1].max()), L) - (r0 // TILE) * TILE) // TILE)
    return fwd, bwd


def kernel_record(B, L, H, D, docs_per_row, reps, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    q, k, v, do = (torch.randn(B, L, H * D, device=dev, generator=g, dtype=torch.bfloat16) for _ in range(4))
    qg, kg, vg = (t.clone().requires_grad_() for t in (q, k, v))
    layouts = {n: ops.document_layout((torch.arange(L, device=dev) // (L // n)).expand(B, L).contiguous()) for n in docs_per_row}
    legs = [("causal", lambda a, b, c: ops.causal_attention(a, b, c, H))]
    legs += [(f"doc_{n}x{L // n}", (lambda lay: lambda a, b, c: ops.document_attention(a, b, c, H, lay))(layouts[n]))
             for n in docs_per_row]

    def fwd(fn):
        def run():
            with torch.no_grad():
                fn(q, k, v)
        return run

    def fwd_bwd(fn):
        def run():
            torch.autograd.grad(fn(qg, kg, vg), (qg, kg, vg), do)
        return run
    f_ms, f_span = ab_time([fwd(fn) for _, fn in legs], reps)
    fb_ms, fb_span = ab_time([fwd_bwd(fn) for _, fn in legs], reps)
    t_causal = tiles_walked(np.zeros(L, dtype=np.int64), np.full(L, L, dtype=np.int64))
    rec = {"kind": "kernel", "device": torch.cuda.get_device_name(0), "dtype": "bf16", "B": B, "L": L, "H": H, "D": D, "reps": reps,
           "legs": {}}
    for j, (name, fn) in enumerate(legs):
        leg = {"fwd_ms": f_ms[j], "fwd_ms_min_max": f_span[j], "fwd_bwd_ms": fb_ms[j], "fwd_bwd_ms_min_max": fb_span[j],
               "fwd_vs_causal": f_ms[j] / f_ms[0], "fwd_bwd_vs_causal": fb_ms[j] / fb_ms[0]}
        if j:
            n = docs_per_row[j - 1]
            lay = layouts[n]
            t = tiles_walked(lay.start[0].cpu().numpy().astype(np.int64), lay.end[0].cpu().numpy().astype(np.int64))
            leg["tiles_vs_causal"] = {"fwd_dq": t[0] / t_causal[0], "dkv": t[1] / t_causal[1]}
            # the same results as the causal kernels on every document alone, at the shape that is timed
            n_q = tuple(x.reshape(B * n, L // n, H * D) for x in (q, k, v, do))
            got = torch.autograd.grad(fn(qg, kg, vg), (qg, kg, vg), do)
            a, b, c = (x.clone().requires_grad_() for x in n_q[:3])
            want = torch.autograd.grad(ops.causal_attention(a, b, c, H), (a, b, c), n_q[3])
            with torch.no_grad():
                o, o_want = fn(q, k, v).reshape(n_q[0].shape), ops.causal_attention(*n_q[:3], H)
            pairs = [(o, o_want)] + [(x.reshape(y.shape), y) for x, y in zip(got, want)]
            leg["bits_of_causal_per_document"] = {nm: bool(torch.equal(x, y)) for nm, (x, y) in zip(("O", "dQ", "dK", "dV"), pairs)}
            if not all(torch.allclose(x.float(), y.float(), rtol=2e-2, atol=2e-2) for x, y in pairs):
                raise RuntimeError(f"{name}: results differ from the causal kernels run on every document alone")
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
    model = A.create_apertis_model("125M", vocab_size_override=vocab, attention_type_override="standard_mha").to(dev).train()
    model.fused_lm_head_loss = True
    opt = build_optimizer(model, 1e-4, 0.01)
    params = [p for p in model.parameters() if p.requires_grad]

    def batches(ds):
        out = []
        for at in range(0, len(ds) - rows_per_batch + 1, rows_per_batch):
            rows = [ds[i] for i in range(at, at + rows_per_batch)]
            out.append({k_: torch.stack([r[k_] for r in rows]).to(dev) for k_ in rows[0]})
        return out
    legs = {"padded": batches(items), "packed": batches(packed)}

    def step(batch):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = model(**batch)[0]
        loss.backward()
        clip_and_step(opt, params, 1.0)
        opt.zero_grad(set_to_none=True)

    for name in legs:                                     # warm-up both
        for i in range(3):
            step(legs[name][i % len(legs[name])])
    torch.cuda.synchronize()
    per = {name: {"s": [], "tokens": [], "peak": 0} for name in legs}
    for r in range(steps):                                # alternate single steps
        for name, bs in legs.items():
            batch = bs[r % len(bs)]
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            step(batch)
            torch.cuda.synchronize()
            per[name]["s"].append(time.perf_counter() - t0)
            per[name]["tokens"].append(int((batch["labels"] != -100).sum()))
            per[name]["peak"] = max(per[name]["peak"], torch.cuda.max_memory_allocated())
    rec = {"kind": "step", "device": torch.cuda.get_device_name(0), "model": "125M standard_mha", "autocast": "bf16",
           "optimizer": "AdamW (clip 1.0)", "lengths": f"uniform {32}..{max_length}, numpy RandomState({seed}), {n_items} items",
           "max_length": max_length, "rows_per_batch": rows_per_batch, "items": n_items, "packed_rows": len(packed),
           "mean_length": float(lengths.mean()), "steps_timed": steps, "legs": {}}
    for name, p in per.items():
        total_s, total_tok = sum(p["s"]), sum(p["tokens"])
        rec["legs"][name] = {"step_ms_median": sorted(p["s"])[len(p["s"]) // 2] * 1e3, "real_tokens_per_step": total_tok / steps,
                             "real_tokens_per_s": total_tok / total_s, "peak_memory_MiB": p["peak"] / 2 ** 20}
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
        raise SystemExit("prof_packed.py measures on a ROCm GPU; none is visible")
    dev = torch.device("cuda:0")
    recs = [kernel_record(8, 4096, 12, 64, (1, 8, 64), args.reps, dev),
            kernel_record(64, 512, 12, 64, (1, 8), args.reps, dev),
            step_record(args.train_steps, dev)]
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "packed_mi355x.jsonl"), "w") as f:
        for r in recs:
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
