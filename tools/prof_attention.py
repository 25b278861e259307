"""Fused standard_mha attention (ops.causal_attention, csrc/attention.hip) against the stock path it replaces
(ApertisAttention's ops.ATTN_FUSED = False branch: head transposes, the dense [L, L] additive causal mask, F.scaled_dot_product_
attention, the transpose back), bf16, HIP-event timed after a warm-up, A and B alternating call by call; then a full training
step of the 125M standard_mha model (bf16 autocast, AdamW) in tokens/s both ways.

    python tools/prof_attention.py [--out DIR] [--reps N] [--train-steps N]

Writes DIR/attention_mi355x.json and DIR/attention_mi355x.txt (DIR defaults to profiles/).  FLOPs: causal forward
4*B*H*D*L(L+1)/2, backward 2.5x that (five products); share of the 2.5 PF/s dense bf16 MFMA peak."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                    # noqa: E402
import torch.nn.functional as F                 # noqa: E402

import apertis_llm_amd as A                     # noqa: E402
from apertis_llm_amd import ops                 # noqa: E402

PEAK = 2.5e15
SHAPES = [(2, 512, 14, 64), (8, 4096, 12, 64), (4, 4096, 8, 128)]


def stock_attention(q, k, v, H):
    B, L, W = q.shape
    D = W // H
    qh, kh, vh = (t.view(B, L, H, D).transpose(1, 2) for t in (q, k, v))
    i = torch.arange(L, device=q.device).unsqueeze(1)
    mask = torch.zeros(L, L, device=q.device, dtype=qh.dtype).masked_fill_(
        i < torch.arange(L, device=q.device).unsqueeze(0), torch.finfo(qh.dtype).min)
    o = F.scaled_dot_product_attention(qh, kh, vh, attn_mask=mask)
    return o.transpose(1, 2).reshape(B, L, W)


def fused_attention(q, k, v, H):
    return ops.causal_attention(q, k, v, H)


def ab_time(fns, reps, warm=3):
    """Median ms per function; the functions alternate call by call so drift hits both alike."""
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
    return [sorted(t)[len(t) // 2] for t in times]


def attention_rows(reps, dev):
    rows = []
    for B, L, H, D in SHAPES:
        g = torch.Generator(device=dev).manual_seed(0)
        q, k, v, do = (torch.randn(B, L, H * D, device=dev, generator=g, dtype=torch.bfloat16) for _ in range(4))
        qg, kg, vg = (t.clone().requires_grad_() for t in (q, k, v))
        fwd_flops = 4.0 * B * H * D * L * (L + 1) / 2

        def fwd(fn):
            def run():
                with torch.no_grad():
                    fn(q, k, v, H)
            return run

        def fwd_bwd(fn):
            def run():
                o = fn(qg, kg, vg, H)
                torch.autograd.grad(o, (qg, kg, vg), do)
            return run
        f_ms, s_ms = ab_time([fwd(fused_attention), fwd(stock_attention)], reps)
        fb_ms, sb_ms = ab_time([fwd_bwd(fused_attention), fwd_bwd(stock_attention)], reps)
        fb_flops = 3.5 * fwd_flops
        row = {"B": B, "L": L, "H": H, "D": D, "dtype": "bf16",
               "fwd_ms": {"fused": f_ms, "stock": s_ms}, "fwd_bwd_ms": {"fused": fb_ms, "stock": sb_ms},
               "fwd_tflops": {"fused": fwd_flops / f_ms / 1e9, "stock": fwd_flops / s_ms / 1e9},
               "fwd_bwd_tflops": {"fused": fb_flops / fb_ms / 1e9, "stock": fb_flops / sb_ms / 1e9},
               "fwd_speedup": s_ms / f_ms, "fwd_bwd_speedup": sb_ms / fb_ms}
        row["fused_fwd_share_of_peak"] = row["fwd_tflops"]["fused"] * 1e12 / PEAK
        row["fused_fwd_bwd_share_of_peak"] = row["fwd_bwd_tflops"]["fused"] * 1e12 / PEAK
        rows.append(row)
        print(json.dumps(row), flush=True)
        del q, k, v, do, qg, kg, vg
        torch.cuda.empty_cache()
    return rows


def train_rows(steps, dev, B=8, L=512):
    torch.manual_seed(0)
    model = A.create_apertis_model("125M", vocab_size_override=32000).to(dev).train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4)
    ids = torch.randint(4, 32000, (B, L), device=dev)

    def step():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = model(input_ids=ids, labels=ids, use_cache=False)[0]
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)

    out = {}
    per = {True: [], False: []}
    for mode in (True, False):              # warm-up both
        ops.ATTN_FUSED = mode
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    for r in range(steps):                   # alternate single steps
        for mode in (True, False):
            ops.ATTN_FUSED = mode
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            per[mode].append(time.perf_counter() - t0)
    ops.ATTN_FUSED = True
    for mode, name in ((True, "fused"), (False, "stock")):
        med = sorted(per[mode])[len(per[mode]) // 2]
        out[name] = {"step_ms": med * 1e3, "tokens_per_s": B * L / med}
    out.update({"model": "125M standard_mha (H896, 10 layers, 14 x 64)", "B": B, "L": L, "autocast": "bf16", "optimizer": "AdamW",
                "steps_timed": steps, "speedup": out["stock"]["step_ms"] / out["fused"]["step_ms"]})
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--train-steps", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "peak_bf16_flops": PEAK,
           "attention": attention_rows(args.reps, dev), "train_step": train_rows(args.train_steps, dev)}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "attention_mi355x.json"), "w") as f:
        json.dump(res, f, indent=1)
    lines = ["causal attention, bf16: fused (HIP) vs stock (dense mask + SDPA), median ms, A/B alternating",
             f"{'B':>2} {'L':>5} {'HxD':>7} | {'fwd fused':>9} {'stock':>8} {'x':>5} {'TF/s':>6} {'peak':>5} | "
             f"{'f+b fused':>9} {'stock':>8} {'x':>5} {'TF/s':>6} {'peak':>5}"]
    for r in res["attention"]:
        lines.append(f"{r['B']:>2} {r['L']:>5} {str(r['H']) + 'x' + str(r['D']):>7} | {r['fwd_ms']['fused']:9.3f} "
                     f"{r['fwd_ms']['stock']:8.3f} {r['fwd_speedup']:5.2f} {r['fwd_tflops']['fused']:6.1f} "
                     f"{100 * r['fused_fwd_share_of_peak']:4.1f}% | {r['fwd_bwd_ms']['fused']:9.3f} {r['fwd_bwd_ms']['stock']:8.3f} "
                     f"{r['fwd_bwd_speedup']:5.2f} {r['fwd_bwd_tflops']['fused']:6.1f} {100 * r['fused_fwd_bwd_share_of_peak']:4.1f}%")
    t = res["train_step"]
    lines.append(f"training step, {t['model']}, B={t['B']} L={t['L']}, bf16 autocast, AdamW: fused "
                 f"{t['fused']['tokens_per_s']:.0f} tokens/s ({t['fused']['step_ms']:.1f} ms), stock "
                 f"{t['stock']['tokens_per_s']:.0f} tokens/s ({t['stock']['step_ms']:.1f} ms), x{t['speedup']:.3f}")
    with open(os.path.join(args.out, "attention_mi355x.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
