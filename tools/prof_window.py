"""Sliding-window attention (ops.ATTN_WINDOW, config.sliding_window): what the window form of the attention kernels costs
against the two other routes to the same numbers, and what a bounded cache read does to generate().

    python tools/prof_window.py [--out DIR] [--reps N] [--decode-rounds N] [--skip-decode]

One process, HIP-event / synchronised host-clock timing after a warm-up, the legs of a comparison alternating call by call,
every timed round listed.  DIR/window_mi355x.jsonl (DIR defaults to profiles/) is rewritten, one JSON record per line:
  kind "kernel"  8 x 4096 x 12x64 bf16, one record per W in {256, 1024, 4096}: the window form (ops.window_attention), the
                 document form fed the equivalent arrays (ops.document_attention on ops.window_layout: the route to this
                 mask without the window mode, the baseline) and the plain causal kernels (another mask: the full
                 triangle); forward and forward + backward, median ms and every round; the ratios window / document-fed
                 and window / causal; and whether the window form's outputs have the document-fed form's bits at THIS shape
  kind "decode"  125M standard_mha, bf16 autocast, greedy, a 1 920-token prompt, W 512, 128 new tokens, batch 1 and 16: new
                 tokens per second of generate() with ops.ATTN_WINDOW on and off (the eager loop on both legs; the prefill is
                 timed apart and left out), and the decode kernel's own time per launch on each leg."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                    # noqa: E402

import apertis_llm_amd as A                     # noqa: E402
from apertis_llm_amd import ops                 # noqa: E402


def ab_time(fns, reps, warm=3):
    """Per function: every timed round in ms, in order; the functions alternate call by call so drift hits all alike."""
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


def _median(t):
    return sorted(t)[len(t) // 2]


def kernel_record(B, L, H, D, W, reps, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    q, k, v, do = (torch.randn(B, L, H * D, device=dev, generator=g, dtype=torch.bfloat16) for _ in range(4))
    qg, kg, vg = (t.clone().requires_grad_() for t in (q, k, v))
    layout = ops.window_layout((B, L), W, dev)
    legs = [("window", lambda a, b, c: ops.window_attention(a, b, c, H, W)),
            ("document_fed", lambda a, b, c: ops.document_attention(a, b, c, H, layout)),
            ("causal", lambda a, b, c: ops.causal_attention(a, b, c, H))]

    def fwd(fn):
        def run():
            with torch.no_grad():
                fn(q, k, v)
        return run

    def fwd_bwd(fn):
        def run():
            torch.autograd.grad(fn(qg, kg, vg), (qg, kg, vg), do)
        return run
    f = ab_time([fwd(fn) for _, fn in legs], reps)
    fb = ab_time([fwd_bwd(fn) for _, fn in legs], reps)
    rec = {"kind": "kernel", "device": torch.cuda.get_device_name(0), "dtype": "bf16", "B": B, "L": L, "H": H, "D": D, "W": W,
           "reps": reps, "pairs_vs_causal": ops.window_pairs(L, W) / (L * (L + 1) / 2), "legs": {}}
    for j, (name, _) in enumerate(legs):
        rec["legs"][name] = {"fwd_ms": _median(f[j]), "fwd_bwd_ms": _median(fb[j]), "fwd_rounds_ms": f[j], "fwd_bwd_rounds_ms": fb[j]}
    for what, t in (("fwd", f), ("fwd_bwd", fb)):
        rec[f"{what}_window_vs_document_fed"] = _median(t[0]) / _median(t[1])
        rec[f"{what}_window_vs_causal"] = _median(t[0]) / _median(t[2])
    got = (legs[0][1](q, k, v).detach(), *torch.autograd.grad(legs[0][1](qg, kg, vg), (qg, kg, vg), do))
    want = (legs[1][1](q, k, v).detach(), *torch.autograd.grad(legs[1][1](qg, kg, vg), (qg, kg, vg), do))
    rec["bits_of_document_fed"] = {n: bool(torch.equal(x, y)) for n, x, y in zip(("O", "dQ", "dK", "dV"), got, want)}
    return rec


def decode_records(rounds, dev, prompt=1920, W=512, new=128, batches=(1, 16)):
    torch.manual_seed(0)
    model = A.create_apertis_model("125M", vocab_size_override=32000, attention_type_override="standard_mha").to(dev).eval()
    model.config.sliding_window = W
    if model.config.max_position_embeddings < prompt + new:
        raise SystemExit(f"the 125M preset's rotary table ({model.config.max_position_embeddings}) is shorter than {prompt + new}")
    recs = []
    for B in batches:
        ids = torch.randint(4, 32000, (B, prompt), generator=torch.Generator().manual_seed(B)).to(dev)

        def run(n_new):
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                model.generate(ids, max_new_tokens=n_new, eos_token_id=[-1], use_cache=True, do_sample=False)
                torch.cuda.synchronize()
                return time.perf_counter() - t0
        legs = {"window_on": True, "window_off": False}
        per = {name: {"prefill_s": [], "total_s": []} for name in legs}
        for r in range(1 + rounds):                           # (round 0 warms both legs up)
            for name, on in legs.items():
                ops.ATTN_WINDOW = on
                p, t = run(1), run(new)
                if r:
                    per[name]["prefill_s"].append(p)
                    per[name]["total_s"].append(t)
        rec = {"kind": "decode", "device": torch.cuda.get_device_name(0), "model": "125M standard_mha", "autocast": "bf16",
               "B": B, "prompt": prompt, "W": W, "new_tokens": new, "rounds": rounds, "legs": {}}
        for name, on in legs.items():
            ops.ATTN_WINDOW = on
            timer = ops.KernelTimer(["apertis_attention_decode"])
            ops.set_kernel_timer(timer)
            try:
                run(new)
            finally:
                ops.set_kernel_timer(None)
            s = timer.summary()["apertis_attention_decode"]
            steps = [t - p for p, t in zip(per[name]["prefill_s"], per[name]["total_s"])]
            rec["legs"][name] = {"new_tokens_per_s": B * (new - 1) / _median(steps), "decode_rounds_s": steps,
                                 "prefill_rounds_s": per[name]["prefill_s"], "step_ms": _median(steps) / (new - 1) * 1e3,
                                 "decode_kernel_us_per_launch": s["ms"] / s["launches"] * 1e3, "decode_launches": s["launches"]}
        ops.ATTN_WINDOW = False
        rec["on_vs_off_new_tokens_per_s"] = rec["legs"]["window_on"]["new_tokens_per_s"] / rec["legs"]["window_off"]["new_tokens_per_s"]
        recs.append(rec)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--decode-rounds", type=int, default=3)
    ap.add_argument("--skip-decode", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prof_window.py measures on a ROCm GPU; none is visible")
    dev = torch.device("cuda:0")
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "window_mi355x.jsonl"), "w") as f:
        def emit(r):
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        for W in (256, 1024, 4096):
            emit(kernel_record(8, 4096, 12, 64, W, args.reps, dev))
        if not args.skip_decode:
            for r in decode_records(args.decode_rounds, dev):
                emit(r)


if __name__ == "__main__":
    main()
