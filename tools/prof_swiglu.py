"""The SwiGLU gate kernels (csrc/swiglu.hip) alone, and a use_swiglu model's training step and decode with ops.SWIGLU_FUSED on and off.

    python tools/prof_swiglu.py [--out FILE] [--no-step] [--no-decode] [--batch B]

1. Kernels alone, through the C ABI: T = 44 x 4096 rows, F = 2048, bf16.  Device events around every call, warm-up, then the
   median and range of the timed calls.  `bytes` = the tensors the call must move once: 3 T F 2 forward (g, u read, h written),
   6 T F 2 backward with h_out (dh, g, u read; dg, du, h written); `hbm_fraction` = bytes / time over the 8 TB/s HBM peak
   (the kernels do nothing but move bytes: that is the bound).
2. A training step of bench.py's 125m configuration (selective_ssm, per-GPU batch 32 x 2048, bf16 autocast, TrainStep) built
   with use_swiglu=True and use_rmsnorm=True: legs of --leg-steps steps with ops.SWIGLU_FUSED on and off, interleaved in one
   process after a warm-up of both, torch.cuda.max_memory_allocated per leg.  The off leg is the stock torch line of
   model.SwiGLUFFN, which is what such a model ran before the op existed.
3. Decode: new tokens per second of a 128-token greedy generate() (64-token prompt, bf16 autocast) at batch 1 and 16, on and
   off, alternated, the median of --decode-reps runs each.
Prints one JSON line per measurement and writes them to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12


def kernels(dev, emit, iters=30):
    import torch
    from apertis_llm_amd import _lib
    lib, P, S = _lib.load(), _lib.ptr, _lib.stream_ptr
    T, F, B = 44 * 4096, 2048, _lib.BF16
    bf = torch.bfloat16
    gen = torch.Generator(device=dev).manual_seed(0)
    gu = torch.empty(T, 2 * F, device=dev, dtype=bf).uniform_(-6.0, 6.0, generator=gen)
    dh = torch.empty(T, F, device=dev, dtype=bf).uniform_(-1.0, 1.0, generator=gen)
    h, dgu = torch.empty_like(dh), torch.empty_like(gu)
    n = T * F * 2
    calls = {
        "swiglu_fwd": (3 * n, lambda: lib.apertis_swiglu_fwd(P(gu), P(h), T, F, B, S())),
        "swiglu_bwd": (6 * n, lambda: lib.apertis_swiglu_bwd(P(dh), P(gu), P(dgu), P(h), T, F, B, S())),
        "swiglu_bwd_no_h": (5 * n, lambda: lib.apertis_swiglu_bwd(P(dh), P(gu), P(dgu), None, T, F, B, S())),
    }
    for what, (nbytes, fn) in calls.items():
        for _ in range(5):
            assert fn() == 0
        torch.cuda.synchronize()
        v = []
        for _ in range(iters):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            rc = fn()
            e.record()
            e.synchronize()
            assert rc == 0
            v.append(s.elapsed_time(e) * 1e3)
        med = statistics.median(v)
        emit({"what": "kernel", "kernel": what, "T": T, "F": F, "dtype": "bf16", "bytes": nbytes, "us_median": round(med, 1),
              "us_min": round(min(v), 1), "us_max": round(max(v), 1), "TBps": round(nbytes / (med * 1e-6) / 1e12, 2),
              "hbm_fraction": round(nbytes / (med * 1e-6) / HBM_PEAK, 3), "iters": iters})


def _model(dev):
    import torch
    import apertis_llm_amd as A
    from bench import CONFIGS
    target, moe, mm, seq, dbatch = CONFIGS["125m"]
    torch.manual_seed(0)
    model = A.create_apertis_model(target, vocab_size_override=32000, multimodal=mm, use_expert_system=moe,
                                   attention_type_override="selective_ssm",
                                   config_overrides={"use_swiglu": True, "use_rmsnorm": True})
    return model.to(dev), seq, dbatch


def train_step(dev, emit, batch, leg_steps, legs):
    import torch
    from apertis_llm_amd import ops
    from apertis_llm_amd.training import TrainStep
    model, seq, dbatch = _model(dev)
    cfg = model.config
    model.train()
    B = batch or dbatch
    total = 2 * legs * leg_steps + 16
    step = TrainStep(model, lr=5e-5, weight_decay=0.01, max_grad_norm=1.0, total_steps=total, bf16=True)
    gen = torch.Generator(device=dev).manual_seed(1000)

    def run(n):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for _ in range(n):
            ids = torch.randint(4, cfg.vocab_size, (B, seq), device=dev, generator=gen)
            loss = step(input_ids=ids, attention_mask=torch.ones_like(ids), labels=ids)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n, float(loss), torch.cuda.max_memory_allocated()
    for fused in (True, False, True, False):          # warm-up of both legs
        ops.SWIGLU_FUSED = fused
        run(2)
    res, mem = {True: [], False: []}, {True: 0, False: 0}
    for _ in range(legs):
        for fused in (True, False):
            ops.SWIGLU_FUSED = fused
            t, loss, peak = run(leg_steps)
            assert loss == loss, "NaN loss"
            res[fused].append(1e3 * t)
            mem[fused] = max(mem[fused], peak)
    ops.SWIGLU_FUSED = True
    ffn_dim = model.model.layers[0].feed_forward.ffn.ffn_dim
    for fused, v in res.items():
        emit({"what": "train_step", "config": "125m+use_swiglu+use_rmsnorm", "hidden_size": cfg.hidden_size, "ffn_dim": ffn_dim,
              "layers": cfg.num_hidden_layers, "per_gpu_batch": B, "seq_len": seq, "swiglu_fused": fused,
              "ms_per_step_median": round(statistics.median(v), 2), "ms_per_step_min": round(min(v), 2),
              "ms_per_step_max": round(max(v), 2), "legs_ms": [round(x, 2) for x in v], "leg_steps": leg_steps,
              "tokens_per_s": round(B * seq / (statistics.median(v) * 1e-3)),
              "max_memory_allocated_GiB": round(mem[fused] / 2 ** 30, 2)})
    del step
    return model


def decode(dev, emit, model, reps, new=128, prompt=64):
    import torch
    from apertis_llm_amd import ops
    if model is None:
        model = _model(dev)[0]
    cfg = model.config
    model.eval()
    for B in (1, 16):
        ids = torch.randint(4, cfg.vocab_size, (B, prompt), device=dev, generator=torch.Generator(device=dev).manual_seed(7))

        def run(n_new):
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = model.generate(ids, max_new_tokens=n_new, eos_token_id=[-1], use_cache=True)
                torch.cuda.synchronize()
                return time.perf_counter() - t0, out
        res, toks = {True: [], False: []}, {}
        for fused in (True, False):                   # warm-up: prepared weights, allocator, kernels, the graph capture path
            ops.SWIGLU_FUSED = fused
            run(new)
        for _ in range(reps):
            for fused in (True, False):
                ops.SWIGLU_FUSED = fused
                t_pre, _ = run(1)                     # prefill + first token
                t_all, out = run(new)
                assert out.shape == (B, prompt + new)
                res[fused].append(B * (new - 1) / (t_all - t_pre))
                toks[fused] = out
        ops.SWIGLU_FUSED = True
        same = float((toks[True] == toks[False]).float().mean())
        for fused, v in res.items():
            emit({"what": "decode", "config": "125m+use_swiglu+use_rmsnorm", "batch": B, "prompt": prompt, "new_tokens": new,
                  "dtype": "bf16", "swiglu_fused": fused, "tokens_per_s_median": round(statistics.median(v), 1),
                  "tokens_per_s_min": round(min(v), 1), "tokens_per_s_max": round(max(v), 1), "reps": reps,
                  "tokens_equal_to_other_leg": round(same, 4)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-decode", action="store_true")
    ap.add_argument("--batch", type=int, default=0, help="per-GPU batch of the training step (0 = bench.py's default for 125m)")
    ap.add_argument("--leg-steps", type=int, default=6)
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--decode-reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("prof_swiglu.py needs a ROCm GPU")
    dev = torch.device("cuda:0")
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)
        if args.out:                       # (kept up to date line by line: a run cut short leaves what it measured)
            with open(args.out, "w") as f:
                for x in lines:
                    f.write(json.dumps(x) + "\n")
    kernels(dev, emit)
    model = None
    if not args.no_step:
        model = train_step(dev, emit, args.batch, args.leg_steps, args.legs)
        torch.cuda.empty_cache()
    if not args.no_decode:
        decode(dev, emit, model, args.decode_reps)


if __name__ == "__main__":
    main()
