"""The RMSNorm row kernels (csrc/rmsnorm.hip) next to their LayerNorm siblings, and a use_rmsnorm training step with the kernels on and off.

    python tools/prof_rmsnorm.py [--out FILE] [--no-step] [--batch B]

1. Kernels alone, through the C ABI at the bench row width: T = 44 x 4096 rows of H = 704, fp32 residual stream, bf16
   activations.  Forward, backward (plain, and with the residual gradient added and the masked block gradient written) and the
   dense block boundary, each RMSNorm entry point alternated with its LayerNorm sibling: device events around every call,
   warm-up, then the median and range of the timed calls.  `bytes` = the row tensors the call must read and write once (the
   per-row statistics, 4 or 8 bytes beside 4 to 11 KB of row, are left out); `hbm_fraction` = bytes / time over the 8 TB/s HBM
   peak.
2. A training step of bench.py's 125m configuration (selective_ssm, per-GPU batch 32 x 2048, bf16 autocast, TrainStep) built
   with use_rmsnorm=True: legs of --leg-steps steps with ops.RMSNORM_FUSED on and off, interleaved in one process after a
   warm-up of both.  The off leg is the stock torch module at every norm site, which is what such a model ran before the
   kernels existed.
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
    T, H, p, seed, eps = 44 * 4096, 704, 0.1, 12345, 1e-12
    F, B = _lib.F32, _lib.BF16
    bf = torch.bfloat16
    torch.manual_seed(0)
    x = torch.randn(T, H, device=dev)
    blk, dy = torch.randn(T, H, device=dev).to(bf), torch.randn(T, H, device=dev).to(bf)
    dres = torch.randn(T, H, device=dev)
    g, b = torch.randn(H, device=dev), torch.randn(H, device=dev)
    y32, dx = torch.empty_like(x), torch.empty_like(x)
    y, dblk = torch.empty_like(blk), torch.empty_like(blk)
    rms, mean, rstd = (torch.empty(T, device=dev) for _ in range(3))
    dg, db = torch.empty(H, device=dev), torch.empty(H, device=dev)
    part_r = torch.empty(lib.apertis_rmsnorm_bwd_blocks(T, H), H, device=dev)
    part_l = torch.empty(lib.apertis_layernorm_bwd_blocks(T, H), 2, H, device=dev)
    n = T * H
    pairs = {
        "fwd": (n * 6,
                lambda: lib.apertis_rmsnorm_fwd(P(x), P(g), eps, P(y), P(rms), T, H, F, B, S()),
                lambda: lib.apertis_layernorm_fwd(P(x), P(g), P(b), eps, P(y), P(mean), P(rstd), T, H, F, B, S())),
        "bwd_plain": (n * 10,
                      lambda: lib.apertis_rmsnorm_bwd(P(x), P(g), P(rms), eps, P(dy), None, P(dx), None, 0.0, 0, P(part_r), P(dg),
                                                      T, H, F, B, S()),
                      lambda: lib.apertis_layernorm_bwd(P(x), P(g), P(mean), P(rstd), P(dy), None, P(dx), None, 0.0, 0, P(part_l),
                                                        P(dg), P(db), T, H, F, B, S())),
        "bwd_full": (n * 16,
                     lambda: lib.apertis_rmsnorm_bwd(P(x), P(g), P(rms), eps, P(dy), P(dres), P(dx), P(dblk), p, seed, P(part_r),
                                                     P(dg), T, H, F, B, S()),
                     lambda: lib.apertis_layernorm_bwd(P(x), P(g), P(mean), P(rstd), P(dy), P(dres), P(dx), P(dblk), p, seed,
                                                       P(part_l), P(dg), P(db), T, H, F, B, S())),
        "boundary_fwd": (n * 12,
                         lambda: lib.apertis_dropout_add_rmsnorm_fwd(P(blk), None, None, 0, P(x), P(g), eps, P(y32), P(y), P(rms), T,
                                                                     H, p, seed, F, B, S()),
                         lambda: lib.apertis_dropout_add_layernorm_fwd(P(blk), None, None, 0, P(x), P(g), P(b), eps, P(y32), P(y),
                                                                       P(mean), P(rstd), T, H, p, seed, F, B, S())),
    }
    for what, (nbytes, rms_call, ln_call) in pairs.items():
        times = {"rmsnorm": [], "layernorm": []}
        for _ in range(5):
            assert rms_call() == 0 and ln_call() == 0
        torch.cuda.synchronize()
        for _ in range(iters):
            for name, fn in (("rmsnorm", rms_call), ("layernorm", ln_call)):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                rc = fn()
                e.record()
                e.synchronize()
                assert rc == 0
                times[name].append(s.elapsed_time(e) * 1e3)
        for name, v in times.items():
            med = statistics.median(v)
            emit({"what": "kernel", "kernel": what, "norm": name, "T": T, "H": H, "x": "f32", "out": "bf16", "bytes": nbytes,
                  "us_median": round(med, 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1),
                  "hbm_fraction": round(nbytes / (med * 1e-6) / HBM_PEAK, 3), "iters": iters})


def train_step(dev, emit, batch, leg_steps, legs):
    import torch
    import apertis_llm_amd as A
    from apertis_llm_amd import ops
    from apertis_llm_amd.training import TrainStep
    from bench import CONFIGS
    target, moe, mm, seq, dbatch = CONFIGS["125m"]
    B = batch or dbatch
    torch.manual_seed(0)
    model = A.create_apertis_model(target, vocab_size_override=32000, multimodal=mm, use_expert_system=moe,
                                   attention_type_override="selective_ssm", config_overrides={"use_rmsnorm": True})
    cfg = model.config
    model = model.to(dev).train()
    total = 2 * legs * leg_steps + 8
    step = TrainStep(model, lr=5e-5, weight_decay=0.01, max_grad_norm=1.0, total_steps=total, bf16=True)
    gen = torch.Generator(device=dev).manual_seed(1000)

    def run(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            ids = torch.randint(4, cfg.vocab_size, (B, seq), device=dev, generator=gen)
            loss = step(input_ids=ids, attention_mask=torch.ones_like(ids), labels=ids)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n, float(loss)
    for fused in (True, False, True, False):          # warm-up of both legs
        ops.RMSNORM_FUSED = fused
        run(2)
    res = {True: [], False: []}
    for _ in range(legs):
        for fused in (True, False):
            ops.RMSNORM_FUSED = fused
            t, loss = run(leg_steps)
            assert loss == loss, "NaN loss"
            res[fused].append(1e3 * t)
    ops.RMSNORM_FUSED = True
    for fused, v in res.items():
        emit({"what": "train_step", "config": "125m+use_rmsnorm", "hidden_size": cfg.hidden_size, "layers": cfg.num_hidden_layers,
              "per_gpu_batch": B, "seq_len": seq, "rmsnorm_fused": fused, "ms_per_step_median": round(statistics.median(v), 2),
              "ms_per_step_min": round(min(v), 2), "ms_per_step_max": round(max(v), 2), "legs_ms": [round(x, 2) for x in v],
              "leg_steps": leg_steps, "tokens_per_s": round(B * seq / (statistics.median(v) * 1e-3))})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--batch", type=int, default=0, help="per-GPU batch of the training step (0 = bench.py's default for 125m)")
    ap.add_argument("--leg-steps", type=int, default=6)
    ap.add_argument("--legs", type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("prof_rmsnorm.py needs a ROCm GPU")
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
    if not args.no_step:
        train_step(dev, emit, args.batch, args.leg_steps, args.legs)


if __name__ == "__main__":
    main()
