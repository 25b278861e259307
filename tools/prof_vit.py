"""The bidirectional attention kernels (csrc/attention.hip, CAUSAL = false) alone, the vision tower alone and a training step
of bench.py's 1.5b-moe-mm configuration with ops.VIT_FUSED on and off.

    python tools/prof_vit.py [--out FILE] [--no-encoder] [--no-step] [--batch B]

a. Kernels alone, through the C ABI, at the tower's shape: B 72, L 197, H 12, D 64, bf16, with and without dropout p = 0.1.
   Device events around every call, warm-up, then the median and range of the timed calls.  Beside them stock non-causal
   F.scaled_dot_product_attention forward and backward on the SAME tensors (read as [B, H, L, D] views, which is what the
   stock layer hands it after its head transposes; the transposes themselves are not in the timing).  `flops` = 4 B H D L^2
   forward, 2.5 x that backward - the algorithm's, the same figure for both providers.
b. The encoder alone at its real geometry (224^2, patch 16, 12 layers x 768, 12 heads), batch 72, train mode, bf16 autocast,
   forward + backward: legs of --leg-steps steps with the switch on and off, interleaved in one process after a warm-up of
   both, torch.cuda.max_memory_allocated per leg.  The off leg is the stock nn.TransformerEncoderLayer path.
c. A training step of bench.py's 1.5b-moe-mm configuration (per-GPU batch 72 x (197 + 2048), bf16 autocast, TrainStep), legs
   interleaved the same way.
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


def _timed(fn, iters, warm=5):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    v = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        v.append(s.elapsed_time(e) * 1e3)
    return v


def kernels(dev, emit, iters=30):
    import torch
    import torch.nn.functional as F
    from apertis_llm_amd import _lib
    lib, P, S = _lib.load(), _lib.ptr, _lib.stream_ptr
    B, L, H, D = 72, 197, 12, 64
    W, bf = H * D, torch.bfloat16
    gen = torch.Generator(device=dev).manual_seed(0)
    q, k, v, do = (torch.randn(B, L, W, device=dev, generator=gen).to(bf) for _ in range(4))
    out, dq, dk, dv = (torch.empty_like(q) for _ in range(4))
    lse = torch.empty(B, H, L, device=dev, dtype=torch.float32)
    ws = torch.empty(lib.apertis_attention_bwd_workspace_bytes(B, L, H) // 4, device=dev, dtype=torch.float32)
    flops = 4.0 * B * H * D * L * L

    def ok(rc):
        assert rc == 0, rc
    for p in (0.0, 0.1):
        fwd = lambda: ok(lib.apertis_attention_full_fwd(P(q), W, P(k), W, P(v), W, None, P(out), W, P(lse), B, L, H, D, p, 1234,  # noqa: E731
                                                        _lib.BF16, S()))
        bwd = lambda: ok(lib.apertis_attention_full_bwd(P(q), W, P(k), W, P(v), W, P(out), W, P(do), W, P(lse), None, P(ws), P(dq),  # noqa: E731
                                                        P(dk), P(dv), W, B, L, H, D, p, 1234, _lib.BF16, S()))
        qh, kh, vh = (t.view(B, L, H, D).transpose(1, 2).detach().requires_grad_() for t in (q, k, v))
        doh = do.view(B, L, H, D).transpose(1, 2)
        sdpa = lambda: F.scaled_dot_product_attention(qh, kh, vh, dropout_p=p)      # noqa: E731
        with torch.no_grad():
            t_sf = _timed(sdpa, iters)
        o = sdpa()
        t_sb = _timed(lambda: torch.autograd.grad(o, (qh, kh, vh), doh, retain_graph=True), iters)
        for what, prov, mult, t in (("attention_full_fwd", "hip", 1.0, _timed(fwd, iters)),
                                    ("attention_full_bwd", "hip", 2.5, _timed(bwd, iters)),
                                    ("sdpa_noncausal_fwd", "stock", 1.0, t_sf), ("sdpa_noncausal_bwd", "stock", 2.5, t_sb)):
            med = statistics.median(t)
            emit({"what": "kernel", "kernel": what, "provider": prov, "B": B, "L": L, "H": H, "D": D, "dtype": "bf16",
                  "dropout_p": p, "flops": mult * flops, "us_median": round(med, 1), "us_min": round(min(t), 1),
                  "us_max": round(max(t), 1), "TFLOPs": round(mult * flops / (med * 1e-6) / 1e12, 1), "iters": iters})


def _legs(run, set_switch, legs, leg_steps):
    """Warm both legs, then `legs` alternations of (on, off): {switch: [seconds per step]}, {switch: peak bytes}."""
    for fused in (True, False, True, False):
        set_switch(fused)
        run(2)
    res, mem = {True: [], False: []}, {True: 0, False: 0}
    for _ in range(legs):
        for fused in (True, False):
            set_switch(fused)
            t, peak = run(leg_steps)
            res[fused].append(1e3 * t)
            mem[fused] = max(mem[fused], peak)
    set_switch(False)
    return res, mem


def _leg_fields(v, mem, leg_steps):
    return {"ms_per_step_median": round(statistics.median(v), 2), "ms_per_step_min": round(min(v), 2),
            "ms_per_step_max": round(max(v), 2), "legs_ms": [round(x, 2) for x in v], "leg_steps": leg_steps,
            "max_memory_allocated_GiB": round(mem / 2 ** 30, 2)}


def encoder(dev, emit, batch, leg_steps, legs):
    import torch
    import apertis_llm_amd as A
    from apertis_llm_amd import ops
    cfg = A.ApertisConfig(hidden_size=704, num_attention_heads=11, multimodal=True)
    torch.manual_seed(0)
    enc = A.UnifiedMultimodalEncoder(cfg).to(dev).train()
    px = torch.randn(batch, 3, cfg.image_size, cfg.image_size, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    timer = ops.KernelTimer(["apertis_attention_full_fwd"])

    def run(n):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for _ in range(n):
            enc.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = enc(px).float().square().mean()
            loss.backward()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss.detach()).all()), "loss is not finite"
        return (time.perf_counter() - t0) / n, torch.cuda.max_memory_allocated()
    ops.set_kernel_timer(timer)
    res, mem = _legs(run, lambda on: setattr(ops, "VIT_FUSED", on), legs, leg_steps)
    ops.set_kernel_timer(None)
    ran = timer.summary().get("apertis_attention_full_fwd", {"launches": 0})["launches"]
    assert ran == cfg.vision_layers * (4 + legs * leg_steps), ran          # the on legs, and only they, took the kernels
    for fused, v in res.items():
        emit({"what": "encoder_fwd_bwd", "image": cfg.image_size, "patch": cfg.vision_patch_size, "layers": cfg.vision_layers,
              "width": cfg.vision_embed_dim, "heads": cfg.vision_heads, "batch": batch, "dtype": "bf16 autocast", "mode": "train",
              "vit_fused": fused, **_leg_fields(v, mem[fused], leg_steps)})


def train_step(dev, emit, batch, leg_steps, legs):
    import torch
    import apertis_llm_amd as A
    from apertis_llm_amd import ops
    from apertis_llm_amd.training import TrainStep
    from bench import CONFIGS
    target, moe, mm, seq, dbatch = CONFIGS["1.5b-moe-mm"]
    torch.manual_seed(0)
    model = A.create_apertis_model(target, vocab_size_override=32000, multimodal=mm, use_expert_system=moe,
                                   attention_type_override="selective_ssm").to(dev).train()
    cfg = model.config
    B = batch or dbatch
    step = TrainStep(model, lr=5e-5, weight_decay=0.01, max_grad_norm=1.0, total_steps=2 * legs * leg_steps + 16, bf16=True)
    gen = torch.Generator(device=dev).manual_seed(1000)

    def run(n):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for _ in range(n):
            ids = torch.randint(4, cfg.vocab_size, (B, seq), device=dev, generator=gen)
            px = torch.randn(B, 3, cfg.image_size, cfg.image_size, device=dev, generator=gen)
            loss = step(input_ids=ids, attention_mask=torch.ones_like(ids), labels=ids, pixel_values=px)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss.detach()).all()), "loss is not finite"
        return (time.perf_counter() - t0) / n, torch.cuda.max_memory_allocated()
    res, mem = _legs(run, lambda on: setattr(ops, "VIT_FUSED", on), legs, leg_steps)
    tokens = B * (seq + model.model.multimodal_encoder.num_patches + 1)
    for fused, v in res.items():
        emit({"what": "train_step", "config": "1.5b-moe-mm", "per_gpu_batch": B, "seq_len": seq,
              "image_tokens": model.model.multimodal_encoder.num_patches + 1, "vit_fused": fused,
              **_leg_fields(v, mem[fused], leg_steps), "tokens_per_s": round(tokens / (statistics.median(v) * 1e-3))})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-encoder", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--batch", type=int, default=0, help="per-GPU batch of the training step (0 = bench.py's default, 72)")
    ap.add_argument("--encoder-batch", type=int, default=72)
    ap.add_argument("--leg-steps", type=int, default=4)
    ap.add_argument("--legs", type=int, default=4)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("prof_vit.py needs a ROCm GPU")
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
    if not args.no_encoder:
        encoder(dev, emit, args.encoder_batch, args.leg_steps, args.legs)
        torch.cuda.empty_cache()
    if not args.no_step:
        train_step(dev, emit, args.batch, args.leg_steps, args.legs)


if __name__ == "__main__":
    main()
