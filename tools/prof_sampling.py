"""Sampled decode, fused sampler (ops.sample_next, csrc/sampling.hip) against the stock torch block of generate().

    python tools/prof_sampling.py [--out FILE] [--no-e2e]

1. Kernel alone: one sample_next launch against the stock block (topk, sort, softmax, cumsum, scatter, masked_fill, softmax,
   multinomial) at B in {1, 16}, V = 32 000, fp32 and bf16 logits, chat's parameters (T 0.7, top_k 50, top_p 0.9).  Device
   events around each call, warm-up, then the median of A/B-alternated calls.
2. End to end: generate() new tokens/s on bench.py's 1.5b-moe config with bench's decode protocol (2048-token prefill, 128
   new tokens, bf16 autocast; per token step = (t(128) - t(1)) / 127), B in {1, 16}: chat's parameters, the same with
   repetition_penalty 1.1, and greedy; each with SAMPLE_FUSED on and off, alternated in one process.  The stock penalty
   loop issues one launch per history token and row per step: its B = 16 run decodes 16 new tokens instead of 128.
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


def stock_block(x, temp=0.7, top_k=50, top_p=0.9):
    """model.py's stock sampling block (reference core.py:1613-1626)."""
    import torch
    import torch.nn.functional as F
    x = x.float() / temp
    kth = torch.topk(x, top_k).values[:, -1:]
    x = x.masked_fill(x < kth, float("-inf"))
    srt, order = torch.sort(x, descending=True)
    drop = torch.cumsum(F.softmax(srt, dim=-1), dim=-1) > top_p
    drop[..., 1:] = drop[..., :-1].clone()
    drop[..., 0] = False
    x = x.masked_fill(torch.zeros_like(drop).scatter_(-1, order, drop), float("-inf"))
    return torch.multinomial(F.softmax(x, dim=-1), 1).squeeze(1)


def kernel_ab(dev, emit, iters=200):
    import torch
    from apertis_llm_amd import ops
    for B in (1, 16):
        for dt in (torch.float32, torch.bfloat16):
            logits = (torch.randn(B, 32000, device=dev) * 3).to(dt)
            alive = torch.ones(B, dtype=torch.long, device=dev)
            err = torch.zeros(1, dtype=torch.int32, device=dev)
            out = torch.empty(B, dtype=torch.long, device=dev)
            a_out = torch.empty_like(alive)
            step = torch.zeros(1, dtype=torch.long, device=dev)

            def fused():
                ops.sample_next(logits, alive, err, do_sample=True, temperature=0.7, top_k=50, top_p=0.9, seed=1, step=step,
                                alive_out=a_out, out=out)

            def stock():
                stock_block(logits)
            times = {"fused": [], "stock": []}
            for _ in range(10):
                fused()
                stock()
            torch.cuda.synchronize()
            for _ in range(iters):
                for name, fn in (("fused", fused), ("stock", stock)):
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    fn()
                    e.record()
                    e.synchronize()
                    times[name].append(s.elapsed_time(e) * 1e3)
            assert int(err[0]) == 0
            emit({"what": "kernel", "B": B, "V": 32000, "dtype": str(dt).split(".")[-1],
                  "fused_us_median": statistics.median(times["fused"]), "stock_us_median": statistics.median(times["stock"]),
                  "iters": iters})


def e2e(dev, emit):
    import torch
    import apertis_llm_amd as A
    from apertis_llm_amd import ops
    sys.path.insert(0, ROOT)
    from bench import CONFIGS
    target, moe, mm, seq, _ = CONFIGS["1.5b-moe"]
    torch.manual_seed(0)
    model = A.create_apertis_model(target, vocab_size_override=32000, multimodal=mm, use_expert_system=moe,
                                   attention_type_override="selective_ssm").to(dev).eval()
    modes = {"chat": dict(do_sample=True, temperature=0.7, top_k=50, top_p=0.9),
             "chat_penalty": dict(do_sample=True, temperature=0.7, top_k=50, top_p=0.9, repetition_penalty=1.1),
             "greedy": dict(do_sample=False)}
    for B in (1, 16):
        ids = torch.randint(4, 32000, (B, 2048), device=dev, generator=torch.Generator(device=dev).manual_seed(7))

        def run(n_new, kw):
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = model.generate(ids, max_new_tokens=n_new, eos_token_id=[-1], use_cache=True, **kw)
                torch.cuda.synchronize()
                return time.perf_counter() - t0, out
        for mode, kw in modes.items():
            res = {}
            for rep in range(2):
                for fused in (True, False):
                    ops.SAMPLE_FUSED = fused
                    new = 16 if (not fused and B == 16 and mode == "chat_penalty") else 128
                    torch.manual_seed(rep)
                    run(4, kw)
                    t1, _ = run(1, kw)
                    tn, out = run(new, kw)
                    assert out.shape == (B, 2048 + new)
                    per_tok = (tn - t1) / (new - 1)
                    res.setdefault(fused, []).append(per_tok)
            ops.SAMPLE_FUSED = True
            for fused, v in res.items():
                per_tok = min(v)
                emit({"what": "generate", "mode": mode, "B": B, "sample_fused": fused, "ms_per_token_step": 1e3 * per_tok,
                      "tokens_per_s": B / per_tok, "runs_ms": [round(1e3 * x, 3) for x in v]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-e2e", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("prof_sampling.py needs a ROCm GPU")
    dev = torch.device("cuda:0")
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)
    kernel_ab(dev, emit)
    if not args.no_e2e:
        e2e(dev, emit)
    if args.out:
        with open(args.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
