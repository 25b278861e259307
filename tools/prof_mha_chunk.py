"""standard_mha multi-token KV-cache steps: the HIP kernels (ops.kv_append_rope_chunk + ops.attention_chunk,
csrc/attention_decode.hip) against the stock torch branch they replace, and generate() from a kept cache against generate()
without one.

    python tools/prof_mha_chunk.py [--out FILE] [--run N] [--no-layer] [--no-ttft] [--quick]

1. One layer-step alone ("chunk_layer_step"): append + attention on a `multi_token` cache against the stock branch of
   ApertisAttention.forward on the same cache without the flag (RotaryEmbedding twice, torch.cat of the whole past twice, head
   transposes, a dense Lq x Lk mask, F.scaled_dot_product_attention) at create-model's 125M shape (14 heads x 64) and at
   8 x 128, bf16 and fp32, Lq in {16, 64, 256, 1024} x n in {0, 512, 1920} x B in {1, 16}.  Device events around each call,
   warm-up of every shape, then the median of A/B-alternated calls; a 512 MiB read runs before every timed call, so K / V come
   from HBM as in a real step.  `attn_us` times the attention launch(es) alone at the rule's split count; `hbm_share` is its
   q / K / V / out bytes over that time as a share of 6.29 TB/s, `mfma_share` its flops (4 B H D Lq (n + (Lq + 1) / 2)) as a
   share of the MFMA peak of the dtype (bf16 2 516 TF, fp32 157 TF), `bound` the larger of the two floors.  `sweep_us`:
   the attention alone at forced split counts 1, 2, 4, ... 64 - what places apertis_attention_chunk_splits' rule.
2. Time to first token of a second turn ("second_turn_ttft"): create_apertis_model("125M") and ("350M"), standard_mha, bf16
   autocast, a conversation of 1 920 cached + 64 new tokens, B in {1, 16}: generate(max_new_tokens=1, past_key_values=cache)
   against the same call without a cache (the whole conversation prefilled again), legs alternated, every run listed.
Both legs of 2. are timed on the host (time.perf_counter between device synchronisations, no cache-flushing read): the call is
a whole generate(), host-bound at batch 1, and what a user waits for is its wall time.
Prints one JSON line per measurement and writes them to --out.  With --run N every line carries "run": N and --out is
APPENDED to, so `--out F --run 1` followed by `--out F --run 2` leaves both runs in F (without --run the file is rewritten).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 6.29e12
MFMA_PEAK = {"bfloat16": 2516e12, "float32": 157.3e12}


def _timer(dev):
    import torch
    flush = torch.zeros(64 << 20, dtype=torch.int64, device=dev)

    def timed(fn):
        flush.sum()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) * 1e3
    return timed


def layer_step(dev, emit, iters=20, quick=False):
    import torch
    import torch.nn.functional as F
    import apertis_llm_amd as A
    from apertis_llm_amd import ops
    timed = _timer(dev)
    for H, D in ((14, 64), (8, 128)):
        W = H * D
        rope = A.model.RotaryEmbedding(W, 4096).to(dev)
        cos, sin = rope.cos_cached, rope.sin_cached
        for dt in (torch.bfloat16,) if quick else (torch.bfloat16, torch.float32):
            name = str(dt).split(".")[-1]
            for B in (1, 16):
                for n in (0, 512, 1920):
                    for Lq in (16, 64, 256, 1024):
                        Lk = n + Lq
                        gen = torch.Generator(device=dev).manual_seed(Lk + B)
                        q, k, v = (torch.randn(B, Lq, W, device=dev, generator=gen).to(dt) for _ in range(3))
                        past = tuple(torch.randn(B, n, W, device=dev, generator=gen).to(dt) for _ in range(2))
                        cache = ops.KVCache.from_prefill((past,), Lk, multi_token=True)
                        plain = ops.KVCache.from_prefill((past,), Lk)            # no flag: the stock branch reads its views
                        pos = torch.arange(n, Lk, device=dev).unsqueeze(0).expand(B, -1)
                        hold = {}

                        def fused():
                            cache.lengths[0] = n
                            hold["q"] = ops.kv_append_rope_chunk(q, k, v, cache, 0, n, cos, sin)
                            return ops.attention_chunk(hold["q"], cache, 0, H)

                        def attn_only(splits=0):
                            return ops.attention_chunk(hold["q"], cache, 0, H, splits=splits)

                        def stock():
                            qr, kr = rope(q, pos), rope(k, pos)
                            pk, pv = plain[0]
                            kk, vv = torch.cat([pk, kr], dim=1), torch.cat([pv, v], dim=1)
                            qh, kh, vh = (t.view(B, t.shape[1], H, D).transpose(1, 2) for t in (qr, kk, vv))
                            i = torch.arange(Lq, device=dev).unsqueeze(1) + n
                            m = torch.zeros(Lq, Lk, device=dev, dtype=dt).masked_fill_(
                                i < torch.arange(Lk, device=dev).unsqueeze(0), torch.finfo(dt).min)
                            return F.scaled_dot_product_attention(qh, kh, vh, attn_mask=m).transpose(1, 2).reshape(B, Lq, W)
                        rule = ops.attention_chunk_splits(B, H, Lq, Lk, D)
                        counts = [s for s in (1, 2, 4, 8, 16, 32, 64) if s == 1 or B * H * -(-Lq // 64) * s <= 2048]
                        fns = [("fused", fused), ("attn", attn_only), ("stock", stock)]
                        fns += [(f"s{s}", (lambda s=s: attn_only(s))) for s in counts]
                        with torch.no_grad():
                            ref, got = stock(), fused()
                            err = float((got.float() - ref.float()).abs().max())
                            times = {nm: [] for nm, _ in fns}
                            for _ in range(3):
                                for _, fn in fns:
                                    fn()
                            torch.cuda.synchronize()
                            for _ in range(iters):
                                for nm, fn in fns:
                                    times[nm].append(timed(fn))
                        med = {nm: statistics.median(t) for nm, t in times.items()}
                        nbytes = (2.0 * B * Lk + 2.0 * B * Lq) * W * q.element_size()
                        flops = 4.0 * B * W * Lq * (n + (Lq + 1) / 2)
                        t_hbm, t_mfma = nbytes / HBM_PEAK * 1e6, flops / MFMA_PEAK[name] * 1e6
                        emit({"what": "chunk_layer_step", "heads": H, "D": D, "B": B, "n": n, "Lq": Lq, "dtype": name,
                              "splits": rule, "fused_us": round(med["fused"], 2), "attn_us": round(med["attn"], 2),
                              "stock_us": round(med["stock"], 2), "stock_over_fused": round(med["stock"] / med["fused"], 3),
                              "bytes": nbytes, "flops": flops, "hbm_share": round(t_hbm / med["attn"], 4),
                              "mfma_share": round(t_mfma / med["attn"], 4), "bound": "hbm" if t_hbm >= t_mfma else "mfma",
                              "sweep_us": {str(s): round(med[f"s{s}"], 2) for s in counts},
                              "max_abs_diff_vs_stock": err, "iters": iters})


def ttft(dev, emit, reps=5):
    import torch
    import apertis_llm_amd as A
    CACHED, NEW = 1920, 64
    for size in ("125M", "350M"):
        torch.manual_seed(0)
        model = A.create_apertis_model(size, vocab_size_override=32000, attention_type_override="standard_mha").to(dev).eval()
        cfg = model.config
        for B in (1, 16):
            ids = torch.randint(4, 32000, (B, CACHED + NEW), device=dev, generator=torch.Generator(device=dev).manual_seed(7))
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                cache = model.new_kv_cache(B, CACHED + NEW + 8)
                # the first turn, untimed: the cache then holds CACHED rows (prompt CACHED, one new token)
                model.generate(ids[:, :CACHED], max_new_tokens=1, eos_token_id=[-1], past_key_values=cache, prefill_chunk=512)
                cache.lengths = [CACHED] * len(cache)

                def with_cache():
                    cache.lengths = [CACHED] * len(cache)            # (rewind: the same second turn again)
                    return model.generate(ids, max_new_tokens=1, eos_token_id=[-1], past_key_values=cache)

                def without():
                    return model.generate(ids, max_new_tokens=1, eos_token_id=[-1])
                legs = (("cache", with_cache), ("no_cache", without))
                outs = {nm: fn() for nm, fn in legs}
                for _, fn in legs:
                    fn()
                runs = {nm: [] for nm, _ in legs}
                for _ in range(reps):
                    for nm, fn in legs:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        runs[nm].append(1e3 * (time.perf_counter() - t0))
            med = {nm: statistics.median(v) for nm, v in runs.items()}
            emit({"what": "second_turn_ttft", "model": size, "layers": cfg.num_hidden_layers, "hidden": cfg.hidden_size,
                  "heads": cfg.num_attention_heads, "B": B, "cached": CACHED, "new": NEW,
                  "cache_ms": round(med["cache"], 3), "no_cache_ms": round(med["no_cache"], 3),
                  "no_cache_over_cache": round(med["no_cache"] / med["cache"], 3),
                  "cache_runs_ms": [round(x, 3) for x in runs["cache"]], "no_cache_runs_ms": [round(x, 3) for x in runs["no_cache"]],
                  "same_first_token": bool(torch.equal(outs["cache"], outs["no_cache"]))})
        del model
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--run", type=int, default=None, help="tag every line with this run number and append to --out")
    ap.add_argument("--no-layer", action="store_true")
    ap.add_argument("--no-ttft", action="store_true")
    ap.add_argument("--quick", action="store_true", help="bf16 only in the layer-step grid")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("prof_mha_chunk.py needs a ROCm GPU")
    dev = torch.device("cuda:0")
    lines = []

    def emit(d):
        if args.run is not None:
            d = {"run": args.run, **d}
        print(json.dumps(d), flush=True)
        lines.append(d)
        if args.out and args.run is not None:         # (written as it goes: an interrupted run keeps what it measured)
            with open(args.out, "a") as f:
                f.write(json.dumps(d) + "\n")
        elif args.out:
            with open(args.out, "w") as f:
                for x in lines:
                    f.write(json.dumps(x) + "\n")
    if not args.no_ttft:
        ttft(dev, emit)
    if not args.no_layer:
        layer_step(dev, emit, quick=args.quick)


if __name__ == "__main__":
    main()
