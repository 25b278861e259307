"""standard_mha KV-cache decode: the HIP kernels (ops.kv_append_rope + ops.attention_decode, csrc/attention_decode.hip) against
the stock torch step they replace.

    python tools/prof_mha_decode.py [--out FILE] [--no-e2e] [--no-layer] [--no-layer-at]

1. One layer-step alone: append + attention against the stock branch of ApertisAttention.forward (RotaryEmbedding twice,
   torch.cat twice, head transposes, F.scaled_dot_product_attention) at create-model's 125M shape (14 heads x 64) and at
   12 x 64 and 8 x 128, B in {1, 16}, Lk in {128, 512, 2047}, bf16 and fp32.  Device events around each call, warm-up of
   every shape, then the median of A/B-alternated calls; a 512 MiB read runs before every timed call, so K / V come from HBM
   as they do in a real step (the other layers' weights and caches pass through the caches in between; a read, not a fill:
   a fill leaves dirty lines whose write-back would share the timed call's bandwidth).  `attn_us` times the
   attention kernel(s) alone; `hbm_share` is its K / V bytes over that time as a share of 6.29 TB/s.
   Then the device-length attention (ops.attention_decode_at, what a replayed graph runs) at the ONE split count a graph
   tail fixes - the heuristic's at the length the tail ends at - against the by-value kernel at the heuristic's count for
   the length at hand, at the short and the long end of a 1 920 + 128 and of a 128 + 128 generation ("layer_step_at").  The
   replayed step always reads the cache's validity buffer (a sequence may finish inside the tail), so the by-value kernel
   gets the same all-ones mask; `by_value_no_mask_us` is the eager loop's call while nothing is padded (key_valid = None).
2. End to end: generate() new tokens/s on create_apertis_model("125M") and ("350M"), standard_mha, bf16 autocast, B in
   {1, 16}, 1 920-token prefill + 128 new tokens, per token step = (t(128) - t(1)) / 127 as bench.py --decode computes it,
   greedy and chat's sampling parameters, three legs alternated in one process: the stock path (ATTN_DECODE_FUSED off), the
   decode kernels from the eager loop ("fused"), and the same kernels replayed as a graph ("graph": ATTN_DECODE_GRAPH on).
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

HBM_PEAK = 6.29e12


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


def layer_step(dev, emit, iters=40):
    import torch
    import torch.nn.functional as F
    import apertis_llm_amd as A
    from apertis_llm_amd import ops
    timed = _timer(dev)
    for H, D in ((14, 64), (12, 64), (8, 128)):
        W = H * D
        rope = A.model.RotaryEmbedding(W, 2048).to(dev)
        for dt in (torch.bfloat16, torch.float32):
            for B in (1, 16):
                for Lk in (128, 512, 2047):
                    gen = torch.Generator(device=dev).manual_seed(Lk + B)
                    q, k, v = (torch.randn(B, 1, W, device=dev, generator=gen).to(dt) for _ in range(3))
                    past_k, past_v = (torch.randn(B, Lk - 1, W, device=dev, generator=gen).to(dt) for _ in range(2))
                    cache = ops.KVCache.from_prefill(((past_k, past_v),), Lk + 1)
                    pos = torch.full((B, 1), Lk - 1, dtype=torch.long, device=dev)
                    hold = {}

                    def fused():
                        cache.lengths[0] = Lk - 1
                        hold["q"] = ops.kv_append_rope(q, k, v, cache, 0, Lk - 1, rope.cos_cached, rope.sin_cached)
                        return ops.attention_decode(hold["q"], cache, 0, H)

                    def attn_only():
                        return ops.attention_decode(hold["q"], cache, 0, H)

                    def stock():
                        qr, kr = rope(q, pos), rope(k, pos)
                        kk, vv = torch.cat([past_k, kr], dim=1), torch.cat([past_v, v], dim=1)
                        qh, kh, vh = (t.view(B, t.shape[1], H, D).transpose(1, 2) for t in (qr, kk, vv))
                        return F.scaled_dot_product_attention(qh, kh, vh).transpose(1, 2).reshape(B, 1, W)
                    with torch.no_grad():
                        ref, got = stock(), fused()
                        err = float((got.float() - ref[:, 0].float()).abs().max())
                        fns = (("fused", fused), ("attn", attn_only), ("stock", stock))
                        times = {n: [] for n, _ in fns}
                        for _ in range(5):
                            for _, fn in fns:
                                fn()
                        torch.cuda.synchronize()
                        for _ in range(iters):
                            for n, fn in fns:
                                times[n].append(timed(fn))
                    med = {n: statistics.median(t) for n, t in times.items()}
                    nbytes = 2.0 * B * Lk * W * q.element_size()
                    emit({"what": "layer_step", "heads": H, "D": D, "B": B, "Lk": Lk, "dtype": str(dt).split(".")[-1],
                          "splits": ops.attention_decode_splits(B, H, Lk, D), "fused_us": round(med["fused"], 2),
                          "attn_us": round(med["attn"], 2), "stock_us": round(med["stock"], 2),
                          "stock_over_fused": round(med["stock"] / med["fused"], 3), "kv_bytes": nbytes,
                          "hbm_share": round(nbytes / (med["attn"] * 1e-6) / HBM_PEAK, 4), "max_abs_diff_vs_stock": err,
                          "iters": iters})


def layer_step_at(dev, emit, iters=40):
    """attention_decode_at at a graph tail's fixed split count against attention_decode at the heuristic's, bf16."""
    import torch
    from apertis_llm_amd import ops
    timed = _timer(dev)
    dt = torch.bfloat16
    for H, D in ((14, 64), (8, 128)):
        W = H * D
        for B in (1, 16):
            for start, end in ((1920, 2047), (128, 255)):
                fixed = ops.attention_decode_splits(B, H, end, D)
                for Lk in (start, end):
                    gen = torch.Generator(device=dev).manual_seed(Lk + B)
                    q = torch.randn(B, W, device=dev, generator=gen).to(dt)
                    kv = tuple(torch.randn(B, Lk, W, device=dev, generator=gen).to(dt) for _ in range(2))
                    cache = ops.KVCache.from_prefill((kv,), end + 1)
                    cache.step_state_begin(H, splits=fixed)
                    cache.dev_len.fill_(Lk - 1)
                    heur = ops.attention_decode_splits(B, H, Lk, D)
                    ones = cache.dev_valid
                    fns = (("at_fixed", lambda: ops.attention_decode_at(q, cache, 0, H)),
                           ("by_value_heuristic", lambda: ops.attention_decode(q, cache, 0, H, ones)),
                           ("by_value_fixed", lambda: ops.attention_decode(q, cache, 0, H, ones, splits=fixed)),
                           ("by_value_no_mask", lambda: ops.attention_decode(q, cache, 0, H)))
                    with torch.no_grad():
                        same = bool(torch.equal(fns[0][1](), fns[2][1]()))
                        times = {n: [] for n, _ in fns}
                        for _ in range(5):
                            for _, fn in fns:
                                fn()
                        torch.cuda.synchronize()
                        for _ in range(iters):
                            for n, fn in fns:
                                times[n].append(timed(fn))
                    med = {n: round(statistics.median(t), 2) for n, t in times.items()}
                    emit({"what": "layer_step_at", "heads": H, "D": D, "B": B, "generation": [start, end], "Lk": Lk,
                          "dtype": "bfloat16", "splits_fixed": fixed, "splits_heuristic": heur, "at_fixed_us": med["at_fixed"],
                          "by_value_heuristic_us": med["by_value_heuristic"], "by_value_fixed_us": med["by_value_fixed"],
                          "by_value_no_mask_us": med["by_value_no_mask"],
                          "same_bits_as_by_value_fixed": same, "iters": iters})


def e2e(dev, emit):
    import torch
    import apertis_llm_amd as A
    from apertis_llm_amd import ops
    modes = {"greedy": dict(do_sample=False), "chat": dict(do_sample=True, temperature=0.7, top_k=50, top_p=0.9)}
    PREFILL, NEW = 1920, 128
    for size in ("125M", "350M"):
        torch.manual_seed(0)
        model = A.create_apertis_model(size, vocab_size_override=32000, attention_type_override="standard_mha").to(dev).eval()
        cfg = model.config
        for B in (1, 16):
            ids = torch.randint(4, 32000, (B, PREFILL), device=dev, generator=torch.Generator(device=dev).manual_seed(7))

            def run(n_new, kw):
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = model.generate(ids, max_new_tokens=n_new, eos_token_id=[-1], use_cache=True, **kw)
                    torch.cuda.synchronize()
                    return time.perf_counter() - t0, out
            for mode, kw in modes.items():
                res = {}
                for rep in range(3):
                    for fused in ("graph", True, False):
                        ops.ATTN_DECODE_FUSED = bool(fused)
                        ops.ATTN_DECODE_GRAPH = fused == "graph"
                        torch.manual_seed(rep)
                        run(4, kw)
                        t1, _ = run(1, kw)
                        tn, out = run(NEW, kw)
                        assert out.shape == (B, PREFILL + NEW)
                        res.setdefault(fused, []).append((tn - t1) / (NEW - 1))
                ops.ATTN_DECODE_FUSED, ops.ATTN_DECODE_GRAPH = True, False
                for fused, v in res.items():
                    per_tok = min(v)
                    emit({"what": "generate", "model": size, "layers": cfg.num_hidden_layers, "hidden": cfg.hidden_size,
                          "heads": cfg.num_attention_heads, "mode": mode, "B": B, "decode_fused": bool(fused), "decode_graph": fused == "graph",
                          "ms_per_token_step": round(1e3 * per_tok, 4), "tokens_per_s": round(B / per_tok, 1),
                          "runs_ms": [round(1e3 * x, 3) for x in v]})
        del model
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--no-layer", action="store_true")
    ap.add_argument("--no-layer-at", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("prof_mha_decode.py needs a ROCm GPU")
    dev = torch.device("cuda:0")
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)
        if args.out:                                  # (written as it goes: an interrupted run keeps what it measured)
            with open(args.out, "w") as f:
                for x in lines:
                    f.write(json.dumps(x) + "\n")
    if not args.no_layer:
        layer_step(dev, emit)
    if not args.no_layer_at:
        layer_step_at(dev, emit)
    if not args.no_e2e:
        e2e(dev, emit)


if __name__ == "__main__":
    main()
