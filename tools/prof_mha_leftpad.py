"""standard_mha generate() on a LEFT-PADDED batch: the stock path such a batch takes by default against the HIP kernels it
takes with ops.ATTN_LEFT_PAD (APERTIS_MHA_LEFT_PAD=1), where ops.attention_dead_rows fills the pad rows in.

    python tools/prof_mha_leftpad.py [--out FILE] [--no-e2e] [--no-fill]

1. End to end: create_apertis_model("125M"), standard_mha, bf16 autocast, greedy, B in {1, 16}, 128 new tokens.  Prompt
   lengths spread evenly from 200 to 1 920 tokens (B = 1: 1 060), left-padded to 1 920.  Four legs alternated in one process,
   three rounds, the best of each: "off" (the switch off: stock torch everywhere), "on" (the kernels from the eager loop),
   "on_graph" (ops.ATTN_DECODE_GRAPH too) and "unpadded" (the same ids with every key valid, the kernels from the eager loop:
   the ceiling - no mask to read, no fill).  Per leg the prefill (a generate() of one token) and the token step,
   (t(128) - t(1)) / 127 as bench.py --decode computes it.
2. The fill alone at the prefill's shape (V [B, 1 920, 896] bf16, the masks of 1.): device events around each call, a 512 MiB
   read before every timed call so that V comes from HBM, the median of 40 calls; `hbm_share` is the V bytes of the padded
   sequences over that time as a share of 6.29 TB/s.  One such call per layer and prefill.
Prints one JSON line per measurement and writes them to --out (profiles/mha_leftpad_mi355x.jsonl is such a file).
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
PREFILL, NEW = 1920, 128


def _lengths(B):
    return [1060] if B == 1 else [round(200 + (PREFILL - 200) * b / (B - 1)) for b in range(B)]


def _mask(B, dev):
    import torch
    mask = torch.ones(B, PREFILL, dtype=torch.long, device=dev)
    for b, n in enumerate(_lengths(B)):
        mask[b, :PREFILL - n] = 0
    return mask


def e2e(dev, emit):
    import torch
    import apertis_llm_amd as A
    from apertis_llm_amd import ops
    torch.manual_seed(0)
    model = A.create_apertis_model("125M", vocab_size_override=32000, attention_type_override="standard_mha").to(dev).eval()
    cfg = model.config
    legs = {"off": (False, False, True), "on": (True, False, True), "on_graph": (True, True, True),
            "unpadded": (True, False, False)}              # (ATTN_LEFT_PAD, ATTN_DECODE_GRAPH, padded)
    for B in (1, 16):
        ids = torch.randint(4, 32000, (B, PREFILL), device=dev, generator=torch.Generator(device=dev).manual_seed(7))
        padded = _mask(B, dev)

        def run(n_new, mask):
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = model.generate(ids, attention_mask=mask, max_new_tokens=n_new, do_sample=False, eos_token_id=[-1],
                                     pad_token_id=0, use_cache=True)
                torch.cuda.synchronize()
                return time.perf_counter() - t0, out
        res, toks = {}, {}
        for _ in range(3):
            for leg, (pad_on, graph, is_padded) in legs.items():
                ops.ATTN_LEFT_PAD, ops.ATTN_DECODE_GRAPH = pad_on, graph
                mask = padded if is_padded else None
                run(4, mask)
                t1, _ = run(1, mask)
                tn, out = run(NEW, mask)
                assert out.shape == (B, PREFILL + NEW)
                res.setdefault(leg, []).append((t1, (tn - t1) / (NEW - 1)))
                toks[leg] = out[:, PREFILL:]
        ops.ATTN_LEFT_PAD, ops.ATTN_DECODE_GRAPH = False, False
        for leg, v in res.items():
            prefill, per_tok = min(x[0] for x in v), min(x[1] for x in v)
            emit({"what": "generate_leftpad", "model": "125M", "layers": cfg.num_hidden_layers, "hidden": cfg.hidden_size,
                  "heads": cfg.num_attention_heads, "B": B, "leg": leg, "left_pad": legs[leg][0], "decode_graph": legs[leg][1],
                  "padded": legs[leg][2], "prompt_lengths": _lengths(B) if legs[leg][2] else [PREFILL] * B,
                  "prefill_ms": round(1e3 * prefill, 3), "ms_per_token_step": round(1e3 * per_tok, 4),
                  "tokens_per_s": round(B / per_tok, 1), "step_speedup_over_off": round(min(x[1] for x in res["off"]) / per_tok, 3),
                  "prefill_speedup_over_off": round(min(x[0] for x in res["off"]) / prefill, 3),
                  # (bf16 on random weights: near-ties flip between the kernels' and the stock path's rounding, and a greedy run
                  #  then goes its own way; the fp32 tests compare tokens where the margins are known)
                  "share_of_tokens_equal_to_off": float((toks[leg] == toks["off"]).float().mean()) if legs[leg][2] else None,
                  "runs_ms_per_step": [round(1e3 * x[1], 4) for x in v], "runs_prefill_ms": [round(1e3 * x[0], 3) for x in v]})
    del model
    torch.cuda.empty_cache()


def fill_alone(dev, emit, iters=40):
    import torch
    from apertis_llm_amd import ops
    flush = torch.zeros(64 << 20, dtype=torch.int64, device=dev)
    W = 896                                          # (create-model 125M: 14 heads x 64)
    for B in (1, 16):
        gen = torch.Generator(device=dev).manual_seed(B)
        v = torch.randn(B, PREFILL, W, device=dev, generator=gen).to(torch.bfloat16)
        out = torch.zeros_like(v)
        for name, mask in (("padded", _mask(B, dev)), ("unpadded", torch.ones(B, PREFILL, dtype=torch.long, device=dev))):
            for _ in range(5):
                ops.attention_dead_rows(out, v, mask)
            torch.cuda.synchronize()
            ts = []
            for _ in range(iters):
                flush.sum()
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                ops.attention_dead_rows(out, v, mask)
                e.record()
                e.synchronize()
                ts.append(s.elapsed_time(e) * 1e3)
            us = statistics.median(ts)
            n_pad = int((mask[:, 0] == 0).sum())
            nbytes = float(n_pad) * PREFILL * W * v.element_size()
            emit({"what": "fill_alone", "B": B, "Lk": PREFILL, "W": W, "dtype": "bfloat16", "mask": name,
                  "padded_sequences": n_pad, "dead_rows": int((mask == 0).sum()), "fill_us": round(us, 2), "v_bytes": nbytes,
                  "hbm_share": round(nbytes / (us * 1e-6) / HBM_PEAK, 4), "iters": iters})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--no-fill", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("prof_mha_leftpad.py needs a ROCm GPU")
    dev = torch.device("cuda:0")
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)
        if args.out:                                  # (written as it goes: an interrupted run keeps what it measured)
            with open(args.out, "w") as f:
                for x in lines:
                    f.write(json.dumps(x) + "\n")
    if not args.no_fill:
        fill_alone(dev, emit)
    if not args.no_e2e:
        e2e(dev, emit)


if __name__ == "__main__":
    main()
