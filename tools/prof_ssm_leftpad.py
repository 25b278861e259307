"""selective_ssm generate() on a LEFT-PADDED batch: what ops.SSM_LEFT_PAD (APERTIS_SSM_LEFT_PAD=1) costs and what it replaces.

    python tools/prof_ssm_leftpad.py [--out FILE] [--config 1.5b-moe] [--rounds 3] [--modes greedy,chat]

The model of `bench.py --decode` (create_apertis_model, selective_ssm, bf16 autocast), 16 prompts of 200 ... 1 920 tokens
left-padded to 1 920, 128 new tokens, greedy and chat's sampling (T 0.7, top_k 50, top_p 0.9).  Three legs, alternated in one
process, --rounds times each:
  "on"     the batch with the switch on: every row gets what it gets alone
  "alone"  the same 16 prompts as 16 batch-1 calls without padding - the only correct form without the switch
  "off"    the batch with the switch off: the pads run through conv and scan, so the padded rows' tokens are wrong; a COST
           reference only - the same launches but for the conv form - for the prefill time of "on"
Per leg and round the prefill (a generate() of one token) and the token step, (t(128) - t(1)) / 127 as bench.py --decode
computes it; "alone" sums its 16 calls.  Reported per leg: the best and every round's value, tokens/s = new tokens of all
16 rows over the token-step time.  Prints one JSON line per leg and mode and writes them to --out
(profiles/ssm_leftpad_mi355x.jsonl is such a file).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, PREFILL, NEW = 16, 1920, 128
MODES = {"greedy": dict(do_sample=False), "chat": dict(do_sample=True, temperature=0.7, top_k=50, top_p=0.9)}


def _lengths():
    return [round(200 + (PREFILL - 200) * b / (B - 1)) for b in range(B)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--config", default="1.5b-moe")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--modes", default="greedy,chat")
    args = ap.parse_args()
    import bench                                      # (first: it sets the allocator's environment, as for --decode)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("prof_ssm_leftpad.py needs a ROCm GPU")
    import apertis_llm_amd as A
    from apertis_llm_amd import ops
    dev = torch.device("cuda:0")
    target, moe, mm, _, _ = bench.CONFIGS[args.config]
    torch.manual_seed(0)
    model = A.create_apertis_model(target, vocab_size_override=32000, multimodal=mm, use_expert_system=moe,
                                   attention_type_override="selective_ssm").to(dev).eval()
    cfg = model.config
    lens = _lengths()
    ids = torch.randint(4, cfg.vocab_size, (B, PREFILL), device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    mask = torch.ones(B, PREFILL, dtype=torch.long, device=dev)
    for b, n in enumerate(lens):
        mask[b, :PREFILL - n] = 0
    ids = ids * mask
    rows = [(ids[b:b + 1, PREFILL - n:].contiguous(), mask[b:b + 1, PREFILL - n:].contiguous()) for b, n in enumerate(lens)]

    def gen(i, m, n_new, kw):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = model.generate(i, attention_mask=m, max_new_tokens=n_new, eos_token_id=[-1], pad_token_id=0, use_cache=True, **kw)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out

    def leg(name, n_new, kw):
        """(seconds, new tokens [B, n_new]) of one generate() of the leg."""
        ops.SSM_LEFT_PAD = name == "on"
        if name != "alone":
            t, out = gen(ids, mask, n_new, kw)
            return t, out[:, PREFILL:]
        ts, outs = zip(*(gen(i, m, n_new, kw) for i, m in rows))
        return sum(ts), torch.cat([o[:, -n_new:] for o in outs])

    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)
        if args.out:                                  # (written as it goes: an interrupted run keeps what it measured)
            with open(args.out, "w") as f:
                for x in lines:
                    f.write(json.dumps(x) + "\n")
    try:
        for mode in args.modes.split(","):
            kw = MODES[mode]
            res, toks = {}, {}
            for name in ("on", "alone", "off"):           # warm-up: prepared weights, allocator, kernels, the graphs' shapes
                leg(name, 4, kw)
            for _ in range(args.rounds):
                for name in ("on", "alone", "off"):
                    t1, _ = leg(name, 1, kw)
                    tn, toks[name] = leg(name, NEW, kw)
                    res.setdefault(name, []).append((t1, (tn - t1) / (NEW - 1)))
            for name, v in res.items():
                prefill, per_tok = min(x[0] for x in v), min(x[1] for x in v)
                emit({"what": "ssm_generate_leftpad", "config": args.config, "layers": cfg.num_hidden_layers,
                      "hidden": cfg.hidden_size, "d_inner": cfg.ssm_d_inner, "dtype": "bf16", "mode": mode, "leg": name,
                      "left_pad": name == "on", "calls": B if name == "alone" else 1, "prompt_lengths": lens,
                      "padded_to": None if name == "alone" else PREFILL, "new_tokens": NEW,
                      "prefill_ms": round(1e3 * prefill, 3), "ms_per_token_step": round(1e3 * per_tok, 4),
                      "tokens_per_s": round(B / per_tok, 1),
                      "runs_prefill_ms": [round(1e3 * x[0], 3) for x in v], "runs_tokens_per_s": [round(B / x[1], 1) for x in v],
                      # (bf16 on random weights: a near-tie flips between a batch's and a single row's GEMM rounding and a
                      #  greedy row then goes its own way; the fp32 tests compare tokens where the margins are known.  A sampled
                      #  draw hashes the row index: not comparable at all)
                      "rows_with_alone_tokens": int((toks[name] == toks["alone"]).all(1).sum()) if mode == "greedy" else None,
                      "first_tokens_equal_to_alone": int((toks[name][:, 0] == toks["alone"][:, 0]).sum()) if mode == "greedy" else None})
    finally:
        ops.SSM_LEFT_PAD = False


if __name__ == "__main__":
    main()
