"""generate_many() against the two forms it replaces, on a workload with unequal prompts and unequal budgets.

    python tools/prof_generate_many.py [--out FILE] [--config 1.5b-moe] [--rounds 3] [--modes greedy,chat] [--bursts 16]

The model of `bench.py --decode` (create_apertis_model, selective_ssm, bf16 autocast), 64 prompts of 200 ... 1 920 tokens and
a budget of new tokens per prompt drawn uniformly from 16 ... 256 (fixed seeds), no eos: a prompt is done at its budget.
Greedy and chat's sampling (T 0.7, top_k 50, top_p 0.9).  Three legs, alternated in one process, --rounds times each:
  "many"     generate_many(slots=16), once per value of --bursts (model.GENERATE_MANY_BURST)
  "leftpad"  the same prompts in arrival order as four left-padded generate() batches of 16 under ops.SSM_LEFT_PAD, each run
             to its group's largest budget; only each row's own budgeted tokens count
  "alone"    64 batch-1 generate() calls
The metric is budgeted new tokens of all prompts over wall time, prefills included.  "many" also reports, from the call's
stats, the token steps it ran and the share of slot-steps that were live; "leftpad" the steps its four groups ran.  Prints
one JSON line per leg and mode with every round's value and writes them to --out (profiles/generate_many_mi355x.jsonl is
such a file).
"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, SLOTS, LEN_LO, LEN_HI, NEW_LO, NEW_HI = 64, 16, 200, 1920, 16, 256
MODES = {"greedy": dict(do_sample=False), "chat": dict(do_sample=True, temperature=0.7, top_k=50, top_p=0.9)}


def workload():
    rng = random.Random(7)
    lens = [rng.randint(LEN_LO, LEN_HI) for _ in range(N)]
    budgets = [rng.randint(NEW_LO, NEW_HI) for _ in range(N)]
    return lens, budgets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--config", default="1.5b-moe")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--modes", default="greedy,chat")
    ap.add_argument("--bursts", default="16", help="values of model.GENERATE_MANY_BURST to run the 'many' leg at")
    args = ap.parse_args()
    import bench                                      # (first: it sets the allocator's environment, as for --decode)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("prof_generate_many.py needs a ROCm GPU")
    import apertis_llm_amd as A
    from apertis_llm_amd import ops
    dev = torch.device("cuda:0")
    target, moe, mm, _, _ = bench.CONFIGS[args.config]
    torch.manual_seed(0)
    model = A.create_apertis_model(target, vocab_size_override=32000, multimodal=mm, use_expert_system=moe,
                                   attention_type_override="selective_ssm").to(dev).eval()
    cfg = model.config
    lens, budgets = workload()
    gen = torch.Generator(device=dev).manual_seed(7)
    prompts = [torch.randint(4, cfg.vocab_size, (n,), device=dev, generator=gen) for n in lens]
    groups = []                                       # the left-padded batches: (ids, mask, the group's budgets)
    for g in range(0, N, SLOTS):
        rows, width = prompts[g:g + SLOTS], max(lens[g:g + SLOTS])
        ids = torch.zeros(len(rows), width, dtype=torch.long, device=dev)
        mask = torch.zeros_like(ids)
        for b, p in enumerate(rows):
            ids[b, width - len(p):] = p
            mask[b, width - len(p):] = 1
        groups.append((ids, mask, budgets[g:g + SLOTS]))
    bursts = [int(x) for x in args.bursts.split(",")]
    common = dict(eos_token_id=[-1], pad_token_id=0)

    def many(kw, n=N):
        return model.generate_many(prompts[:n], max_new_tokens=budgets[:n], slots=SLOTS, return_stats=True, **common, **kw)[1]

    def leftpad(kw, n=N):
        steps = live = 0
        for ids, mask, bud in groups[:max(1, n // SLOTS)]:
            out = model.generate(ids, attention_mask=mask, max_new_tokens=max(bud), use_cache=True, **common, **kw)
            assert out.shape[1] == ids.shape[1] + max(bud)
            steps += max(bud) - 1
            live += sum(b - 1 for b in bud)
        return {"steps": steps, "slot_steps": steps * SLOTS, "live_slot_steps": live}

    def alone(kw, n=N):
        for p, m in zip(prompts[:n], budgets[:n]):
            model.generate(p[None], max_new_tokens=m, use_cache=True, **common, **kw)
        return {"steps": sum(b - 1 for b in budgets[:n])}

    def timed(fn, *a):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stats = fn(*a)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, stats

    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)
        if args.out:                                  # (written as it goes: an interrupted run keeps what it measured)
            with open(args.out, "w") as f:
                for x in lines:
                    f.write(json.dumps(x) + "\n")

    legs = [(f"many/{b}", many, b) for b in bursts] + [("leftpad", leftpad, None), ("alone", alone, None)]
    total = sum(budgets)
    prev_pad, prev_burst = ops.SSM_LEFT_PAD, A.model.GENERATE_MANY_BURST
    try:
        for mode in args.modes.split(","):
            kw = MODES[mode]
            res = {}
            for r in range(args.rounds + 1):              # round 0 is the warm-up, on the first group only
                for name, fn, burst in legs:
                    ops.SSM_LEFT_PAD = name == "leftpad"
                    if burst is not None:
                        A.model.GENERATE_MANY_BURST = burst
                    if r == 0:
                        timed(fn, kw, SLOTS)
                    else:
                        res.setdefault(name, []).append(timed(fn, kw))
                        print(f"[{mode} round {r}] {name}: {total / res[name][-1][0]:.1f} tokens/s", file=sys.stderr, flush=True)
            for name, _, burst in legs:
                runs = res[name]
                best_t, stats = min(runs, key=lambda x: x[0])
                d = {"what": "generate_many", "config": args.config, "layers": cfg.num_hidden_layers, "hidden": cfg.hidden_size,
                     "dtype": "bf16", "mode": mode, "leg": name.split("/")[0], "burst": burst, "prompts": N,
                     "slots": 1 if name == "alone" else SLOTS, "prompt_tokens": sum(lens), "budgeted_new_tokens": total,
                     "seconds": round(best_t, 3), "tokens_per_s": round(total / best_t, 1),
                     "runs_tokens_per_s": [round(total / t, 1) for t, _ in runs], "token_steps": stats["steps"]}
                if "slot_steps" in stats:
                    d["live_share_of_slot_steps"] = round(stats["live_slot_steps"] / stats["slot_steps"], 4)
                if "prefills" in stats:
                    d.update(prefills=stats["prefills"], graph_replays=stats["replays"], fallbacks=len(stats["fallbacks"]))
                emit(d)
    finally:
        ops.SSM_LEFT_PAD, A.model.GENERATE_MANY_BURST = prev_pad, prev_burst


if __name__ == "__main__":
    main()
