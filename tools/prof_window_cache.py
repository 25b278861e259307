"""Sliding window past the window on the KV-cache kernels (ops.ATTN_WINDOW + ops.ATTN_WINDOW_CACHE): what the graph replay of
the windowed token step and the windowed chunk kernel buy generate().

    python tools/prof_window_cache.py [--out DIR] [--rounds N] [--reps N]

One process, synchronised host-clock timing after a warm-up round, the legs of a comparison alternating call by call, every
timed round listed.  DIR/window_cache_mi355x.jsonl (DIR defaults to profiles/) is rewritten, one JSON record per line.  The model
is the 125M standard_mha preset under bf16 autocast, greedy, W 512:
  kind "replay"  a 1 920-token prompt, 128 new tokens, batch 1 and 16: new tokens per second (the prefill timed apart and left
                 out; a graph leg's warm-up and capture are inside its time, as a user pays them) of
                   window_eager  the windowed model on the eager loop (ops.attention_decode(window=), what ATTN_WINDOW alone gives)
                   window_graph  the windowed model on the graph replay (apertis_attention_decode_window_at)
                   full_graph    the unwindowed model on the graph replay (apertis_attention_decode_at), the reference point
                 and whether the two windowed legs selected the same tokens
  kind "chunk"   the first token of a 64-token turn on 1 920 cached rows, batch 1 and 16: the forward of the 64 tokens against
                 the cache alone, in ms, of
                   window_chunk  the windowed model on apertis_attention_chunk_window
                   full_chunk    the unwindowed model on apertis_attention_chunk
                   window_stock  the windowed model with ATTN_WINDOW_CACHE off: the stock branch with its band, which keeps no
                                 cache (generate(past_key_values=) raises there, so only the forward can be timed)
                 and, of the two kernel legs, generate(max_new_tokens=1, past_key_values=cache) and the chunk kernel's own
                 time per launch (HIP events, in three forwards apart from the timed rounds)."""
import argparse
import itertools
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                    # noqa: E402

import apertis_llm_amd as A                     # noqa: E402
from apertis_llm_amd import ops                 # noqa: E402

W, PROMPT, NEW, CACHED, TURN = 512, 1920, 128, 1920, 64


def _switches(window, cache, graph):
    ops.ATTN_WINDOW, ops.ATTN_WINDOW_CACHE, ops.ATTN_DECODE_GRAPH = window, cache, graph


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def replay_records(model, rounds, dev, batches=(1, 16)):
    legs = {"window_eager": (True, True, False), "window_graph": (True, True, True), "full_graph": (False, False, True)}
    for B in batches:
        ids = torch.randint(4, 32000, (B, PROMPT), generator=torch.Generator().manual_seed(B)).to(dev)

        def run(n_new):
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                return _wall(lambda: model.generate(ids, max_new_tokens=n_new, eos_token_id=[-1], use_cache=True, do_sample=False))
        per = {name: {"prefill_s": [], "total_s": []} for name in legs}
        toks = {}
        for r in range(1 + rounds):                           # (round 0 warms every leg up)
            for name, sw in legs.items():
                _switches(*sw)
                p, (t, out) = run(1)[0], run(NEW)
                toks[name] = out
                if r:
                    per[name]["prefill_s"].append(p)
                    per[name]["total_s"].append(t)
        rec = {"kind": "replay", "device": torch.cuda.get_device_name(0), "model": "125M standard_mha", "autocast": "bf16", "B": B,
               "prompt": PROMPT, "W": W, "new_tokens": NEW, "rounds": rounds, "legs": {}}
        for name in legs:
            steps = [t - p for p, t in zip(per[name]["prefill_s"], per[name]["total_s"])]
            med = statistics.median(steps)
            rec["legs"][name] = {"new_tokens_per_s": B * (NEW - 1) / med, "step_ms": med / (NEW - 1) * 1e3, "decode_rounds_s": steps,
                                 "prefill_rounds_s": per[name]["prefill_s"]}
        tps = {name: rec["legs"][name]["new_tokens_per_s"] for name in legs}
        rec["window_graph_over_window_eager"] = tps["window_graph"] / tps["window_eager"]
        rec["window_graph_over_full_graph"] = tps["window_graph"] / tps["full_graph"]
        rec["windowed_legs_same_tokens"] = bool(torch.equal(toks["window_eager"], toks["window_graph"]))
        yield rec
    _switches(False, False, False)


def chunk_records(model, reps, dev, batches=(1, 16)):
    legs = {"window_chunk": (True, True, False), "full_chunk": (False, False, False), "window_stock": (True, False, False)}
    for B in batches:
        ids = torch.randint(4, 32000, (B, CACHED + TURN), generator=torch.Generator().manual_seed(7 + B)).to(dev)
        mask = torch.ones_like(ids)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            caches = {}
            for name, sw in legs.items():                     # the first turn, untimed, per leg: its cache then holds CACHED rows
                _switches(sw[0], True, False)
                caches[name] = model.new_kv_cache(B, CACHED + TURN + 8)
                model.generate(ids[:, :CACHED], max_new_tokens=1, eos_token_id=[-1], past_key_values=caches[name], prefill_chunk=512)

            def forward(name):
                cache = caches[name]
                cache.lengths = [CACHED] * len(cache)         # (rewind: the same second turn again)
                return model(input_ids=ids[:, CACHED:], attention_mask=mask, position_ids=None, past_key_values=cache, use_cache=True)

            def first_token(name):
                cache = caches[name]
                cache.lengths = [CACHED] * len(cache)
                return model.generate(ids, max_new_tokens=1, eos_token_id=[-1], past_key_values=cache)
            fwd = {name: [] for name in legs}
            gen = {name: [] for name in legs if name != "window_stock"}
            kept = {}
            for r in range(2 + reps):                         # (two warm-up rounds)
                for name, sw in legs.items():
                    _switches(*sw)
                    t, out = _wall(lambda: forward(name))
                    kept[name] = out[4] is caches[name]
                    if r >= 2:
                        fwd[name].append(1e3 * t)
                    if name in gen:
                        t, _ = _wall(lambda: first_token(name))
                        if r >= 2:
                            gen[name].append(1e3 * t)
            launch_us = {}
            for name in gen:                                  # the chunk kernel's own time per launch (HIP events), apart
                _switches(*legs[name])
                timer = ops.KernelTimer(["apertis_attention_chunk", "apertis_attention_chunk_window"])
                ops.set_kernel_timer(timer)
                try:
                    for _ in range(3):
                        forward(name)
                finally:
                    ops.set_kernel_timer(None)
                launch_us[name] = {k: {"launches": s["launches"], "us_per_launch": s["ms"] / s["launches"] * 1e3}
                                   for k, s in timer.summary().items()}
        rec = {"kind": "chunk", "device": torch.cuda.get_device_name(0), "model": "125M standard_mha", "autocast": "bf16", "B": B,
               "cached": CACHED, "turn": TURN, "W": W, "reps": reps, "legs": {}}
        for name in legs:
            rec["legs"][name] = {"forward_ms": statistics.median(fwd[name]), "forward_rounds_ms": fwd[name], "kept_the_cache": kept[name]}
            if name in gen:
                rec["legs"][name].update(first_token_ms=statistics.median(gen[name]), first_token_rounds_ms=gen[name],
                                         chunk_kernel=launch_us[name])
        f = {name: rec["legs"][name]["forward_ms"] for name in legs}
        rec["window_chunk_over_full_chunk"] = f["window_chunk"] / f["full_chunk"]
        rec["window_chunk_over_window_stock"] = f["window_chunk"] / f["window_stock"]
        yield rec
    _switches(False, False, False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--rounds", type=int, default=3, help="timed rounds of every generate() leg")
    ap.add_argument("--reps", type=int, default=7, help="timed rounds of every second-turn leg")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prof_window_cache.py measures on a ROCm GPU; none is visible")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = A.create_apertis_model("125M", vocab_size_override=32000, attention_type_override="standard_mha").to(dev).eval()
    model.config.sliding_window = W
    if model.config.max_position_embeddings < PROMPT + NEW:
        raise SystemExit(f"the 125M preset's rotary table ({model.config.max_position_embeddings}) is shorter than {PROMPT + NEW}")
    before = ops.ATTN_WINDOW, ops.ATTN_WINDOW_CACHE, ops.ATTN_DECODE_GRAPH
    os.makedirs(args.out, exist_ok=True)
    try:
        with open(os.path.join(args.out, "window_cache_mi355x.jsonl"), "w") as f:
            for rec in itertools.chain(replay_records(model, args.rounds, dev), chunk_records(model, args.reps, dev)):
                line = json.dumps(rec)
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()
    finally:
        ops.ATTN_WINDOW, ops.ATTN_WINDOW_CACHE, ops.ATTN_DECODE_GRAPH = before


if __name__ == "__main__":
    main()
