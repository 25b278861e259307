"""generate_many() of a standard_mha model on KV-cache slots (ops.ATTN_SLOTS) against the two forms it replaces, on a workload
with unequal prompts and unequal budgets.

    python tools/prof_generate_many_mha.py [--out FILE] [--rounds 3]

create_apertis_model("125M"), standard_mha, bf16 autocast, greedy; 64 prompts of 200 ... 1 920 tokens and a budget of new
tokens per prompt drawn uniformly from 16 ... 256 and cut so that length + budget stays inside the 2 048-position rotary
table (fixed seeds), no eos: a prompt is done at its budget.  Three legs, alternated in one process, --rounds times each:
  "many"           generate_many(slots=16) under ops.ATTN_SLOTS (the step replays as a graph: model.DECODE_GRAPH)
  "many_prefill_N" the same with prefill_tokens=N, N = 4 096, 8 192, 16 384, 32 768: the waiting prompts of a refill round
                   as one packed row (prefill_packed).  A row length that the layout or the document kernels decline ends
                   that leg, and its line says what declined it
  "leftpad"       the same prompts in arrival order as four left-padded generate() batches of 16 under ops.ATTN_LEFT_PAD,
  "leftpad_graph"  each run to its group's largest budget - or to the end of the rotary table, whichever comes first: the
                   padded width is every row's position - from the eager loop and with ops.ATTN_DECODE_GRAPH; only each
                   row's own budgeted tokens count, and the line says how many of them the table cut off
  "alone"          64 batch-1 generate() calls, from the eager loop and with ops.ATTN_DECODE_GRAPH
  "alone_graph"
The metric is the budgeted new tokens a leg produced over wall time, prefills included.  "many" also reports, from the call's
stats, the token steps it ran and the share of slot-steps that were live; the "many" legs also report the prefill forwards
they made and the summed time of their refill phases (RefillClock: events, no synchronisation inside the call).

Two more lines, measured once:
  "slot_step"      16 prompts of 1 024 tokens, 129 new tokens each (no refill): the replayed slot step's wall time (first to last
                   replay of the call, the bursts' host reads inside) beside the replayed step of ONE left-padded batch of
                   the same shape on the one-length kernels; and the launches of apertis_rope_kv_append_at and
                   apertis_attention_decode_at per token step, counted from the ops' launch records (ops.KernelTimer) on a
                   short eager call - not from a second run under a profiler
Prints one JSON line per leg with every round's value and writes them to --out (profiles/generate_many_mha_mi355x.jsonl is
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

N, SLOTS, LEN_LO, LEN_HI, NEW_LO, NEW_HI, TABLE = 64, 16, 200, 1920, 16, 256, 2048
CAPS = (4096, 8192, 16384, 32768)                     # generate_many(prefill_tokens=...): the "many_prefill_<cap>" legs
CAP_OF = {f"many_prefill_{cap}": cap for cap in CAPS}


def workload():
    rng = random.Random(7)
    lens = [rng.randint(LEN_LO, LEN_HI) for _ in range(N)]
    budgets = [min(rng.randint(NEW_LO, NEW_HI), TABLE - n) for n in lens]
    return lens, budgets


class RefillClock:
    """The refill phases of one generate_many() call, timed apart from its token steps with events and no synchronisation
    of its own: a phase opens at the first prefill forward (a batch-1 forward without a cache, or prefill_packed) after a
    step and closes when the next graph replay - or the graph's capture - is about to start, so it holds the prefill
    forwards of the phase's rounds, the first-token selections with their host reads, the installs and the rewrite of the
    alive flags.  ms() reads the events after the caller's own synchronize()."""

    def __init__(self, model):
        self.model, self.spans, self.open = model, [], None

    def _event(self):
        import torch
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def _close(self):
        if self.open is not None:
            self.spans.append((self.open, self._event()))
            self.open = None

    def __enter__(self):
        import torch
        model, clock = self.model, self
        forward, packed, capture, self.replay = model.forward, model.prefill_packed, model._capture_step, torch.cuda.CUDAGraph.replay

        def spy_forward(*a, **k):
            if k.get("past_key_values") is not None:
                clock._close()                         # (an eager token step ends the phase as a replay does)
            elif clock.open is None:
                clock.open = clock._event()
            return forward(*a, **k)

        def spy_packed(*a, **k):
            if clock.open is None:
                clock.open = clock._event()
            return packed(*a, **k)

        def spy_capture(*a, **k):
            clock._close()
            return capture(*a, **k)

        def spy_replay(graph):
            clock._close()
            return clock.replay(graph)
        model.forward, model.prefill_packed, model._capture_step = spy_forward, spy_packed, spy_capture
        torch.cuda.CUDAGraph.replay = spy_replay
        return self

    def __exit__(self, *exc):
        import torch
        self._close()
        del self.model.forward, self.model.prefill_packed, self.model._capture_step
        torch.cuda.CUDAGraph.replay = self.replay
        return False

    def ms(self):
        return sum(a.elapsed_time(b) for a, b in self.spans)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import bench                                      # noqa: F401  (first: it sets the allocator's environment, as for --decode)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("prof_generate_many_mha.py needs a ROCm GPU")
    import apertis_llm_amd as A
    from apertis_llm_amd import ops
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = A.create_apertis_model("125M", vocab_size_override=32000, attention_type_override="standard_mha").to(dev).eval()
    cfg = model.config
    assert cfg.max_position_embeddings == TABLE, cfg.max_position_embeddings
    lens, budgets = workload()
    gen = torch.Generator(device=dev).manual_seed(7)
    prompts = [torch.randint(4, cfg.vocab_size, (n,), device=dev, generator=gen) for n in lens]

    def padded(rows):
        width = max(len(p) for p in rows)
        ids = torch.zeros(len(rows), width, dtype=torch.long, device=dev)
        mask = torch.zeros_like(ids)
        for b, p in enumerate(rows):
            ids[b, width - len(p):] = p
            mask[b, width - len(p):] = 1
        return ids, mask

    groups = [padded(prompts[g:g + SLOTS]) + (budgets[g:g + SLOTS],) for g in range(0, N, SLOTS)]
    common = dict(eos_token_id=[-1], pad_token_id=0, do_sample=False)

    def many(n=N, cap=None):
        with RefillClock(model) as clock:
            stats = model.generate_many(prompts[:n], max_new_tokens=budgets[:n], slots=SLOTS, return_stats=True,
                                        prefill_tokens=cap, **common)[1]
        stats.setdefault("prefill_forwards", stats["prefills"])           # (without the knob every prefill is a forward)
        return dict(stats, tokens=sum(budgets[:n]), refill=clock)

    def leftpad(n=N):
        steps = live = tokens = cut = 0
        for ids, mask, bud in groups[:max(1, n // SLOTS)]:
            run = min(max(bud), TABLE - ids.shape[1])             # (the padded width positions every row)
            out = model.generate(ids, attention_mask=mask, max_new_tokens=run, use_cache=True, **common)
            assert out.shape[1] == ids.shape[1] + run
            steps += run - 1
            live += sum(min(b, run) - 1 for b in bud)
            tokens += sum(min(b, run) for b in bud)
            cut += sum(b - min(b, run) for b in bud)
        return {"steps": steps, "slot_steps": steps * SLOTS, "live_slot_steps": live, "tokens": tokens, "cut_by_table": cut}

    def alone(n=N):
        for p, m in zip(prompts[:n], budgets[:n]):
            model.generate(p[None], max_new_tokens=m, use_cache=True, **common)
        return {"steps": sum(b - 1 for b in budgets[:n]), "tokens": sum(budgets[:n])}

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

    # leg -> (function, ops.ATTN_SLOTS, ops.ATTN_LEFT_PAD, ops.ATTN_DECODE_GRAPH)
    legs = {"many": (many, True, False, False)}
    for cap in CAPS:
        legs[f"many_prefill_{cap}"] = (lambda n=N, cap=cap: many(n, cap), True, False, False)
    legs.update({"leftpad": (leftpad, False, True, False), "leftpad_graph": (leftpad, False, True, True),
                 "alone": (alone, False, False, False), "alone_graph": (alone, False, False, True)})
    declined = {}
    prev = ops.ATTN_SLOTS, ops.ATTN_LEFT_PAD, ops.ATTN_DECODE_GRAPH, A.model.DECODE_GRAPH
    base = {"what": "generate_many_mha", "config": "125M", "layers": cfg.num_hidden_layers, "hidden": cfg.hidden_size,
            "heads": cfg.num_attention_heads, "dtype": "bf16", "mode": "greedy"}
    try:
        res = {}
        for r in range(args.rounds + 1):              # round 0 is the warm-up, on the first group only
            for name, (fn, slots_on, pad_on, graph_on) in legs.items():
                ops.ATTN_SLOTS, ops.ATTN_LEFT_PAD, ops.ATTN_DECODE_GRAPH = slots_on, pad_on, graph_on
                if name in declined:
                    continue
                try:
                    run = timed(fn, SLOTS) if r == 0 else timed(fn)
                except (ValueError, IndexError, ops.ApertisHipError) as e:
                    if not name.startswith("many_prefill_"):
                        raise
                    declined[name] = f"{type(e).__name__}: {e}"      # (a row length the layout or the kernels decline)
                    res.pop(name, None)
                    continue
                if r:
                    res.setdefault(name, []).append(run)
                    t, st = run
                    print(f"[round {r}] {name}: {st['tokens'] / t:.1f} tokens/s", file=sys.stderr, flush=True)
        for name in legs:
            if name in declined:
                emit(dict(base, leg=name, prompts=N, slots=SLOTS, declined=declined[name]))
                continue
            runs = res[name]
            best_t, stats = min(runs, key=lambda x: x[0])
            d = dict(base, leg=name, prompts=N, slots=1 if name.startswith("alone") else SLOTS, prompt_tokens=sum(lens),
                     budgeted_new_tokens=sum(budgets), counted_new_tokens=stats["tokens"], seconds=round(best_t, 3),
                     tokens_per_s=round(stats["tokens"] / best_t, 1),
                     runs_tokens_per_s=[round(st["tokens"] / t, 1) for t, st in runs], token_steps=stats["steps"])
            if "slot_steps" in stats:
                d["live_share_of_slot_steps"] = round(stats["live_slot_steps"] / stats["slot_steps"], 4)
            if "cut_by_table" in stats:
                d["tokens_cut_by_rotary_table"] = stats["cut_by_table"]
            if "prefills" in stats:
                d.update(prefills=stats["prefills"], graph_replays=stats["replays"], graphs=stats["graphs"],
                         fallbacks=len(stats["fallbacks"]))
            if "refill" in stats:
                d.update(prefill_tokens=CAP_OF.get(name), prefill_forwards=stats["prefill_forwards"],
                         refill_phases=len(stats["refill"].spans), refill_ms=round(stats["refill"].ms(), 2),
                         runs_seconds=[round(t, 4) for t, _ in runs],
                         runs_refill_ms=[round(st["refill"].ms(), 2) for _, st in runs])
            emit(d)

        # ---- the replayed step, slots against the one-length kernels, and the launches of a slot step
        L, NEW = 1024, 129
        same = [torch.randint(4, cfg.vocab_size, (L,), device=dev, generator=gen) for _ in range(SLOTS)]
        real = torch.cuda.CUDAGraph.replay

        def step_ms(fn):
            """(ms per replay from before the call's first replay to after its last, the replays)."""
            first, last, n = [], [], [0]

            def replay(self):
                if not first:
                    first.append(torch.cuda.Event(enable_timing=True))
                    first[0].record()
                real(self)
                n[0] += 1
                last[:] = [torch.cuda.Event(enable_timing=True)]
                last[0].record()
            torch.cuda.CUDAGraph.replay = replay
            try:
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                    fn()
                torch.cuda.synchronize()
            finally:
                torch.cuda.CUDAGraph.replay = real
            return first[0].elapsed_time(last[0]) / n[0], n[0]

        ops.ATTN_SLOTS, ops.ATTN_LEFT_PAD, ops.ATTN_DECODE_GRAPH = True, False, False
        slot_runs = [step_ms(lambda: model.generate_many(same, max_new_tokens=NEW, slots=SLOTS, **common)) for _ in range(3)]
        ops.ATTN_SLOTS, ops.ATTN_DECODE_GRAPH = False, True
        ids = torch.stack(same)
        one_runs = [step_ms(lambda: model.generate(ids, max_new_tokens=NEW, use_cache=True, **common)) for _ in range(3)]
        # launches per step from the ops' launch records, on a short eager call
        ops.ATTN_SLOTS, ops.ATTN_DECODE_GRAPH, A.model.DECODE_GRAPH = True, False, False
        names = ("apertis_rope_kv_append_at", "apertis_attention_decode_at")
        timer = ops.KernelTimer(names)
        ops.set_kernel_timer(timer)
        try:
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                stats = model.generate_many([p[:32] for p in same], max_new_tokens=5, slots=SLOTS, return_stats=True, **common)[1]
        finally:
            ops.set_kernel_timer(None)
        summary = timer.summary()
        emit(dict(base, leg="slot_step", slots=SLOTS, prompt_len=L, new_tokens=NEW,
                  slot_step_ms=[round(ms, 4) for ms, _ in slot_runs], slot_step_replays=slot_runs[0][1],
                  one_length_step_ms=[round(ms, 4) for ms, _ in one_runs], one_length_step_replays=one_runs[0][1],
                  launches_per_step={k: summary[k]["launches"] / stats["steps"] for k in names},
                  eager_launch_ms={k: round(summary[k]["ms"] / summary[k]["launches"], 5) for k in names}))
    finally:
        ops.set_kernel_timer(None)
        ops.ATTN_SLOTS, ops.ATTN_LEFT_PAD, ops.ATTN_DECODE_GRAPH, A.model.DECODE_GRAPH = prev


if __name__ == "__main__":
    main()
