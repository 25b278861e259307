"""Bookkeeping of ApertisForCausalLM.generate_many: which prompt sits in which row (slot) of the decode batch, what each has
produced, and when a slot is free for the next prompt.  Plain Python on host integers: no torch, no device object.  The loop
that owns the GPU state (model.py) asks `head()` for the next prompt in arrival order, either installs it into a free slot
(`place`, with the first token its prefill selected) or finishes it outside the slots (`complete`), and after every burst
of token steps hands over what each slot's row emitted (`feed`).  A prompt's run ends with its first eos, inclusive, or at
its budget; whatever a row emitted beyond that before the host looked is dropped here.  With generate_many(prefill_tokens=N)
the loop fills its free slots in rounds: `waiting(k)` lists the next prompts, `prefill_round` says how many of them one
packed prefill takes.
"""


def mha_slot_capacity(lens, budgets):
    """Rows a KV-cache slot needs so that every prompt fits: max_i(len_i + budget_i) - 1, at least 1.  The last kept token
    of prompt i is selected after the step that appends row len_i + budget_i - 2, so rows [0, len_i + budget_i - 1) are all
    a slot ever has to hold."""
    return max([int(n) + int(m) - 1 for n, m in zip(lens, budgets)] + [1])


def mha_slot_overrun(lens, budgets, max_pos):
    """Index of the first prompt whose len_i + budget_i - 1 exceeds a rotary table of `max_pos` positions (its last step
    would be positioned at len_i + budget_i - 2 >= max_pos, or - budget 1 - its prefill does not fit), None when all fit."""
    return next((i for i, (n, m) in enumerate(zip(lens, budgets)) if int(n) + int(m) - 1 > max_pos), None)


def prefill_round(waiting_lens, free_slots, cap):
    """Which of the waiting prompts one refill round of generate_many(prefill_tokens=cap) takes, as indices into
    `waiting_lens`, their lengths in arrival order.  A prefix - arrival order is kept - of at most `free_slots` prompts
    (one per free slot) whose lengths sum to `cap` at the most, and never less than one prompt: a prompt longer than the
    cap is taken alone.  Empty only when nothing waits or no slot is free."""
    taken, total = [], 0
    for j, n in enumerate(waiting_lens[:max(int(free_slots), 0)]):
        if taken and total + int(n) > cap:
            break
        taken.append(j)
        total += int(n)
    return taken


class SlotSchedule:
    """`n_prompts` prompts, `budgets[i]` new tokens at most for prompt i, `slots` rows.  Invariant between calls:
    len(live()) + pending + done == n_prompts."""

    def __init__(self, n_prompts, budgets, slots):
        if isinstance(budgets, int):
            budgets = [budgets] * n_prompts
        budgets = [int(b) for b in budgets]
        if len(budgets) != n_prompts:
            raise ValueError(f"SlotSchedule: {len(budgets)} budgets for {n_prompts} prompts")
        if slots < 1:
            raise ValueError(f"SlotSchedule: {slots} slots")
        self.n, self.budgets, self.slots = n_prompts, budgets, slots
        self.tokens = [[] for _ in range(n_prompts)]       # the new tokens of every prompt, in arrival order
        self.slot = [None] * slots                         # slot -> prompt index, None: free
        self.done = 0
        self.fed = 0                                       # tokens kept out of all bursts: the slot-steps that were live
        self._next = 0
        self._skip_empty()

    # ---- state -------------------------------------------------------------------------------------------------------
    @property
    def pending(self):
        return self.n - self._next

    def live(self):
        """The occupied slots, ascending."""
        return [b for b, i in enumerate(self.slot) if i is not None]

    def free(self):
        return [b for b, i in enumerate(self.slot) if i is None]

    def finished(self):
        return self.pending == 0 and not self.live()

    def remaining(self, b):
        """Tokens slot b's prompt may still emit."""
        i = self.slot[b]
        return self.budgets[i] - len(self.tokens[i])

    def burst(self, cap):
        """Token steps to run before the host looks again, at most `cap`: up to the last live slot's budget, and - while a
        prompt waits - no further than the first budget that runs out, so that its slot is refilled without idle steps."""
        left = [self.remaining(b) for b in self.live()]
        if not left:
            return 0
        return min(cap, min(left) if self.pending else max(left))

    # ---- arrival order -----------------------------------------------------------------------------------------------
    def head(self):
        """Index of the next prompt in arrival order, None when none waits."""
        return self._next if self._next < self.n else None

    def waiting(self, k):
        """The next `k` prompts in arrival order (fewer when fewer wait), the head first: what k calls of place() or
        complete() in a row would take.  Prompts with nothing to generate are skipped, as head() skips them."""
        out, i = [], self._next
        while i < self.n and len(out) < k:
            if self.budgets[i] > 0:
                out.append(i)
            i += 1
        return out

    def place(self, b, first, eos=()):
        """The head prompt goes into free slot b with `first`, the token its prefill selected.  Returns whether the slot is
        now live: a prompt that ends with its first token is done at once and the slot stays free."""
        if self.slot[b] is not None:
            raise ValueError(f"SlotSchedule: slot {b} holds prompt {self.slot[b]}")
        i = self._pop()
        self.slot[b] = i
        self._extend(b, [first], eos)
        return self.slot[b] is not None

    def complete(self, tokens, eos=()):
        """The head prompt ran outside the slots: `tokens` are its new tokens (cut here like a slot's)."""
        i = self._pop()
        self.tokens[i] = self._cut(tokens, self.budgets[i], eos)[0]
        self.done += 1

    # ---- bursts ------------------------------------------------------------------------------------------------------
    def feed(self, rows, eos=()):
        """`rows[b]`: the tokens slot b's row emitted in the burst, oldest first (rows of free slots are ignored).  Returns
        the slots this burst freed."""
        freed = []
        for b in self.live():
            self.fed += self._extend(b, rows[b], eos)
            if self.slot[b] is None:
                freed.append(b)
        return freed

    # ---- internals ---------------------------------------------------------------------------------------------------
    @staticmethod
    def _cut(tokens, room, eos):
        """(the first `room` tokens up to and with the first eos, whether the run ended there)."""
        kept = []
        for t in tokens:
            if len(kept) >= room:
                break
            kept.append(int(t))
            if kept[-1] in eos:
                return kept, True
        return kept, len(kept) >= room

    def _extend(self, b, tokens, eos):
        i = self.slot[b]
        kept, ended = self._cut(tokens, self.remaining(b), eos)
        self.tokens[i].extend(kept)
        if ended:
            self.slot[b] = None
            self.done += 1
        return len(kept)

    def _pop(self):
        i = self.head()
        if i is None:
            raise ValueError("SlotSchedule: no prompt is pending")
        self._next += 1
        self._skip_empty()
        return i

    def _skip_empty(self):
        while self._next < self.n and self.budgets[self._next] <= 0:    # (nothing to generate: done without a slot)
            self._next += 1
            self.done += 1
