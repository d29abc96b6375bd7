"""The task passes of a long bag as concurrent GROUPS on their own HIP streams -- the one statement of the mechanics.

The calling stream records a fork event; every group runs behind it on a stream of its own, with its own workspace slot, tape and flat
gradient set (the token-side dW products are read-modify-write: two groups must not accumulate into one buffer); the calling stream
joins the group streams; the extra sets are summed into the store's own.  One group's HBM-bound kernels (LayerNorm family, branch mix,
combine) run under the other's MFMA-bound ones (GEMMs, attention), and the tails of one group's launches fill with the other's
workgroups.  Same box, ms per train step, batched -> two groups: eager at L = 10 000: 42.0 -> 40.4-40.8 (the same groups on ONE stream:
45.0; tools/experiments/pass_overlap.py); hipGraph replay: L = 16 000: 69.5 -> 67.6; 12 000: 51.4 -> 50.6; 10 000: 41.8 -> 40.5;
9 000: 37.7 -> 36.5; 8 000: 33.7 -> 32.9; 6 500: 26.6 -> 27.4 (!); 4 096: 18.2 -> 18.1; 2 500: 12.1 -> 12.2; 1 024: 8.2 -> 8.1.

Users: trainer.TrainStep, evaluate.EmbeddingExtractor (forward only: no gradient sets), the module bridge (aggregators._ModelFn /
_bridge_backward) and module_graph.ModuleReplay (the bridge's two halves captured as a pair, on the module's PassGroups).  What runs
inside a group, which sets a half zeroes and where the sum sits stay with the caller: every launch is enqueued where the caller stands.
"""
import os
from contextlib import contextmanager
from typing import List, Optional, Sequence, Tuple

import torch

from . import ops
from .tape import Tape

SPLIT_MIN_PATCHES = 7500      # shorter bags run the batched pass (the replay figures above)


def group_bounds(B: int, singles: bool = False) -> List[Tuple[int, int]]:
    """Row ranges of the groups of B task passes: B - B // 3 and B // 3 passes (B = 2: one each; B = 1: one group); singles
    (experiments, MT_PASS_GROUPS=singles for TrainStep, MT_MODULE_GROUPS=singles for ModuleReplay): every pass a group of its own."""
    if singles or B < 3:
        return [(i, i + 1) for i in range(max(1, B))]
    return [(0, B - B // 3), (B - B // 3, B)]


def group_slots(groups: Sequence[Tuple[int, int]], base: int = 0) -> List[int]:
    """Workspace slot per group: the engine keys its workspace storage on the pass count, so concurrent groups of EQUAL size must
    not share it (two one-pass groups did until ADVICE r5) -- base + the number of earlier groups of the same size."""
    return [base + sum(1 for a2, b2 in groups[:gi] if b2 - a2 == b - a) for gi, (a, b) in enumerate(groups)]


def split_mode() -> str:
    """MT_SPLIT_PASSES: "off" (0 / off: always the batched pass), "force" (groups wherever they are possible), "auto" (unset / auto:
    the threshold, and TrainStep's trial for a geometry about to be captured) or "on" (anything else: the threshold only)."""
    v = os.environ.get("MT_SPLIT_PASSES", "auto")
    return "off" if v in ("0", "off") else v if v in ("force", "auto") else "on"


def eligible(engine, passes: int, patches: Optional[int], threshold: int, enabled: bool, min_passes: int = 3) -> bool:
    """Groups are the schedule of `passes` task passes over `patches` patches (None: whatever the length): a multi-task model, no
    per-block taps, at least `min_passes` passes and `threshold` patches."""
    return bool(enabled and passes >= min_passes and (patches is None or patches >= threshold) and engine.cfg.is_multi
                and not engine.collect_taps)


def new_tapes(device, n: int, on_realloc=None) -> List[Tape]:
    """n long-lived tapes; on_realloc: the owner's hook for a moved gradient arena (captured graphs point into it)."""
    tapes = [Tape(device) for _ in range(n)]
    for t in tapes:
        t.on_realloc = on_realloc
    return tapes


class PassGroups:
    """The streams, gradient sets (set 0 is the store's own) and tapes of one user's groups, created on first use, and the primitives
    on them.  grad_sets False: a forward-only user; tapes: one long-lived tape per group (tape_on_realloc: see new_tapes)."""

    def __init__(self, engine, grad_sets: bool = True, tapes: bool = False, tape_on_realloc=None):
        self.engine, self._want = engine, (grad_sets, tapes, tape_on_realloc)
        self.streams, self.sets, self.tapes = [], [], []
        self.main, self._fork, self.n = None, None, 0       # the last fork: its stream, its event, its groups

    def ensure(self, n: int) -> "PassGroups":
        """The resources of n groups exist from here on (fork() calls it; call it earlier where the allocations must not sit there)."""
        store, (grad_sets, tapes, on_realloc) = self.engine.store, self._want
        while len(self.streams) < n:
            self.streams.append(torch.cuda.Stream(device=self.engine.device))
        while grad_sets and len(self.sets) < n:
            self.sets.append(store.new_grad_set() if self.sets else (store.flat_grad, store.grads))
        if tapes:
            self.tapes += new_tapes(self.engine.device, n - len(self.tapes), on_realloc)
        return self

    def fork(self, n: int, wait_all: bool = False):
        """Record the fork event for n groups on the current stream.  A group's stream waits for it when the group is entered;
        wait_all: every stream waits now (the re-fork behind a capture cut, the groups being in the middle of their backwards)."""
        self.ensure(n).n = n
        self.main, self._fork = torch.cuda.current_stream(), torch.cuda.Event()
        self._fork.record(self.main)
        for st in self.streams[:n] if wait_all else ():
            st.wait_event(self._fork)

    @contextmanager
    def group(self, gi: int, wait: bool = True, bind: bool = True, zero: Optional[str] = None):
        """Inside group gi: its stream is current (behind the fork event if `wait`); bind: the store points at its gradient set and is put
        back on the way out, whatever happens; zero: "all" -- the group's set is zeroed on its stream; "extra" -- unless it is the store's."""
        st, store = self.streams[gi], self.engine.store
        if wait:
            st.wait_event(self._fork)
        with torch.cuda.stream(st):
            old = store.use_grad_set(*self.sets[gi]) if bind and self.sets else None
            try:
                if zero == "all" or (zero == "extra" and gi > 0):
                    self.sets[gi][0].zero_()
                yield st
            finally:
                if old is not None:
                    store.use_grad_set(*old)

    def join(self):
        """The forking stream waits for what the groups have enqueued so far."""
        for st in self.streams[:self.n]:
            self.main.wait_stream(st)

    def sum_sets(self, ranges: Optional[Sequence[Tuple[int, int]]] = None):
        """Add the extra gradient sets into the store's own on the current stream: whole, or the (offset, n) ranges only."""
        fg = self.sets[0][0]
        for o, n in ([(0, fg.numel())] if ranges is None else ranges):
            for flat, _ in self.sets[1:self.n]:
                ops.axpy(fg[o:o + n], flat[o:o + n], 1.0, fg[o:o + n])

    def backward(self, groups: Sequence[Tuple[int, int]], backward):
        """The backward half of groups whose forwards ran earlier (the module bridge, eager or captured): fork, `backward(gi, a, b)` on
        group gi's stream with the EXTRA sets zeroed there (the store's own was zeroed by the caller), join, the sets summed."""
        self.fork(len(groups))
        for gi, (a, b) in enumerate(groups):
            with self.group(gi, bind=False, zero="extra"):
                backward(gi, a, b)
        self.join()
        self.sum_sets()
