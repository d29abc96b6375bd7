"""The captured hipGraphs of recurring bag geometries -- the one statement of the bookkeeping around a replay.

Real data has a new bag length almost every slide, so a geometry (the owner's key) runs the eager schedule until it has been seen
`capture_after` times; then the owner captures it, and up to `size` captures stay (LRU).  What this module keeps:

  visits      eager visits per key, OUTSIDE the LRU: a stream of one-off lengths neither evicts the capture of a hot geometry nor
              resets its count (beyond 4 096 keys the counts are wiped: a hot geometry without a capture is then counted afresh).
  entries     the LRU.  Entries are the owner's own objects; the cache reads one thing, `entry.generation`: the engine generation
              the entry was captured under.  The generation moves when a buffer that graphs point to is gone (a workspace grew, the
              fp16 caches were rebuilt, the stochastic toggle, a tape's gradient arena moved); sync() drops every entry of another
              generation, and get() never returns one -- also not an entry that was held outside the cache meanwhile and put back.
  the pool    ONE private graph memory pool for every capture of an owner: its graphs never run concurrently, so a later capture may
              reuse the blocks an evicted (or still cached) geometry's temporaries occupied.  A fresh pool per capture left every
              evicted graph's segments reserved-but-unusable until the allocator's out-of-memory sweep: +0.24 GiB per recapture at
              L ~ 4 000 when more lengths rotate than the LRU holds (tools/soak.py).  A pool dies with the last graph captured into
              it, so the cache knows those graphs (weakly) and takes a fresh handle only when none is alive; a dead graph that is
              not collected yet keeps the old handle in use, which is the safe direction.
  the ritual  capture(): gc.collect() first -- dead models that sit in reference cycles (a module and its ModuleReplay point at each
              other) keep their hipGraphs until the cyclic collector runs, on whatever allocation, and a graph finalised INSIDE a
              capture aborts the process (torch.cuda.graph collects on entry for the same reason); ONE long-lived capture stream --
              the allocator hands a freed block only to the stream it was allocated on, and torch.cuda.Stream() walks a ring of 32
              streams; capture_error_mode "thread_local" -- RCCL's watchdog thread must not invalidate the capture; on an error
              capture_end() with its own exception swallowed.

Users: trainer.TrainStep (the whole step, cut at the gradient-bucket joins when world > 1, and the optimiser graph as a second capture
into the same pool; with an accumulation window, accumulate > 1, the owner's key is (geometry, ROLE) -- role = (the call zeroes the
gradient buffer, the call is the boundary that reduces and runs the optimiser) -- so visits, admission and the LRU all count
(geometry, role) pairs: a hot geometry is admitted and captured once per role it is met in, at most three, and `size` bounds those
captures, not the geometries), module_graph.ModuleReplay (forward and backward as a pair: one cut) and evaluate.EmbeddingExtractor (one graph
under torch.cuda.graph: only the pool handle comes from here).  What is captured, the key and the entry stay with the owner.
"""
import gc
import weakref
from collections import OrderedDict
from contextlib import contextmanager

import torch

MAX_VISIT_KEYS = 4096


class Capture:
    """A capture in progress on the cache's stream: `graphs` are the finished ones, in order."""

    def __init__(self, cache: "GraphCache"):
        self.cache, self.graphs, self.cur = cache, [], None

    def begin(self):
        self.cur = torch.cuda.CUDAGraph()
        self.cur.capture_begin(pool=self.cache.pool_for(self.cur), capture_error_mode="thread_local")

    def end(self):
        self.cur.capture_end()
        self.graphs.append(self.cur)
        self.cur = None

    def cut(self):
        """End the current graph and begin the next in the same pool (the finished one is alive: the handle stays)."""
        self.end()
        self.begin()

    def abort(self):
        try:
            self.cur.capture_end()
        except Exception:
            pass


class GraphCache:
    def __init__(self, size: int, capture_after: int):
        self.size, self.capture_after = int(size), int(capture_after)      # (read when used: owners change both while running)
        self.entries: "OrderedDict[tuple, object]" = OrderedDict()
        self.visits = {}                   # public and writable: ModuleReplay counts its priming visits itself
        self.generation = -1               # of the last sync()
        self.stream = None
        self._pool = None
        self._pooled = weakref.WeakSet()   # the graphs captured into _pool

    # ---------------------------------------------------------------- admission
    def admit(self, key) -> bool:
        """False: `key` has not been seen `capture_after` times -- this visit is counted and the caller runs it eagerly."""
        seen = self.visits.get(key, 0)
        if seen >= self.capture_after:
            return True
        if len(self.visits) > MAX_VISIT_KEYS:
            self.visits.clear()
        self.visits[key] = seen + 1
        return False

    # ---------------------------------------------------------------- the LRU
    def get(self, key):
        """The entry of `key` captured under the generation of the last sync() (now the most recently used one), or None."""
        ent = self.entries.get(key)
        if ent is None or ent.generation != self.generation:
            return None
        self.entries.move_to_end(key)
        return ent

    def put(self, key, ent):
        self.entries[key] = ent
        self.entries.move_to_end(key)
        while len(self.entries) > max(1, self.size):
            self.entries.popitem(last=False)

    def pop(self, key):
        return self.entries.pop(key, None)

    def clear(self):
        self.entries.clear()

    def sync(self, generation: int) -> bool:
        """Drop every entry captured under another generation than `generation`; True if there was one.  Visit counts stay."""
        self.generation = generation
        stale = [k for k, e in self.entries.items() if e.generation != generation]
        for k in stale:
            del self.entries[k]
        return bool(stale)

    # ---------------------------------------------------------------- capturing
    def pool_for(self, graph):
        """The pool handle `graph` is to be captured into."""
        if self._pool is None or not self._pooled:
            self._pool = torch.cuda.graph_pool_handle()
        self._pooled.add(graph)
        return self._pool

    @contextmanager
    def capture(self):
        """Inside: the cache's stream is current (behind the caller's) and a Capture has begun; it is ended on the way out -- aborted
        if the body raised -- and the caller's stream waits for the cache's."""
        gc.collect()
        main = torch.cuda.current_stream()
        if self.stream is None:
            self.stream = torch.cuda.Stream(device=main.device)
        self.stream.wait_stream(main)
        cap = Capture(self)
        with torch.cuda.stream(self.stream):
            cap.begin()
            try:
                yield cap
            except BaseException:
                cap.abort()
                raise
            cap.end()
        main.wait_stream(self.stream)
