"""hipGraph replay under the nn.Module bridge (modaltune_amd.aggregators): the reference trainer's loop -- three model(...) calls, torch
loss, GradScaler.scale(loss).backward() (train_modaltune.py:172-177,225-238) -- with the engine's ~1 000 launches per step issued as TWO
graph replays, one inside the first forward call of a slide (all task passes: the speculative batching of `_forward_one_task`), one inside
the backward node.  What it buys: the trainer's own loop synchronises the host in front of the backward (its `text[[0, 1, 3], :]` index
goes through a pageable host-to-device copy), so an eager backward starts on an idle GPU and its first hundred small launches run at the
host's pace; a replay does not (bench.py `module_api`).

A bag geometry (patch count, pass count, gene count) that has been seen `capture_after` times with gradients enabled is run twice more
through this class WITHOUT capture (same launches on the long-lived workspaces and tapes: the tapes size their zero-initialised gradient
arenas from those two visits, as TrainStep's eager visits do) and captured on the next visit; other geometries, chained calls (a slide's later calls that were not part of the batched pass) and every no-grad call keep the eager
path.  The captured pair works on long-lived workspaces of its own (the engine's slots 8 ..: a TrainStep, an EmbeddingExtractor or a no-grad
forward on the same engine use slots 0 ..), so only ONE replayed forward may be waiting for its backward at a time: a second forward before
that backward runs eagerly on a private workspace.  Dropout / DropPath:
the forward graph advances the engine's device-side Philox state first, so every replay draws fresh masks (the backward graph
regenerates them from the same state).
"""
from __future__ import annotations

import os
import weakref
from typing import Optional

import torch

from . import ops, pass_groups
from .engine import F32, flatten_genes
from .graph_cache import GraphCache


class _Lease:
    """Held by the autograd node of a forward this class served until its backward has run (or the node has died)."""
    __slots__ = ("done", "ent", "calls", "groups", "split", "__weakref__")

    def __init__(self, ent, calls, groups, split):
        self.done = False
        self.ent, self.calls, self.groups, self.split = ent, calls, groups, split      # calls None: captured (the backward is a replay)


class _Entry:
    __slots__ = ("gf", "gb", "logits", "dl", "split", "generation")

    def __init__(self, generation: int):
        self.gf = self.gb = self.logits = self.dl = None
        self.split, self.generation = False, generation


class ModuleReplay:
    cache_size = property(lambda o: o.graphs.size, lambda o, v: setattr(o.graphs, "size", int(v)))
    capture_after = property(lambda o: o.graphs.capture_after, lambda o, v: setattr(o.graphs, "capture_after", int(v)))
    visits = property(lambda o: o.graphs.visits, lambda o, v: setattr(o.graphs, "visits", v))      # (the priming visits are counted here too)

    def __init__(self, module, capture_after: int = 2, cache_size: int = 4):
        self.module = module
        self.enabled = os.environ.get("MT_MODULE_GRAPH", "1") not in ("0", "off")
        self.graphs = GraphCache(cache_size, capture_after)      # key -> _Entry
        self.static_key = None
        self.sgenes = self.sonehots = self.sclin = None
        self.lease = None                 # weakref to the _Lease of the replayed forward whose backward is still to come
        self.tapes = None                 # [0]: the batched pass, [1] ..: the pass groups (their streams and gradient sets: module._split_state)
        self.replays = self.captures = self.eager_fallbacks = self.primed = 0
        self.ncap = {}                    # captures per geometry: one that had to be captured AGAIN was evicted in between -> the cache grows

    # ---------------------------------------------------------------- resources
    def _busy(self) -> bool:
        l = self.lease() if self.lease is not None else None
        return l is not None and not l.done

    def _resources(self, groups):
        """This class's tapes, and the module's PassGroups (shared with its eager split path) when `groups` are pass groups."""
        eng = self.module.engine
        if self.tapes is None:
            self.tapes = pass_groups.new_tapes(eng.device, 5, eng._bump_generation)      # captured graphs point into the tapes' gradient arenas
        return self.module._split_state(len(groups)) if len(groups) > 1 else None

    SLOT0 = 8         # workspace slots of this class: its own, so that a TrainStep / EmbeddingExtractor / no-grad forward on the same engine
                      # (slots 0 ..) between a replayed forward and its backward cannot overwrite the saved activations

    # ---------------------------------------------------------------- forward
    def forward(self, x, coords, genes, onehots, clinical, token) -> Optional[tuple]:
        """Returns (logits [B, O] -- a fresh tensor --, lease) when this call was served by a replay, by a priming visit or by the
        capture that makes the next ones replays; None when the eager path has to run it."""
        m = self.module
        eng = m.engine
        if not self.enabled or token is not None or eng.collect_taps or not eng.MODULE_REPLAY:
            return None
        x2 = x.reshape(-1, x.shape[-1])
        L, B = int(x2.shape[0]), int(onehots.shape[0])
        if m.is_multi and B != m.cfg.multi_task:
            return None                    # (a single task's call: its siblings chain behind it -- eager)
        if torch.cuda.is_current_stream_capturing():
            return None
        gl = [genes] if torch.is_tensor(genes) else list(genes)
        ngenes = int(sum(g.numel() for g in gl))
        split = pass_groups.eligible(eng, B, L, m.split_min_patches, m.split_passes)
        key = (L, B, ngenes, split, bool(eng.stochastic), None if clinical is None else tuple(clinical.shape))
        graphs = self.graphs
        ent = graphs.get(key)
        seen = self.visits.get(key, 0)
        if (ent is None or ent.gf is None) and not graphs.admit(key):
            return None
        if self._busy():
            self.eager_fallbacks += 1
            return None
        if not eng._caches_ready:
            eng._build_caches()
        skey = (ngenes, B, int(onehots.shape[1]), None if clinical is None else int(clinical.numel()))
        if self.static_key != skey:
            self.static_key = skey
            dev = eng.device
            self.sgenes = torch.empty(ngenes, dtype=F32, device=dev)
            self.sonehots = torch.empty(B, int(onehots.shape[1]), dtype=F32, device=dev)
            self.sclin = torch.empty(1, int(clinical.numel()), dtype=F32, device=dev) if clinical is not None else None
            graphs.clear()
        groups = pass_groups.group_bounds(B, singles=os.environ.get("MT_MODULE_GROUPS") == "singles") if split else [(0, B)]      # (experiments)
        slots = pass_groups.group_slots(groups, base=self.SLOT0)
        for (a, b), sl in list(zip(groups, slots))[1:]:
            eng._workspace(b - a, L, slot=sl)                       # (all workspaces exist -- and have grown -- before anything is captured)
        eng.stage_inputs(x2, coords, eng._workspace(groups[0][1] - groups[0][0], L, slot=slots[0]))      # (may grow the workspace: bumps eng.generation)
        gflat = flatten_genes(gl)
        self.sgenes.copy_(gflat.to(F32) if len(gl) > 1 else gflat, non_blocking=True)
        self.sonehots.copy_(onehots, non_blocking=True)
        if self.sclin is not None:
            self.sclin.copy_(clinical.reshape(1, -1), non_blocking=True)
        graphs.sync(eng.generation)               # buffers the old captures point to are gone
        ent = graphs.get(key)
        if ent is None:
            ent = _Entry(eng.generation)
            graphs.put(key, ent)
        self._buffers(ent, B)
        calls = None
        if ent.gf is None and seen < self.capture_after + 2:
            # priming visit: the same launches, eagerly (the tapes' gradient arenas are sized from these two visits)
            self.visits[key] = seen + 1
            hook, eng.grad_ready_hook = eng.grad_ready_hook, None
            try:
                calls = self._forward_body(ent, L, B, groups, slots, split)
            finally:
                eng.grad_ready_hook = hook
            self.primed += 1
        else:
            if ent.gf is None:
                self.ncap[key] = self.ncap.get(key, 0) + 1
                if self.ncap[key] >= 2 and self.cache_size < 16 and len(graphs.entries) >= self.cache_size:
                    self.cache_size *= 2      # more recurring geometries than entries (a rotation would recapture on every visit)
                self._capture(ent, L, B, groups, slots, split)
                if graphs.sync(eng.generation):   # the capture itself moved a buffer: these graphs are stale -- prime and capture again
                    self.visits[key] = self.capture_after
                    return None
            ent.gf.replay()
            self.replays += 1
        lease = _Lease(ent, calls, groups, split)
        self.lease = weakref.ref(lease)
        return ent.logits.clone(), lease

    def _forward_body(self, ent, L, B, groups, slots, split):
        m = self.module
        eng = m.engine
        pg = self._resources(groups)
        if eng.stochastic:
            ops.rng_advance(eng.rng)
        if not split:
            logits = eng.forward(None, None, self.sgenes, self.sonehots, need_grad=True, staged=True, geometry=(B, L), clinical=self.sclin,
                                 tape=self.tapes[0], site_group=1, ws_slot=slots[0])
            ent.logits.copy_(logits)
            return [eng.last_call]
        ws0 = eng._workspace(groups[0][1] - groups[0][0], L, slot=slots[0])
        eng._embed_patches(None, None, ws0, True, L)            # task-independent: once, in front of the fork
        share = {"x0": ws0["x0"]}
        pg.fork(len(groups))
        calls = []
        for gi, (a, b) in enumerate(groups):
            with pg.group(gi):
                logits = eng.forward(None, None, self.sgenes, self.sonehots[a:b], need_grad=True, staged=True, geometry=(b - a, L),
                                     clinical=self.sclin, share=share, tape=self.tapes[1 + gi], site_group=gi + 1, ws_slot=slots[gi])
                calls.append(eng.last_call)
                ent.logits[a:b].copy_(logits)
        pg.join()
        return calls

    def _backward_body(self, ent, calls, groups, split):
        eng = self.module.engine
        if not split:
            eng.backward(ent.dl, call=calls[0])
            return
        self._resources(groups).backward(groups, lambda gi, a, b: eng.backward(ent.dl[a:b], call=calls[gi]))

    def _buffers(self, ent, B):
        eng = self.module.engine
        if ent.logits is None or ent.logits.shape[0] != B:
            O = int(eng.store.tensors["final_project.bias"].numel())
            ent.logits = torch.zeros(B, O, dtype=F32, device=eng.device)
            ent.dl = torch.zeros(B, O, dtype=F32, device=eng.device)

    def _capture(self, ent, L, B, groups, slots, split):
        eng = self.module.engine
        ent.split = split
        self._resources(groups)
        hook, eng.grad_ready_hook = eng.grad_ready_hook, None
        try:
            with self.graphs.capture() as cap:
                calls = self._forward_body(ent, L, B, groups, slots, split)
                cap.cut()
                self._backward_body(ent, calls, groups, split)
        finally:
            eng.grad_ready_hook = hook
        ent.gf, ent.gb = cap.graphs
        self.captures += 1

    # ---------------------------------------------------------------- backward
    def backward(self, lease, scaled_into):
        """`scaled_into(dst)`: writes the scaled fp32 gradient of the logits into the entry's static buffer; then the backward graph (or,
        on a priming visit, the same launches eagerly)."""
        ent = lease.ent
        scaled_into(ent.dl)
        if lease.calls is None:
            ent.gb.replay()
        else:
            self._backward_body(ent, lease.calls, lease.groups, lease.split)
            lease.calls = None
        lease.done = True
