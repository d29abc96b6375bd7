"""One slide train step exactly as train_modaltune.py:195-240 does it, on the HIP engine:
frozen text projector -> 3 task passes (batched) -> KL distillation loss -> backward -> GradScaler-style
unscale/skip -> data-parallel mean of the flat gradient buffer -> fused AdamW.

Data parallelism follows the reference's intent (base_trainer.py:192-211: one process per GPU, DDP mean of the
trainable gradients): slides shard over ranks; the collective is a bucketed SUM all-reduce of the flat fp32 gradient
buffer (RCCL on GPUs, gloo in the rehearsals) whose buckets are launched from inside the backward, as soon as the
stage that owns them has run (dp.grad_buckets: head + interaction block 2, block 1, block 0, gene encoder), and waited
for just before AdamW -- the collectives of the upper blocks run under the backward of the lower ones.
"""
from __future__ import annotations

import contextlib
import os
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import dp, ops, optim, pass_groups
from ._lib import rowmap
from .engine import Engine, F32, flatten_genes
from .graph_cache import GraphCache
from .tape import Param, Var


class _Captured:
    """The hipGraphs of one bag geometry: `segs` = [(graph, bucket or None)] replayed in order; after a segment with a
    bucket index the reducer starts that bucket (world_size > 1 cuts the backward at the bucket boundaries; on one GPU
    the whole step, optimiser included, is a single segment)."""
    __slots__ = ("segs", "logits", "generation")

    def __init__(self, generation: int):
        self.segs, self.logits, self.generation = None, None, generation


class TrainStep:
    graph_cache_size = property(lambda o: o._gcache.size, lambda o, v: setattr(o._gcache, "size", int(v)))      # (both live on the cache: assigned after construction too)
    capture_after = property(lambda o: o._gcache.capture_after, lambda o, v: setattr(o._gcache, "capture_after", int(v)))

    def __init__(self, engine: Engine, lr: float = 1e-4 / 20, weight_decay: float = 0.01, betas=(0.9, 0.999),
                 eps: float = 1e-8, init_scale: float = 2.0 ** 15, growth_interval: int = 2000,
                 process_group=None, task_ids: Sequence[int] = (0, 1, 2), text_rows: Sequence[int] = (0, 1, 3),
                 graph_cache_size: int = 8, capture_after: int = 2, split_passes="auto", accumulate: int = 1,
                 max_grad_norm: Optional[float] = None, verify_every: int = 0, param_groups: Optional[Sequence[dict]] = None,
                 ema_decay: Optional[float] = None, ema_warmup: bool = False):
        self.engine, self.dev = engine, engine.device
        # Exponential moving average of the trainable weights (every step is taken on ONE slide: the weights at an epoch's end are a noisy
        # sample of the trajectory, the average is what to evaluate and save).  `ema` is one more flat fp32 buffer laid out like the
        # parameters, a copy of them at construction, moved INSIDE the AdamW launch (mt_adamw_step_groups_ema: e += w * (p_new - e)
        # with w = 1 - decay, or 1 - min(decay, (1 + t) / (10 + t)) at optimiser step t with ema_warmup) -- so it moves exactly when
        # the parameters do: at a window's boundary, not at micro-steps, not at a skipped step; in eager steps, replays and the world
        # > 1 optimiser graph alike; with a sharded last bucket a rank averages its own shard only (completed where it is read:
        # state_dict(), ema_weights()).  ema_decay / ema_warmup are launch arguments (set_ema_decay drops the captures).  A step without
        # parameter groups goes through the grouped kernel with a one-segment table (lr_mult 1, the step's weight_decay): the bits of
        # mt_adamw_step.  None (the default): nothing is allocated, nothing is launched differently.
        self.ema_decay, self.ema_warmup = _valid_ema_decay(ema_decay), bool(ema_warmup)
        self.ema, self._ema_seg, self._ema_swapped = None, None, False
        # Replica canary (data parallel): every `verify_every`-th boundary call ends with verify_replicas() -- the 8-byte checksum of the
        # flat parameter buffer, MIN- and MAX-reduced over the group, raises on every rank when the replicas differ.  The count of
        # boundary calls is HOST state.  0 (the default): nothing is launched, allocated or synchronised for it.
        if int(verify_every) < 0:
            raise ValueError(f"verify_every must be >= 0 (got {verify_every})")
        self.verify_every, self._boundaries = int(verify_every), 0
        self._cs_ws = None      # int64: mt_checksum64's workspace, allocated by the first checksum (never inside a capture)
        # Gradient accumulation and global-norm clipping.  A WINDOW is `accumulate` consecutive calls of step() / step_graphed(), mixed
        # freely: calls 1 .. k-1 are micro-steps (dropout counter, forward, loss, backward ADDING into the flat gradient buffer; no
        # collective, no optimiser, no scaler update), the k-th is the boundary (reduce, inf check, AdamW, scaler update) and applies
        # the MEAN over the window: grad_mult = 1 / (world * k).  The loss scale therefore cannot move inside a window and one inf
        # anywhere in it skips the whole window's update (torch's accumulate-then-scaler.step).  max_grad_norm: at the boundary
        # mt_grad_sumsq stands in for mt_check_finite, mt_grad_clip_coef forms torch's clip_grad_norm_ coefficient on the device and
        # AdamW divides by `scale / coef` -- nothing is read back; float("inf") only reports the norm.  `window_pos` (micro-steps the
        # open window holds) is HOST state.  accumulate == 1 and max_grad_norm None: the step as it always was, launch for launch.
        if int(accumulate) < 1 or (max_grad_norm is not None and not float(max_grad_norm) >= 0.0):
            raise ValueError(f"accumulate must be >= 1 and max_grad_norm >= 0 (got {accumulate}, {max_grad_norm})")
        self.accumulate = int(accumulate)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.window_pos = 0
        self._clip_out = torch.zeros(3, dtype=F32, device=self.dev)      # mt_grad_clip_coef's {total norm, coefficient, scale / coefficient}
        self.grad_norm, self.clip_coef = self._clip_out[0:1], self._clip_out[1:2]      # (written at a boundary, when max_grad_norm is set)
        self._clip_scale = self._clip_out[2:3]
        self._sumsq = self._sumsq_ws = None      # float64: one sum-of-squares slot per optimiser piece, mt_grad_sumsq's workspace
        self.wd, self.betas, self.eps = weight_decay, betas, eps
        n = engine.store.n_flat
        self.m = torch.zeros(n, dtype=F32, device=self.dev)
        self.v = torch.zeros(n, dtype=F32, device=self.dev)
        self.scale = torch.full((1,), float(init_scale), dtype=F32, device=self.dev)
        # the loss scale the gradients now in the flat buffer were produced with (copied on the device where the loss reads
        # `scale`: the scaler update behind an update=True step moves `scale` on to the NEXT step's value)
        self.grad_scale = torch.full((1,), float(init_scale), dtype=F32, device=self.dev)
        self.tracker = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.found_inf = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.growth_interval = growth_interval
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=self.dev)   # completed optimiser steps (skips excluded)
        # the learning rate lives on the device: AdamW reads it there, so a scheduler (the reference steps
        # GradualWarmupScheduler + CosineAnnealingLR every epoch, TM:151-154,242) reaches captured graphs as well
        self.lr_dev = torch.full((1,), float(lr), dtype=F32, device=self.dev)
        self._lr = float(lr)
        self.pg = process_group
        self.task_ids, self.text_rows = list(task_ids), list(text_rows)
        nt = engine.cfg.multi_task
        if engine.cfg.is_multi:
            self.onehots = torch.eye(nt, dtype=F32, device=self.dev)[self.task_ids].contiguous()
        else:       # single-task model (is_multi False, TM:172-179): one pass, no task token; its [1, O] logits meet all 3 targets
            self.onehots = torch.zeros(1, 1, dtype=F32, device=self.dev)
        self.loss = torch.zeros(1, dtype=F32, device=self.dev)
        self.proj: Optional[Dict[str, torch.Tensor]] = None
        self.last_logits: Optional[torch.Tensor] = None
        # data-parallel reducer (buckets in the order the backward finalises them)
        nint = len(engine.cfg.interaction_indexes)
        self._nint = nint
        # (MT_DP_SHARD_LAST=0: the last bucket is all-reduced like the others instead of reduce-scattered -- the reducer's other form)
        self.reducer = dp.GradReducer(engine.store.flat_grad, dp.grad_buckets(engine.store.slots, nint, n), process_group,
                                      flat_param=engine.store.flat, shard_last=os.environ.get("MT_DP_SHARD_LAST", "1") != "0")
        engine.store.sync = self.reducer.wait_params      # state_dict() / a forward outside the step see complete parameters
        if self.max_grad_norm is not None:      # (allocated here: never inside a capture)
            self._sumsq = torch.zeros(len(self.reducer.norm_pieces(n)[0]), dtype=torch.float64, device=self.dev)
            self._sumsq_ws = torch.empty(ops.grad_sumsq_partials_elems(n), dtype=torch.float64, device=self.dev)
        if self.ema_decay is not None:      # (allocated here: never inside a capture; a fresh engine has no parameter gather in flight)
            self.ema = engine.store.flat.detach().clone()
            self._ema_seg = (torch.full((1,), n, dtype=torch.int32, device=self.dev), torch.zeros(1, dtype=torch.uint8, device=self.dev))
        self._gcache = GraphCache(graph_cache_size, capture_after)      # the captured bag geometries: key -> _Captured
        # Parameter groups: per-group lr multiplier and weight decay (optim.resolve_param_groups has the rule format).  The resolved
        # groups are STATE (host values, saved with a checkpoint); the device table mt_adamw_step_groups reads (segment ends and group
        # ids of the flat buffer, optim.segment_table) is derived from them and lives in two buffers sized once for the worst case (one
        # segment per tensor), so a change lands in place.  lr_mult / weight_decay are launch arguments, baked into a capture like
        # weight_decay always was: set_group() and a load that changes them drop the captures.  The learning rate stays the ONE device
        # scalar (set_lr): every group trains at lr x lr_mult.  None -- and rules that resolve to lr_mult 1 and one weight_decay
        # everywhere -- is the one mt_adamw_step launch per piece as ever.
        self._pgroups, self._group_of, self._seg_end, self._seg_group, self._nseg = None, None, None, None, 0
        if param_groups is not None:
            kinds = {k: kind for k, _, kind, train in engine.store.specs if train}
            self._set_groups(optim.resolve_param_groups([(k, kinds[k]) for k in engine.store.slots], param_groups, weight_decay)[0])
        self._opt_graph, self._opt_gen = None, -1      # world > 1: the optimiser's graph and the generation it was captured under
        self._cap, self._cap_buckets = None, []      # the graph_cache.Capture of a step in progress, the bucket behind each of its cuts
        self._static_key = None
        self.graph_replays = 0
        self.eager_steps = 0
        self.patch_size_lv0 = 1024          # TITAN configuration only (titan_adapter.py:335)
        # bench.py --gpus N: set to a list to collect, per step, HIP events around the two places a collective can be EXPOSED on the
        # compute stream -- ("grad", e0, e1): last backward kernel -> the optimiser may start (bucket all-reduces / the last bucket's
        # reduce-scatter not hidden under the backward); ("param", e0, e1): the next step's wait for the sharded parameter all-gather
        self.comm_events: Optional[list] = None
        # Measured rank imbalance (optional): a dp.StepTimer whose start() / stop() bracket every call's forward + backward -- two events
        # on the compute stream, the second ahead of the reducer wait, never inside a capture; nothing is read back before its report().
        self.step_timer: Optional["dp.StepTimer"] = None
        # The task passes of a step as TWO concurrent groups (B = 2 and B = 1 on two HIP streams) instead of one batched B = 3 pass
        # (pass_groups.py has the mechanics and the measurements).  The groups share the staged input and the patch embedding (computed
        # once before the fork).  The loss is a sum over the task rows (TM:225-233), so each group runs loss + backward behind its own
        # forward; the streams meet once, in front of the optimiser.  split_passes=False (or split_mode() "off"): the batched pass.
        B = int(self.onehots.shape[0])
        self.split_passes = bool(split_passes) and B >= 2 and pass_groups.split_mode() != "off"
        self._groups = pass_groups.group_bounds(B, singles=os.environ.get("MT_PASS_GROUPS") == "singles")      # (experiments: B streams)
        self._group_slots = pass_groups.group_slots(self._groups)
        self._pg = pass_groups.PassGroups(engine, tapes=True, tape_on_realloc=engine._bump_generation)      # (captured graphs point into the tapes' gradient arenas)
        self._loss_parts = None
        self._group_hook = None             # tests: called on the host after each group has been enqueued (throttles the interleaving)
        self.split_min_patches = pass_groups.SPLIT_MIN_PATCHES
        # ... but between ~4 000 and ~7 500 patches the winner changes with the tile rounding of every GEMM and attention launch (round 6,
        # same box, ms batched -> groups: 4 096: 18.37 -> 17.68; 5 500: 23.47 -> 23.11; 6 500: 26.44 -> 27.09; 7 000: 28.65 -> 28.61), so a
        # geometry that is about to be CAPTURED (it keeps coming back) is decided by measurement: both schedules run eagerly a few times
        # with update=False semantics (nothing but the dropout counter moves, and that is restored) and the faster one is captured.
        # Geometries that never repeat keep the threshold.  split_passes="auto" (the default) / True (threshold only) / False.
        # A deterministic engine (Engine(deterministic=True)) runs no trial: a schedule chosen by a stopwatch is not reproducible, and the
        # batched pass and the groups sum their gradients in different orders -- "auto" then means the threshold rule.
        self.deterministic = bool(getattr(engine, "deterministic", False))
        self.auto_split = split_passes == "auto" and pass_groups.split_mode() == "auto" and not self.deterministic
        self.split_decisions: Dict[int, bool] = {}
        self.split_trials: Dict[int, dict] = {}
        # Data-parallel schedule of a long bag (world > 1).  "groups_joined": the two pass groups with PER-BUCKET joins -- their backwards
        # run stage by stage (a stage = one interaction block); when both groups have left a block the main stream sums that bucket's
        # ranges of the two gradient sets and starts its all-reduce, the groups keep running below (DDP's overlap of the reduction with
        # the backward, base_trainer.py:205-211, under the two-stream schedule).  "groups_exposed": round 5's form -- every bucket starts
        # behind the groups' final join, the whole reduction is exposed in front of AdamW.  "batched": one B = 3 pass, buckets started
        # from inside its backward.  bench.py --gpus N times all three at start-up and keeps the fastest (`comm.schedule_chosen`).
        # MT_DP_SCHEDULE overrides; on one GPU "groups_joined" only matters when forced (what the extra joins cost: DESIGN section 6).
        self.dp_schedule = os.environ.get("MT_DP_SCHEDULE", "groups_joined")
        self.force_bucket_joins = os.environ.get("MT_BUCKET_JOINS") == "force"
        self.buckets_started_early = 0      # per step: buckets whose all-reduce was started before the last backward kernel was enqueued

    # ------------------------------------------------------------------ learning-rate schedule hook
    @property
    def lr(self) -> float:
        return self._lr

    @lr.setter
    def lr(self, value: float):
        self.set_lr(value)

    def set_lr(self, lr: float):
        """Scheduler hook: call once per epoch / step with the schedule's value (fill kernel, no host sync); eager steps
        and replays of already captured graphs both train with it from the next step on."""
        self._lr = float(lr)
        self.lr_dev.fill_(float(lr))

    # ------------------------------------------------------------------ parameter groups
    @property
    def param_groups(self):
        """The resolved groups, [{"names", "lr_mult", "weight_decay"}]: the default group (unmatched tensors) first when it has tensors,
        then the constructor's rules in order.  Without rules: the one group of all trainable tensors."""
        if self._pgroups is None:
            return [{"names": list(self.engine.store.slots), "lr_mult": 1.0, "weight_decay": float(self.wd)}]
        return [dict(g, names=list(g["names"])) for g in self._pgroups]

    @property
    def group_of(self) -> Dict[str, int]:
        """{tensor name: index into param_groups}."""
        return dict(self._group_of) if self._pgroups is not None else {k: 0 for k in self.engine.store.slots}

    def _grouped(self) -> bool:
        """The optimiser launch is mt_adamw_step_groups: some group has another lr_mult than 1 or another weight_decay than the rest."""
        gs = self._pgroups
        return gs is not None and not all(g["lr_mult"] == 1.0 and g["weight_decay"] == gs[0]["weight_decay"] for g in gs)

    def _baked_groups(self):
        """What a capture holds of the groups: which entry point, its values, the segment count (the table itself is read in place)."""
        return (tuple((g["lr_mult"], g["weight_decay"]) for g in self._pgroups), self._nseg) if self._grouped() else None

    def _drop_captures(self):
        self._gcache.clear()
        self._opt_graph = None

    def _set_groups(self, groups: Optional[Sequence[dict]]):
        """Install resolved groups ([{"names", "lr_mult", "weight_decay"}] covering every trainable tensor once, or None): the host list,
        the device table in place, self.wd when the groups are uniform; captures that hold other values are dropped."""
        slots = self.engine.store.slots
        was = self._baked_groups(), self.wd
        table_was = None if self._seg_end is None else (self._seg_end[:self._nseg].clone(), self._seg_group[:self._nseg].clone())
        if groups is None:
            self._pgroups, self._group_of = None, None
        else:
            groups = [{"names": list(g["names"]), "lr_mult": float(g["lr_mult"]), "weight_decay": float(g["weight_decay"])} for g in groups]
            group_of = {k: i for i, g in enumerate(groups) for k in g["names"]}
            if len(groups) > optim.MAX_GROUPS or sorted(k for g in groups for k in g["names"]) != sorted(slots):
                raise ValueError(f"param groups: {len(groups)} groups over {sum(len(g['names']) for g in groups)} tensors; at most "
                                 f"{optim.MAX_GROUPS} groups, and every one of the {len(slots)} trainable tensors in exactly one")
            end, grp = optim.segment_table([(o, n, group_of[k]) for k, (o, n, _) in slots.items()])
            if self._seg_end is None:      # (sized for one segment per tensor: later tables land in place)
                self._seg_end = torch.zeros(len(slots), dtype=torch.int32, device=self.dev)
                self._seg_group = torch.zeros(len(slots), dtype=torch.uint8, device=self.dev)
            self._nseg = int(end.numel())
            self._seg_end[:self._nseg].copy_(end)
            self._seg_group[:self._nseg].copy_(grp)
            self._pgroups, self._group_of = groups, group_of
            if not self._grouped():
                self.wd = groups[0]["weight_decay"]
        same_table = table_was is not None and self._pgroups is not None and table_was[0].numel() == self._nseg and \
            torch.equal(table_was[0], self._seg_end[:self._nseg]) and torch.equal(table_was[1], self._seg_group[:self._nseg])
        if was != (self._baked_groups(), self.wd) or (self._grouped() and not same_table):
            self._drop_captures()

    def set_group(self, index: int, lr_mult: Optional[float] = None, weight_decay: Optional[float] = None):
        """Change a group's lr multiplier and / or weight decay from the next step on (lr_mult = 0 with weight_decay = 0 holds its
        tensors still: the parameter bits do not move, the moments keep updating).  They are launch arguments: captures that hold the
        old values are dropped and the recurring geometries are captured again."""
        groups = self.param_groups
        g = groups[index]
        lm = g["lr_mult"] if lr_mult is None else float(lr_mult)
        wd = g["weight_decay"] if weight_decay is None else float(weight_decay)
        if not (lm >= 0.0 and wd >= 0.0):
            raise ValueError(f"set_group: lr_mult and weight_decay must be >= 0 (got {lm}, {wd})")
        g["lr_mult"], g["weight_decay"] = lm, wd
        self._set_groups(groups)

    # ------------------------------------------------------------------ EMA of the trainable weights
    def _not_averaged(self, what: str):
        """Inside ema_weights() the parameter buffer holds the average: nothing that trains, saves or loads may run there."""
        if getattr(self, "_ema_swapped", False):
            raise RuntimeError(f"{what} inside ema_weights(): the parameter buffer holds the averaged weights -- leave the context first")

    def _need_ema(self, what: str):
        if getattr(self, "ema", None) is None:
            raise RuntimeError(f"{what}: this TrainStep keeps no average (construct it with ema_decay=...)")

    def set_ema_decay(self, decay: float, warmup: Optional[bool] = None):
        """Change the EMA's decay (and warm-up flag) from the next step on.  Launch arguments: captures that hold the old values are
        dropped and the recurring geometries are captured again."""
        self._need_ema("set_ema_decay")
        decay = _valid_ema_decay(decay)
        if decay is None:
            raise ValueError("set_ema_decay: a decay in [0, 1) is expected (the average cannot be switched off after construction)")
        warmup = self.ema_warmup if warmup is None else bool(warmup)
        if (decay, warmup) != (self.ema_decay, self.ema_warmup):
            self.ema_decay, self.ema_warmup = decay, warmup
            self._drop_captures()

    def ema_reset(self):
        """The average starts again from the current parameters."""
        self._need_ema("ema_reset")
        self._not_averaged("ema_reset()")
        if self.engine.store.sync is not None:
            self.engine.store.sync()
        self.ema.copy_(self.engine.store.flat)

    def ema_state(self) -> Dict[str, torch.Tensor]:
        """{name: view into the average} under the reference's state_dict names, for load_state_dict(..., strict=False) into the module
        path or the reference.  Data parallel with a sharded last bucket: complete after state_dict() or inside / behind ema_weights()
        (they gather the shards); between steps a rank holds its own shard's average only."""
        self._need_ema("ema_state")
        return {k: self.ema[o:o + n].view(shape) for k, (o, n, shape) in self.engine.store.slots.items()}

    @contextlib.contextmanager
    def ema_weights(self):
        """Evaluate with the averaged weights: on entry the parameter buffer and the average are exchanged in place (mt_swap_f32) and the
        fp16 operand caches refreshed, on exit they are exchanged back and refreshed again.  No address changes, so captured graphs --
        an EmbeddingExtractor's included -- stay valid and simply see the average.  Data parallel: a COLLECTIVE on entry (the shards of
        the average are gathered), every rank enters at the same position.  Inside, step / step_graphed / finish_window / state_dict /
        load_state_dict raise; so do nesting and entering inside an open accumulation window."""
        self._need_ema("ema_weights")
        self._not_averaged("ema_weights()")
        if self.window_pos > 0:
            raise RuntimeError(f"ema_weights() inside an open accumulation window ({self.window_pos} of {self.accumulate} micro-steps): "
                               "call finish_window() first, or evaluate at a boundary")
        eng, store = self.engine, self.engine.store
        if store.sync is not None:
            store.sync()                          # a parameter gather in flight writes into the buffer about to be exchanged
        self.reducer.gather_shards_(self.ema)
        ops.swap_f32(store.flat, self.ema, store.n_flat)
        self._ema_swapped = True
        try:
            eng.refresh_trainable_caches()
            yield self
        finally:
            ops.swap_f32(store.flat, self.ema, store.n_flat)
            self._ema_swapped = False
            eng.refresh_trainable_caches()

    # frozen random text projector (train_modaltune.py:44-59,114-116)
    def set_projector(self, state: Dict[str, "np.ndarray | torch.Tensor"]):
        self.proj = {k: (torch.from_numpy(np.asarray(v)) if not torch.is_tensor(v) else v).to(self.dev, F32).contiguous()
                     for k, v in state.items()}

    def project_text(self, text: torch.Tensor) -> torch.Tensor:
        """Projection_layer + row L2 normalisation (TM:211-213); returns the 3 target rows [3, O] (unnormalised
        softmax inputs are the L2-normalised projections, as in the reference)."""
        p, tape = self.proj, self.engine.tape
        was = tape.grad_enabled
        tape.grad_enabled = False
        fr = lambda t: Param(t, None)
        x = Var(text.to(self.dev, F32).reshape(-1, text.shape[-1]).contiguous(), needs_grad=False)
        O = p["conv1.0.bias"].numel()
        h = tape.linear(x, fr(p["conv1.0.weight"].view(O, -1)), fr(p["conv1.0.bias"]))
        h = tape.layernorm(h, fr(p["conv1.1.weight"].view(-1)), fr(p["conv1.1.bias"].view(-1)))
        r = Var(tape.new(*h.data.shape))
        ops.act_fwd(h.data, r.data, ops.ACT_RELU)
        h = tape.linear(r, fr(p["conv1.3.weight"].view(O, -1)), fr(p["conv1.3.bias"]))
        out = tape.new(len(self.text_rows), O)
        ops_l2norm_rows(h.data, out, self.text_rows)
        tape.grad_enabled = was
        return out

    # ------------------------------------------------------------------ the step's two halves
    def _world(self) -> int:
        return self.reducer.world

    def _dp(self) -> bool:
        """Collectives are part of the step (world > 1, or dp.single_rank_rehearsal())."""
        return self.reducer.active

    def _on_grad_ready(self, block: int):
        """Engine callback from inside the backward: the gradients of interaction block `block` (and above) are final."""
        b = self._nint - 1 - block
        if self._cap is not None:
            self._segment_break(b)
        else:
            self.reducer.start(b)

    @property
    def _pass_streams(self):
        return self._pg.streams or None       # (None until the first step that ran as groups)

    def _group_workspaces(self, L: int, split: bool, first: int = 0):
        """The workspaces of a step over L patches (one per pass group, or the batched pass's) from group `first` on, grown to size."""
        shapes = list(zip([b - a for a, b in self._groups], self._group_slots)) if split else [(int(self.onehots.shape[0]), 0)]
        return [self.engine._workspace(nb, L, slot=sl) for nb, sl in shapes[first:]]

    def _can_split(self) -> bool:
        """The pass groups are possible at all for this engine: a multi-task model, no per-block taps.  TITAN configuration: possible
        (native backbone with its native embedding), parity-green -- and never a win: round 6, every geometry of the bench rotation
        tried both ways, ms per replayed step batched / groups: 2 516 tokens 8.03 / 9.05, 3 027: 9.40 / 10.20, 4 001: 12.42 / 13.27,
        4 589: 14.50 / 14.78, 5 491: 18.10 / 18.56, 6 061: 19.96 / 20.83 (twice the token-side launches for half-sized big kernels)
        -- so no trial is spent on it; only pass_groups.split_mode() "force" runs it."""
        eng = self.engine
        if not pass_groups.eligible(eng, len(self.onehots), None, 0, self.split_passes, min_passes=2):
            return False
        return bool(eng.PASS_GROUPS or (pass_groups.split_mode() == "force" and eng.replayable))

    def _split_now(self, L: Optional[int] = None) -> bool:
        """This step runs as pass groups: "force" wherever possible, else a trial's decision for L patches, else the threshold."""
        if not self._can_split() or (self._dp() and self.dp_schedule == "batched"):
            return False
        if L is None or pass_groups.split_mode() == "force":
            return True
        return self.split_decisions[L] if L in self.split_decisions else L >= self.split_min_patches

    def _fwd_bwd_split(self, x, coords, genes, text, clinical, staged_geometry=None, reduce: bool = True, zero: bool = True,
                       micro: bool = False):
        """_fwd_bwd with the task passes in two concurrent groups (see __init__).  zero False (a window's later micro-steps): the
        store's own set keeps what the window holds -- the extra sets are zeroed as ever and sum_sets adds them into it."""
        eng, pg, ngroups = self.engine, self._pg, len(self._groups)
        if self._loss_parts is None:
            pg.ensure(ngroups)
            self._loss_parts = [torch.zeros(1, dtype=F32, device=self.dev) for _ in self._groups]
        self._wait_params()
        eng.grad_ready_hook = None            # (world > 1: the buckets start behind the join, optimizer_step -> start_rest)
        if eng.stochastic:
            ops.rng_advance(eng.rng)
        target = self.project_text(text)
        if eng.store.sync is not None:
            eng.store.sync()
        if not eng._caches_ready:
            eng._build_caches()
        # task-independent, once in front of the fork: the upload (step_graphed has staged the slide into the first group's workspace)
        # and the patch embedding; TITAN configuration: gridding, token gather, patch-embedding MLP and the ALiBi distance table
        share, staged_rows = {}, None if staged_geometry is None else staged_geometry[1]
        L = eng.slide_prologue(x, coords, share, self._groups[0][1] - self._groups[0][0], staged_rows=staged_rows,
                               patch_size_lv0=self.patch_size_lv0)
        self._group_workspaces(L, True)
        R, O = target.shape
        logits_all = torch.empty(R, O, dtype=F32, device=self.dev)
        self.grad_scale.copy_(self.scale)
        pg.fork(ngroups)
        # per-bucket joins: the groups' backwards advance stage by stage so that a bucket's all-reduce starts as soon as BOTH groups
        # have left its interaction block (see __init__: dp_schedule)
        joined = ((self._dp() and self.dp_schedule == "groups_joined" and reduce) or self.force_bucket_joins) and not micro
        eng.record_markers = bool(joined)
        calls, summed = [], set()
        self.buckets_started_early = 0
        try:
            for gi, (a, b) in enumerate(self._groups):
                with pg.group(gi, zero="all" if zero else "extra"):
                    logits = eng.forward_slide(None, None, genes, self.onehots[a:b], staged_rows=L, patch_size_lv0=self.patch_size_lv0,
                                               need_grad=True, clinical=clinical, share=share, tape=pg.tapes[gi], site_group=gi + 1,
                                               ws_slot=self._group_slots[gi])
                    call = eng.last_call
                    dlogits = torch.empty_like(logits)
                    ops.distill_loss(logits, target[a:b], self._loss_parts[gi], dlogits, b - a, O, 1.0, self.scale)
                    if joined:
                        eng.backward_begin(dlogits, call)
                        calls.append(call)
                    else:
                        eng.backward(dlogits, call=call)
                    logits_all[a:b].copy_(logits)
                if self._group_hook is not None:
                    self._group_hook(gi)
            nint = self._nint
            for stage in range(nint + 1 if joined else 0):
                for gi, call in enumerate(calls):
                    with pg.group(gi, wait=False, bind=False):
                        blk = eng.backward_stage(call)
                        if blk != (nint - 1 - stage if stage < nint else None):
                            raise RuntimeError(f"pass group {gi}: backward stage {stage} ended at block marker {blk}")
                if stage == nint:
                    break
                # bucket `stage` (= the parameters of block nint - 1 - stage, and the head for stage 0) is final in every group's
                # set: sum its ranges on the main stream and start its all-reduce; the groups keep running their lower blocks
                pg.join()
                pg.sum_sets(self.reducer.buckets[stage])
                summed.add(stage)
                self.buckets_started_early += 1
                if self._cap is not None:
                    # under capture the graph is cut here (the collective is launched eagerly between two replays): a cut needs
                    # every forked stream back on the capture stream, so the groups re-fork behind it
                    self._segment_break(stage)
                    pg.fork(ngroups, wait_all=True)
                else:
                    self.reducer.start(stage)
        finally:
            eng.record_markers = False
            pg.join()
        # the streams have met: one gradient buffer, one loss (buckets summed at their own joins are left alone: their all-reduce
        # may be in flight)
        if summed:
            for b, bk in enumerate(self.reducer.buckets):
                if b not in summed:
                    pg.sum_sets(bk)
        else:
            pg.sum_sets()
        ops.axpy(self._loss_parts[0], self._loss_parts[1], 1.0, self.loss)
        for part in self._loss_parts[2:]:
            ops.axpy(self.loss, part, 1.0, self.loss)
        self.last_logits = logits_all

    def _fwd_bwd(self, x, coords, genes, text, clinical, staged_geometry=None, reduce: bool = True, zero: bool = True, micro: bool = False):
        """Forward, loss and backward of one slide.  zero: the flat gradient buffer is cleared first (False: a window's later
        micro-steps add to it); micro: a micro-step of an accumulation window -- like reduce False, and no bucket join either."""
        eng = self.engine
        Lnow = staged_geometry[1] if staged_geometry is not None else (x.reshape(-1, x.shape[-1]).shape[0] if torch.is_tensor(x) else None)
        if self._split_now(Lnow):
            return self._fwd_bwd_split(x, coords, genes, text, clinical, staged_geometry, reduce=reduce, zero=zero, micro=micro)
        self._wait_params()               # the all-gather of the last step's sharded parameter update (no-op otherwise)
        eng.grad_ready_hook = self._on_grad_ready if (reduce and self._dp()) else None
        if eng.stochastic:
            ops.rng_advance(eng.rng)          # a fresh set of dropout / DropPath masks per step
        target = self.project_text(text)
        if zero:
            eng.store.flat_grad.zero_()
        # (TITAN configuration: gridding + backbone embed first; staged: step_graphed has uploaded / gridded the slide)
        logits = eng.forward_slide(x, coords, genes, self.onehots, staged_rows=None if staged_geometry is None else staged_geometry[1],
                                   patch_size_lv0=self.patch_size_lv0, need_grad=True, clinical=clinical)
        self.last_logits = logits
        R, O = target.shape
        self.grad_scale.copy_(self.scale)
        if logits.shape[0] == R:
            dlogits = torch.empty_like(logits)
            ops.distill_loss(logits, target, self.loss, dlogits, R, O, 1.0, self.scale)
        else:       # single-task: nn.KLDivLoss broadcasts the one logits row over the R text rows (TM:225-233)
            rows = torch.empty(R, O, dtype=F32, device=self.dev)
            ops.copy_rows(logits, rows, R, O, smap=rowmap(1, 0, 0))
            drows = torch.empty_like(rows)
            ops.distill_loss(rows, target, self.loss, drows, R, O, 1.0, self.scale)
            dlogits = torch.empty(1, O, dtype=F32, device=self.dev)
            ops.copy_rows(drows[0:1], dlogits, 1, O)
            for r in range(1, R):
                ops.copy_rows(drows[r:r + 1], dlogits, 1, O, accumulate=True)
        try:
            eng.backward(dlogits)
        finally:
            eng.grad_ready_hook = None        # a later direct eng.forward / backward must not start stray collectives

    def _check_finite(self):
        """GradScaler's inf check over what this rank holds; with a sharded last bucket the flag is MAX-reduced so that every
        rank takes the same skip decision (a collective: never inside a captured graph)."""
        eng = self.engine
        if self.max_grad_norm is not None:
            # clipping: the sums of squares of what this rank holds stand in for the check; the slots of its shards are SUM-reduced
            # (as doubles) so that every rank forms the same coefficient -- both collectives outside any captured graph
            self.reducer.sync_sumsq_(self._grad_sumsq())
        else:
            ops.check_finite(eng.store.flat_grad, eng.store.n_flat, self.found_inf)
        self.reducer.sync_flag_(self.found_inf)

    def _grad_sumsq(self) -> torch.Tensor:
        """mt_grad_sumsq over every range this rank's optimiser step reads (reducer.norm_pieces: the shards' slots last), one slot
        each; found_inf is ORed on the way.  Returns the slots of the shards (empty without a sharded bucket)."""
        n = self.engine.store.n_flat
        pieces, shared = self.reducer.norm_pieces(n)
        g = self.engine.store.flat_grad
        for i, (o, k) in enumerate(pieces):
            ops.grad_sumsq(g[o:o + k], k, self._sumsq_ws, self._sumsq[i:i + 1], self.found_inf)
        return self._sumsq[shared:]

    def _adam_and_refresh(self, world: int, check: bool = True, micro_steps: Optional[int] = None):
        """Inf check (unless the caller ran it), clip coefficient, AdamW over the MEAN of the `micro_steps` (default: `accumulate`)
        slides of the window on every rank, scaler update, weight-cache refresh."""
        eng = self.engine
        n = eng.store.n_flat
        grad_mult = 1.0 / (world * (self.accumulate if micro_steps is None else micro_steps))
        clip = self.max_grad_norm is not None
        if check and clip:
            self._grad_sumsq()
        elif check:
            ops.check_finite(eng.store.flat_grad, n, self.found_inf)
        scale = self.scale
        if clip:
            ops.grad_clip_coef(self._sumsq, self._sumsq.numel(), grad_mult, self.scale, self.max_grad_norm, self.found_inf, self._clip_out)
            scale = self._clip_scale      # = scale / coef (scale itself, bit for bit, when nothing is clipped)
        p, g = eng.store.flat, eng.store.flat_grad
        grouped = self._grouped()
        hp = [(q["lr_mult"], q["weight_decay"]) for q in self._pgroups] if grouped else None
        ema = self.ema
        if ema is not None:      # the grouped kernel's EMA form; without groups: a one-segment table, the bits of mt_adamw_step
            seg_end, seg_group, nseg = (self._seg_end, self._seg_group, self._nseg) if grouped else (*self._ema_seg, 1)
            hp = hp if grouped else [(1.0, self.wd)]
        for o, k in self.reducer.adam_pieces(n):      # one launch, or: everything but the sharded bucket + this rank's shards
            if ema is not None:
                ops.adamw_step_groups_ema(p[o:o + k], g[o:o + k], self.m[o:o + k], self.v[o:o + k], k, o, seg_end, seg_group, hp, self._lr,
                                          self.betas[0], self.betas[1], self.eps, 0, ema[o:o + k], self.ema_decay, self.ema_warmup,
                                          scale=scale, found_inf=self.found_inf, grad_mult=grad_mult, step_dev=self.step_dev,
                                          lr_dev=self.lr_dev, nseg=nseg)
                continue
            if grouped:      # (the piece's absolute position picks its segments out of the one table)
                ops.adamw_step_groups(p[o:o + k], g[o:o + k], self.m[o:o + k], self.v[o:o + k], k, o, self._seg_end, self._seg_group, hp,
                                      self._lr, self.betas[0], self.betas[1], self.eps, 0, scale=scale, found_inf=self.found_inf,
                                      grad_mult=grad_mult, step_dev=self.step_dev, lr_dev=self.lr_dev, nseg=self._nseg)
                continue
            ops.adamw_step(p[o:o + k], g[o:o + k], self.m[o:o + k], self.v[o:o + k], k, self._lr, self.betas[0], self.betas[1], self.eps,
                           self.wd, 0, scale=scale, found_inf=self.found_inf, grad_mult=grad_mult, step_dev=self.step_dev,
                           lr_dev=self.lr_dev)
        ops.scaler_update(self.scale, self.tracker, self.found_inf, self.step_dev, 2.0, 0.5, self.growth_interval)
        eng.refresh_trainable_caches()

    def _mark(self):
        if self.comm_events is None or self._cap is not None:
            return None
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def _wait_params(self):
        e0 = self._mark() if self.reducer._param_pending else None
        self.reducer.wait_params()
        if e0 is not None:
            self.comm_events.append(("param", e0, self._mark()))

    def optimizer_step(self, micro_steps: Optional[int] = None):
        """Launch whatever buckets the backward has not started, wait for the collectives, AdamW + weight-cache refresh; with
        a sharded last bucket (world > 1) the updated shards are then all-gathered asynchronously (waited for at the top of the
        next step)."""
        e0 = self._mark()
        self.reducer.start_rest()
        world = self.reducer.wait()
        if self.reducer.sharded:
            self._check_finite()
        if e0 is not None:
            self.comm_events.append(("grad", e0, self._mark()))
        if self.reducer.sharded:
            self._adam_and_refresh(world, check=False, micro_steps=micro_steps)
            self.reducer.start_param_gather()
        else:
            self._adam_and_refresh(world, micro_steps=micro_steps)

    def _window_role(self):
        """(first, boundary) of the call about to run: first -- the window is empty, the gradient buffer is zeroed; boundary -- the
        call that completes the window and runs the optimiser.  accumulate == 1: (True, True) always."""
        return self.window_pos == 0, self.window_pos + 1 >= self.accumulate

    def step(self, x, coords, genes, text, update: bool = True, clinical=None) -> torch.Tensor:
        """One train step on one slide, eager launches.  Returns the (device) loss scalar; no host sync happens here.  With
        accumulate > 1 the call is a micro-step or the boundary of its window (see __init__); update=False (gradients only, nothing
        else moves) has no meaning inside a window and raises there."""
        self._not_averaged("step()")
        if self.accumulate > 1 and not update:
            raise ValueError("step(update=False) is not defined with accumulate > 1: micro-steps accumulate by themselves")
        first, boundary = self._window_role()
        timer = self.step_timer
        if timer is not None:
            timer.start()
        self._fwd_bwd(x, coords, genes, text, clinical, reduce=update and boundary, zero=first, micro=not boundary)
        if timer is not None:
            timer.stop()
        self.eager_steps += 1
        if not boundary:
            self.window_pos += 1
        elif update:
            self.optimizer_step()
            self.window_pos = 0
            self._after_boundary()
        return self.loss

    def finish_window(self):
        """Apply a partial window (an epoch ended inside it): the boundary's reduce, check, clip and AdamW over the MEAN of the
        micro-steps seen, eagerly.  A no-op on an empty window.  Data parallel: every rank calls it at the same position."""
        self._not_averaged("finish_window()")
        if self.window_pos == 0:
            return
        seen, self.window_pos = self.window_pos, 0
        self.optimizer_step(micro_steps=seen)
        self._after_boundary()

    # ------------------------------------------------------------------ hipGraph replay of the whole step
    def step_graphed(self, x, coords, genes, text, clinical=None) -> torch.Tensor:
        """Same arithmetic as step().  A bag geometry (patch count, gene count) that keeps coming back is captured into
        hipGraphs after `capture_after` eager visits and replayed from then on (the ~900 launches of a step become a few
        host calls); up to `graph_cache_size` geometries stay captured (LRU).  Inputs are uploaded into static buffers
        first.  With world_size > 1 the capture is cut where a gradient bucket becomes final: the reducer starts that
        bucket's all-reduce between two replays, and the optimiser graph runs after the wait."""
        self._not_averaged("step_graphed()")
        eng = self.engine
        if not eng._caches_ready:
            eng._build_caches()
        x = x.reshape(-1, x.shape[-1])
        L = x.shape[0]
        B = self.onehots.shape[0]
        gflat = flatten_genes(genes)
        skey = (int(gflat.numel()), tuple(text.shape))
        if self._static_key != skey:
            self._static_key = skey
            self._sgenes = torch.empty(int(gflat.numel()), dtype=F32, device=self.dev)     # one flat static buffer
            self._stext = torch.empty(tuple(text.shape), dtype=F32, device=self.dev)
            self._sclin = torch.empty(1, eng.cfg.clinfeat_dim, dtype=F32, device=self.dev) if eng.cfg.clinical else None
            self._gcache.clear()
        # All workspaces exist -- and have grown, which bumps eng.generation -- before anything is captured.  The engines differ in when
        # the row count Lv is known: the patch count, so the other groups' workspaces grow in front of the upload into the first one's;
        # or (TITAN configuration) the token count that the gridding kernels' one host read-back brings, so every workspace grows behind
        # it -- gridding and read-back run eagerly, the captured part starts at the token gather and is keyed on (patches, TOKENS).
        split = self._split_now(L)      # (ROWS_FROM_STAGING: forced or never, whatever the length)
        if not eng.ROWS_FROM_STAGING:
            self._group_workspaces(L, split, first=1)
        Lv = eng.stage_slide(x, coords, self.patch_size_lv0, B=self._groups[0][1] - self._groups[0][0] if split else B)
        self._group_workspaces(Lv, split)
        if self.auto_split and Lv not in self.split_decisions and B >= 3 and Lv >= 2048 and not self._dp() and self._can_split():
            # this geometry's schedule is still to be decided by a trial (below, on the visit that captures it): the workspaces of BOTH
            # schedules exist and have grown NOW, on an eager visit -- a growth bumps eng.generation and retires every capture
            self._group_workspaces(Lv, False)
            self._group_workspaces(Lv, True)
        self._wait_params()                       # last step's sharded parameter all-gather ran under the staging above
        self._sgenes.copy_(gflat, non_blocking=True)
        self._stext.copy_(text, non_blocking=True)
        if self._sclin is not None:
            self._sclin.copy_(clinical.reshape(1, -1), non_blocking=True)
        world, dp_on = self._world(), self._dp()
        cache, gen = self._gcache, eng.generation
        cache.sync(gen)                           # buffers the old captures point to are gone
        if self._opt_gen != gen:
            self._opt_graph = None
        # (the data-parallel schedule is part of the key: bench.py --gpus N times the three schedules one after the other)
        key = (L, Lv, world, bool(eng.stochastic), self.dp_schedule if dp_on else None, self.force_bucket_joins)
        first, boundary = self._window_role()
        if self.accumulate > 1:
            # the capture ROLE of the call is part of the key: a window's first call zeroes the gradient buffer, its later ones add to
            # it, only the boundary carries the reducer cuts and the optimiser -- a recurring geometry is captured once per role it is
            # met in (at most three: first, middle, boundary) and `graph_cache_size` counts (geometry, role) captures, not geometries.
            # accumulate == 1 has the one role, with or without clipping: the keys are what they were.
            key += ((first, boundary),)
        ent = cache.get(key)
        if (self.auto_split and not dp_on and first and Lv not in self.split_decisions and B >= 3 and Lv >= 2048 and self._can_split()
                and (ent is None or ent.segs is None) and cache.visits.get(key, 0) >= cache.capture_after
                and not torch.cuda.is_current_stream_capturing()):
            self._trial_split(x, coords, genes, text, clinical, Lv, key)     # (sets split_decisions[Lv]; training state untouched)
            return self.step_graphed(x, coords, genes, text, clinical=clinical)

        def fwd_bwd():
            self._fwd_bwd(None, None, self._sgenes, self._stext, self._sclin, staged_geometry=(B, Lv), reduce=boundary, zero=first,
                          micro=not boundary)

        next_pos = 0 if boundary else self.window_pos + 1      # (window_pos moves behind the work, as in step(): a call that raises leaves it)
        timer = self.step_timer
        if ent is None or ent.segs is None:
            if not cache.admit(key):              # eager visits (allocator, lazy kernel attributes, the tape's gradient arena
                if timer is not None:             # sized from the last step)
                    timer.start()
                fwd_bwd()
                if timer is not None:
                    timer.stop()
                self.eager_steps += 1
                if boundary:
                    self.optimizer_step()
                self.window_pos = next_pos
                if boundary:
                    self._after_boundary()
                return self.loss
            if ent is None:
                ent = _Captured(gen)
                cache.put(key, ent)               # (evicts BEFORE the capture: it may reuse the evicted graphs' blocks)
            self._capture(ent, fwd_bwd, world, boundary)
        if timer is not None:
            timer.start()
        for g, bucket in ent.segs:
            g.replay()
            if bucket is not None:
                self.reducer.start(bucket)
        if timer is not None:                     # (world == 1: the captured step holds the optimiser too)
            timer.stop()
        self.last_logits = ent.logits
        self.graph_replays += 1
        if dp_on and boundary:
            e0 = self._mark()
            self.reducer.start_rest()
            self.reducer.wait()
            if self.reducer.sharded:
                self._check_finite()
            if e0 is not None:
                self.comm_events.append(("grad", e0, self._mark()))
            self._opt_graph.replay()
            self.reducer.start_param_gather()
        self.window_pos = next_pos
        if boundary:
            self._after_boundary()
        return self.loss

    def _trial_split(self, x, coords, genes, text, clinical, L: int, key: tuple, reps: int = 3):
        """Decide the schedule of bag length L by timing what will actually run: the step captured both ways (batched / two pass groups)
        and each capture replayed `reps` times behind one untimed replay.  Eager timings do not rank the two (the groups' ~1 300 eager
        launches are partly host-bound: 18.8 / 19.0 ms eager against 18.4 / 17.7 replayed at L = 4 096).  The replays are real steps, so
        every piece of training state they touch -- weights, moments, step count, loss scale, dropout counter -- is saved in front and
        restored behind them (lr is irrelevant then); the winner's capture is kept for the step that follows.
        With accumulate > 1 the trial runs at a window's FIRST position only (the gradient buffer holds nothing the window needs) and
        times whole steps: `accumulate` is 1 while it runs, so every replay is a complete first-and-boundary step under the key
        without a role; window_pos is 0 before and after, and those captures are dropped (no window of k > 1 replays that role).  While
        it runs the LRU holds one entry more, so the throw-away capture evicts no live (geometry, role) capture.  The decision is for
        the geometry, but it reaches a role's capture only if that role is captured after the trial: a later position of the window
        that was captured earlier, under the threshold rule, keeps its schedule until its capture is retired -- a window may mix
        schedules as it may mix geometries, the gradients add up either way."""
        import time
        eng = self.engine
        saved = [(t, t.clone()) for t in (eng.store.flat, self.m, self.v, self.step_dev, self.scale, self.tracker, self.found_inf, eng.rng,
                                          self._clip_out) + (() if self.ema is None else (self.ema,))]
        was_auto, self.auto_split = self.auto_split, False
        timer, self.step_timer = self.step_timer, None      # (the trial's replays are not steps of the epoch)
        k_window = self.accumulate
        if k_window > 1:
            assert self.window_pos == 0
            self.accumulate, key = 1, key[:-1]
            self._gcache.size += 1
            self._gcache.visits[key] = max(self._gcache.visits.get(key, 0), self._gcache.capture_after)
        counters = (self.graph_replays, self.eager_steps, self._boundaries)
        res, caps = {}, {}
        try:
            for split in (False, True):
                self.split_decisions[L] = split
                self._gcache.pop(key)             # (same key for both schedules: capture afresh)
                for i in range(reps + 2):         # capture (visit counts are already past capture_after), one untimed replay, reps timed
                    if i == 2:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                    self.step_graphed(x, coords, genes, text, clinical=clinical)
                torch.cuda.synchronize()
                res["groups" if split else "batched"] = round(1e3 * (time.perf_counter() - t0) / reps, 3)
                caps[split] = self._gcache.get(key)
        finally:
            self.auto_split, self.accumulate, self.window_pos, self.step_timer = was_auto, k_window, 0, timer
            if k_window > 1:
                self._gcache.pop(key)
                self._gcache.size -= 1
            self.graph_replays, self.eager_steps, self._boundaries = counters
            for t, c in saved:
                t.copy_(c)
            eng.refresh_trainable_caches()
        win = res["groups"] < res["batched"]
        self.split_decisions[L] = win
        self.split_trials[L] = res
        if k_window == 1 and caps.get(win) is not None:
            self._gcache.put(key, caps[win])      # (if the generation moved while it was held outside, get() never returns it and the next sync drops it)

    @property
    def _graphs(self):
        """Captured segment lists of the cached geometries (None when nothing is captured yet)."""
        segs = [e.segs for e in self._gcache.entries.values() if e.segs is not None]
        return segs or None

    def _capture(self, ent: _Captured, fwd_bwd, world: int, boundary: bool = True):
        torch.cuda.synchronize()
        with self._gcache.capture() as cap:
            self._cap, self._cap_buckets = cap, []
            try:
                fwd_bwd()
                if boundary and not self._dp():
                    self.optimizer_step()
            finally:
                self._cap = None
        segs, logits = list(zip(cap.graphs, self._cap_buckets + [None])), self.last_logits
        if boundary and self._dp() and self._opt_graph is None:
            with self._gcache.capture() as cap:
                self._adam_and_refresh(world, check=not self.reducer.sharded)
            self._opt_graph, self._opt_gen = cap.graphs[0], ent.generation
        ent.segs, ent.logits = segs, logits

    def _segment_break(self, bucket: int):
        """Inside a capture with world_size > 1: close the current graph at a gradient-bucket boundary, open the next."""
        self._cap.cut()
        self._cap_buckets.append(bucket)

    # ------------------------------------------------------------------ replica canary
    def _checksum_into(self, t: torch.Tensor, out: torch.Tensor):
        """out[0] (device int64) = mt_checksum64 over the 32-bit words of `t`."""
        n = t.numel() * t.element_size() // 4
        need = ops.checksum64_partials_elems(n)
        if self._cs_ws is None or self._cs_ws.numel() < need:
            self._cs_ws = torch.empty(need, dtype=torch.int64, device=self.dev)
        ops.checksum64(t, n, self._cs_ws, out)

    def param_checksum(self) -> torch.Tensor:
        """The exact 64-bit checksum of the flat parameter buffer as a device int64[1] (the unsigned value's bits); formed by
        mt_checksum64 on the current stream behind a parameter all-gather in flight, nothing is read back."""
        self._wait_params()
        out = torch.empty(1, dtype=torch.int64, device=self.dev)
        self._checksum_into(self.engine.store.flat, out)
        return out

    def verify_replicas(self):
        """Replicated parameters must be bit-identical on every rank after every step: MIN- and MAX-reduce param_checksum() over the group
        (two 8-byte collectives, outside any graph), read both back, and raise RuntimeError("replicas diverged ...") on EVERY rank
        when they differ.  A collective: every rank calls it at the same position.  World size 1: returns at once."""
        if self._world() == 1:
            return
        import torch.distributed as dist
        lo = self.param_checksum()
        hi = lo.clone()
        self.reducer.collectives += 2
        dist.all_reduce(lo, op=dist.ReduceOp.MIN, group=self.pg)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX, group=self.pg)
        lo_v, hi_v = int(lo), int(hi)
        if lo_v != hi_v:
            raise RuntimeError(f"replicas diverged: the parameter checksums of the {self._world()} ranks span {lo_v & (2 ** 64 - 1):#018x} .. "
                               f"{hi_v & (2 ** 64 - 1):#018x} after {int(self.step_dev)} optimiser steps; rank {self.reducer.rank}")

    def _after_boundary(self):
        if self.verify_every > 0:
            self._boundaries += 1
            if self._boundaries % self.verify_every == 0:
                self.verify_replicas()

    # ------------------------------------------------------------------ checkpoint / resume (the format: checkpoint.py)
    def state_dict(self, include_frozen: bool = False) -> dict:
        """Everything a resume needs, as CPU tensors and plain Python values (checkpoint.py has the format): weights, AdamW moments and
        step count in torch.optim.AdamW.state_dict() format, the loss scaler in GradScaler.state_dict() format, the Philox state, the
        learning rate, an open accumulation window with its summed gradient, the pass-group decisions, and the checksums of the three
        flat buffers formed on the device.  Synchronises, as loss_value() does.  Data parallel: a COLLECTIVE -- every rank calls it at
        the same position, the moments of the sharded bucket are all-gathered from their owners, every rank returns the same complete
        dict (rank 0 writes it); inside an open window it raises there (micro-step gradients are rank-local): finish_window() first."""
        from . import _lib, checkpoint
        self._not_averaged("state_dict()")
        eng, store = self.engine, self.engine.store
        world = self._world()
        if world > 1 and self.window_pos > 0:
            raise RuntimeError(f"state_dict() inside an open accumulation window ({self.window_pos} of {self.accumulate} micro-steps) with "
                               f"world size {world}: the micro-step gradients are rank-local -- call finish_window() first, or save at a boundary")
        if store.sync is not None:
            store.sync()
        self.reducer.gather_shards_(self.m)
        self.reducer.gather_shards_(self.v)
        sealed = (store.flat, self.m, self.v)
        if self.ema is not None:      # (the average of the sharded bucket lives with its owners, like the moments)
            self.reducer.gather_shards_(self.ema)
            sealed += (self.ema,)
        sums = torch.empty(len(sealed), dtype=torch.int64, device=self.dev)
        for i, t in enumerate(sealed):
            self._checksum_into(t, sums[i:i + 1])
        sums = [checkpoint.as_unsigned(c) for c in sums.cpu().tolist()]
        names = list(store.slots)
        keys = list(store.tensors) if include_frozen else names
        window = None
        if self.window_pos > 0:
            window = {"pos": int(self.window_pos), "accumulate": int(self.accumulate), "grad_scale": float(self.grad_scale),
                      "grad": store.flat_grad.detach().cpu()}
        hyper = {"lr": self._lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.wd}
        extra = {}
        if self.ema is not None:      # ONE optional key (and its checksum): without an average the key set is what it always was
            extra["ema"] = checkpoint.pack_ema(self.ema, store.slots, self.ema_decay, self.ema_warmup)
        return {**extra, "format": checkpoint.FORMAT,
                "model": {k: store.tensors[k].detach().cpu().clone() for k in keys},
                "optimizer": checkpoint.pack_optimizer(self.m, self.v, int(self.step_dev), store.slots, names, hyper, groups=self._pgroups),
                "scaler": checkpoint.pack_scaler(float(self.scale), int(self.tracker), self.growth_interval),
                "rng": eng.rng.detach().cpu().clone(), "stochastic": bool(eng.stochastic), "lr": float(self._lr), "window": window,
                "schedule": {"split_decisions": {int(k): bool(v) for k, v in self.split_decisions.items()}},
                "checksums": {"flat": sums[0], "m": sums[1], "v": sums[2], **({"ema": sums[3]} if self.ema is not None else {})},
                "build_id": _lib.build_info()["build_id"], "world": int(world),
                "config": checkpoint.config_dict(eng.cfg, store.group_sizes)}

    def load_state_dict(self, sd: dict, verify: bool = True):
        """Resume from state_dict()'s dict -- or from one assembled from the module path, {"model": model.state_dict(), "optimizer":
        opt.state_dict(), "scaler": scaler.state_dict()} (then the Philox state stays, the window is empty and nothing is verified).
        Everything is checked first (format, key set, every shape against this engine's slots: ValueError / KeyError naming the tensor;
        a `stochastic` that differs from the engine's mode and an open window of another `accumulate`: ValueError); then the state is
        copied IN PLACE into the existing device tensors -- captured graphs stay valid, nothing is re-bound --, the slot padding of the
        moments is zeroed, the fp16 operand caches are refreshed (the frozen ones rebuilt only when a frozen tensor changed: that
        retires the captured graphs), and with `verify` the three checksums are recomputed on the device: RuntimeError naming the
        buffer on a mismatch.  A different build_id only warns: bit equality with the saved run is then not promised.  Data parallel:
        every rank loads the complete state (a rank never reads the moments outside its shard)."""
        import warnings
        from . import _lib, checkpoint
        self._not_averaged("load_state_dict()")
        eng, store = self.engine, self.engine.store
        full = checkpoint.check_format(sd)
        names = list(store.slots)
        checkpoint.check_model_shapes(sd["model"], {k: tuple(t.shape) for k, t in store.tensors.items()}, names)
        flat, m, v, step, hyper = checkpoint.flat_buffers(sd, store.slots, store.n_flat)
        scaler = checkpoint.unpack_scaler(sd["scaler"]) if len(sd["scaler"]) else None      # ({}: a disabled GradScaler -- the scaler stays)
        window = sd["window"] if full else None
        ema_in = checkpoint.unpack_ema(sd["ema"], store.slots, store.n_flat) if "ema" in sd else None      # (flat, decay, warm-up)
        if full and bool(sd["stochastic"]) != bool(eng.stochastic):
            raise ValueError(f"checkpoint: written with stochastic={bool(sd['stochastic'])}, this engine runs stochastic={bool(eng.stochastic)} "
                             "(Engine.set_stochastic): the Philox state would mean something else")
        if full and tuple(sd["rng"].shape) != tuple(eng.rng.shape):
            raise ValueError(f"checkpoint: rng has shape {tuple(sd['rng'].shape)}, this engine holds {tuple(eng.rng.shape)}")
        if window is not None:
            if int(window["accumulate"]) != self.accumulate:
                raise ValueError(f"checkpoint: saved inside an accumulation window of accumulate={int(window['accumulate'])} "
                                 f"({int(window['pos'])} micro-steps held), this step runs accumulate={self.accumulate}")
            if self._world() > 1:
                raise ValueError("checkpoint: saved inside an accumulation window; such a file resumes at world size 1 only")
            if tuple(window["grad"].shape) != (store.n_flat,) or not 0 < int(window["pos"]) < self.accumulate:
                raise ValueError(f"checkpoint: window.grad has shape {tuple(window['grad'].shape)} at position {int(window['pos'])}, this "
                                 f"engine's flat gradient holds {store.n_flat} elements")
        # ---- everything checked: from here on the state moves, in place
        if store.sync is not None:
            store.sync()
        store.flat.copy_(flat)
        frozen_changed = False
        for k, t in sd["model"].items():
            if k not in store.slots:
                src = t.detach().to(self.dev, F32)
                if not torch.equal(store.tensors[k], src):
                    store.tensors[k].copy_(src)
                    frozen_changed = True
        self.m.copy_(m)
        self.v.copy_(v)
        self.step_dev.fill_(int(step))
        if scaler is not None:
            self.scale.fill_(scaler[0])
            self.tracker.fill_(scaler[1])
        baked = (tuple(self.betas), self.eps, self.wd, self.growth_interval)
        self.betas, self.eps, self.wd = tuple(hyper["betas"]), hyper["eps"], hyper["weight_decay"]
        if scaler is not None:
            self.growth_interval = scaler[2]
        if baked != (tuple(self.betas), self.eps, self.wd, self.growth_interval):
            self._gcache.clear()          # (these are launch arguments: captured graphs carry the old values)
            self._opt_graph = None
        # the checkpoint's groups win over the constructor's, as its hyper-parameters do (a uniform checkpoint: no groups); the table
        # lands in place, captures are dropped when what they hold of the groups differs
        self._set_groups(hyper.get("groups"))
        # the average: the checkpoint's, with its decay and warm-up flag (they win like the hyper-parameters; captures that hold others
        # are dropped); a checkpoint without one starts the average at the loaded parameters; a step without one ignores it
        if self.ema is not None and ema_in is not None:
            self.ema.copy_(ema_in[0])      # (zero slot padding, like the moments)
            self.set_ema_decay(ema_in[1], ema_in[2])
        elif self.ema is not None:
            warnings.warn("checkpoint: no `ema` entry (written by a step without an average): the average starts at the loaded parameters")
            self.ema.copy_(store.flat)
        elif ema_in is not None:
            warnings.warn("checkpoint: its `ema` entry is ignored, this TrainStep keeps no average (ema_decay=None)")
        self.set_lr(sd["lr"] if full else hyper["lr"])
        self.found_inf.zero_()
        self.window_pos = 0
        if full:
            eng.rng.copy_(sd["rng"])
            self.split_decisions = {int(k): bool(b) for k, b in sd["schedule"]["split_decisions"].items()}
            if window is not None:
                store.flat_grad.copy_(window["grad"])
                self.grad_scale.fill_(float(window["grad_scale"]))
                self.window_pos = int(window["pos"])
        if frozen_changed or not eng._caches_ready:
            eng._build_caches()
        else:
            eng.refresh_trainable_caches()
        if full and verify:
            sealed = {"flat": store.flat, "m": self.m, "v": self.v}
            if self.ema is not None and ema_in is not None and "ema" in sd["checksums"]:
                sealed["ema"] = self.ema
            sums = torch.empty(len(sealed), dtype=torch.int64, device=self.dev)
            for i, t in enumerate(sealed.values()):
                self._checksum_into(t, sums[i:i + 1])
            for name, have in zip(sealed, sums.cpu().tolist()):
                have, want = checkpoint.as_unsigned(have), checkpoint.as_unsigned(sd["checksums"][name])
                if have != want:
                    raise RuntimeError(f"checkpoint: checksum of `{name}` on the device is {have:#018x} after the load, the checkpoint "
                                       f"records {want:#018x}")
        if full and sd["build_id"] != _lib.build_info()["build_id"]:
            warnings.warn(f"checkpoint written by build {str(sd['build_id'])[:12]}, this is build {_lib.build_info()['build_id'][:12]}: the "
                          "resumed run is not promised to continue with the saved run's bits")

    def loss_value(self) -> float:
        """The last step's loss on the host.  This is where the trainer synchronises anyway (`loss.item()`, TM:239), so the
        deferred input check (bad / non-finite coords binned on the device) is raised here too."""
        v = float(self.loss)
        self.engine.check_inputs()
        return v

    def unscaled_grads(self) -> Dict[str, torch.Tensor]:
        """The last step's gradients divided by the loss scale THEY carry (`grad_scale`) -- not by `scale`, which after an
        update=True step that backed off or grew is already the next step's.  After a skipped step they are not finite.
        With accumulate > 1 this is the SUM over the micro-steps the window holds so far (after a boundary: the whole window's sum,
        not its mean), and it is never clipped: max_grad_norm acts inside AdamW, the buffer keeps the raw gradient."""
        s = float(self.grad_scale)
        return {k: g / s for k, g in self.engine.store.grads.items()}


def _valid_ema_decay(decay) -> Optional[float]:
    """None (no average) or the decay as a float in [0, 1) -- mt_adamw_step_groups_ema's range; anything else: ValueError."""
    if decay is None:
        return None
    if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 <= float(decay) < 1.0:
        raise ValueError(f"ema_decay must be None or a number in [0, 1) (got {decay!r})")
    return float(decay)


def ops_l2norm_rows(h: torch.Tensor, out: torch.Tensor, rows: Sequence[int]):
    """out[i] = h[rows[i]] / ||h[rows[i]]||: R <= 4 rows of O = 256, one tiny launch per row."""
    O = h.shape[-1]
    for i, r in enumerate(rows):
        ops.l2norm_row(h[r], out[i], O)
