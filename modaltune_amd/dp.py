"""Data-parallel pieces of the hot path: slide sharding and the one gradient collective.

Host/torch.distributed logic only, so it is exercised on CPU with gloo (tests/test_dp_cpu.py) and runs unchanged
over RCCL on GPUs ("nccl" backend).  The reference's intent: torch DistributedSampler + DDP mean of the trainable
gradients (utils/base_trainer.py:192-211, 283-286, 483-484).

Ragged bags (opt-in): `plan_epoch` / `shard_indices(lengths=, window=)` deal bags of similar length to the ranks of one synchronous
step, `LengthWindowSampler` is the sampler over it, `StepCost` / `plan_stats` predict a plan's imbalance (tools/scale_model.py) and
`StepTimer` measures it.  All host logic: tests/test_length_sharding_cpu.py.
"""
from __future__ import annotations

import math
import os
from typing import List, Optional, Sequence

import torch
import torch.distributed as dist


def _epoch_order(n_items: int, world: int, epoch: int, seed: int, shuffle: bool, drop_last: bool):
    """The DistributedSampler list of one epoch -- seeded (seed + epoch) permutation, padded by wrap-around to a multiple of `world`
    (or truncated to one: drop_last) -- and the generator behind it (None without shuffle)."""
    g = None
    if shuffle:
        g = torch.Generator()
        g.manual_seed(seed + epoch)
        idx = torch.randperm(n_items, generator=g).tolist()
    else:
        idx = list(range(n_items))
    if drop_last and n_items % world:
        total = (n_items // world) * world
        idx = idx[:total]
    else:
        total = math.ceil(n_items / world) * world
        pad = total - len(idx)
        if pad:
            idx += (idx * math.ceil(pad / max(1, len(idx))))[:pad]
    return idx, g


class StepCost:
    """Predicted cost of one train step as a function of the bag length: linear interpolation through measured (rows, ms) points,
    clamped below the first point (a short bag pays the launch floor), extended along the last segment above the last one.  The
    committed default (`step_cost.json`: DESIGN §5's `sizes` line) holds SINGLE-GPU step times: what it predicts is the cost of one
    bag RELATIVE to another -- which is all the dealing and `plan_stats` use -- not the time of a data-parallel step."""

    _default: Optional["StepCost"] = None

    def __init__(self, points: Sequence[Sequence[float]]):
        pts = sorted((float(r), float(ms)) for r, ms in points)
        if len(pts) < 2:
            raise ValueError(f"StepCost needs at least two (rows, ms) points (got {len(pts)})")
        if any(a[0] == b[0] for a, b in zip(pts, pts[1:])):
            raise ValueError("StepCost: two points share one row count")
        self.points = pts

    @classmethod
    def from_measurements(cls, pairs: Sequence[Sequence[float]]) -> "StepCost":
        """From a user's own (rows, ms) timings, in any order (e.g. `bench.py --patches L` at a few lengths on the target box)."""
        return cls(pairs)

    @classmethod
    def default(cls) -> "StepCost":
        if cls._default is None:
            import json
            with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "step_cost.json")) as f:
                cls._default = cls(json.load(f)["points"])
        return cls._default

    def __call__(self, rows) -> float:
        p, x = self.points, float(rows)
        if x <= p[0][0]:
            return p[0][1]
        i = len(p) - 2
        while i > 0 and x < p[i][0]:
            i -= 1
        (x0, y0), (x1, y1) = p[i], p[i + 1]
        return y0 + (x - x0) * (y1 - y0) / (x1 - x0)


def _deal_greedy(run: List[List[int]], world: int, lengths, cost) -> List[List[int]]:
    """One accumulation run (the steps between two synchronisations): every step's longest member goes to the rank with the least
    accumulated cost so far, its second longest to the next, ...; ties by rank.  Returns the steps with their members in rank order."""
    load = [0.0] * world
    out = []
    for members in run:
        ranks = sorted(range(world), key=lambda r: (load[r], r))
        longest_first = sorted(members, key=lambda i: (lengths[i], i), reverse=True)
        row = [0] * world
        for r, i in zip(ranks, longest_first):
            row[r] = i
            load[r] += cost(lengths[i])
        out.append(row)
    return out


def plan_epoch(n_items: int, world: int, epoch: int = 0, seed: int = 0, shuffle: bool = True, drop_last: bool = False, *,
               lengths: Optional[Sequence[float]] = None, window: int = 1, accumulate: int = 1, cost=None,
               _deal: Optional[str] = None) -> List[List[int]]:
    """The whole epoch as a table [world][steps]: rank r runs plan[r][t] in step t.  A pure function of its arguments, so every rank
    computes the same table without communication.

    lengths None or window == 1: the DistributedSampler rule (`_epoch_order`, rank r takes every world-th entry from r).
    Otherwise the ranks of one step get bags of SIMILAR length -- a synchronous step costs what its slowest rank costs:
      1. the same seeded permutation and padding / truncation;
      2. cut into consecutive windows of world * window entries (the last may be shorter, still a multiple of world);
      3. inside a window sort stably by (lengths[i], i) and cut the sorted run into steps of `world` neighbours;
      4. permute the steps of the window with the same generator (shuffle=False: they stay in ascending order), so long and short
         steps stay interleaved over the epoch -- only the members of ONE step are correlated in length, and an index never leaves
         the window the seeded permutation put it in;
      5. deal each step to the ranks.  accumulate == 1: rotated by the global step number (no rank always gets the longest member).
         accumulate = a > 1 (TrainStep(accumulate=a): ranks meet at the window boundaries only): per run of `a` consecutive steps,
         `_deal_greedy` with `cost` (default StepCost.default()); the load starts at zero in every run.
    `lengths`: any per-item proxy that grows with the step cost (patch counts -- data.case_lengths --, token counts for TITAN).
    `_deal` ("rotate" / "greedy"): the dealing of step 5 whatever `accumulate` is (tests compare the two on one plan)."""
    if int(window) < 1 or int(accumulate) < 1:
        raise ValueError(f"window and accumulate must be >= 1 (got {window}, {accumulate})")
    if lengths is not None and len(lengths) != n_items:
        raise ValueError(f"lengths has {len(lengths)} entries for {n_items} items")
    window, accumulate = int(window), int(accumulate)
    idx, g = _epoch_order(n_items, world, epoch, seed, shuffle, drop_last)
    total = len(idx)
    if lengths is None or window == 1:
        return [idx[r:total:world] for r in range(world)]
    if window % accumulate:
        raise ValueError(f"window={window} is not a multiple of accumulate={accumulate}: an accumulation run would straddle two windows")
    deal = _deal or ("rotate" if accumulate == 1 else "greedy")
    if deal not in ("rotate", "greedy"):
        raise ValueError(f"_deal must be 'rotate' or 'greedy' (got {_deal!r})")
    if deal == "greedy" and cost is None:
        cost = StepCost.default()
    plan: List[List[int]] = [[] for _ in range(world)]
    t = 0                                    # global step number
    for w0 in range(0, total, world * window):
        run_sorted = sorted(idx[w0:w0 + world * window], key=lambda i: (lengths[i], i))
        steps = [run_sorted[s:s + world] for s in range(0, len(run_sorted), world)]
        if g is not None:
            steps = [steps[j] for j in torch.randperm(len(steps), generator=g).tolist()]
        if deal == "rotate":
            rows = [[members[(r + t + k) % world] for r in range(world)] for k, members in enumerate(steps)]
        else:                                # (window % accumulate == 0: a run never leaves its window; the epoch's last may be short)
            rows = [row for a0 in range(0, len(steps), accumulate) for row in _deal_greedy(steps[a0:a0 + accumulate], world, lengths, cost)]
        for row in rows:
            for r in range(world):
                plan[r].append(row[r])
        t += len(steps)
    return plan


def shard_indices(n_items: int, world: int, rank: int, epoch: int = 0, seed: int = 0, shuffle: bool = True,
                  drop_last: bool = False, *, lengths: Optional[Sequence[float]] = None, window: int = 1, accumulate: int = 1,
                  cost=None, _deal: Optional[str] = None) -> List[int]:
    """torch.utils.data.DistributedSampler rule: seeded (seed + epoch) permutation, padded by wrap-around to a
    multiple of `world`, rank r takes every world-th index starting at r.  With `lengths` and `window` > 1: row `rank` of
    `plan_epoch` -- the same multiset of indices over the ranks, dealt so that the ranks of one step get bags of similar length."""
    return plan_epoch(n_items, world, epoch, seed, shuffle, drop_last, lengths=lengths, window=window, accumulate=accumulate,
                      cost=cost, _deal=_deal)[rank]


def _imbalance(costs: Sequence[Sequence[float]], accumulate: int = 1) -> dict:
    """costs[rank][step] -> {"efficiency", "gap", "steps"}: the ranks synchronise after every `accumulate` steps, so a run costs its
    slowest rank's sum.  efficiency = sum of the runs' mean / sum of their max (1: nobody ever waits); gap = mean over the runs of
    max - mean (what the average rank idles per synchronisation, in the cost's unit); steps = number of runs."""
    if int(accumulate) < 1:
        raise ValueError(f"accumulate must be >= 1 (got {accumulate})")
    world, n = len(costs), len(costs[0]) if costs else 0
    if any(len(c) != n for c in costs):
        raise ValueError("every rank must have the same number of steps")
    sum_mean = sum_max = 0.0
    runs = 0
    for a0 in range(0, n, int(accumulate)):
        per_rank = [sum(c[a0:a0 + accumulate]) for c in costs]
        sum_mean += sum(per_rank) / world
        sum_max += max(per_rank)
        runs += 1
    return {"efficiency": sum_mean / sum_max if sum_max > 0 else 1.0, "gap": (sum_max - sum_mean) / runs if runs else 0.0, "steps": runs}


def plan_stats(plan: Sequence[Sequence[int]], lengths: Sequence[float], cost=None, accumulate: int = 1) -> dict:
    """PREDICTED imbalance of a plan under `cost` (default StepCost.default()): see `_imbalance`."""
    cost = cost or StepCost.default()
    return _imbalance([[cost(lengths[i]) for i in row] for row in plan], accumulate)


class LengthWindowSampler(torch.utils.data.Sampler):
    """torch.utils.data.DistributedSampler's surface (dataset, num_replicas / rank from the process group, shuffle, seed, drop_last,
    set_epoch, __len__) over `shard_indices`, with its keywords lengths / window / accumulate / cost: the drop-in for the sampler line
    of the reference trainer (utils/base_trainer.py:283-286).  Without `lengths`, or with window == 1, it yields what
    DistributedSampler yields."""

    def __init__(self, dataset, num_replicas: Optional[int] = None, rank: Optional[int] = None, shuffle: bool = True, seed: int = 0,
                 drop_last: bool = False, *, lengths: Optional[Sequence[float]] = None, window: int = 1, accumulate: int = 1, cost=None):
        if num_replicas is None or rank is None:
            if not (dist.is_available() and dist.is_initialized()):
                raise RuntimeError("LengthWindowSampler: num_replicas / rank default from the process group, and none is initialised")
            num_replicas = dist.get_world_size() if num_replicas is None else num_replicas
            rank = dist.get_rank() if rank is None else rank
        if not 0 <= rank < num_replicas:
            raise ValueError(f"rank {rank} is outside [0, {num_replicas - 1}]")
        self.dataset, self.num_replicas, self.rank = dataset, int(num_replicas), int(rank)
        self.shuffle, self.seed, self.drop_last, self.epoch = bool(shuffle), int(seed), bool(drop_last), 0
        self.lengths = None if lengths is None else list(lengths)
        self.window, self.accumulate, self.cost = int(window), int(accumulate), cost
        n = len(dataset)
        self.num_samples = n // self.num_replicas if (drop_last and n % self.num_replicas) else math.ceil(n / self.num_replicas)
        self.total_size = self.num_samples * self.num_replicas
        self._indices()                      # (bad arguments raise here, not in the first epoch)

    def _indices(self) -> List[int]:
        return shard_indices(len(self.dataset), self.num_replicas, self.rank, self.epoch, self.seed, self.shuffle, self.drop_last,
                             lengths=self.lengths, window=self.window, accumulate=self.accumulate, cost=self.cost)

    def __iter__(self):
        return iter(self._indices())

    def __len__(self) -> int:
        return self.num_samples

    def set_epoch(self, epoch: int):
        self.epoch = int(epoch)


class StepTimer:
    """MEASURED imbalance of a data-parallel epoch (optional: `TrainStep.step_timer = StepTimer()`).  TrainStep brackets every call's
    forward + backward with start() / stop() ahead of the reducer wait: two events on the current stream, nothing is read back inside
    the step.  report() at the epoch's end reads the elapsed times, all_gather_object()s them and returns `plan_stats`' dict over the
    measured milliseconds plus "times" ([world][steps]); it starts the next epoch empty.  Ranks that SHARE one GPU time each other's
    kernels too: such numbers mean nothing."""

    def __init__(self, group=None):
        self.group = group
        self.pairs: list = []
        self._open = None

    @staticmethod
    def _mark():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def start(self):
        self._open = self._mark()

    def stop(self):
        if self._open is not None:
            self.pairs.append((self._open, self._mark()))
            self._open = None

    def report(self, accumulate: int = 1) -> dict:
        """A collective with world > 1: every rank calls it at the same position, with the same number of timed steps."""
        if self.pairs:
            self.pairs[-1][1].synchronize()
        mine = [float(a.elapsed_time(b)) for a, b in self.pairs]
        self.pairs = []
        times = [mine]
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(self.group) > 1:
            times = [None] * dist.get_world_size(self.group)
            dist.all_gather_object(times, mine, group=self.group)
        out = _imbalance(times, accumulate)
        out["times"] = times
        return out


def single_rank_rehearsal() -> bool:
    """MT_DP_REHEARSE=1: with an initialised process group of ONE rank, issue every collective of the data-parallel step anyway (a
    one-rank RCCL communicator runs them as copies): the only way to execute the `nccl` branches -- asynchronous all-reduce per
    bucket, reduce-scatter / all-gather of the sharded bucket, the flag MAX, the constructor broadcast -- on a one-GPU box."""
    return os.environ.get("MT_DP_REHEARSE") == "1" and dist.is_available() and dist.is_initialized()


def allreduce_sum_(flat: torch.Tensor, group=None) -> int:
    """In-place SUM all-reduce of the flat gradient buffer; returns the world size (the mean is folded into the AdamW
    kernel as grad_mult = 1/world).  No-op without an initialised process group."""
    if not (dist.is_available() and dist.is_initialized()):
        return 1
    world = dist.get_world_size(group)
    if world > 1 or single_rank_rehearsal():
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
    return world


def broadcast_params_(flat: torch.Tensor, src: int = 0, group=None):
    """DDP's constructor broadcast: every rank starts from rank `src`'s trainable parameters."""
    if dist.is_available() and dist.is_initialized() and (dist.get_world_size(group) > 1 or single_rank_rehearsal()):
        dist.broadcast(flat, src=src, group=group)


# ------------------------------------------------------------------------------------------------
# Bucketed gradient all-reduce, started while the backward still runs (the reference wraps the model in
# DistributedDataParallel, whose reducer does the same per 25 MB bucket: utils/base_trainer.py:205-211).
#
# The backward of the hot path finalises parameter gradients in a fixed order: fusion head and interaction block 2
# first, then block 1, block 0, and last the gene encoder / gene_pe / task tokens (the gene tokens feed every block, so
# their gradient closes only at the very end).  The flat gradient buffer is in state_dict order, so each of these
# stages is a handful of contiguous ranges.
# ------------------------------------------------------------------------------------------------
def _merge_ranges(slots: Sequence[tuple]) -> List[tuple]:
    """[(offset, numel)] of 16-byte aligned slots -> maximal contiguous (offset, length) ranges."""
    out: List[list] = []
    for off, n in sorted(slots):
        n_al = (n + 3) // 4 * 4
        if out and out[-1][0] + out[-1][1] == off:
            out[-1][1] += n_al
        else:
            out.append([off, n_al])
    return [(a, b) for a, b in out]


def grad_buckets(slots: dict, n_interactions: int, n_flat: int) -> List[List[tuple]]:
    """Bucket b (b = 0 .. n_interactions) = ranges of the flat gradient buffer that are final when the backward has
    left interaction block n_interactions - 1 - b; the last bucket (everything else: gene encoder, gene_pe, task /
    clinical tokens) closes with the backward itself.  `slots`: ParamStore.slots (key -> (offset, numel, shape))."""
    stage_of = {}
    last = n_interactions
    for k in slots:
        st = last
        if k.startswith("interactions.") or k.startswith("prompt_selfattention."):
            st = n_interactions - 1 - int(k.split(".")[1])
        elif k.startswith("final_norm.") or k.startswith("final_project."):
            st = 0
        stage_of[k] = st
    buckets = []
    for b in range(last + 1):
        buckets.append(_merge_ranges([(slots[k][0], slots[k][1]) for k in slots if stage_of[k] == b]))
    covered = sum(n for bk in buckets for _, n in bk)
    if covered != n_flat:
        raise AssertionError(f"gradient buckets cover {covered} of {n_flat} elements")
    return buckets


class GradReducer:
    """start(b): launch the collective of bucket b's ranges (asynchronous: RCCL runs it on its own stream behind everything
    enqueued so far on the current stream); wait(): make the current stream wait for every collective in flight.  These are
    the `mt_grad_allreduce_start / _wait` of SURVEY §8b; they live above the C ABI because the communicator belongs to
    torch.distributed ("nccl" = RCCL over xGMI on the GPUs, gloo in the rehearsals).

    Buckets 0 .. last-1 are SUM all-reduced.  The LAST bucket (gene encoder + token parameters: 3 MB with toy pathways, 100 MB
    with the reference's 331) closes with the backward itself, so nothing can hide it; with `flat_param` given it is SHARDED
    instead (reduce-scatter + all-gather as separate exchanges): reduce-scatter of the gradients -> every rank runs
    AdamW on its 1/W of the bucket (`adam_pieces`) -> all-gather of the updated PARAMETERS (`start_param_gather`, waited for at
    the top of the next step by `wait_params`, i.e. under the next slide's input staging).  What is exposed in front of AdamW is
    the reduce-scatter alone -- half the bytes of the all-reduce -- and the optimiser touches 1/W of the bucket."""

    def __init__(self, flat_grad: torch.Tensor, buckets: List[List[tuple]], group=None, flat_param: Optional[torch.Tensor] = None,
                 shard_last: bool = True):
        self.flat, self.buckets, self.group = flat_grad, buckets, group
        self.world = dist.get_world_size(group) if (dist.is_available() and dist.is_initialized()) else 1
        # `active`: collectives are issued (world > 1, or the one-rank rehearsal); `world` stays the arithmetic world size (1 / world)
        self.active = self.world > 1 or single_rank_rehearsal()
        self.rank = dist.get_rank(group) if self.active else 0
        self.views = [[flat_grad[o:o + n] for o, n in bk] for bk in buckets]
        self.pending: list = []
        self.started: set = set()
        self.collectives = 0                  # collectives issued so far (a micro-step of an accumulation window issues none)
        self.param = flat_param
        self.sharded = bool(self.active and shard_last and flat_param is not None and len(buckets) > 0)
        self._param_pending: list = []
        self._rs: list = []                   # (range offset, elements per rank, reduce-scatter output buffer)
        self._tails: list = []                # (offset, length) of the few elements past W * s of a range: plain all-reduce
        if self.sharded:
            W = self.world
            for o, n in buckets[-1]:
                s = (n // (4 * W)) * 4        # elements per rank: 16-byte aligned shards, [o, o + W s) is reduce-scattered
                if s > 0:
                    self._rs.append((o, s, torch.empty(s, dtype=flat_grad.dtype, device=flat_grad.device)))
                if n - W * s > 0:
                    self._tails.append((o + W * s, n - W * s))
        self._host = self.active and dist.get_backend(group) == "gloo"      # rehearsal backend: RS / AG through host copies

    # -- gradient side
    def start(self, b: int):
        if not self.active or b in self.started:
            return
        self.started.add(b)
        if self.sharded and b == len(self.buckets) - 1:
            for o, s, out in self._rs:
                src = self.flat[o:o + self.world * s]
                self.collectives += 1
                if self._host:
                    h = torch.empty(s, dtype=src.dtype)
                    dist.reduce_scatter_tensor(h, src.cpu(), op=dist.ReduceOp.SUM, group=self.group)
                    out.copy_(h)
                else:
                    self.pending.append(dist.reduce_scatter_tensor(out, src, op=dist.ReduceOp.SUM, group=self.group, async_op=True))
            for o, n in self._tails:
                self.collectives += 1
                self.pending.append(dist.all_reduce(self.flat[o:o + n], op=dist.ReduceOp.SUM, group=self.group, async_op=True))
            return
        for v in self.views[b]:
            self.collectives += 1
            self.pending.append(dist.all_reduce(v, op=dist.ReduceOp.SUM, group=self.group, async_op=True))

    def start_rest(self):
        for b in range(len(self.buckets)):
            self.start(b)

    def wait(self) -> int:
        """Returns the world size (the mean is folded into AdamW as grad_mult = 1 / world).  Sharded: this rank's slice of the
        last bucket now holds the summed gradient (the other slices keep their local values and are not read)."""
        for w in self.pending:
            w.wait()
        self.pending.clear()
        if self.sharded and (len(self.buckets) - 1) in self.started:
            for o, s, out in self._rs:
                self.flat[o + self.rank * s:o + (self.rank + 1) * s].copy_(out)
        self.started.clear()
        return self.world

    def sync_flag_(self, flag: torch.Tensor):
        """found_inf must be the same on every rank (GradScaler skips the WHOLE step): with a sharded bucket a rank only sees
        its own slice of the sums, so the flags are MAX-reduced (4 bytes)."""
        if self.sharded:
            self.collectives += 1
            dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=self.group)

    def sync_sumsq_(self, shard_sums: torch.Tensor):
        """Global-norm clipping with a sharded bucket: a rank holds the reduced gradient of its own shards only, so the float64
        sums of squares over them (the trailing slots of `norm_pieces`) are SUM-reduced; the slots of everything else were formed from
        all-reduced gradients and are equal on every rank already.  Every rank then adds the same slots in the same order: one
        coefficient, bit for bit.  A collective: beside sync_flag_, never inside a captured graph."""
        if self.sharded and shard_sums.numel():
            self.collectives += 1
            dist.all_reduce(shard_sums, op=dist.ReduceOp.SUM, group=self.group)

    def norm_pieces(self, n_flat: int):
        """(`adam_pieces` reordered -- the ranges every rank holds reduced first, this rank's shards last --, number of the former)."""
        pieces = self.adam_pieces(n_flat)
        mine = {(o + self.rank * s, s) for o, s, _ in self._rs} if self.sharded else set()
        shared = [p for p in pieces if p not in mine]
        return shared + [p for p in pieces if p in mine], len(shared)

    def adam_pieces(self, n_flat: int) -> List[tuple]:
        """(offset, length) ranges of the flat buffers THIS rank's optimiser step updates: everything outside the sharded
        bucket, the tails, and its own shard of every reduce-scattered range."""
        if not self.sharded:
            return [(0, n_flat)]
        skip = sorted((o, o + self.world * s, s) for o, s, _ in self._rs)
        out, cur = [], 0
        for a, b, s in skip:
            if a > cur:
                out.append((cur, a - cur))
            out.append((a + self.rank * s, s))
            cur = b
        if cur < n_flat:
            out.append((cur, n_flat - cur))
        return out

    # -- parameter side (sharded bucket only)
    def start_param_gather(self):
        """After the optimiser step: every rank's updated shard -> all ranks (asynchronous)."""
        if not self.sharded:
            return
        W, r = self.world, self.rank
        for o, s, _ in self._rs:
            self.collectives += 1
            full = self.param[o:o + W * s]
            mine = self.param[o + r * s:o + (r + 1) * s]
            if self._host:
                h = torch.empty(W * s, dtype=full.dtype)
                dist.all_gather_into_tensor(h, mine.cpu(), group=self.group)
                full.copy_(h)
            else:       # gathered into a staging buffer (no aliasing of a collective's input and output), copied back in wait_params
                stage = torch.empty(W * s, dtype=full.dtype, device=full.device)
                work = dist.all_gather_into_tensor(stage, mine.clone(), group=self.group, async_op=True)
                self._param_pending.append((work, full, stage))

    def gather_shards_(self, buf: torch.Tensor):
        """Checkpointing (TrainStep.state_dict): a flat buffer laid out like the parameters of which every rank holds valid values for its
        own shard of each reduce-scattered range only (the AdamW moments) -> complete on every rank, in place and synchronously.  A
        collective; a no-op without a sharded bucket."""
        if not self.sharded:
            return
        W, r = self.world, self.rank
        for o, s, _ in self._rs:
            self.collectives += 1
            full, mine = buf[o:o + W * s], buf[o + r * s:o + (r + 1) * s]
            if self._host:
                h = torch.empty(W * s, dtype=full.dtype)
                dist.all_gather_into_tensor(h, mine.cpu(), group=self.group)
                full.copy_(h)
            else:
                stage = torch.empty(W * s, dtype=full.dtype, device=full.device)
                dist.all_gather_into_tensor(stage, mine.clone(), group=self.group)
                full.copy_(stage)

    def wait_params(self):
        for work, full, stage in self._param_pending:
            work.wait()
            full.copy_(stage)
        self._param_pending.clear()
