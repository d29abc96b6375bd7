"""CPU: length-aware data-parallel sharding (dp.plan_epoch / shard_indices(lengths=, window=, accumulate=), dp.StepCost, dp.plan_stats,
dp.LengthWindowSampler, data.case_lengths, tools/scale_model.py).

The plan is a pure function, so everything about it is checked here: the defaults are the DistributedSampler rule, the windowed plan
covers the same multiset, the members of a step are neighbours in their window's (length, index) order, and -- conditions on a stated
synthetic cohort, not measurements -- the predicted imbalance falls by the factors below."""
import math
import os
import socket
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from torch.utils.data import DistributedSampler

from modaltune_amd import data, dp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS, WORLDS = (1, 5, 11, 64), (1, 2, 3, 8)


def _lengths(n, seed=0, spike=False):
    """min(25000, floor(exp(U(ln 300, ln 60000)))); spike: every third entry at the 25 000 cap as well."""
    u = np.random.default_rng(seed).uniform(math.log(300), math.log(60000), n)
    out = [int(min(25000, math.floor(math.exp(v)))) for v in u]
    if spike:
        out = [25000 if i % 3 == 0 else v for i, v in enumerate(out)]
    return out


# ------------------------------------------------------------------------------------------------ defaults unchanged
@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("shuffle", [False, True])
def test_defaults_are_the_distributed_sampler_rule(shuffle, drop_last):
    for n in NS:
        L = _lengths(n, seed=n)
        for W in WORLDS:
            for epoch in (0, 3):
                for r in range(W):
                    samp = DistributedSampler(list(range(n)), num_replicas=W, rank=r, shuffle=shuffle, seed=7, drop_last=drop_last)
                    samp.set_epoch(epoch)
                    want = list(samp)
                    kw = dict(epoch=epoch, seed=7, shuffle=shuffle, drop_last=drop_last)
                    assert dp.shard_indices(n, W, r, **kw) == want, (n, W, r)
                    assert dp.shard_indices(n, W, r, lengths=L, window=1, **kw) == want, (n, W, r)
                    assert dp.shard_indices(n, W, r, lengths=None, window=8, **kw) == want, (n, W, r)
                    assert len(want) == len(samp)


# ------------------------------------------------------------------------------------------------ cover
COVER = [(n, W, window, acc) for n in (5, 11, 64, 200) for W in (2, 3, 8) for window, acc in ((2, 1), (8, 1), (4, 2), (8, 4))]


@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("n,W,window,acc", COVER)
def test_the_windowed_plan_covers_what_the_plain_rule_covers(n, W, window, acc, drop_last):
    L = _lengths(n, seed=n + W)
    kw = dict(epoch=2, seed=5, drop_last=drop_last)
    plain = dp.plan_epoch(n, W, **kw)
    plan = dp.plan_epoch(n, W, lengths=L, window=window, accumulate=acc, **kw)
    assert Counter(i for row in plan for i in row) == Counter(i for row in plain for i in row)      # padding duplicates included
    assert len(plan) == W and len({len(row) for row in plan}) == 1 and len(plan[0]) == len(plain[0])
    for r in range(W):
        assert plan[r] == dp.shard_indices(n, W, r, lengths=L, window=window, accumulate=acc, **kw)
    assert plan == dp.plan_epoch(n, W, lengths=L, window=window, accumulate=acc, **kw)              # a pure function
    if len(plan[0]) * W >= 8:        # (an epoch of one or two steps may repeat itself)
        assert plan != dp.plan_epoch(n, W, lengths=L, window=window, accumulate=acc, **dict(kw, epoch=3))
    if n >= 64 and not drop_last:
        assert plan != plain                                                                        # (the feature did something)


def _windows_of(plan, W, window):
    """The plan's steps ([members in rank order]) grouped by window."""
    steps = [[plan[r][t] for r in range(W)] for t in range(len(plan[0]))]
    return [steps[s:s + window] for s in range(0, len(steps), window)]


def _check_neighbours(plan, plain, L, W, window):
    """Every window keeps the entries the seeded, padded permutation gave it, and every step is W consecutive entries of the window's
    (length, index) order (the epoch's last, shorter window included)."""
    order = [plain[t % W][t // W] for t in range(len(plain[0]) * W)]
    for k, steps in enumerate(_windows_of(plan, W, window)):
        span = order[k * W * window:(k + 1) * W * window]
        assert Counter(i for s in steps for i in s) == Counter(span)
        ranked = sorted(span, key=lambda i: (L[i], i))
        for members in steps:
            m = sorted(members, key=lambda i: (L[i], i))
            assert any(ranked[p:p + W] == m for p in range(0, len(ranked), W)), (k, members)


@pytest.mark.parametrize("n,W,window,acc", COVER)
def test_the_members_of_a_step_are_neighbours_in_their_window(n, W, window, acc):
    L = _lengths(n, seed=n)
    plan = dp.plan_epoch(n, W, epoch=1, seed=3, lengths=L, window=window, accumulate=acc)
    _check_neighbours(plan, dp.plan_epoch(n, W, epoch=1, seed=3), L, W, window)


def test_no_rank_always_gets_the_longest_member():
    n, W = 256, 4
    L = _lengths(n, seed=9)
    plan = dp.plan_epoch(n, W, seed=1, lengths=L, window=8)
    longest = Counter(max(range(W), key=lambda r: (L[plan[r][t]], plan[r][t])) for t in range(len(plan[0])))
    assert all(longest[r] == len(plan[0]) // W for r in range(W)), longest                          # rotation: exactly a W-th each


def test_ties_at_the_threshold_spike_are_deterministic_and_cover():
    n, W = 90, 4
    L = _lengths(n, seed=4, spike=True)
    assert sum(v == 25000 for v in L) >= n // 3
    for acc, window in ((1, 8), (4, 8)):
        a = dp.plan_epoch(n, W, seed=2, lengths=L, window=window, accumulate=acc)
        assert a == dp.plan_epoch(n, W, seed=2, lengths=list(L), window=window, accumulate=acc)
        assert Counter(i for row in a for i in row) == Counter(i for row in dp.plan_epoch(n, W, seed=2) for i in row)
        assert set(i for row in a for i in row) == set(range(n))


def test_edges():
    # fewer items than ranks: the wrap-around padding fills the one step
    plan = dp.plan_epoch(3, 8, seed=1, lengths=[5, 1, 9], window=4)
    assert [len(r) for r in plan] == [1] * 8 and Counter(i for r in plan for i in r) == Counter(i for r in dp.plan_epoch(3, 8, seed=1) for i in r)
    assert dp.plan_epoch(3, 8, seed=1, lengths=[5, 1, 9], window=4, drop_last=True) == [[] for _ in range(8)]
    # a window larger than the epoch: one global sort
    L = _lengths(11, seed=2)
    plan = dp.plan_epoch(11, 2, seed=1, lengths=L, window=1000)
    assert len(plan[0]) == 6
    _check_neighbours(plan, dp.plan_epoch(11, 2, seed=1), L, 2, 1000)
    # shuffle=False: no randomness anywhere -- the steps of a window stay in ascending order
    plan = dp.plan_epoch(8, 2, shuffle=False, lengths=[8, 7, 6, 5, 4, 3, 2, 1], window=2)
    assert [sorted((plan[0][t], plan[1][t])) for t in range(4)] == [[2, 3], [0, 1], [6, 7], [4, 5]]
    assert plan == dp.plan_epoch(8, 2, epoch=5, shuffle=False, lengths=[8, 7, 6, 5, 4, 3, 2, 1], window=2)
    # every refusal
    with pytest.raises(ValueError):
        dp.shard_indices(5, 2, 0, lengths=[1, 2, 3], window=2)
    with pytest.raises(ValueError):
        dp.shard_indices(5, 2, 0, lengths=[1] * 5, window=0)
    with pytest.raises(ValueError):
        dp.shard_indices(5, 2, 0, lengths=[1] * 5, window=2, accumulate=0)
    with pytest.raises(ValueError):
        dp.shard_indices(5, 2, 0, lengths=[1] * 5, window=6, accumulate=4)
    with pytest.raises(ValueError):
        dp.plan_epoch(5, 2, lengths=[1] * 5, window=6, accumulate=4)


# ------------------------------------------------------------------------------------------------ balance (conditions, not measurements)
def _stats(n, W, s, window, acc, deal=None):
    L, cost = _lengths(n, seed=s), dp.StepCost.default()
    plan = dp.plan_epoch(n, W, epoch=0, seed=s, lengths=L, window=window, accumulate=acc, cost=cost, _deal=deal)
    return dp.plan_stats(plan, L, cost, accumulate=acc)


@pytest.mark.parametrize("s", [0, 1, 2])
@pytest.mark.parametrize("W,min_ratio,min_eff", [(2, 3.0, 0.85), (4, 4.0, 0.80), (8, 4.0, 0.80)])
def test_windows_of_eight_cut_the_predicted_gap(W, min_ratio, min_eff, s):
    plain, win = _stats(1000, W, s, 1, 1), _stats(1000, W, s, 8, 1)
    print(f"W={W} seed={s}: plain eff {plain['efficiency']:.3f} gap {plain['gap']:.2f} ms; window 8 eff {win['efficiency']:.3f} "
          f"gap {win['gap']:.2f} ms; ratio {plain['gap'] / win['gap']:.2f}")
    assert plain["steps"] == win["steps"] == math.ceil(1000 / W)
    assert plain["gap"] / win["gap"] >= min_ratio
    assert win["efficiency"] >= min_eff


@pytest.mark.parametrize("s", [0, 1, 2])
@pytest.mark.parametrize("W", [4, 8])
def test_greedy_dealing_under_accumulation(W, s):
    plain, greedy, rot = _stats(1000, W, s, 1, 4), _stats(1000, W, s, 8, 4), _stats(1000, W, s, 8, 4, deal="rotate")
    print(f"W={W} seed={s} accumulate=4: plain gap {plain['gap']:.2f} ms; greedy {greedy['gap']:.2f}; rotation {rot['gap']:.2f}; "
          f"plain / greedy {plain['gap'] / greedy['gap']:.2f}")
    assert greedy["steps"] == math.ceil(math.ceil(1000 / W) / 4)
    assert plain["gap"] / greedy["gap"] >= 4.0
    assert greedy["gap"] <= rot["gap"]


def test_plan_stats_by_hand():
    cost = dp.StepCost.from_measurements([(0, 0.0), (10, 10.0)])
    plan, L = [[0, 1], [2, 3]], [1, 3, 3, 5]
    st = dp.plan_stats(plan, L, cost)                    # steps (1, 3) and (3, 5): mean 2 + 4, max 3 + 5
    assert st["steps"] == 2 and st["efficiency"] == pytest.approx(6 / 8) and st["gap"] == pytest.approx(1.0)
    st = dp.plan_stats(plan, L, cost, accumulate=2)      # one run: ranks 4 and 8
    assert st["steps"] == 1 and st["efficiency"] == pytest.approx(6 / 8) and st["gap"] == pytest.approx(2.0)


# ------------------------------------------------------------------------------------------------ StepCost
def test_step_cost():
    c = dp.StepCost.default()
    for rows, ms in ((512, 6.7), (4096, 17.6), (10000, 40.0), (25000, 112.4)):
        assert c(rows) == pytest.approx(ms, abs=1e-12)
    assert c(1) == c(300) == c(512) == 6.7                                             # clamped below the first point
    assert c(2304) == pytest.approx(6.7 + (17.6 - 6.7) * (2304 - 512) / (4096 - 512))  # linear between
    slope = (112.4 - 40.0) / 15000
    assert c(30000) == pytest.approx(112.4 + 5000 * slope) and c(40000) - c(30000) == pytest.approx(10000 * slope)
    m = dp.StepCost.from_measurements([(1000, 9.0), (100, 3.0), (500, 5.0)])
    assert m.points == [(100.0, 3.0), (500.0, 5.0), (1000.0, 9.0)] and m(300) == pytest.approx(4.0) and m(750) == pytest.approx(7.0)
    with pytest.raises(ValueError):
        dp.StepCost.from_measurements([(100, 3.0)])
    with pytest.raises(ValueError):
        dp.StepCost.from_measurements([])
    import json
    with open(os.path.join(ROOT, "modaltune_amd", "step_cost.json")) as f:
        d = json.load(f)
    assert d["points"] == [[512, 6.7], [4096, 17.6], [10000, 40.0], [25000, 112.4]] and "SINGLE-GPU" in d["caveat"]


# ------------------------------------------------------------------------------------------------ the sampler, two gloo processes
def _sampler_worker(rank, world, port):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        n = 37
        ds, L = list(range(n)), _lengths(n, seed=6)
        samp = dp.LengthWindowSampler(ds, seed=11, lengths=L, window=4, accumulate=2)                 # replicas / rank from the group
        assert samp.num_replicas == world and samp.rank == rank and len(samp) == 19 and samp.total_size == 38
        per_epoch = []
        for epoch in (0, 1):
            samp.set_epoch(epoch)
            mine = list(samp)
            assert mine == list(samp) == dp.shard_indices(n, world, rank, epoch=epoch, seed=11, lengths=L, window=4, accumulate=2)
            gathered = [None] * world
            dist.all_gather_object(gathered, mine)
            flat = sorted(i for g in gathered for i in g)
            assert set(flat) == set(range(n)) and len(flat) == 38 and all(len(g) == len(samp) for g in gathered)
            per_epoch.append(gathered)
        assert per_epoch[0] != per_epoch[1]
        # a DataLoader takes it like any sampler
        got = [int(b) for b in torch.utils.data.DataLoader(ds, batch_size=None, sampler=samp)]
        assert got == list(samp)
        # without lengths it is DistributedSampler
        plain = dp.LengthWindowSampler(ds, seed=11, drop_last=True)
        ref = DistributedSampler(ds, seed=11, drop_last=True)
        plain.set_epoch(2); ref.set_epoch(2)
        assert list(plain) == list(ref) and len(plain) == len(ref) == 18
    finally:
        dist.destroy_process_group()


def test_length_window_sampler_on_two_gloo_ranks():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_sampler_worker, args=(2, port), nprocs=2, join=True)


def test_sampler_without_a_process_group():
    with pytest.raises(RuntimeError):
        dp.LengthWindowSampler(list(range(4)))
    with pytest.raises(ValueError):
        dp.LengthWindowSampler(list(range(4)), num_replicas=2, rank=0, lengths=[1, 2, 3], window=2)
    s = dp.LengthWindowSampler(list(range(4)), num_replicas=1, rank=0, shuffle=False)
    assert list(s) == [0, 1, 2, 3] and len(s) == 4


# ------------------------------------------------------------------------------------------------ case_lengths
def test_case_lengths_reads_shapes_only(tmp_path):
    rows = {"a": 7, "b": 12, "c": 30}
    pts, prefixes = {}, {}
    for k, n in rows.items():
        pts[k] = str(tmp_path / f"{k}.pt")
        torch.save({"features": torch.randn(n, 16), "coords": torch.randint(0, 1000, (n, 2))}, pts[k])
        prefixes[k] = str(tmp_path / f"{k}_shard")
        data.convert_to_f16_shard(pts[k], prefixes[k])
    for src in (pts, prefixes):
        cases = [[src["a"]], [src["a"], src["b"]], [src["c"], src["b"]], src["b"]]
        got = data.case_lengths(cases, threshold=25)
        assert got == [7, 19, 25, 12] and all(type(v) is int for v in got)       # one slide, two slides, capped, a bare string
        assert data.case_lengths(cases[:3]) == [7, 19, 42]
    # what it predicts is what the loaders return
    g = torch.Generator().manual_seed(0)
    assert len(data.load_case([pts["c"], pts["b"]], threshold=25, generator=g)[0]) == 25
    assert len(data.load_case_shards([prefixes["a"], prefixes["b"]], threshold=25)[0]) == 19


# ------------------------------------------------------------------------------------------------ the tool
def test_scale_model_prints_the_predicted_table():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "scale_model.py"), "--n", "200", "--seeds", "0"], capture_output=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    out = p.stdout.decode()
    assert "predicted, unmeasured on hardware" in out
    rows = [l.split() for l in out.splitlines() if l.split() and l.split()[0] in ("2", "4", "8")]
    assert len(rows) == 6
    for r in rows:      # W, accumulate, then efficiency / gap per window: 1, 2, 4, 8, 16 ("-": accumulate does not divide the window)
        cells = " ".join(r[2:]).replace(" / ", "/").split()
        assert len(cells) == 5 and (cells[1] == "-") == (r[1] == "4")
        eff = [float(c.split("/")[0]) for c in cells if c != "-"]
        assert all(0.0 < e <= 1.0 for e in eff) and eff[-1] > eff[0]
