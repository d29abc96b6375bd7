"""PREDICTED data-parallel efficiency of an epoch under `dp.plan_epoch`: plain DistributedSampler sharding (window = 1) against
length windows, for W = 2 / 4 / 8 ranks and accumulate 1 / 4.  CPU only; nothing here is measured on more than one GPU.

  python tools/scale_model.py [--n 1000] [--seeds 0 1 2] [--cost ROWS:MS ROWS:MS ...] [--markdown]

Bag lengths: min(cap, floor(exp(U(ln lo, ln hi)))) from numpy.random.default_rng(seed) -- a few hundred patches up to the 25 000-patch
cap of the dataset (data_utils/datasets.py:274-281 of the reference), a spike at the cap.  Cost of a step: dp.StepCost.default() (this
project's single-GPU step times) or --cost pairs of your own.  A synchronous step costs what its slowest rank costs:
efficiency = sum over the steps of the ranks' mean cost / sum of their max; gap = mean over the steps of max - mean, in ms.
"""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from modaltune_amd import dp  # noqa: E402

WORLDS, WINDOWS, ACCUMULATES = (2, 4, 8), (1, 2, 4, 8, 16), (1, 4)


def bag_lengths(n: int, seed: int, lo: float = 300.0, hi: float = 60000.0, cap: int = 25000):
    u = np.random.default_rng(seed).uniform(math.log(lo), math.log(hi), n)
    return [int(min(cap, math.floor(math.exp(v)))) for v in u]


def table(n: int, seeds, cost):
    """{(world, accumulate, window): (mean efficiency, mean gap)} over the seeds; windows that `accumulate` does not divide are left out."""
    out = {}
    for world in WORLDS:
        for acc in ACCUMULATES:
            for window in WINDOWS:
                if window > 1 and window % acc:
                    continue
                eff, gap = [], []
                for s in seeds:
                    lengths = bag_lengths(n, s)
                    plan = dp.plan_epoch(n, world, epoch=0, seed=s, lengths=lengths, window=window, accumulate=acc, cost=cost)
                    st = dp.plan_stats(plan, lengths, cost, accumulate=acc)
                    eff.append(st["efficiency"])
                    gap.append(st["gap"])
                out[(world, acc, window)] = (float(np.mean(eff)), float(np.mean(gap)))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=1000, help="cases per epoch")
    ap.add_argument("--seeds", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--cost", nargs="+", metavar="ROWS:MS", help="measured (rows, ms) points instead of the committed default")
    ap.add_argument("--markdown", action="store_true", help="print the table as markdown rows")
    a = ap.parse_args()
    cost = dp.StepCost.from_measurements([tuple(float(v) for v in p.split(":")) for p in a.cost]) if a.cost else dp.StepCost.default()
    res = table(a.n, a.seeds, cost)
    print(f"predicted, unmeasured on hardware: n = {a.n}, seeds {a.seeds}, cost points {cost.points}")
    sep = " | " if a.markdown else "  "
    head = ["W", "accumulate"] + [f"window {w}" for w in WINDOWS]
    print(("| " if a.markdown else "") + sep.join(f"{h:>14}" for h in head) + (" |" if a.markdown else ""))
    if a.markdown:
        print("|" + "|".join(["---"] * len(head)) + "|")
    for world in WORLDS:
        for acc in ACCUMULATES:
            cells = [f"{world}", f"{acc}"]
            for window in WINDOWS:
                v = res.get((world, acc, window))
                cells.append("-" if v is None else f"{v[0]:.3f} / {v[1]:.2f}")
            print(("| " if a.markdown else "") + sep.join(f"{c:>14}" for c in cells) + (" |" if a.markdown else ""))
    print("cell: efficiency / gap in ms per synchronisation (window 1 = the DistributedSampler rule)")


if __name__ == "__main__":
    main()
