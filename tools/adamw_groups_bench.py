"""mt_adamw_step_groups against mt_adamw_step on the model's flat buffers (one process, one GPU, device events):

    python tools/adamw_groups_bench.py > profiles/adamw_groups.txt

Two buffer sizes: the shipped configuration's flat parameter buffer (ModelConfig(), six toy pathways: 244 tensors) and the one with the
reference's 331 pathways (1 544 tensors).  Per size three launches alternate, window by window, on the same four buffers:
    uniform    mt_adamw_step                                       (what the default step launches)
    one_group  mt_adamw_step_groups, every tensor in one group     (one segment)
    alternate  mt_adamw_step_groups, tensor i in group i % 2       (one segment per tensor: the most lookups a layout can ask for)
A window is WINDOW_S seconds of back-to-back launches between two events (the count comes from an untimed calibration window); ROUNDS
rounds of the three windows, so every variant is timed for ROUNDS * WINDOW_S >= 1 s and a drift of the clock hits all three alike.
Reported per variant: the windows' us per launch, their median, and the spread (max - min) / median -- the uniform variant's spread is
the noise floor a difference has to clear.  The launches run back to back on the SAME four buffers, so the figures are WARM ones: a
launch moves 28 B per parameter, 258 MB at the shipped size -- about the size of the 256 MB MALL, which can serve much of it (the TB/s
printed there is not an HBM rate) -- and 939 MB with the 331 pathways, which is HBM traffic.  The three variants see the same cache
state, so their ratio is like for like at either size."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from modaltune_amd import checkpoint, ops, optim, synth  # noqa: E402
from modaltune_amd.config import ModelConfig  # noqa: E402

WINDOW_S, ROUNDS = 0.15, 8
LR, B1, B2, EPS, WD = 1e-6, 0.9, 0.999, 1e-8, 0.01


def _window(fn, count):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(count):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / count      # us per launch


def bench(label, sizes):
    slots, n = checkpoint.slots_of(synth.param_specs(ModelConfig(), sizes))
    g = torch.Generator(device="cuda").manual_seed(1)
    p, grad = torch.randn(n, device="cuda", generator=g), 1e-3 * torch.randn(n, device="cuda", generator=g)
    m, v = 1e-3 * torch.randn(n, device="cuda", generator=g), 1e-6 * torch.rand(n, device="cuda", generator=g)
    tables = {}
    for name, group_of in (("one_group", lambda i: 0), ("alternate", lambda i: i % 2)):
        end, grp = optim.segment_table([(o, k, group_of(i)) for i, (o, k, _) in enumerate(slots.values())])
        tables[name] = (end.cuda(), grp.cuda(), int(end.numel()))
    step_dev = torch.full((1,), 1000, dtype=torch.int32, device="cuda")
    lr_dev = torch.full((1,), LR, device="cuda")
    scale = torch.full((1,), 1024.0, device="cuda")
    found_inf = torch.zeros(1, dtype=torch.int32, device="cuda")
    kw = dict(scale=scale, found_inf=found_inf, grad_mult=1.0, step_dev=step_dev, lr_dev=lr_dev)      # the fused step's call
    hp = {"one_group": [(1.0, WD)], "alternate": [(1.0, WD), (0.5, 0.0)]}
    fns = {"uniform": lambda: ops.adamw_step(p, grad, m, v, n, LR, B1, B2, EPS, WD, 0, **kw)}
    for name, (end, grp, _) in tables.items():
        fns[name] = (lambda end=end, grp=grp, name=name: ops.adamw_step_groups(p, grad, m, v, n, 0, end, grp, hp[name], LR, B1, B2, EPS, 0, **kw))
    counts = {}
    for name, fn in fns.items():      # warm-up and calibration (untimed)
        _window(fn, 20)
        counts[name] = max(20, int(WINDOW_S * 1e6 / _window(fn, 100)))
    times = {name: [] for name in fns}
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            times[name].append(_window(fn, counts[name]))
    print(f"{label}: {len(slots)} tensors, n_flat {n} = {4 * n / 1e6:.1f} MB per buffer, {28 * n / 1e6:.0f} MB moved per launch; segments: "
          f"one_group {tables['one_group'][2]}, alternate {tables['alternate'][2]}")
    med = {}
    for name, ts in times.items():
        med[name] = float(np.median(ts))
        print(f"  {name:9s} {counts[name]:5d} launches x {ROUNDS} windows: us per launch {[round(t, 2) for t in ts]}  median {med[name]:.2f} us "
              f"({28 * n / med[name] / 1e6:.2f} TB/s)  spread {(max(ts) - min(ts)) / med[name] * 100:.2f} %")
    for name in ("one_group", "alternate"):
        print(f"  {name} / uniform at the medians: {med[name] / med['uniform']:.4f}")
    assert bool(torch.isfinite(p).all()) and int(found_inf) == 0
    return {"label": label, "n_flat": n, "median_us": med}


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("adamw_groups_bench: needs a GPU (a CPU run measures nothing)")
    print(f"# mt_adamw_step_groups against mt_adamw_step, HIP events, {ROUNDS} alternating rounds of {WINDOW_S} s windows per variant; "
          f"{torch.cuda.get_device_name(0)}")
    out = [bench("shipped configuration, 6 toy pathways", synth.toy_group_sizes()),
           bench("331 pathways", json.load(open(os.path.join(ROOT, "tests", "golden", "pathway_sizes_331.json"))))]
    print(json.dumps(out))
