"""mt_adamw_step_groups_ema against mt_adamw_step_groups on the model's flat buffers (one process, one GPU, device events):

    python tools/ema_bench.py > profiles/ema.txt

Two buffer sizes: the shipped configuration's flat parameter buffer (ModelConfig(), six toy pathways: 244 tensors) and the one with the
reference's 331 pathways (1 544 tensors), each with the layout's one-segment-per-tensor table (tensor i in group i % 2, as in
tools/adamw_groups_bench.py: the grouped launch a step with parameter groups makes).  Per size three launches alternate, window by
window, on the SAME buffers:
    plain      mt_adamw_step_groups                       28 B per parameter
    ema        mt_adamw_step_groups_ema, warm-up off      36 B per parameter: the average is read and written as well
    swap       mt_swap_f32(parameters, average)           16 B per parameter (what ema_weights() launches on entry and on exit)
A window is WINDOW_S seconds of back-to-back launches between two events (the count comes from an untimed calibration window); ROUNDS
rounds of the windows, so every variant is timed for ROUNDS * WINDOW_S >= 1 s and a drift of the clock hits all alike.  Reported per
variant: the windows' us per launch, their median, and the spread (max - min) / median -- the plain variant's spread is the noise floor
the ema / plain ratio is judged against; traffic alone says 36 / 28 = 1.286.  The launches run back to back on the same buffers, so the
figures are WARM ones: at the shipped size a launch moves 258 MB (plain) / 332 MB (ema) -- about the size of the 256 MB MALL, which can
serve much of it (the TB/s printed there is not an HBM rate) -- and 939 / 1 207 MB with the 331 pathways, which is HBM traffic."""
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
LR, B1, B2, EPS, WD, DECAY = 1e-6, 0.9, 0.999, 1e-8, 0.01, 0.999
BYTES = {"plain": 28, "ema": 36, "swap": 16}


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
    ema = p.clone()
    end, grp = optim.segment_table([(o, k, i % 2) for i, (o, k, _) in enumerate(slots.values())])
    end, grp, hp = end.cuda(), grp.cuda(), [(1.0, WD), (0.5, 0.0)]
    step_dev = torch.full((1,), 1000, dtype=torch.int32, device="cuda")
    lr_dev = torch.full((1,), LR, device="cuda")
    scale = torch.full((1,), 1024.0, device="cuda")
    found_inf = torch.zeros(1, dtype=torch.int32, device="cuda")
    kw = dict(scale=scale, found_inf=found_inf, grad_mult=1.0, step_dev=step_dev, lr_dev=lr_dev)      # the fused step's call
    fns = {"plain": lambda: ops.adamw_step_groups(p, grad, m, v, n, 0, end, grp, hp, LR, B1, B2, EPS, 0, **kw),
           "ema": lambda: ops.adamw_step_groups_ema(p, grad, m, v, n, 0, end, grp, hp, LR, B1, B2, EPS, 0, ema, DECAY, False, **kw),
           "swap": lambda: ops.swap_f32(p, ema, n)}
    counts = {}
    for name, fn in fns.items():      # warm-up and calibration (untimed)
        _window(fn, 20)
        counts[name] = max(20, int(WINDOW_S * 1e6 / _window(fn, 100))) // 2 * 2      # (even: the swaps leave the buffers where they were)
    times = {name: [] for name in fns}
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            times[name].append(_window(fn, counts[name]))
    print(f"{label}: {len(slots)} tensors, n_flat {n} = {4 * n / 1e6:.1f} MB per buffer, {int(end.numel())} segments; moved per launch: "
          + ", ".join(f"{k} {b * n / 1e6:.0f} MB" for k, b in BYTES.items()))
    med = {}
    for name, ts in times.items():
        med[name] = float(np.median(ts))
        print(f"  {name:5s} {counts[name]:5d} launches x {ROUNDS} windows: us per launch {[round(t, 2) for t in ts]}  median {med[name]:.2f} us "
              f"({BYTES[name] * n / med[name] / 1e6:.2f} TB/s)  spread {(max(ts) - min(ts)) / med[name] * 100:.2f} %")
    print(f"  ema / plain at the medians: {med['ema'] / med['plain']:.4f}  (traffic alone: {36 / 28:.4f}; per window, in order: "
          f"{[round(a / b, 4) for a, b in zip(times['ema'], times['plain'])]})")
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(ema).all()) and int(found_inf) == 0
    return {"label": label, "n_flat": n, "median_us": med, "ema_over_plain": med["ema"] / med["plain"]}


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("ema_bench: needs a GPU (a CPU run measures nothing)")
    print(f"# mt_adamw_step_groups_ema against mt_adamw_step_groups (and mt_swap_f32), HIP events, {ROUNDS} alternating rounds of {WINDOW_S} s "
          f"windows per variant; {torch.cuda.get_device_name(0)}")
    out = [bench("shipped configuration, 6 toy pathways", synth.toy_group_sizes()),
           bench("331 pathways", json.load(open(os.path.join(ROOT, "tests", "golden", "pathway_sizes_331.json"))))]
    print(json.dumps(out))
