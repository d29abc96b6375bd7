"""Cost of Integrated Gradients over the patch embeddings (attribution.IntegratedGradients, inputs="patches") beside the eager train step
and beside the gene-input form, on the same engine in the same run: steps = 32 on task 0, three points per pass (12 engine passes).
An IG pass is the B = 3 step's forward and backward without the loss plus mt_patch_points_fwd and mt_patch_ig_accumulate -- about
0.2 GB of traffic at L = 10 000 from byte counts (x0p 92 MB written once and read by the first Injector, ex / eb 31 MB each) -- so the
expectation is "what that step costs"; informational, not a pass bar.

    python tools/patch_ig_bench.py [L ...] (default: 10000)

Prints one JSON line per bag length, with the box's measured MFMA peak."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from modaltune_amd import ops, synth  # noqa: E402
from modaltune_amd.attribution import IntegratedGradients  # noqa: E402
from modaltune_amd.config import ModelConfig  # noqa: E402
from modaltune_amd.engine import Engine  # noqa: E402
from modaltune_amd.trainer import TrainStep  # noqa: E402

lengths = [int(a) for a in sys.argv[1:]] or [10000]
STEPS, REPS = 32, 5
dev = torch.device("cuda", 0)
cfg = ModelConfig()
sizes = synth.toy_group_sizes(6)
eng = Engine(cfg, sizes, dev)
eng.load_state_dict(synth.synth_state_dict(cfg, sizes, seed=0))
ts = TrainStep(eng, split_passes=False)           # the batched B = 3 pass: what an IG pass of three points is shaped like
ts.set_projector(synth.projector_state(0))
igs = {k: IntegratedGradients(eng, (0,), steps=STEPS, inputs=k) for k in ("genes", "patches", "both")}
target = torch.ones(cfg.output_dim, device=dev) / 16
peak = ops.measured_mfma_peak_tflops()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


for L in lengths:
    inp = synth.synth_inputs(L, sizes, seed=1000, grid=128 if L <= 128 * 128 else 512)
    x = torch.from_numpy(inp["x"]).to(dev).half().reshape(L, -1).contiguous()
    coords = torch.from_numpy(inp["coords"]).to(dev)
    genes = [torch.from_numpy(a).to(dev) for a in inp["genes"]]
    text = torch.from_numpy(inp["text"])
    for _ in range(3):
        ts.step(x, coords, genes, text, update=False)
    step_ms = [timed(lambda: ts.step(x, coords, genes, text, update=False)) for _ in range(REPS)]
    IntegratedGradients(eng, (0,), steps=4, inputs="both")(x, coords, genes, target)      # warm-up: workspaces and arenas of this geometry
    call_ms = {k: [timed(lambda: ig(x, coords, genes, target)) for _ in range(3)] for k, ig in igs.items()}
    npass = igs["patches"].passes
    print(json.dumps({"metric": "Integrated Gradients over the patch embeddings: ms per engine pass beside the eager train step",
                      "patches": L, "steps": STEPS, "tasks": 1, "points_per_pass": igs["patches"].points_per_pass, "engine_passes": npass,
                      "ig_call_ms_median_of_3": {k: round(statistics.median(v), 2) for k, v in call_ms.items()},
                      "ig_ms_per_pass": {k: round(statistics.median(v) / npass, 3) for k, v in call_ms.items()},
                      "train_step_no_update_ms": round(statistics.median(step_ms), 3),
                      "train_step_min_max": [round(min(step_ms), 3), round(max(step_ms), 3)], "mfma_peak_measured": round(peak, 1)}),
          flush=True)
