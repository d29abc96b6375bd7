"""Cost of gradient accumulation and global-norm clipping in the fused train step: ms per SLIDE at L = 10 000 through
TrainStep.step_graphed (hipGraph replay, the schedule the headline number is quoted on) for four settings of (accumulate, clip):
(1, off) -- the step as it always was --, (1, on), (4, off), (4, on).  Expected from byte counts only: the clip costs what
mt_check_finite costs (the 37 MB gradient buffer read once, ~10 us per boundary); accumulate = k saves the optimiser's ~28 bytes per
parameter on k - 1 of k slides.  Informational, not a pass bar.

    python tools/accum_clip_bench.py [--patches 10000] [--windows 12] [--limit 240]

Every setting runs in a fresh child process under its own time limit (--limit seconds); a child that fails or runs out of time ends
the run -- nothing more is started on the device.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = [(1, False), (1, True), (4, False), (4, True)]


def child(patches: int, k: int, clip: bool, windows: int):
    import torch
    sys.path.insert(0, ROOT)
    from modaltune_amd import synth
    from modaltune_amd.config import ModelConfig
    from modaltune_amd.engine import Engine
    from modaltune_amd.trainer import TrainStep
    dev = torch.device("cuda", 0)
    cfg = ModelConfig()
    sizes = synth.toy_group_sizes(6)
    eng = Engine(cfg, sizes, dev)
    eng.load_state_dict(synth.synth_state_dict(cfg, sizes, seed=0))
    eng.set_stochastic(True, seed=0)
    ts = TrainStep(eng, accumulate=k, max_grad_norm=1.0 if clip else None, capture_after=2)
    ts.set_projector(synth.projector_state(0))
    ts.auto_split = False                      # (the threshold rule: the same schedule in all four settings, no trial inside the timing)
    inp = synth.synth_inputs(patches, sizes, seed=1000, grid=128 if patches <= 128 * 128 else 512)
    x = torch.from_numpy(inp["x"]).to(dev).half().reshape(patches, -1).contiguous()
    coords = torch.from_numpy(inp["coords"]).to(dev)
    genes = [torch.from_numpy(a).to(dev) for a in inp["genes"]]
    text = torch.from_numpy(inp["text"])
    for _ in range(4 * k):                     # eager visits, the capture of every window position, one replayed window
        ts.step_graphed(x, coords, genes, text)
    torch.cuda.synchronize()
    replays = ts.graph_replays
    per_slide = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(k):
            ts.step_graphed(x, coords, genes, text)
        b.record()
        b.synchronize()
        per_slide.append(a.elapsed_time(b) / k)
    assert ts.graph_replays == replays + windows * k, "a timed slide was not a replay"
    print(json.dumps({"accumulate": k, "clip": clip, "ms_per_slide_median": round(statistics.median(per_slide), 3),
                      "ms_per_slide_min_max": [round(min(per_slide), 3), round(max(per_slide), 3)], "windows": windows,
                      "optimiser_steps": int(ts.step_dev), "grad_norm": float(ts.grad_norm) if clip else None,
                      "pass_groups": ts._pass_streams is not None}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patches", type=int, default=10000)
    ap.add_argument("--windows", type=int, default=12)
    ap.add_argument("--limit", type=int, default=240, help="seconds per setting")
    ap.add_argument("--child", nargs=2, metavar=("K", "CLIP"))
    a = ap.parse_args()
    if a.child:
        return child(a.patches, int(a.child[0]), a.child[1] == "1", a.windows)
    rows, error = [], None
    for k, clip in SETTINGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--patches", str(a.patches), "--windows", str(a.windows), "--child", str(k), str(int(clip))]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            error = f"(accumulate {k}, clip {clip}) ran past {a.limit} s"
            break
        if p.returncode != 0:
            error = f"(accumulate {k}, clip {clip}) exited with {p.returncode}: {p.stderr[-300:]}"
            break
        rows.append(json.loads(p.stdout.strip().splitlines()[-1]))
    print(json.dumps({"metric": "fused train step, hipGraph replay: ms per slide by (accumulate, clip)", "patches": a.patches,
                      "settings": rows, "error": error}), flush=True)
    return 1 if error else 0


if __name__ == "__main__":
    sys.exit(main() or 0)
