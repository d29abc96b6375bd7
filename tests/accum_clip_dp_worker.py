"""Rank process of tests/test_accum_clip_dp_gpu.py: `python tests/accum_clip_dp_worker.py RANK WORLD PORT OUT` (gloo, every rank on
GPU 0, as tests/dp_worker.py).  Three windows of accumulate = 2 with clipping through step_graphed (capture_after = 1: an eager
window, a window that captures every position, a replayed window); rank r takes slides 2 r and 2 r + 1 of SLIDES in every window."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from modaltune_amd import dp, synth  # noqa: E402
from modaltune_amd.config import ModelConfig  # noqa: E402

L, SEED, NGRIDS, WINDOWS, SLIDES, MAX_NORM, LR = 150, 5, 32, 3, 4, 1e-3, 1e-3


def cfg():
    return ModelConfig(depth=3, interaction_indexes=((0, 0), (1, 1), (2, 2)), slide_ngrids=NGRIDS, dropout=0.0, drop_path_rate=0.0)


def slide(i, sizes):
    inp = synth.synth_inputs(L, sizes, seed=900 + i, grid=NGRIDS)
    return (torch.from_numpy(inp["x"]).cuda(), torch.from_numpy(inp["coords"]).cuda(), [torch.from_numpy(a).cuda() for a in inp["genes"]],
            torch.from_numpy(inp["text"]).cuda())


def build(**ts_kw):
    from modaltune_amd.engine import Engine
    from modaltune_amd.trainer import TrainStep
    sizes = synth.toy_group_sizes()
    eng = Engine(cfg(), sizes, "cuda")
    eng.load_state_dict(synth.synth_state_dict(cfg(), sizes, SEED))
    ts = TrainStep(eng, lr=LR, weight_decay=0.01, max_grad_norm=MAX_NORM, **ts_kw)
    ts.set_projector(synth.projector_state(SEED))
    ts.auto_split = False
    return eng, ts, sizes


def main(rank, world, out):
    eng, ts, sizes = build(accumulate=2, capture_after=1)
    dp.broadcast_params_(eng.store.flat)
    slides = [slide(2 * rank + i, sizes) for i in range(2)]
    n = eng.store.n_flat
    held = torch.zeros(n, dtype=torch.bool, device="cuda")      # the elements whose REDUCED gradient this rank holds after a boundary
    for o, k in ts.reducer.adam_pieces(n):
        held[o:o + k] = True
    rec = {k: [] for k in ("micro_collectives", "boundary_collectives", "clip", "flat", "replayed", "steps")}
    grad0 = None
    for w in range(WINDOWS):
        c0, r0 = ts.reducer.collectives, ts.graph_replays
        ts.step_graphed(*slides[0])
        torch.cuda.synchronize()
        rec["micro_collectives"].append(ts.reducer.collectives - c0)
        c1 = ts.reducer.collectives
        ts.step_graphed(*slides[1])
        if eng.store.sync is not None:
            eng.store.sync()             # the sharded parameter all-gather of this boundary
        torch.cuda.synchronize()
        rec["boundary_collectives"].append(ts.reducer.collectives - c1)
        rec["replayed"].append(ts.graph_replays - r0)
        rec["clip"].append(ts._clip_out.cpu().numpy().copy())
        rec["flat"].append(eng.store.flat.cpu().numpy().copy())
        rec["steps"].append(int(ts.step_dev))
        if w == 0:
            grad0 = (eng.store.flat_grad.double() / float(ts.grad_scale)).cpu().numpy()
    eng.check_inputs()
    np.savez(out, grad0=grad0, held=held.cpu().numpy(), sharded=int(ts.reducer.sharded), split=int(ts._pass_streams is not None),
             schedule=ts.dp_schedule, window_pos=ts.window_pos, **{k: np.array(v) for k, v in rec.items()})


if __name__ == "__main__":
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", port
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        main(rank, world, out)
    finally:
        dist.destroy_process_group()
