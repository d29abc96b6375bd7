"""Rank process of tests/test_length_sharding_gpu.py: `python tests/length_sharding_worker.py MODE RANK WORLD PORT OUT` (gloo, every rank
on GPU 0, as tests/dp_worker.py).  Eight synthetic cases of LENGTHS patches, sharded by dp.LengthWindowSampler.

fixed: deterministic engine, lr = 0 (the whole data-parallel step runs -- reducer, sharded bucket, AdamW -- and moves nothing); one epoch
       with window = 1 and one with window = 2 of the same seeded permutation; the loss of every case this rank ran, per sharding.
train: lr = 1e-3, accumulate = 2, window = 2, step_graphed with capture_after = 1, a dp.StepTimer on the step; two epochs."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from modaltune_amd import dp, synth  # noqa: E402
from modaltune_amd.config import ModelConfig  # noqa: E402

LENGTHS = [37, 150, 41, 163, 96, 300, 100, 290]
SEED, NGRIDS, SAMPLER_SEED = 5, 32, 1


def cfg():
    return ModelConfig(depth=3, interaction_indexes=((0, 0), (1, 1), (2, 2)), slide_ngrids=NGRIDS)


def case(i, sizes):
    inp = synth.synth_inputs(LENGTHS[i], sizes, seed=400 + i, grid=NGRIDS)
    return (torch.from_numpy(inp["x"]).cuda(), torch.from_numpy(inp["coords"]).cuda(), [torch.from_numpy(a).cuda() for a in inp["genes"]],
            torch.from_numpy(inp["text"]).cuda())


def build(deterministic=False, **ts_kw):
    from modaltune_amd.engine import Engine
    from modaltune_amd.trainer import TrainStep
    sizes = synth.toy_group_sizes()
    eng = Engine(cfg(), sizes, "cuda", deterministic=deterministic)
    eng.load_state_dict(synth.synth_state_dict(cfg(), sizes, SEED))
    dp.broadcast_params_(eng.store.flat)
    ts = TrainStep(eng, **ts_kw)
    ts.set_projector(synth.projector_state(SEED))
    return eng, ts, [case(i, sizes) for i in range(len(LENGTHS))]


def fixed(rank, world, out):
    eng, ts, cases = build(deterministic=True, lr=0.0)
    flat0 = eng.store.flat.clone()
    rec = {}
    for window in (1, 2):
        order = list(dp.LengthWindowSampler(cases, seed=SAMPLER_SEED, lengths=LENGTHS, window=window))
        losses = [float(ts.step(*cases[i])) for i in order]
        rec[f"order{window}"], rec[f"loss{window}"] = np.array(order), np.array(losses, dtype=np.float64)
    if eng.store.sync is not None:
        eng.store.sync()
    torch.cuda.synchronize()
    eng.check_inputs()
    np.savez(out, held=int(torch.equal(eng.store.flat, flat0)), steps=int(ts.step_dev), sharded=int(ts.reducer.sharded),
             collectives=int(ts.reducer.collectives), **rec)


def train(rank, world, out):
    eng, ts, cases = build(lr=1e-3, accumulate=2, capture_after=1)
    samp = dp.LengthWindowSampler(cases, seed=SAMPLER_SEED, lengths=LENGTHS, window=2, accumulate=2)
    ts.step_timer = dp.StepTimer()
    flat0 = eng.store.flat.clone()
    orders, window_pos, reports, verified = [], [], [], 0
    for epoch in range(2):
        samp.set_epoch(epoch)
        order = list(samp)
        for i in order:
            ts.step_graphed(*cases[i])
        window_pos.append(int(ts.window_pos))
        ts.finish_window()
        rep = ts.step_timer.report(accumulate=2)
        ts.verify_replicas()                 # raises on every rank when the replicas differ
        verified += 1
        orders.append(order)
        reports.append(rep)
    if eng.store.sync is not None:
        eng.store.sync()
    torch.cuda.synchronize()
    eng.check_inputs()
    np.savez(out, flat=eng.store.flat.cpu().numpy(), moved=float((eng.store.flat - flat0).abs().mean()), orders=np.array(orders),
             window_pos=np.array(window_pos), verified=verified, steps=int(ts.step_dev), replays=int(ts.graph_replays),
             sharded=int(ts.reducer.sharded), times=np.array([r["times"] for r in reports], dtype=np.float64),
             report_steps=np.array([r["steps"] for r in reports]), efficiency=np.array([r["efficiency"] for r in reports]),
             gap=np.array([r["gap"] for r in reports]))


if __name__ == "__main__":
    mode, rank, world, port, out = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", port
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        {"fixed": fixed, "train": train}[mode](rank, world, out)
    finally:
        dist.destroy_process_group()
