"""Rank process of tests/test_adamw_groups_dp_gpu.py: `python tests/adamw_groups_dp_worker.py RANK WORLD PORT OUT`.

tests/dp_worker.py's `trainstep` mode (two gloo ranks on GPU 0, one slide per rank, eager visit -> segmented capture -> replays, the
last gradient bucket reduce-scattered and its AdamW run on this rank's shard) with parameter groups set: the grouped AdamW runs once
per piece of the flat buffer this rank updates, each piece at its absolute position in the one segment table."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dp_worker as W  # noqa: E402
from modaltune_amd import dp, synth  # noqa: E402

RULES = [{"match": r"^gene_encoder\.mlp_mixer\.0\.", "lr_mult": 0.0, "weight_decay": 0.0},      # held still, inside the sharded (last) bucket
         {"match": r"^gene_encoder\.", "lr_mult": 0.1},
         {"kinds": ("b", "lnw", "lnb", "gamma", "tok"), "weight_decay": 0.0}]


def main(rank, world, out):
    from modaltune_amd.engine import Engine
    from modaltune_amd.trainer import TrainStep
    sizes = synth.toy_group_sizes()
    cfg = W._cfg()
    eng = Engine(cfg, sizes, "cuda")
    eng.load_state_dict(synth.synth_state_dict(cfg, sizes, W.SEED))
    dp.broadcast_params_(eng.store.flat)
    ts = TrainStep(eng, lr=1e-3, capture_after=1, param_groups=RULES, verify_every=1)      # (the replica canary after every step)
    ts.set_projector(synth.projector_state(W.SEED))
    x, coords, genes, text = W._slide(rank, sizes)
    launches = []
    from modaltune_amd import ops
    real = ops.adamw_step_groups
    ops.adamw_step_groups = lambda *a, **k: (launches.append((int(a[5]), int(a[4]))), real(*a, **k))[1]      # (index_base, n) of every piece
    losses = []
    for _ in range(W.STEPS):
        losses.append(float(ts.step_graphed(x, coords, genes, text)))
    ts.verify_replicas()
    sd = eng.store.state_dict()
    torch.cuda.synchronize()
    pieces = ts.reducer.adam_pieces(eng.store.n_flat)
    np.savez(out, flat=eng.store.flat.cpu().numpy(), losses=np.array(losses), replays=ts.graph_replays, steps=int(ts.step_dev),
             sharded=int(ts.reducer.sharded), pieces=np.array(pieces), launches=np.array(launches), ngroups=len(ts.param_groups),
             grouped=int(ts._grouped()), backend=dist.get_backend())
    del sd


if __name__ == "__main__":
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", port
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        main(rank, world, out)
    finally:
        dist.destroy_process_group()
