"""CPU (gloo, world_size 2): dp.GradReducer.gather_shards_, the collective behind TrainStep.state_dict() -- a flat buffer of which
every rank holds valid values for its own shard of the reduce-scattered ranges only (the AdamW moments under the sharded last bucket)
becomes complete and equal on every rank, through the host-staging arm (gloo rehearsals) and through the device-tensor arm (what RCCL
runs; gloo executes the same call on CPU tensors, as tests/test_dp_cpu.py drives the reducer's other `else:` arms)."""
import os

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from modaltune_amd import dp

from test_dp_cpu import _free_port


def _worker(rank, world, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from modaltune_amd import synth
        from modaltune_amd.config import ModelConfig
        from modaltune_amd.engine import ParamStore
        cfg = ModelConfig(depth=3, interaction_indexes=((0, 0), (1, 1), (2, 2)))
        st = ParamStore(cfg, synth.toy_group_sizes(), "cpu")
        buckets = dp.grad_buckets(st.slots, 3, st.n_flat)
        truth = torch.sin(torch.arange(st.n_flat, dtype=torch.float32) * 0.37)          # what the owners hold, on every rank
        for host in (True, False):
            red = dp.GradReducer(st.flat_grad, buckets, flat_param=st.flat)
            assert red.sharded and red._rs and red._host
            red._host = host
            # this rank's moments: valid on its adam_pieces, garbage (its rank number) everywhere else
            m = torch.full((st.n_flat,), float(100 + rank))
            for o, k in red.adam_pieces(st.n_flat):
                m[o:o + k] = truth[o:o + k]
            assert not torch.equal(m, truth)
            c0 = red.collectives
            red.gather_shards_(m)
            assert red.collectives - c0 == len(red._rs)
            assert torch.equal(m, truth), (host, int((m != truth).sum()))
        plain = dp.GradReducer(st.flat_grad, buckets)          # no sharded bucket: nothing to gather, nothing issued
        m = torch.full((st.n_flat,), 5.0)
        plain.gather_shards_(m)
        assert plain.collectives == 0 and bool((m == 5.0).all())
    finally:
        dist.destroy_process_group()


def test_gather_shards_completes_the_moments_on_every_rank():
    mp.spawn(_worker, args=(2, _free_port()), nprocs=2, join=True)
