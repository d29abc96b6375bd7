"""GPU, two processes: TrainStep(param_groups=...) under data parallelism -- the twin of
test_dp_gpu.py::test_two_rank_trainstep_matches_gradient_averaging with groups set.  Two gloo ranks on GPU 0, the last gradient
bucket sharded: every rank's grouped AdamW runs over the pieces of the flat buffer it owns, each at its absolute position in the one
segment table.  Three processes hold the GPU (this one and the two ranks); each rank runs under a time limit of its own and the first
rank that fails ends the other."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor, as_completed

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "adamw_groups_dp_worker.py")
RANK_TIMEOUT = 300          # seconds, per rank process (a run takes ~20)


def _run_ranks(tmp_path, world=2):
    from test_dp_gpu import _free_port
    port = str(_free_port())
    outs = [str(tmp_path / f"groups_{r}.npz") for r in range(world)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"), MT_TEST_BACKEND="gloo")
    env.pop("MT_DP_SHARD_LAST", None)          # (the sharded last bucket is the default: make sure it is on)
    procs = [subprocess.Popen(["timeout", "-k", "10", str(RANK_TIMEOUT), sys.executable, WORKER, str(r), str(world), port, outs[r]], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    logs = {}
    with ThreadPoolExecutor(max_workers=world) as ex:
        waits = {ex.submit(p.communicate): r for r, p in enumerate(procs)}
        for fut in as_completed(waits):
            r = waits[fut]
            logs[r] = fut.result()[0].decode()[-3000:]
            if procs[r].returncode != 0:          # the first rank that fails ends the others: nothing waits for a peer that is gone
                for q in procs:
                    if q.poll() is None:
                        q.kill()
    assert all(p.returncode == 0 for p in procs), "\n----\n".join(f"rank {r} (exit {procs[r].returncode}):\n{logs.get(r, '')}" for r in range(world))
    return [np.load(o) for o in outs]


def test_two_rank_trainstep_with_groups_matches_gradient_averaging(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import adamw_groups_dp_worker as GW
    import dp_worker as W
    from test_dp_gpu import synth_flat
    from modaltune_amd import synth
    from modaltune_amd.engine import Engine
    from modaltune_amd.trainer import TrainStep
    r0, r1 = _run_ranks(tmp_path)
    for r in (r0, r1):
        assert int(r["steps"]) == W.STEPS and int(r["replays"]) == W.STEPS - 1 and int(r["sharded"]) == 1 and int(r["grouped"]) == 1
        # one grouped launch per piece this rank updates, each with the piece's absolute position, at every step (the eager visit and
        # the capture launch from Python; replays do not)
        pieces = [tuple(int(v) for v in p) for p in r["pieces"]]
        launches = [tuple(int(v) for v in p) for p in r["launches"]]
        assert len(pieces) >= 2 and launches[:len(pieces)] == pieces and set(launches) == set(pieces) and len(launches) % len(pieces) == 0
    assert [tuple(p) for p in r0["pieces"].tolist()] != [tuple(p) for p in r1["pieces"].tolist()]      # (each rank its own shard)
    assert np.array_equal(r0["flat"], r1["flat"])                                  # verify_replicas() passed on both; seen here again
    assert not np.allclose(r0["losses"], r1["losses"])                             # (different slides)
    # single-process reference: gradients of both slides summed, the grouped AdamW with grad_mult = 1/2
    sizes = synth.toy_group_sizes()
    cfg = W._cfg()
    eng = Engine(cfg, sizes, "cuda")
    eng.load_state_dict(synth.synth_state_dict(cfg, sizes, W.SEED))
    ts = TrainStep(eng, lr=1e-3, param_groups=GW.RULES)
    ts.set_projector(synth.projector_state(W.SEED))
    assert int(r0["ngroups"]) == len(ts.param_groups) == 4
    slides = [W._slide(r, sizes) for r in range(2)]
    ref_losses = []
    for _ in range(W.STEPS):
        acc = torch.zeros_like(eng.store.flat_grad)
        ls = []
        for x, coords, genes, text in slides:
            ls.append(float(ts.step(x, coords, genes, text, update=False)))
            acc += eng.store.flat_grad
        eng.store.flat_grad.copy_(acc)
        ts._adam_and_refresh(2)
        ref_losses.append(ls)
    torch.cuda.synchronize()
    ref_losses = np.array(ref_losses)
    assert np.allclose(r0["losses"], ref_losses[:, 0], rtol=2e-3), (r0["losses"], ref_losses[:, 0])
    assert np.allclose(r1["losses"], ref_losses[:, 1], rtol=2e-3), (r1["losses"], ref_losses[:, 1])
    ref = eng.store.flat.cpu().numpy()
    init = synth_flat(eng, cfg, sizes, W.SEED)
    d = np.abs(r0["flat"] - ref)
    # test_dp_gpu._check_trainstep's bars (AdamW's normalised update is ~lr per step whatever the gradient's size: elements whose
    # gradient is rounding noise may differ by up to 2 lr per step between two runs; everything else agrees to a small fraction of
    # lr), with every group's own lr
    lr_of = np.zeros(eng.store.n_flat)
    for g in ts.param_groups:
        idx = np.concatenate([np.arange(o, o + n) for o, n, _ in (eng.store.slots[k] for k in g["names"])])
        lr_g = 1e-3 * g["lr_mult"]
        lr_of[idx] = lr_g
        assert d[idx].max() <= 2.0 * W.STEPS * lr_g + (1e-7 if lr_g else 0.0), (g["lr_mult"], g["weight_decay"], d[idx].max())
        if lr_g:
            assert np.abs(ref - init)[idx].mean() > 0.5 * lr_g                     # (the group did move, at its own rate)
        else:
            assert idx.size > 0 and np.array_equal(r0["flat"][idx], init[idx])     # held still: the initial bits, on the ranks too
    live = lr_of > 0
    assert np.mean(d[live] > 0.05 * lr_of[live]) < 0.02, (np.mean(d[live] > 0.05 * lr_of[live]), d.max())
