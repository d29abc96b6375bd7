"""GPU, two rank processes on one GPU over gloo (as tests/test_dp_gpu.py): length-aware sharding under the real data-parallel step.

The plan itself is checked on the CPU (tests/test_length_sharding_cpu.py).  Here: (1) with the weights held fixed the sharding only
moves work between ranks -- every case is seen once and its loss has the same bits under window = 1, under window = 2 and in one
process; (2) a real run with accumulate = 2, window = 2 and hipGraph replay keeps the replicas bit-identical, closes every
accumulation window at the epoch's end, and dp.StepTimer reports one time per step and rank (two ranks sharing a GPU: the times
themselves mean nothing and are not looked at)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "length_sharding_worker.py")


def _run_ranks(mode, tmp_path, world=2, timeout=300):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = str(s.getsockname()[1])
    s.close()
    outs = [str(tmp_path / f"{mode}_{r}.npz") for r in range(world)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    procs = [subprocess.Popen([sys.executable, WORKER, mode, str(r), str(world), port, outs[r]], env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(world)]
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o.decode()[-3000:])
    assert all(p.returncode == 0 for p in procs), "\n----\n".join(logs)
    res = []
    for o in outs:
        with np.load(o) as z:
            res.append({k: z[k] for k in z.files})
    return res


def test_sharding_only_moves_work_between_ranks(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import length_sharding_worker as W
    from modaltune_amd import dp
    res = _run_ranks("fixed", tmp_path)
    n = len(W.LENGTHS)
    per_case = {}
    for window in (1, 2):
        seen = {}
        for r, z in enumerate(res):
            assert z[f"order{window}"].tolist() == dp.shard_indices(n, 2, r, seed=W.SAMPLER_SEED, lengths=W.LENGTHS, window=window)
            for i, loss in zip(z[f"order{window}"].tolist(), z[f"loss{window}"].tolist()):
                assert i not in seen, (window, i, "seen twice")
                seen[i] = loss
        assert sorted(seen) == list(range(n))                                   # across the ranks every case exactly once
        per_case[window] = [seen[i] for i in range(n)]
    assert [z["order1"].tolist() for z in res] != [z["order2"].tolist() for z in res], "both shardings dealt alike: the test lost its point"
    for z in res:
        assert int(z["held"]) == 1 and int(z["sharded"]) == 1 and int(z["collectives"]) > 0 and int(z["steps"]) == n      # 2 epochs x 4 steps, lr = 0
    assert np.isfinite(per_case[1]).all() and len(set(per_case[1])) == n
    assert np.array(per_case[1]).tobytes() == np.array(per_case[2]).tobytes(), (per_case[1], per_case[2])
    # one process, the same eight cases
    eng, ts, cases = W.build(deterministic=True, lr=0.0)
    one = [float(ts.step(*c)) for c in cases]
    torch.cuda.synchronize()
    assert np.array(one).tobytes() == np.array(per_case[1]).tobytes(), (one, per_case[1])


def test_two_rank_training_with_length_windows_accumulation_and_replay(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import length_sharding_worker as W
    from modaltune_amd import dp
    a, b = res = _run_ranks("train", tmp_path)
    n = len(W.LENGTHS)
    for r, z in enumerate(res):
        assert int(z["verified"]) == 2                                          # verify_replicas() passed behind both epochs
        assert z["window_pos"].tolist() == [0, 0]
        assert int(z["steps"]) == 4 and int(z["sharded"]) == 1                  # 2 epochs x 4 slides per rank / accumulate 2
        seen, again = set(), 0
        for e in range(2):
            want = dp.shard_indices(n, 2, r, epoch=e, seed=W.SAMPLER_SEED, lengths=W.LENGTHS, window=2, accumulate=2)
            assert z["orders"][e].tolist() == want
            for k, i in enumerate(want):         # capture_after = 1: a (case, window role) met again is captured and replayed
                again += (i, k % 2) in seen
                seen.add((i, k % 2))
        assert int(z["replays"]) == again >= 1, (int(z["replays"]), again)
        # the timer's report: plan_stats' shape, one time per step and rank, the same table on both ranks
        assert z["times"].shape == (2, 2, 4) and np.isfinite(z["times"]).all() and (z["times"] > 0).all()
        assert z["report_steps"].tolist() == [2, 2] and ((z["efficiency"] > 0) & (z["efficiency"] <= 1)).all() and (z["gap"] >= 0).all()
    assert np.array_equal(a["times"], b["times"])
    for e in range(2):
        assert sorted(a["orders"][e].tolist() + b["orders"][e].tolist()) == list(range(n))
    assert np.array_equal(a["flat"], b["flat"]) and np.isfinite(a["flat"]).all()      # bit-identical replicas
    assert float(a["moved"]) > 1e-4                                                    # (the weights did move)
