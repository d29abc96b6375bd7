"""GPU, two rank processes on one GPU over gloo (the pattern of tests/test_accum_clip_dp_gpu.py; never more than two at a time):
checkpoint / resume of the fused train step under the sharded last bucket, and the replica canary.  Every comparison is a bit-identity
claim (sha256 digests of the buffers, integers, exact floats): no tolerance.  Each rank process has its own time limit and a
non-zero exit fails the test at once."""
import json
import os
import socket
import subprocess
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "checkpoint_dp_worker.py")


def _run_ranks(tmp_path, mode, world=2, timeout=300):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = str(s.getsockname()[1])
    s.close()
    outs = [str(tmp_path / f"{mode}_rank{r}.json") for r in range(world)]
    ckpt = str(tmp_path / "step2.pt")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"), MT_DETERMINISTIC="1",
               MT_DP_SHARD_LAST="1")
    logs = [open(str(tmp_path / f"{mode}_rank{r}.log"), "wb") for r in range(world)]
    procs = [subprocess.Popen([sys.executable, WORKER, mode, str(r), str(world), port, outs[r], ckpt], env=env, stdout=logs[r],
                              stderr=subprocess.STDOUT) for r in range(world)]
    deadline = time.monotonic() + timeout          # each rank's own limit (they start together)
    try:
        while any(p.poll() is None for p in procs):
            for p in procs:
                try:
                    p.wait(timeout=0.5)
                except subprocess.TimeoutExpired:
                    pass
            # stop at the first failure (the other rank would wait for a collective that never comes) and at the time limit
            if any(p.poll() not in (None, 0) for p in procs) or time.monotonic() > deadline:
                break
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
        for f in logs:
            f.close()
    tails = [open(f.name, "rb").read().decode(errors="replace")[-3000:] for f in logs]
    assert all(p.returncode == 0 for p in procs), "\n----\n".join(tails)
    return [json.load(open(o)) for o in outs]


def test_two_ranks_resume_to_the_same_bits_under_the_sharded_bucket(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    a, b = _run_ranks(tmp_path, "save")
    assert a["end"]["sharded"] and b["end"]["sharded"] and a["end"]["pieces"] > 1
    # state_dict() is a collective that returns the same complete dict on every rank
    assert a["sd"].keys() == b["sd"].keys() and len(a["sd"]) > 700
    diff = [k for k in a["sd"] if a["sd"][k] != b["sd"][k]]
    assert not diff, diff[:5]
    assert a["world"] == 2 and a["sd"]["window"] is None
    # ... and the gather did something: before it, a rank held nothing (zeros) where the other rank's AdamW keeps its moments
    for r in (a, b):
        assert r["gather_moved_m"] and r["m_other_was_zero"]
    assert a["end"]["flat"] == b["end"]["flat"] and a["end"]["step_dev"] == 4
    assert a["end"]["m_pieces"] != b["end"]["m_pieces"]          # (each rank compares its own shards)
    resumed = _run_ranks(tmp_path, "resume")
    for saved, res in zip((a, b), resumed):
        assert res["end"] == saved["end"], (res["end"], saved["end"])


def test_open_window_is_refused_and_the_canary_sees_one_ulp_on_one_rank(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    res = _run_ranks(tmp_path, "checks")
    for r in res:
        assert r["window_pos"] == 1 and r["window_error"] is not None and "finish_window()" in r["window_error"], r["window_error"]
        assert r["canary_clean"] is None and r["index_outside_own_shard"] is True
        assert r["canary_perturbed"] is not None and r["canary_perturbed"].startswith("replicas diverged"), r["canary_perturbed"]
        assert r["every_step1"] is None          # the first boundary is not checked
        assert r["every_step2"] is not None and r["every_step2"].startswith("replicas diverged"), r["every_step2"]
