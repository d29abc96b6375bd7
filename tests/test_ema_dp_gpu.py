"""GPU, two rank processes on one GPU over gloo (the pattern of tests/test_checkpoint_dp_gpu.py; never more than two at a time): the
EMA of the trainable weights under the sharded last bucket.  A rank averages its own shard only; state_dict() and ema_weights()
complete the average.  Every comparison is a bit-identity claim (64-bit checksums, sha256 digests, integers): no tolerance.  Each rank
process has its own time limit and a non-zero exit fails the test at once."""
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
WORKER = os.path.join(ROOT, "tests", "ema_dp_worker.py")


def _run_ranks(tmp_path, world=2, timeout=300):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = str(s.getsockname()[1])
    s.close()
    outs = [str(tmp_path / f"rank{r}.json") for r in range(world)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"), MT_DETERMINISTIC="1",
               MT_DP_SHARD_LAST="1")
    logs = [open(str(tmp_path / f"rank{r}.log"), "wb") for r in range(world)]
    procs = [subprocess.Popen([sys.executable, WORKER, str(r), str(world), port, outs[r]], env=env, stdout=logs[r],
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


def test_two_ranks_complete_the_average_where_it_is_read(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    a, b = _run_ranks(tmp_path)
    for r in (a, b):
        assert r["sharded"] and r["pieces"] > 1 and r["step_dev"] == 3
        # between steps a rank holds its own shard's average only: no collective per step for the average
        assert r["other_shard_was_stale"] and r["own_shard_follows_the_host"]
        # state_dict(): the checksum of the completed average -- the device's, the host recurrence's and the file's are one value
        assert r["ema_checksum"] == r["ema_checksum_device"] == r["ema_checksum_host"]
        assert r["sd_ema_is_the_host_recurrence"] and r["sd_ema_differs_from_the_parameters"] and r["decay_warmup"] == [0.9, True]
        assert r["collectives_in_state_dict"] > 0
        # ema_weights(): inside, the parameter buffer holds the complete average; behind it everything is back
        assert r["flat_inside"] == r["ema_checksum"] and r["flat_after"] == r["flat_before"] != r["flat_inside"]
        assert r["ema_after"] == r["ema_checksum"]
        assert r["step_inside"] is not None and r["step_inside"].startswith("step() inside ema_weights()"), r["step_inside"]
        assert r["step_end"] == 4
    assert a["ema_checksum"] == b["ema_checksum"]
    assert a["flat_before"] == b["flat_before"] and a["flat_inside"] == b["flat_inside"] and a["flat_after"] == b["flat_after"]
    assert a["flat_end"] == b["flat_end"]
