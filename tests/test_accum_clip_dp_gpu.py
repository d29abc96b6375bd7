"""GPU, two rank processes on one GPU over gloo (as tests/test_dp_gpu.py; never more than two): gradient accumulation and clipping
under the data-parallel step.  accumulate = 2 with clipping on each rank, for every dp_schedule and both forms of the reducer's last
bucket (reduce-scattered / all-reduced): micro-steps issue no collective, the boundary issues them all, every rank forms the same
clip coefficient bits and ends with the same parameters, and the first window's reduced gradient equals ONE process running the same
four slides with accumulate = 4 (the default-engine bar of tests/test_accum_clip_gpu.py, per tensor: max |delta| <= 1e-3 of the tensor's
own max |expected| + 1e-6 of the largest entry of the expected gradient; that file's docstring has the reasoning)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "accum_clip_dp_worker.py")
BAR, FLOOR = 1e-3, 1e-6
_single = {}


def _run_ranks(tmp_path, env_extra, world=2, timeout=600):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = str(s.getsockname()[1])
    s.close()
    outs = [str(tmp_path / f"rank{r}.npz") for r in range(world)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"), **env_extra)
    procs = [subprocess.Popen([sys.executable, WORKER, str(r), str(world), port, outs[r]], env=env, stdout=subprocess.PIPE,
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
    for o in outs:          # (materialised once: indexing an NpzFile re-reads the whole array on every access)
        with np.load(o) as z:
            res.append({k: z[k] for k in z.files})
    return res


def _single_process_window():
    """The same four slides through ONE process with accumulate = 4 (computed once): gradient sum / scale, norm, slots."""
    if not _single:
        import accum_clip_dp_worker as W
        eng, ts, sizes = W.build(accumulate=4)
        ts.split_min_patches = 1 << 30
        for i in range(W.SLIDES):
            ts.step(*W.slide(i, sizes))
        torch.cuda.synchronize()
        assert int(ts.step_dev) == 1 and float(ts.clip_coef) < 1.0
        _single.update(grad=(eng.store.flat_grad.double() / float(ts.grad_scale)).cpu().numpy(), norm=float(ts.grad_norm),
                       slots={k: (o, n) for k, (o, n, _) in eng.store.slots.items()})
    return _single


@pytest.mark.parametrize("shard_last", [True, False], ids=["sharded", "allreduced"])
@pytest.mark.parametrize("schedule", ["groups_joined", "groups_exposed", "batched"])
def test_two_rank_windows_accumulate_clip_and_stay_identical(tmp_path, schedule, shard_last):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import accum_clip_dp_worker as W
    res = _run_ranks(tmp_path, {"MT_SPLIT_PASSES": "force", "MT_DP_SCHEDULE": schedule, "MT_DP_SHARD_LAST": "1" if shard_last else "0"})
    for r in res:
        assert int(r["sharded"]) == int(shard_last) and str(r["schedule"]) == schedule and int(r["window_pos"]) == 0
        assert int(r["split"]) == int(schedule != "batched")
        assert r["micro_collectives"].tolist() == [0] * W.WINDOWS, r["micro_collectives"]      # no collective inside a window
        assert all(c >= 4 for c in r["boundary_collectives"]), r["boundary_collectives"]        # (at least one per bucket)
        assert r["steps"].tolist() == [1, 2, 3]
        assert r["replayed"].tolist() == [0, 2, 2]          # eager window, capturing window, replayed window: both positions
    a, b = res
    for w in range(W.WINDOWS):
        assert a["clip"][w].tobytes() == b["clip"][w].tobytes(), (w, a["clip"][w], b["clip"][w])      # norm, coefficient, scale / coef
        assert np.array_equal(a["flat"][w], b["flat"][w]), (w, "the ranks' parameters differ")
        assert 0.0 < a["clip"][w][1] < 1.0 and np.isfinite(a["flat"][w]).all()
    assert not np.array_equal(a["flat"][0], a["flat"][2])
    # window 0 against one process with accumulate = 4: each rank on the elements whose reduced gradient it holds
    one = _single_process_window()
    worst, top = (0.0, None), float(np.abs(one["grad"]).max())
    for r in res:
        for k, (o, n) in one["slots"].items():
            held = r["held"][o:o + n]
            d = np.abs(r["grad0"][o:o + n] - one["grad"][o:o + n])[held].max() if held.any() else 0.0
            own = float(np.abs(one["grad"][o:o + n]).max())
            worst = max(worst, (d / top, k))
            assert top > 0 and d <= BAR * own + FLOOR * top, (k, d, own, top)
    norm_dp = float(a["clip"][0][0])
    print(f"accum-clip dp {schedule}/{'sharded' if shard_last else 'allreduced'}: worst max|delta| / largest entry = {worst[0]:.3e} ({worst[1]}); "
          f"grad_norm {norm_dp:.9g} against one process {one['norm']:.9g}")
    assert abs(norm_dp - one["norm"]) <= BAR * one["norm"]
    assert any(not r["held"].all() for r in res) == shard_last
