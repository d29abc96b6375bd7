"""bench.py's own contract: a plain run prints the headline line and nothing that needs runs of its own (those are behind --full);
--dump-outputs writes what the last timed step computed, as float32 .npy files of bounded size, at seeded sample indices."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "roofline_kernels", "roofline_worst", "mfma_peak_measured", "kernel_ms_per_step", "token_side_in_graph",
             "pcie_inclusive", "sizes", "module_api", "titan", "cpu_baseline")


def test_dump_outputs_float32_and_a_seeded_sample_of_long_buffers(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_VALUES", 1000)
    long = torch.arange(5000, dtype=torch.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"loss": torch.tensor([0.25]), "logits": torch.ones(3, 4, dtype=torch.float16), "params": long})
    a = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in ("loss", "logits", "params")}
    assert all(v.dtype == np.float32 for v in a.values())
    assert a["loss"].tolist() == [0.25] and a["logits"].shape == (3, 4)
    p = a["params"]
    assert p.shape == (1000,) and np.all(np.diff(p) > 0) and len(np.unique(p)) == 1000      # sorted, distinct indices
    assert np.array_equal(p, np.load(tmp_path / "b" / "params.npy"))                        # the same sample on every run


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out_dir = tmp_path / "out"
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None); env.pop("RANK", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--patches", "1024", "--steps", "4", "--warmup", "3",
                        "--dump-outputs", str(out_dir)], env=env, capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    out = json.loads([l for l in p.stdout.decode().splitlines() if l.startswith("{")][-1])
    assert out["steps"] == 4 and out["ms_per_step"] > 0 and abs(out["value"] * out["ms_per_step"] - 1e3) < 1e-6 * 1e3
    assert out["unit"] == "slides/s" and out["higher_is_better"] is True and out["dtype"] == "f16" and out["skipped_steps"] == 0
    assert out["launch"] == "hipGraph replay" and out["graph_replays"] >= 4
    assert not [k for k in FULL_ONLY if k in out]
    files = sorted(os.listdir(out_dir))
    assert files == ["grads.npy", "logits.npy", "loss.npy", "params.npy"]
    arrs = {f: np.load(out_dir / f) for f in files}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 * 2 ** 20
    assert abs(float(arrs["loss.npy"].reshape(-1)[0]) - out["loss"]) <= 1e-6 * abs(out["loss"])
    assert arrs["logits.npy"].shape[0] == 3 and np.abs(arrs["grads.npy"]).max() > 0
