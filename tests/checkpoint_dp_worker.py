"""Rank process of tests/test_checkpoint_dp_gpu.py: `python tests/checkpoint_dp_worker.py MODE RANK WORLD PORT OUT CKPT` (gloo, every
rank on GPU 0, the L = 150 toy configuration of tests/accum_clip_dp_worker.py, deterministic engine through MT_DETERMINISTIC=1).

    save    two steps, state_dict() on both ranks (rank 0 writes CKPT), two more steps
    resume  fresh ranks on other weights: load CKPT, two steps
    checks  state_dict() inside an open window; verify_replicas() before and after rank 1 moves one parameter by one ulp; the same under
            verify_every = 2

Large buffers leave the process as sha256 digests (the comparisons are bit-identity claims), written as JSON to OUT."""
import hashlib
import json
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import accum_clip_dp_worker as W  # noqa: E402
from modaltune_amd import dp, synth  # noqa: E402


def build(seed=W.SEED, **ts_kw):
    from modaltune_amd.engine import Engine
    from modaltune_amd.trainer import TrainStep
    sizes = synth.toy_group_sizes()
    eng = Engine(W.cfg(), sizes, "cuda")
    assert eng.deterministic
    state = synth.synth_state_dict(W.cfg(), sizes, W.SEED)
    if seed != W.SEED:          # other TRAINABLE weights; the frozen backbone is not part of a checkpoint (the resuming run brings it)
        other = synth.synth_state_dict(W.cfg(), sizes, seed)
        for k in synth.trainable_keys(W.cfg(), sizes):
            state[k] = other[k]
    eng.load_state_dict(state)
    ts = TrainStep(eng, lr=W.LR, weight_decay=0.01, **ts_kw)
    ts.set_projector(synth.projector_state(W.SEED))
    return eng, ts, sizes


def digest(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def flatten(sd, prefix=""):
    """{path: digest or value} of a checkpoint dict."""
    out = {}
    for k, v in sd.items():
        key = f"{prefix}{k}"
        if isinstance(v, dict):
            out.update(flatten(v, key + "/"))
        elif torch.is_tensor(v):
            out[key] = [list(v.shape), str(v.dtype), digest(v)]
        else:
            out[key] = v if not isinstance(v, tuple) else list(v)
    return out


def end_state(eng, ts, losses):
    if eng.store.sync is not None:
        eng.store.sync()
    torch.cuda.synchronize()
    pieces = ts.reducer.adam_pieces(eng.store.n_flat)
    return {"flat": digest(eng.store.flat), "m_pieces": digest(torch.cat([ts.m[o:o + k] for o, k in pieces])),
            "v_pieces": digest(torch.cat([ts.v[o:o + k] for o, k in pieces])), "scale": float(ts.scale), "tracker": int(ts.tracker),
            "step_dev": int(ts.step_dev), "losses": losses, "sharded": bool(ts.reducer.sharded), "pieces": len(pieces)}


def save(rank, ckpt):
    eng, ts, sizes = build()
    dp.broadcast_params_(eng.store.flat)
    slides = [W.slide(2 * rank + i, sizes) for i in range(2)]
    losses = []
    for i in range(2):
        ts.step(*slides[i])
        losses.append(float(ts.loss))
    # the other rank's shard of the first reduce-scattered range: this rank's AdamW never wrote it
    o, s, _ = ts.reducer._rs[0]
    other = slice(o + (1 - rank) * s, o + (2 - rank) * s)
    before = ts.m[other].clone()
    sd = ts.state_dict()
    rec = {"sd": flatten(sd), "gather_moved_m": not torch.equal(before, ts.m[other]), "m_other_was_zero": not bool(before.any()),
           "world": sd["world"]}
    if rank == 0:
        torch.save(sd, ckpt)
    del sd
    for i in range(2):
        ts.step(*slides[i])
        losses.append(float(ts.loss))
    rec["end"] = end_state(eng, ts, losses[2:])
    return rec


def resume(rank, ckpt):
    eng, ts, sizes = build(seed=W.SEED + 1)
    slides = [W.slide(2 * rank + i, sizes) for i in range(2)]
    ts.load_state_dict(torch.load(ckpt, map_location="cpu", weights_only=True))
    losses = []
    for i in range(2):
        ts.step(*slides[i])
        losses.append(float(ts.loss))
    return {"end": end_state(eng, ts, losses)}


def _replicated_index(eng, ts):
    """An element of an all-reduced bucket (outside every rank's shard) whose value sits mid-binade (|x| >= 1e-2, mantissa nearest 1.5):
    one ulp more stays one ulp more through the following AdamW updates (lr 1e-3: no binade is crossed)."""
    o, n = ts.reducer.buckets[0][0]
    x = eng.store.flat[o:o + n]
    mant = torch.frexp(x.abs())[0] * 2.0
    score = (mant - 1.5).abs() + (x.abs() < 1e-2).float() * 10.0
    return o + int(score.argmin())


def _bump(eng, i):
    v = eng.store.flat[i:i + 1]
    v.copy_(torch.nextafter(v, torch.full_like(v, float("inf"))))


def _raises(fn, exc=RuntimeError):
    try:
        fn()
    except exc as e:
        return str(e)
    return None


def checks(rank):
    rec = {}
    # -- state_dict() inside an open window
    eng, ts, sizes = build(accumulate=2)
    dp.broadcast_params_(eng.store.flat)
    slides = [W.slide(2 * rank + i, sizes) for i in range(2)]
    ts.step(*slides[0])
    rec["window_error"] = _raises(ts.state_dict)
    rec["window_pos"] = ts.window_pos
    ts.finish_window()
    # -- verify_replicas() before and after one ulp on rank 1
    eng, ts, sizes = build()
    dp.broadcast_params_(eng.store.flat)
    for i in range(2):
        ts.step(*slides[i])
    rec["canary_clean"] = _raises(ts.verify_replicas)
    if eng.store.sync is not None:
        eng.store.sync()
    idx = _replicated_index(eng, ts)
    mine = [(o + rank * s, o + (rank + 1) * s) for o, s, _ in ts.reducer._rs]
    rec["index_outside_own_shard"] = not any(a <= idx < b for a, b in mine)
    if rank == 1:
        _bump(eng, idx)
    rec["canary_perturbed"] = _raises(ts.verify_replicas)
    # -- the same perturbation under verify_every = 2: the first boundary is not checked, the second is
    eng, ts, sizes = build(verify_every=2)
    dp.broadcast_params_(eng.store.flat)
    if rank == 1:
        _bump(eng, _replicated_index(eng, ts))
    rec["every_step1"] = _raises(lambda: ts.step(*slides[0]))
    rec["every_step2"] = _raises(lambda: ts.step(*slides[1]))
    if eng.store.sync is not None:
        eng.store.sync()
    torch.cuda.synchronize()
    return rec


if __name__ == "__main__":
    mode, rank, world, port, out, ckpt = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5], sys.argv[6]
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", port
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        rec = {"save": lambda: save(rank, ckpt), "resume": lambda: resume(rank, ckpt), "checks": lambda: checks(rank)}[mode]()
        with open(out, "w") as f:
            json.dump(rec, f)
    finally:
        dist.destroy_process_group()
