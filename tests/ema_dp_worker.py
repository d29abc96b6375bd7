"""Rank process of tests/test_ema_dp_gpu.py: `python tests/ema_dp_worker.py RANK WORLD PORT OUT` (gloo, every rank on GPU 0, the
L = 150 toy configuration of tests/accum_clip_dp_worker.py, deterministic engine through MT_DETERMINISTIC=1, the sharded last bucket).

Three steps with TrainStep(ema_decay=0.9, ema_warmup=True); after each the complete parameter buffer is kept.  Then state_dict() (a
collective: the shards of the average are gathered) against the host recurrence of tests/ema_ref.py over those snapshots, and
ema_weights() with the checksums of the parameter buffer before, inside and behind it.  Written as JSON to OUT."""
import json
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import accum_clip_dp_worker as W  # noqa: E402
import checkpoint_dp_worker as CW  # noqa: E402
from ema_ref import ema_ref  # noqa: E402
from modaltune_amd import checkpoint, dp  # noqa: E402

DECAY, WARMUP, STEPS = 0.9, True, 3


def checksum(ts, t) -> int:
    out = torch.empty(1, dtype=torch.int64, device="cuda")
    ts._checksum_into(t, out)
    return checkpoint.as_unsigned(int(out))


def main(rank):
    eng, ts, sizes = CW.build(ema_decay=DECAY, ema_warmup=WARMUP)
    st = eng.store
    dp.broadcast_params_(st.flat)
    ts.ema_reset()                                 # the average starts at the broadcast parameters
    slides = [W.slide(2 * rank + i, sizes) for i in range(2)]
    host = st.flat.cpu().numpy().copy()
    init = st.flat.clone()
    for i in range(STEPS):
        ts.step(*slides[i % 2])
        st.sync()                                  # the parameter all-gather: the complete buffer, the same on every rank
        torch.cuda.synchronize()
        host = ema_ref(host, st.flat.cpu().numpy(), DECAY, WARMUP, i + 1)
    host = torch.from_numpy(host)
    # the other rank's shard of the first reduce-scattered range: this rank's AdamW never averaged it
    o, s, _ = ts.reducer._rs[0]
    other, mine = slice(o + (1 - rank) * s, o + (2 - rank) * s), slice(o + rank * s, o + (rank + 1) * s)
    rec = {"sharded": bool(ts.reducer.sharded), "pieces": len(ts.reducer.adam_pieces(st.n_flat)), "step_dev": int(ts.step_dev),
           "other_shard_was_stale": bool(torch.equal(ts.ema[other], init[other])),
           "own_shard_follows_the_host": bool(torch.equal(ts.ema[mine].cpu().view(torch.int32), host[mine].view(torch.int32)))}
    collectives = ts.reducer.collectives
    sd = ts.state_dict()
    rec["collectives_in_state_dict"] = ts.reducer.collectives - collectives
    rec["ema_checksum"] = sd["checksums"]["ema"]
    rec["ema_checksum_device"] = checksum(ts, ts.ema)
    rec["ema_checksum_host"] = checkpoint.checksum64_reference(host)
    flat_sd, decay, warmup = checkpoint.unpack_ema(sd["ema"], st.slots, st.n_flat)
    rec["sd_ema_is_the_host_recurrence"] = bool(torch.equal(flat_sd.view(torch.int32), host.view(torch.int32)))
    rec["sd_ema_differs_from_the_parameters"] = not torch.equal(flat_sd, st.flat.cpu())
    rec["decay_warmup"] = [decay, warmup]
    rec["flat_before"] = checksum(ts, st.flat)
    with ts.ema_weights():
        rec["flat_inside"] = checksum(ts, st.flat)
        rec["step_inside"] = CW._raises(lambda: ts.step(*slides[0]))
    rec["flat_after"] = checksum(ts, st.flat)
    rec["ema_after"] = checksum(ts, ts.ema)
    ts.step(*slides[1])                            # training goes on behind the context, on both ranks
    st.sync()
    torch.cuda.synchronize()
    rec["flat_end"], rec["step_end"] = CW.digest(st.flat), int(ts.step_dev)
    return rec


if __name__ == "__main__":
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", port
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        rec = main(rank)
        with open(out, "w") as f:
            json.dump(rec, f)
    finally:
        dist.destroy_process_group()
