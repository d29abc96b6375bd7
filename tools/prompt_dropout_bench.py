"""What the softmax dropout costs in the prompt self-attention kernels: mt_token_mha_fwd / _bwd against their _drop forms, HIP events
around N back-to-back launches on one stream (so the figure is the kernel's own time plus the launch gap, the same for both forms), the
median of several such rounds, in microseconds per launch.

    python tools/prompt_dropout_bench.py [--heads 12 --hd 16 --T 65 --B 3 --p 0.25 --launches 200 --rounds 7]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from modaltune_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--hd", type=int, default=16)
    ap.add_argument("--T", type=int, default=65)
    ap.add_argument("--B", type=int, default=3)
    ap.add_argument("--p", type=float, default=0.25)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    B, T, heads, E = a.B, a.T, a.heads, a.heads * a.hd
    g = torch.Generator(device="cuda").manual_seed(0)
    q, k, v, do = (torch.randn(B, T, E, device="cuda", generator=g) for _ in range(4))
    out, dq, dk, dv = (torch.empty(B, T, E, device="cuda") for _ in range(4))
    probs = torch.empty(B, heads, T, T, device="cuda")
    rng = torch.tensor([1, 0, 1, 0], dtype=torch.int32, device="cuda")
    spec = ops.dropout_spec(rng, 400, a.p)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        us = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / a.launches)
        us.sort()
        return {"median_us": round(us[len(us) // 2], 2), "min_us": round(us[0], 2), "max_us": round(us[-1], 2)}
    res = {"shape": f"{heads}x{a.hd} T={T} B={B} p={a.p}", "launches": a.launches, "rounds": a.rounds}
    for name, drop in (("plain", None), ("drop", spec)):
        res["fwd_" + name] = timed(lambda: ops.token_mha_fwd(q, k, v, out, probs, B, T, E, heads, drop=drop))
        res["bwd_" + name] = timed(lambda: ops.token_mha_bwd(q, k, v, probs, do, dq, dk, dv, B, T, E, heads, drop=drop))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
