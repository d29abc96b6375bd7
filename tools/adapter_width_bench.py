"""Train-step time and the adapter attention kernels' share of it across adapter widths (`cffn_ratio`, `num_heads`).

    python tools/adapter_width_bench.py [--full-width] [steps=10] [L ...=10000 4096]

For each (E, heads) of the six pairs of tests/test_adapter_width_gpu.py -- head dims 16 / 32 / 64 at E = 192 and 384 -- and the full
width E = 768 at 12 x 64 / 24 x 32 (with_cffn=False: no q_proj / output_proj / FFN wrap)
(--full-width: the shipped 12 x 16 and the two full-width rows only) -- and each bag length: the median ms of a hipGraph-replayed train step (TrainStep.step_graphed, 3 task passes, dropout off), and from ONE eager step
with HIP events around every launch (ops.TIMER) the time of the four templated patch-side kernels (inject_attn_fwd / bwd,
extract_attn_fwd / bwd: 3 / 3 / 5 / 5 launches per step), their share of the eager step's kernel time, and the HBM rate each achieves
counted from the tensor sizes (patch-side operands read once, outputs written once; the token side is noise at these lengths).
`gemm_tn_ms` is the time of the weight-gradient products (mt_gemm_tn_f16) of that step.  Prints one JSON line per (pair, L) and a table."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from modaltune_amd import ops, synth  # noqa: E402
from modaltune_amd.config import ModelConfig  # noqa: E402
from modaltune_amd.engine import Engine  # noqa: E402
from modaltune_amd.trainer import TrainStep  # noqa: E402

# (E, heads, with_cffn)
FULL = [(768, 12, False), (768, 24, False)]
PAIRS = [(192, 12, True), (192, 6, True), (192, 3, True), (384, 24, True), (384, 12, True), (384, 6, True)] + FULL
argv = [a for a in sys.argv[1:] if a != "--full-width"]
if "--full-width" in sys.argv:
    PAIRS = [(192, 12, True)] + FULL
KERNELS = ["inject_attn_fwd", "inject_attn_bwd", "extract_attn_fwd", "extract_attn_bwd"]
steps = int(argv[0]) if argv else 10
lengths = [int(a) for a in argv[1:]] or [10000, 4096]
dev = torch.device("cuda", 0)
B = 3


def bytes_per_launch(name, L, E, heads):
    M = B * L
    if name == "inject_attn_fwd":       # q in, a + lse out
        return M * (2 * E + 2 * E + 4 * heads)
    if name == "inject_attn_bwd":       # q, a, da, lse in, dq out
        return M * (4 * 2 * E + 4 * heads)
    if name == "extract_attn_fwd":      # k | v in
        return M * 2 * 2 * E
    return M * 2 * 2 * 2 * E            # extract_attn_bwd: k | v in, dk | dv out


rows = []
for L in lengths:
    for E, heads, cffn in PAIRS:
        cfg = ModelConfig(cffn_ratio=E / 768, with_cffn=cffn, num_heads=heads, dropout=0.0, drop_path_rate=0.0)
        assert cfg.adapter_dim == E and (cffn or E == 768)
        sizes = synth.toy_group_sizes(6)
        eng = Engine(cfg, sizes, dev)
        eng.load_state_dict(synth.synth_state_dict(cfg, sizes, seed=0))
        ts = TrainStep(eng)
        ts.set_projector(synth.projector_state(0))
        inp = synth.synth_inputs(L, sizes, seed=1000, grid=128 if L <= 128 * 128 else 512)
        x = torch.from_numpy(inp["x"]).to(dev)
        genes = [torch.from_numpy(a).to(dev) for a in inp["genes"]]
        text = torch.from_numpy(inp["text"]).to(dev)
        for _ in range(4):                      # eager visits, capture, first replay
            ts.step_graphed(x, inp["coords"], genes, text)
        torch.cuda.synchronize()
        r0, ms = ts.graph_replays, []
        for _ in range(steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ts.step_graphed(x, inp["coords"], genes, text)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        assert ts.graph_replays == r0 + steps, "a timed step did not replay its captured graph"
        ops.TIMER = {}
        ts.split_min_patches = 1 << 30          # one batched pass: every launch on one stream
        ts.step(x, inp["coords"], genes, text, update=False)
        torch.cuda.synchronize()
        kt = {k: [e0.elapsed_time(e1) for e0, e1 in v] for k, v in ops.TIMER.items()}
        ops.TIMER = None
        total = sum(sum(v) for v in kt.values())
        rec = {"patches": L, "E": E, "heads": heads, "head_dim": E // heads, "with_cffn": cffn, "gemm_tn_ms": round(sum(sum(v) for k, v in kt.items() if k.startswith("gemm_tn")), 4),
               "ms_per_step": round(statistics.median(ms), 3),
               "ms_min_max": [round(min(ms), 3), round(max(ms), 3)], "eager_kernel_ms": round(total, 3)}
        ad = 0.0
        for k in KERNELS:
            t = kt.get(k, [])
            ad += sum(t)
            rec[k] = {"launches": len(t), "ms_per_step": round(sum(t), 4),
                      "gb_per_s": round(bytes_per_launch(k, L, E, heads) * len(t) / (sum(t) * 1e-3) / 1e9, 1) if t else None}
        rec["adapter_attn_ms"] = round(ad, 4)
        rec["adapter_attn_share"] = round(ad / total, 4)
        rows.append(rec)
        print(json.dumps(rec), flush=True)
        del ts, eng
        torch.cuda.empty_cache()

print(f"{'L':>6} {'E':>4} {'cffn':>5} {'heads x d':>9} {'ms/step':>8} {'tn ms':>7} {'attn ms':>8} {'share':>6}  " + "  ".join(f"{k + ' ms GB/s':>26}" for k in KERNELS))
for r in rows:
    print(f"{r['patches']:>6} {r['E']:>4} {str(r['with_cffn']):>5} {str(r['heads']) + ' x ' + str(r['head_dim']):>9} {r['ms_per_step']:>8.2f} "
          f"{r['gemm_tn_ms']:>7.3f} {r['adapter_attn_ms']:>8.3f} "
          f"{100 * r['adapter_attn_share']:>5.1f}%  " + "  ".join(f"{r[k]['ms_per_step']:>17.4f} {r[k]['gb_per_s']:>8}" for k in KERNELS))
