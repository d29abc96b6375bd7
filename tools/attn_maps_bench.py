"""Added cost of the adapter attention maps on the eval forward (EmbeddingExtractor, 3 task passes, hipGraph replay): the same slide
timed without a request and with all ten sites, in alternating blocks of replays, with HIP events around each call.

    python tools/attn_maps_bench.py [L=10000] [steps=20]

Prints one JSON line: median ms per slide of both, the difference, and the bytes the ten map kernels move (counted from the tensor
sizes: patch-side operands read once per site, maps written once)."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from modaltune_amd import synth  # noqa: E402
from modaltune_amd.config import ModelConfig, attention_sites  # noqa: E402
from modaltune_amd.engine import Engine  # noqa: E402
from modaltune_amd.evaluate import EmbeddingExtractor  # noqa: E402

L = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
dev = torch.device("cuda", 0)
cfg = ModelConfig()
sizes = synth.toy_group_sizes(6)
eng = Engine(cfg, sizes, dev)
eng.load_state_dict(synth.synth_state_dict(cfg, sizes, seed=0))
plain = EmbeddingExtractor(eng)
maps = EmbeddingExtractor(eng, attention=True)
inp = synth.synth_inputs(L, sizes, seed=1000, grid=128 if L <= 128 * 128 else 512)
x = torch.from_numpy(inp["x"]).to(dev).half().reshape(L, -1).contiguous()
genes = [torch.from_numpy(a).to(dev) for a in inp["genes"]]
times = {"plain": [], "maps": []}
for rnd in range(2):              # plain, maps, plain, maps: each block warms up (eager, capture) and then times replays only
    for tag, ex in (("plain", plain), ("maps", maps)):
        for _ in range(3):
            ex(x, inp["coords"], genes)
        torch.cuda.synchronize()
        r0 = ex.graph_replays
        for _ in range(steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ex(x, inp["coords"], genes)
            b.record()
            b.synchronize()
            times[tag].append(a.elapsed_time(b))
        assert ex.graph_replays == r0 + steps, "a timed call did not replay its captured graph"
B, T, E = 3, eng.T, cfg.adapter_dim
sites = attention_sites(cfg)
moved = 0
for s in sites:
    if s.startswith("prompt_"):
        moved += 4 * B * T * T * (cfg.num_heads + 1)
    elif ".injector." in s:
        moved += B * L * (2 * E + 4 * cfg.num_heads) + 4 * B * L * T       # q fp16 + lse in, [B, L, T] out
    else:
        moved += B * L * 2 * E + 4 * B * T * L                   # k fp16 in, [B, T, L] out
p, m = statistics.median(times["plain"]), statistics.median(times["maps"])
print(json.dumps({"metric": "attention maps: added ms per slide (eval forward, 3 task passes, hipGraph replay)", "patches": L,
                  "sites": len(sites), "ms_plain": round(p, 4), "ms_maps": round(m, 4), "ms_added": round(m - p, 4),
                  "plain_min_max": [round(min(times["plain"]), 4), round(max(times["plain"]), 4)],
                  "maps_min_max": [round(min(times["maps"]), 4), round(max(times["maps"]), 4)], "gb_moved_by_maps": round(moved / 1e9, 4)}))
