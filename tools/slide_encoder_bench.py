"""Forward time of the plain slide encoder (slide_encoder.LongNetViT, 12 layers) beside the three-pass embedding pass of the adapter
model (evaluate.EmbeddingExtractor) on the same frozen tensors, in the same run: hipGraph replay of each, median of REPS.  The plain
forward is one pass over the backbone without adapters, so the expectation is about a third of the embedding pass plus the read-outs
-- informational, not a pass bar.

    python tools/slide_encoder_bench.py [L ...] (default: 512 4096 10000)

Prints one JSON line per bag length, with the box's measured MFMA peak."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from modaltune_amd import ops, synth  # noqa: E402
from modaltune_amd.aggregators import Aggregator  # noqa: E402
from modaltune_amd.config import GIGAPATH_JSON  # noqa: E402
from modaltune_amd.evaluate import EmbeddingExtractor  # noqa: E402

lengths = [int(a) for a in sys.argv[1:]] or [512, 4096, 10000]
REPS = 9
dev = torch.device("cuda", 0)
sizes = synth.toy_group_sizes(6)
model = Aggregator.create("longnetvit_gene_adapter", gene_group_defination={i: ["g"] * n for i, n in enumerate(sizes)}, multi_task=3,
                          **dict(GIGAPATH_JSON, pretrained=False))
model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(model.cfg, sizes, seed=0).items()}, strict=True)
model.eval()
ex = EmbeddingExtractor(model.engine)
enc = {pool: model.slide_encoder(global_pool=pool) for pool in (False, True)}
peak = ops.measured_mfma_peak_tflops()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def median_ms(fn):
    for _ in range(3):          # eager visit, capture, first replay
        fn()
    return round(statistics.median(timed(fn) for _ in range(REPS)), 3)


for L in lengths:
    inp = synth.synth_inputs(L, sizes, seed=1000, grid=128 if L <= 128 * 128 else 512)
    x = torch.from_numpy(inp["x"]).to(dev).half().reshape(L, -1).contiguous()
    coords = torch.from_numpy(inp["coords"]).to(dev).reshape(L, 2)
    genes = [torch.from_numpy(a).to(dev) for a in inp["genes"]]
    row = {"metric": "plain slide encoder forward (hipGraph replay), ms", "patches": L, "depth": model.cfg.depth}
    for pool in (False, True):
        for al in (False, True):
            row[("pool" if pool else "cls") + ("_all_layers" if al else "_single")] = median_ms(lambda: enc[pool](x, coords, all_layer_embed=al))
    row["embedding_pass_3_tasks"] = median_ms(lambda: ex(x, coords, genes))
    row["single_over_third_of_embedding_pass"] = round(row["cls_single"] / (row["embedding_pass_3_tasks"] / 3), 3)
    row["mfma_peak_measured"] = round(peak, 1)
    print(json.dumps(row), flush=True)
