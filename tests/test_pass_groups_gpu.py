"""The pass-group schedule (modaltune_amd/pass_groups.py: fork, one HIP stream + workspace slot + tape + flat gradient set per group,
join, sum of the sets) enqueues what the five hand-written copies it replaced enqueued, in the same order on the same streams.

tests/golden/pass_group_timelines.json is `record_timelines()` below, run at the last commit that had the five copies: per case
the ops.TIMELINE of ONE eager visit reduced to [(key, stream ordinal by first appearance)].  The split is forced at fixture size
(model_L37_d3, split_min_patches = 0: the smallest shape with two groups, two workspace slots and three gradient buckets).

  trainstep            TrainStep.step(update=False)
  trainstep_joined     the same with force_bucket_joins (the backwards advance stage by stage, every bucket summed at its own join)
  trainstep_two_tasks  task_ids = (0, 2): two one-pass groups (two workspace slots)
  extractor            the first visit of an EmbeddingExtractor
  module_eager         model(...) x 3 task ids + backward() through the eager bridge
  module_priming       the same on ModuleReplay's priming visit (the visit after `capture_after`)

After every visit the parameter store points at its own gradient set again, and a group whose forward raises (a host exception from
a stub) leaves the store, the engine's `record_markers` and the next step as they were."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from modaltune_amd import synth  # noqa: E402
from modaltune_amd.config import GIGAPATH_JSON, ModelConfig  # noqa: E402

TIMELINES_JSON = "pass_group_timelines.json"
FIXTURE = "model_L37_d3.npz"


def _fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, FIXTURE))
    meta = dict(L=int(g["L"]), depth=int(g["depth"]), seed=int(g["seed"]), ngrids=int(g["ngrids"]), sizes=[int(s) for s in g["sizes"]],
                inter=[[int(i) for i in p] for p in g["inter"]])
    return meta, synth.synth_inputs(meta["L"], meta["sizes"], meta["seed"], grid=meta["ngrids"])


def _engine(meta):
    from modaltune_amd.engine import Engine
    cfg = ModelConfig(depth=meta["depth"], interaction_indexes=tuple(tuple(p) for p in meta["inter"]), slide_ngrids=meta["ngrids"])
    eng = Engine(cfg, meta["sizes"], "cuda")
    eng.load_state_dict(synth.synth_state_dict(cfg, meta["sizes"], meta["seed"]))
    return eng


def _trainstep(golden_dir, joined=False, **kw):
    """(engine, visit): one untimed batched step has run (weight caches, the batched workspace); `visit` is a step as pass groups."""
    from modaltune_amd.trainer import TrainStep
    meta, inp = _fixture(golden_dir)
    eng = _engine(meta)
    ts = TrainStep(eng, **kw)
    ts.set_projector(synth.projector_state(meta["seed"]))
    ts.auto_split = False
    slide = (torch.from_numpy(inp["x"]).cuda(), inp["coords"], [torch.from_numpy(a).cuda() for a in inp["genes"]], torch.from_numpy(inp["text"]))

    def visit():
        ts.step(*slide, update=False)
        torch.cuda.synchronize()
        return ts
    ts.split_min_patches = 1 << 30
    visit()
    assert ts._pass_streams is None
    ts.split_min_patches, ts.force_bucket_joins = 0, joined
    return eng, visit


def _extractor(golden_dir):
    from modaltune_amd.evaluate import EmbeddingExtractor
    meta, inp = _fixture(golden_dir)
    eng = _engine(meta)
    x, genes = torch.from_numpy(inp["x"]).cuda(), [torch.from_numpy(a).cuda() for a in inp["genes"]]
    EmbeddingExtractor(eng, graphed=False)(x, inp["coords"], genes)          # (weight caches, the batched workspace)
    ex = EmbeddingExtractor(eng)
    ex.split_min_patches = 0

    def visit():
        out = ex(x, inp["coords"], genes)
        torch.cuda.synchronize()
        assert ex._streams is not None and ex.graph_replays == 0
        return out
    return eng, visit


def _module(golden_dir, replay):
    """The reference trainer's loop on the drop-in module.  replay False: the eager bridge; True: the untimed slides run up to
    ModuleReplay's first priming visit, which is `visit`."""
    from modaltune_amd.aggregators import Aggregator
    meta, inp = _fixture(golden_dir)
    groups = {i: ["g"] * n for i, n in enumerate(meta["sizes"])}
    model = Aggregator.create("longnetvit_gene_adapter", gene_group_defination=groups, multi_task=3,
                              **dict(GIGAPATH_JSON, depth=meta["depth"], slide_ngrids=meta["ngrids"], interaction_indexes=meta["inter"],
                                     dropout=0.0, drop_path_rate=0.0))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(model.cfg, meta["sizes"], meta["seed"]).items()}, strict=True)
    model.split_min_patches = 0
    x, coords = torch.from_numpy(inp["x"]).cuda(), torch.from_numpy(inp["coords"]).cuda()
    genes = {i: torch.from_numpy(a).cuda() for i, a in enumerate(inp["genes"])}
    w = torch.randn(3, 256, generator=torch.Generator().manual_seed(1)).cuda()
    eye = torch.eye(3).cuda()
    model.train()
    rp = model._replay
    rp.enabled = replay

    def slide():
        xs = x.clone()
        ys = [model(x=xs, coords=coords, genes=genes, clinical=[], task_token=eye[t].clone()) for t in (0, 1, 2)]
        sum((y * w[t]).sum() for t, y in enumerate(ys)).backward()
        torch.cuda.synchronize()

    def visit():
        slide()
        assert model._split is not None and (rp.primed, rp.captures) == ((1, 0) if replay else (0, 0))
    for _ in range(1 + rp.capture_after if replay else 1):      # learning the task ids (+ the eager visits of the geometry)
        slide()
    assert rp.primed == 0
    return model.engine, visit


CASES = {
    "trainstep": lambda d: _trainstep(d),
    "trainstep_joined": lambda d: _trainstep(d, joined=True),
    "trainstep_two_tasks": lambda d: _trainstep(d, task_ids=(0, 2), text_rows=(0, 3)),
    "extractor": _extractor,
    "module_eager": lambda d: _module(d, False),
    "module_priming": lambda d: _module(d, True),
}


def record_timeline(golden_dir, case):
    """[[key, stream ordinal by first appearance], ...] of the case's one timed visit; the store's gradient set is its own afterwards."""
    from modaltune_amd import ops
    eng, visit = CASES[case](golden_dir)
    own = (eng.store.flat_grad, eng.store.grads)
    ops.TIMER, ops.TIMELINE = {}, []
    try:
        visit()
    finally:
        timeline, ops.TIMER, ops.TIMELINE = ops.TIMELINE, None, None
    assert eng.store.flat_grad is own[0] and eng.store.grads is own[1] and not eng.record_markers
    order = {}
    return [[t[0], order.setdefault(t[3], len(order))] for t in timeline]


def record_timelines(golden_dir):
    """The fixture: {"keys": [every key], "cases": {case: {"key": [index into keys], "stream": [ordinal]}}}."""
    lines = {case: record_timeline(golden_dir, case) for case in CASES}
    keys = sorted({k for tl in lines.values() for k, _ in tl})
    at = {k: i for i, k in enumerate(keys)}
    return {"keys": keys, "cases": {c: {"key": [at[k] for k, _ in tl], "stream": [s for _, s in tl]} for c, tl in lines.items()}}


@pytest.mark.parametrize("case", list(CASES))
def test_one_visit_enqueues_the_recorded_launches_on_the_recorded_streams(golden_dir, case):
    fixture = json.load(open(os.path.join(golden_dir, TIMELINES_JSON)))
    rec = fixture["cases"][case]
    want = [[fixture["keys"][k], s] for k, s in zip(rec["key"], rec["stream"])]
    got = record_timeline(golden_dir, case)
    assert 1 + max(s for _, s in want) == 3, "the recorded visit ran as two groups next to the calling stream"
    first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, (len(got), len(want), first, got[first:first + 3], want[first:first + 3])


def test_a_group_that_raises_leaves_the_store_the_markers_and_the_next_step_as_they_were(golden_dir):
    eng, visit = _trainstep(golden_dir, joined=True)
    own = (eng.store.flat_grad, eng.store.grads)
    before = visit().last_logits.clone()
    assert eng.store.flat_grad is own[0] and eng.store.grads is own[1]
    real, seen = eng.forward, []

    def stub(*a, **k):
        seen.append(1)
        if len(seen) == 2:
            raise ValueError("the second group's forward")
        return real(*a, **k)
    eng.forward = stub
    try:
        with pytest.raises(ValueError, match="second group"):
            visit()
    finally:
        del eng.forward
    torch.cuda.synchronize()
    assert len(seen) == 2
    assert eng.store.flat_grad is own[0] and eng.store.grads is own[1]
    assert eng.record_markers is False
    ts = visit()
    assert torch.equal(ts.last_logits, before) and int(ts.found_inf) == 0
    assert eng.store.flat_grad is own[0] and eng.store.grads is own[1]
