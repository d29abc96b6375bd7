"""The slide protocol (Engine / TitanEngine: stage_slide, slide_prologue, forward_slide, replayable) enqueues for the TITAN
configuration what the callers' own `if titan` arms enqueued, in the same order on the same streams, and computes the same step.

tests/golden/titan_timelines.json is `record_timelines()` below, run at the last commit that had those arms: per case the
ops.TIMELINE of ONE eager visit reduced to [(key, stream ordinal by first appearance)], as tests/test_pass_groups_gpu.py does for the
LongNet configuration.  The slide is the smaller committed TITAN fixture (model_titan_L170_clin: 170 patches, clinical token) on the
stand-in backbone, depth 6, backbone_impl "native"; the Injector gammas are drawn non-zero so that the backward reaches the blocks.
The learning rate is 0: step_graphed's visits run the optimiser, and AdamW turns the sign of a near-zero gradient element -- which
the atomics below do not fix run to run -- into a +-lr step, so with lr > 0 the timed visit's logits differed run to run (seen once:
9.7e-6 of the largest logit); with lr = 0 the staged logits are those of the unstaged step, bit for bit.

  trainstep         TrainStep.step(update=False), batched
  trainstep_groups  the same under MT_SPLIT_PASSES=force: the TITAN arm of the pass groups (prologue in front of the fork)
  trainstep_staged  the visit of step_graphed that is still eager: stage_slide, then the forward from the token gather
  extractor         the first visit of an EmbeddingExtractor
  module_eager      model(...) x 3 task ids + backward() through the eager bridge
  trainstep_torch   backbone_impl "torch": not replayable, the eager route; the timeline holds the HIP launches only

The three native `trainstep*` cases also pin the step's result against the recording: the logits and, per parameter, checkpoint's
checksum64 and the float64 norm of unscaled_grads().  The recording ran every case twice on fresh engines and says per case whether
the two runs agreed bit for bit (`stable`).  The logits did in all three cases (the staged one over four engines), and are compared
bit for bit.  The gradients did in none: the default launchers sum parameter gradients over workgroups with fp32 atomics (what the
deterministic mode replaces, and the TITAN engine refuses that mode) -- 70-odd of the 250 parameters' checksums differ between two
runs of the recording commit itself, the norms by <= 1e-7 -- so in all three cases every gradient norm is held to the bar
tests/test_titan_gpu.py holds it to: within 2e-2 (+ 1e-6 of the largest).  The test prints the figures."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from modaltune_amd import synth  # noqa: E402
from test_titan_cpu import _case  # noqa: E402

import titan_standin  # noqa: E402

TIMELINES_JSON = "titan_timelines.json"
FIXTURE = "titan_L170_clin"
PINNED = ("trainstep", "trainstep_groups", "trainstep_staged")      # (native cases whose logits and gradients are compared)


def _state(cfg, sizes, seed):
    sd = synth.synth_state_dict(cfg, sizes, seed)
    for k in sd:          # Injector gammas start at 0 (init_values): give the backward something to carry into the blocks
        if k.endswith("gamma"):
            sd[k] = (0.1 * torch.randn(sd[k].shape, generator=torch.Generator().manual_seed(len(k)))).numpy().astype(sd[k].dtype)
    return sd


def _trainstep(golden_dir, impl="native", staged=False):
    """(engine, visit, result): one untimed visit has run (weight caches, workspaces); `visit` is the same step again."""
    from modaltune_amd.titan import TitanEngine, make_backbone
    from modaltune_amd.trainer import TrainStep
    g, cfg, sizes, inp, seed, clinical = _case(golden_dir, FIXTURE)
    vit = titan_standin.VisionTransformer()
    titan_standin.init_standin(vit, seed)
    eng = TitanEngine(cfg, sizes, make_backbone(vit.to("cuda"), "cuda", impl), "cuda")
    eng.load_state_dict(_state(cfg, sizes, seed))
    ts = TrainStep(eng, lr=0.0)      # (step_graphed's visits run the optimiser: the weights, and so the timed visit's logits, stay put)
    ts.set_projector(synth.projector_state(seed))
    L = inp["x"].shape[1]
    slide = (torch.from_numpy(inp["x"]).cuda().reshape(L, -1), torch.from_numpy(inp["coords"]).cuda().reshape(L, 2),
             [torch.from_numpy(a).cuda() for a in inp["genes"]], torch.from_numpy(inp["text"]).cuda())
    clin = torch.from_numpy(inp["clinical"]).cuda() if clinical else None

    def visit():
        if staged:
            ts.step_graphed(*slide, clinical=clin)
        else:
            ts.step(*slide, update=False, clinical=clin)
        torch.cuda.synchronize()
        return ts
    visit()
    return eng, visit, lambda: (ts.last_logits, ts.unscaled_grads())


def _groups(golden_dir):
    eng, visit, result = _trainstep(golden_dir)      # (the caller has set MT_SPLIT_PASSES=force: the untimed visit ran as groups too)

    def forced():
        ts = visit()
        assert ts._pass_streams is not None, "the visit ran as pass groups"
        return ts
    return eng, forced, result


def _staged(golden_dir):
    eng, visit, result = _trainstep(golden_dir, staged=True)

    def eager():
        ts = visit()
        assert (ts.eager_steps, ts.graph_replays) == (2, 0), "the second visit of the geometry is still eager"
        return ts
    return eng, eager, result


def _extractor(golden_dir):
    from modaltune_amd.evaluate import EmbeddingExtractor
    eng, _, _ = _trainstep(golden_dir)
    g, cfg, sizes, inp, seed, clinical = _case(golden_dir, FIXTURE)
    x, coords = torch.from_numpy(inp["x"]).cuda(), torch.from_numpy(inp["coords"]).cuda()
    genes = [torch.from_numpy(a).cuda() for a in inp["genes"]]
    clin = torch.from_numpy(inp["clinical"]).cuda() if clinical else None
    ex = EmbeddingExtractor(eng)

    def visit():
        out = ex(x, coords, genes, clin)
        torch.cuda.synchronize()
        assert ex.graph_replays == 0
        return out
    return eng, visit, None


def _module(golden_dir):
    """The reference trainer's loop on the drop-in module: one untimed slide (learning the task ids), then `visit`."""
    from test_titan_gpu import _model
    g, model, sizes, inp, seed, clinical, O = _model(golden_dir, FIXTURE, "native")
    with torch.no_grad():
        for k, p in model._params.items():
            if k.endswith("gamma"):
                p.copy_(0.1 * torch.randn(p.shape, generator=torch.Generator().manual_seed(len(k))).cuda())
    x, coords = torch.from_numpy(inp["x"]).cuda(), torch.from_numpy(inp["coords"]).cuda()
    genes = {i: torch.from_numpy(a).cuda() for i, a in enumerate(inp["genes"])}
    kw = dict(clinical=torch.from_numpy(inp["clinical"]).cuda()) if clinical else {}
    w = torch.randn(3, 256, generator=torch.Generator().manual_seed(1)).cuda()
    eye = torch.eye(3).cuda()
    model.train()

    def slide():
        xs = x.clone()
        ys = [model(x=xs, coords=coords, genes=genes, task_token=eye[t].clone(), **kw) for t in (0, 1, 2)]
        sum((y * w[t]).sum() for t, y in enumerate(ys)).backward()
        torch.cuda.synchronize()
    slide()
    return model.engine, slide, None


CASES = {
    "trainstep": _trainstep,
    "trainstep_groups": _groups,
    "trainstep_staged": _staged,
    "extractor": _extractor,
    "module_eager": _module,
    "trainstep_torch": lambda d: _trainstep(d, impl="torch"),
}


def _force_groups(monkeypatch, case):
    if case == "trainstep_groups":
        monkeypatch.setenv("MT_SPLIT_PASSES", "force")


def record_case(golden_dir, case):
    """([[key, stream ordinal by first appearance], ...] of the case's one timed visit, its result or None); the store's gradient
    set is its own afterwards."""
    from modaltune_amd import ops
    from modaltune_amd.checkpoint import checksum64_reference
    eng, visit, result = CASES[case](golden_dir)
    own = (eng.store.flat_grad, eng.store.grads)
    ops.TIMER, ops.TIMELINE = {}, []
    try:
        visit()
    finally:
        timeline, ops.TIMER, ops.TIMELINE = ops.TIMELINE, None, None
    assert eng.store.flat_grad is own[0] and eng.store.grads is own[1] and not eng.record_markers
    order = {}
    tl = [[t[0], order.setdefault(t[3], len(order))] for t in timeline]
    res = None
    if result is not None and case in PINNED:
        logits, grads = result()
        grads = {k: v.detach().float().cpu() for k, v in grads.items()}
        res = {"logits": [[float(v) for v in row] for row in logits.detach().float().cpu().numpy()],
               "grad_checksums": {k: int(checksum64_reference(v.numpy())) for k, v in grads.items()},
               "grad_norms": {k: float(v.double().norm()) for k, v in grads.items()}}
    return tl, res


def record_timelines(golden_dir, monkeypatch, cases=None):
    """The fixture: {"keys": [every key], "cases": {case: {"key": [index into keys], "stream": [ordinal]}}, "results": {case: logits,
    gradient checksums and norms of the FIRST of two recordings, "stable": {"logits", "grads"}: the second one agreed bit for bit}}."""
    lines, results = {}, {}
    for case in cases or CASES:
        with monkeypatch.context() as mp:
            _force_groups(mp, case)
            (lines[case], res), (again, res2) = record_case(golden_dir, case), record_case(golden_dir, case)
        assert again == lines[case], f"{case}: two visits of fresh engines enqueue different timelines"
        if res is not None:
            res["stable"] = {"logits": res["logits"] == res2["logits"], "grads": res["grad_checksums"] == res2["grad_checksums"]}
            results[case] = res
    keys = sorted({k for tl in lines.values() for k, _ in tl})
    at = {k: i for i, k in enumerate(keys)}
    return {"keys": keys, "cases": {c: {"key": [at[k] for k, _ in tl], "stream": [s for _, s in tl]} for c, tl in lines.items()},
            "results": results}


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


@pytest.mark.parametrize("case", list(CASES))
def test_one_titan_visit_enqueues_the_recorded_launches_and_computes_the_recorded_step(golden_dir, monkeypatch, case):
    fixture = json.load(open(os.path.join(golden_dir, TIMELINES_JSON)))
    rec = fixture["cases"][case]
    want = [[fixture["keys"][k], s] for k, s in zip(rec["key"], rec["stream"])]
    _force_groups(monkeypatch, case)
    got, res = record_case(golden_dir, case)
    if case == "trainstep_groups":
        assert 1 + max(s for _, s in want) == 3, "the recorded visit ran as two groups next to the calling stream"
    first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, (len(got), len(want), first, got[first:first + 3], want[first:first + 3])
    if case not in PINNED:
        return
    ref = fixture["results"][case]
    stable = ref["stable"]
    err = _rel(res["logits"], ref["logits"])
    names = list(ref["grad_norms"])
    assert list(res["grad_norms"]) == names
    top = max(ref["grad_norms"].values())
    worst = max(abs(res["grad_norms"][k] - ref["grad_norms"][k]) / (ref["grad_norms"][k] + 1e-300) for k in names if ref["grad_norms"][k] > 1e-6 * top)
    differ = [k for k in names if res["grad_checksums"][k] != ref["grad_checksums"][k]]
    print(f"titan protocol {case}: recording bit-stable {stable}; logits rel {err:.3e}; {len(differ)} / {len(names)} gradient checksums "
          f"differ; worst gradient-norm deviation {worst:.3e}")
    if stable["logits"]:
        assert res["logits"] == ref["logits"]
    else:
        assert err < 1e-3
    if stable["grads"]:
        assert not differ, differ[:8]
    else:
        bad = [(k, res["grad_norms"][k], ref["grad_norms"][k]) for k in names
               if abs(res["grad_norms"][k] - ref["grad_norms"][k]) > 2e-2 * ref["grad_norms"][k] + 1e-6 * top]
        assert not bad, bad[:8]
