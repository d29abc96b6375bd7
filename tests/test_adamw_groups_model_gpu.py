"""GPU: parameter groups (per-group lr and weight decay) through the two optimiser paths of the model -- `modaltune_amd.optim.AdamW`
under the reference trainer's loop and `TrainStep(param_groups=...)` -- their graph replay, and the checkpoint.

Bars.  Module path against torch.optim.AdamW fed the same gradients: 1e-6 absolute per tensor at lr <= 1e-3, the bar of
test_model_gpu.py::test_fused_adamw_is_torch_adamw_on_the_models_flat_buffers.  Two AdamW runs on gradients that agree only to
rounding (the fused step against the module path): 2.5 * steps * lr per element, test_model_gpu.py::test_graph_replay_matches_eager's
bar -- AdamW's normalised update is at most ~lr per step whatever the gradient's size, so an element whose gradient is rounding noise
may differ by 2 lr per step -- here with every GROUP's own lr (base x lr_mult): a tensor trained at another group's rate leaves it.
Everything in the deterministic mode, and a frozen group, is torch.equal."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from modaltune_amd import ops, optim, synth  # noqa: E402
from modaltune_amd.config import GIGAPATH_JSON  # noqa: E402

from test_checkpoint_gpu import _assert_equal, _fresh, _state  # noqa: E402

SEED, NGRIDS, L = 53, 64, 300
LR = 1e-3
RULES = [{"match": r"^interactions\.0\.", "lr_mult": 0.0, "weight_decay": 0.0},            # held still
         {"match": r"^gene_encoder\.", "kinds": ("w",), "lr_mult": 0.1},                    # the gene encoder at a tenth of the rate ...
         {"match": r"^gene_encoder\.", "lr_mult": 0.1, "weight_decay": 0.0},                # ... its biases and norms without decay
         {"kinds": optim.NO_DECAY_KINDS, "weight_decay": 0.0}]                              # no decay on the small tensors elsewhere
_cache = {}


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _toy_model():
    """The drop-in model of test_fused_adamw_is_torch_adamw_on_the_models_flat_buffers (depth 3, toy pathways), built once; every
    caller gets it with the synthetic weights loaded afresh."""
    from modaltune_amd.aggregators import Aggregator
    sizes = synth.toy_group_sizes()
    if "model" not in _cache:
        groups = {i: ["g"] * n for i, n in enumerate(sizes)}
        _cache["model"] = Aggregator.create("longnetvit_gene_adapter", gene_group_defination=groups, multi_task=3,
                                            **dict(GIGAPATH_JSON, depth=3, slide_ngrids=NGRIDS, interaction_indexes=[[0, 0], [1, 1], [2, 2]],
                                                   dropout=0.0, drop_path_rate=0.0))
        _cache["sd"] = synth.synth_state_dict(_cache["model"].cfg, sizes, SEED)
        inp = synth.synth_inputs(L, sizes, SEED, grid=NGRIDS)
        _cache["inp"] = (torch.from_numpy(inp["x"]).cuda(), torch.from_numpy(inp["coords"]).cuda(),
                         [torch.from_numpy(a).cuda() for a in inp["genes"]], torch.from_numpy(inp["text"]).cuda())
    model = _cache["model"]
    model.load_state_dict({k: torch.from_numpy(v) for k, v in _cache["sd"].items()}, strict=True)
    model.train()
    for p in model.parameters():
        p.grad = None
    return model, sizes, _cache["inp"]


def test_module_path_with_groups_is_one_fused_launch_and_equals_torch_adamw():
    """optim.AdamW over no_decay_groups + a 0.1 x lr gene encoder against torch.optim.AdamW on twins with the same groups, the four
    iterations of test_fused_adamw_is_torch_adamw_on_the_models_flat_buffers (plain, scaled, skipped, scaled): every step is the fused
    launch (before parameter groups existed: torch's own walk, last_step_fused False), every tensor within that test's 1e-6, and the
    state_dict() loads into the torch twin."""
    _gpu()
    model, sizes, (x, c, genes, _) = _toy_model()
    named = [(k, p) for k, p in model.named_parameters() if p.requires_grad]
    groups = optim.no_decay_groups(model, 0.01, rules=[{"match": r"^gene_encoder\.", "lr": 0.1 * LR}])
    assert [(g.get("lr"), g["weight_decay"]) for g in groups] == [(None, 0.01), (None, 0.0), (0.1 * LR, 0.01), (0.1 * LR, 0.0)]
    assert sorted(k for g in groups for k in g["names"]) == sorted(k for k, _ in named)
    kinds = {k: kind for k, _, kind, t in synth.param_specs(model.cfg, sizes) if t}
    assert {kinds[k] for g in groups[1::2] for k in g["names"]} == {"b", "lnw", "lnb", "gamma", "tok"}
    assert {kinds[k] for g in groups[0::2] for k in g["names"]} == {"w"}
    twin_of = {k: torch.nn.Parameter(p.detach().clone()) for k, p in named}
    kw = dict(lr=LR, betas=(0.9, 0.999))
    opt = optim.AdamW(groups, **kw)
    ref = torch.optim.AdamW([{**{k: v for k, v in g.items() if k not in ("params", "names")}, "params": [twin_of[k] for k in g["names"]]}
                             for g in groups], **kw)
    calls = []
    real = ops.adamw_step_groups
    ops.adamw_step_groups = lambda *a, **k: (calls.append(len(a[8])), real(*a, **k))[1]
    try:
        eye = torch.eye(3, device="cuda")
        gdict = {i: a for i, a in enumerate(genes)}
        for it, (scale, inf) in enumerate([(None, None), (64.0, 0.0), (8.0, 1.0), (8.0, 0.0)]):
            logits = torch.cat([model(x=x, coords=c, genes=gdict, task_token=eye[t]) for t in range(3)])
            (logits.square().sum() * (scale or 1.0)).backward()
            for k, p in named:
                twin_of[k].grad = p.grad.detach().clone() / (scale or 1.0)
            if scale is not None:
                opt.grad_scale, opt.found_inf = torch.full((), scale, device="cuda"), torch.full((), inf, device="cuda")
            opt.step()
            if scale is not None:
                del opt.grad_scale, opt.found_inf
            assert opt.last_step_fused is True, "groups that differ in lr / weight_decay only take the fused launch"
            if not inf:
                ref.step()
            opt.zero_grad(); ref.zero_grad()
    finally:
        ops.adamw_step_groups = real
    assert calls == [4, 4, 4, 4]                      # one grouped launch per step, four groups
    worst = max((float((p.detach() - twin_of[k].detach()).abs().max()), k) for k, p in named)
    print(f"adamw-groups module path: worst max|p - torch| = {worst[0]:.3e} ({worst[1]}), bar 1e-6")
    for k, p in named:
        assert float((p.detach() - twin_of[k].detach()).abs().max()) <= 1e-6, k
    # the groups did what they say: the gene encoder moved a tenth as far as the rest (3 counted steps of at most ~lr each)
    init = {k: torch.from_numpy(_cache["sd"][k]).cuda() for k, _ in named}
    far = {k: float((p.detach() - init[k]).abs().max()) for k, p in named}
    assert all(far[k] <= 3.1 * 0.1 * LR for k in groups[2]["names"] + groups[3]["names"])
    assert max(far[k] for k in groups[0]["names"]) > 1.5 * LR
    sd = opt.state_dict()
    assert {float(s["step"]) for s in sd["state"].values()} == {3.0} and [g["names"] for g in sd["param_groups"]] == [g["names"] for g in groups]
    ref.load_state_dict(sd)
    for g_opt, g_ref in zip(opt.param_groups, ref.param_groups):
        assert (g_opt["lr"], g_opt["weight_decay"]) == (g_ref["lr"], g_ref["weight_decay"])
        for p, q in zip(g_opt["params"], g_ref["params"]):
            assert torch.equal(opt.state[p]["exp_avg"], ref.state[q]["exp_avg"]) and torch.equal(opt.state[p]["exp_avg_sq"], ref.state[q]["exp_avg_sq"])
    # a scheduler edits group["lr"]; membership edits rebuild the table; betas that differ are still torch's own step
    opt.param_groups[2]["lr"] = 0.0
    moved = opt.param_groups[3]["params"].pop()
    opt.param_groups[1]["params"].append(moved)
    logits = torch.cat([model(x=x, coords=c, genes=gdict, task_token=eye[t]) for t in range(3)])
    logits.square().sum().backward()
    before = {k: p.detach().clone() for k, p in named}
    opt.step()
    assert opt.last_step_fused is True
    assert all(torch.equal(dict(named)[k].detach(), before[k]) for k in groups[2]["names"])      # lr 0: p * (1 - 0 * wd) - 0, every bit
    assert not torch.equal(moved.detach(), before[[k for k, p in named if p is moved][0]])
    opt.param_groups[1]["betas"] = (0.8, 0.999)
    opt.zero_grad()
    logits = torch.cat([model(x=x, coords=c, genes=gdict, task_token=eye[t]) for t in range(3)])
    logits.square().sum().backward()
    opt.step()
    assert opt.last_step_fused is False


def _fused(param_groups, det=False, **kw):
    from modaltune_amd.engine import Engine
    from modaltune_amd.trainer import TrainStep
    model, sizes, slide = _toy_model()
    eng = Engine(model.cfg, sizes, "cuda", deterministic=det)
    eng.load_state_dict(_cache["sd"])
    ts = TrainStep(eng, lr=LR, weight_decay=0.01, param_groups=param_groups, **kw)
    ts.set_projector(synth.projector_state(SEED))
    ts.auto_split, ts.split_min_patches = False, 1 << 30
    return model, eng, ts, slide


def test_fused_step_with_groups_follows_the_module_path_and_holds_the_frozen_group_still():
    _gpu()
    steps = 3
    model, eng, ts, (x, c, genes, text) = _fused(RULES)
    groups = ts.param_groups
    assert [(g["lr_mult"], g["weight_decay"]) for g in groups] == [(1.0, 0.01), (0.0, 0.0), (0.1, 0.01), (0.1, 0.0), (1.0, 0.0)]
    assert all(ts.group_of[k] == i for i, g in enumerate(groups) for k in g["names"]) and len(ts.group_of) == len(eng.store.slots)
    assert ts._grouped() and 1 < ts._nseg <= len(eng.store.slots)
    init = {k: t.clone() for k, t in eng.store.tensors.items() if k in eng.store.slots}
    # the module path on the same slide: the reference trainer's loop (three calls, KL x 10 on L2-normalised logits, GradScaler)
    named = dict((k, p) for k, p in model.named_parameters() if p.requires_grad)
    assert list(named) == list(eng.store.slots)
    opt = optim.AdamW([{"params": [named[k] for k in g["names"]], "names": g["names"], "lr": LR * g["lr_mult"], "weight_decay": g["weight_decay"]}
                       for g in groups], lr=LR)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 15)
    target = torch.softmax(ts.project_text(text).clone(), dim=1)
    eye, gdict = torch.eye(3, device="cuda"), {i: a for i, a in enumerate(genes)}
    for it in range(steps):
        ts.step(x, c, genes, text)
        logit = torch.cat([model(x=x, coords=c, genes=gdict, task_token=eye[t]) for t in range(3)])
        logit = logit / logit.norm(dim=-1, keepdim=True)
        loss = torch.nn.functional.kl_div(torch.log_softmax(logit, dim=1), target, reduction="sum") * 10
        scaler.scale(loss).backward()
        scaler.step(opt); scaler.update()
        assert opt.last_step_fused is True
        opt.zero_grad()
        if it == 0:      # (the same loss from the same weights, to the two paths' rounding: each is within 1e-3 of the fp64 oracle)
            assert abs(float(loss.detach()) - float(ts.loss)) <= 2e-3 * abs(float(ts.loss)), (float(loss.detach()), float(ts.loss))
    torch.cuda.synchronize()
    assert int(ts.step_dev) == steps and scaler.get_scale() == 2.0 ** 15
    worst = {}
    for i, g in enumerate(groups):
        bar = 2.5 * steps * LR * g["lr_mult"]
        for k in g["names"]:
            d = float((eng.store.tensors[k] - named[k].detach()).abs().max())
            worst[i] = max(worst.get(i, 0.0), d)
            assert d <= bar, (k, i, d, bar)
    print("adamw-groups fused vs module, worst max|delta| per group / its bar:",
          [(round(worst[i] / (2.5 * steps * LR * g["lr_mult"]), 3) if g["lr_mult"] else worst[i]) for i, g in enumerate(groups)])
    # frozen: every bit of interactions.0.* as it was, on both paths, while its moments ran and the neighbours trained
    for k in groups[1]["names"]:
        assert torch.equal(eng.store.tensors[k], init[k]) and torch.equal(named[k].detach(), init[k]), k
        o, n, _ = eng.store.slots[k]
    frozen = torch.cat([torch.arange(o, o + n) for o, n, _ in (eng.store.slots[k] for k in groups[1]["names"])]).cuda()
    assert float(ts.m[frozen].abs().max()) > 0 and float(ts.v[frozen].max()) > 0
    moved = {k: float((eng.store.tensors[k] - init[k]).abs().max()) for k in eng.store.slots}
    assert moved["interactions.1.injector.gamma"] > 1.5 * LR                                 # an unfrozen neighbour moved at the full rate
    # the gene encoder at a tenth of it: per step at most lr_g * (|m^| / sqrt(v^) + wd * |p|), and |m^| / sqrt(v^) <= 1.0036 over the first
    # three steps (Cauchy-Schwarz on the two moving averages with their bias corrections, betas 0.9 / 0.999)
    top = max(float(init[k].abs().max()) for k in groups[2]["names"])
    assert 0 < max(moved[k] for k in groups[2]["names"]) <= steps * 0.1 * LR * (1.0036 + 0.01 * (top + steps * LR)) + 1e-7


def _record(ts, slide, monkeypatch):
    """(launch names, [adamw_step's scalar arguments and whose buffers it got]) of one eager update step."""
    calls = []
    real = ops.adamw_step

    def spy(p, g, m, v, n, lr, b1, b2, eps, wd, step_count, **k):
        calls.append(((n, lr, b1, b2, eps, wd, step_count, k["grad_mult"]),
                      (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), k["scale"].data_ptr(), k["found_inf"].data_ptr(),
                       k["step_dev"].data_ptr(), k["lr_dev"].data_ptr()), sorted(k)))
        return real(p, g, m, v, n, lr, b1, b2, eps, wd, step_count, **k)
    monkeypatch.setattr(ops, "adamw_step", spy)
    monkeypatch.setattr(ops, "TIMER", {})
    monkeypatch.setattr(ops, "TIMELINE", [])
    ts.step(*slide)
    torch.cuda.synchronize()
    names = [rec[0] for rec in ops.TIMELINE]
    monkeypatch.setattr(ops, "TIMER", None)
    monkeypatch.setattr(ops, "TIMELINE", None)
    monkeypatch.setattr(ops, "adamw_step", real)
    return names, calls


def test_default_path_launches_what_the_parent_launched(golden_dir, monkeypatch):
    """param_groups=None, a one-group rule list and rules that resolve to lr_mult 1 and one weight decay everywhere: the launch names of
    an update step are the list recorded before the checkpoint code existed (tests/golden/trainstep_launches_L37_d3.json, which
    test_checkpoint_gpu.py::test_default_step_launches_what_the_parent_commit_launched pins for the default constructor), with `adamw`
    where it was, mt_adamw_step called once with the default constructor's arguments on this step's own buffers, no grouped launch
    and no table on the device."""
    _gpu()
    parent = json.load(open(os.path.join(golden_dir, "trainstep_launches_L37_d3.json")))["launches"]
    seen = []
    for rules in (None, [{"match": "."}], [{"kinds": ("w",)}, {"kinds": optim.NO_DECAY_KINDS, "lr_mult": 1.0, "weight_decay": 0.01}]):
        eng, ts, slide, _ = _fresh(monkeypatch, golden_dir, det=False, **({} if rules is None else {"param_groups": rules}))
        ts.step(*slide)          # (first step: allocations)
        torch.cuda.synchronize()
        names, calls = _record(ts, slide, monkeypatch)
        assert names == parent and "adamw_groups" not in names and names.count("adamw") == 1
        assert not ts._grouped() and ts.wd == 0.01 and (rules is None) == (ts._seg_end is None)
        (scalars, ptrs, keys), = calls
        st = eng.store
        assert scalars == (st.n_flat, ts.lr, 0.9, 0.999, 1e-8, 0.01, 0, 1.0)
        assert ptrs == (st.flat.data_ptr(), st.flat_grad.data_ptr(), ts.m.data_ptr(), ts.v.data_ptr(), ts.scale.data_ptr(), ts.found_inf.data_ptr(),
                        ts.step_dev.data_ptr(), ts.lr_dev.data_ptr())
        seen.append((names, scalars, keys, len(ts.param_groups)))
    assert seen[0][:3] == seen[1][:3] == seen[2][:3] and [s[3] for s in seen] == [1, 1, 2]
    # ... and a set_group that makes the groups differ moves the same step to the grouped launch, at the same position
    ts.set_group(1, weight_decay=0.0)
    names2, calls2 = _record(ts, slide, monkeypatch)
    assert calls2 == [] and names2 == [n if n != "adamw" else "adamw_groups" for n in parent]


def test_replay_with_groups_set_lr_and_set_group_equals_the_eager_twin_bit_for_bit(golden_dir, monkeypatch):
    """Deterministic mode.  A graphed TrainStep and an eager twin walk the same schedule: steps until the geometry is captured and
    replayed, set_lr between replays (the device scalar: the capture stays), one set_group (launch arguments: the capture must go,
    and the geometry is captured again).  Losses, parameters, moments and the step count are torch.equal throughout."""
    _gpu()
    from modaltune_amd.trainer import TrainStep
    twins = []
    for _ in range(2):
        eng, _, slide, (cfg, sizes, seed) = _fresh(monkeypatch, golden_dir, det=True)
        ts = TrainStep(eng, lr=LR, param_groups=RULES)
        ts.set_projector(synth.projector_state(seed))
        twins.append((eng, ts))
    (eng_g, ts_g), (eng_e, ts_e) = twins
    losses_g, losses_e = [], []

    def both(n):
        for _ in range(n):
            ts_g.step_graphed(*slide)
            losses_g.append(ts_g.loss.clone())
            ts_e.step(*slide)
            losses_e.append(ts_e.loss.clone())
    both(4)                                    # two eager visits, the capture, a replay
    assert ts_g._graphs is not None and ts_g.graph_replays == 2
    graphs = ts_g._graphs
    for t in (ts_g, ts_e):
        t.set_lr(0.3 * LR)
    both(2)
    assert ts_g._graphs == graphs and ts_g.graph_replays == 4          # set_lr reached the replays without a new capture
    _assert_equal(_state(eng_g, ts_g), _state(eng_e, ts_e), "replays against eager steps behind set_lr")
    for t in (ts_g, ts_e):
        t.set_group(2, lr_mult=0.5, weight_decay=0.3)
    assert ts_g._graphs is None                                        # the captures held the old values
    assert ts_g.param_groups[2]["lr_mult"] == 0.5 and ts_g.param_groups[2]["weight_decay"] == 0.3
    both(4)
    assert ts_g._graphs is not None and ts_g.graph_replays >= 5
    _assert_equal(_state(eng_g, ts_g), _state(eng_e, ts_e), "replays against eager steps behind set_group")
    assert torch.equal(torch.cat(losses_g), torch.cat(losses_e)) and int(ts_g.step_dev) == int(ts_e.step_dev) == 10
    assert len(set(torch.cat(losses_g).tolist())) >= 8                  # (the steps did move)
    # a set_group that changes nothing keeps the captures
    graphs = ts_g._graphs
    ts_g.set_group(2, lr_mult=0.5)
    assert ts_g._graphs == graphs


def test_checkpoint_saved_at_lr_zero_keeps_its_groups_and_resumes_bit_for_bit(golden_dir, monkeypatch, tmp_path):
    """A warm-up's first epoch: set_lr(0.0), two steps, the checkpoint, then the schedule's next value.  At base 0 every group's written
    lr is 0 and (the decays being equal here) the torch param groups look alike: the groups must come back from their keys, or the
    gene encoder resumes at ten times its rate.  Deterministic mode: the resumed run equals the uninterrupted one bit for bit.  Also: a
    partition whose values are uniform keeps its names across a checkpoint, so set_group addresses the same group afterwards."""
    _gpu()
    rules = [{"match": r"^gene_encoder\.", "lr_mult": 0.1}, {"match": r"^interactions\.0\.", "lr_mult": 0.0}]      # one decay everywhere
    eng_a, ts_a, slide, _ = _fresh(monkeypatch, golden_dir, stochastic=5, lr=LR, param_groups=rules)
    ts_a.set_lr(0.0)
    for _ in range(2):
        ts_a.step(*slide)
    ts_a.set_lr(LR)
    for _ in range(2):
        ts_a.step(*slide)
    end_a = _state(eng_a, ts_a)
    eng_b, ts_b, _, _ = _fresh(monkeypatch, golden_dir, stochastic=5, lr=LR, param_groups=rules)
    ts_b.set_lr(0.0)
    for _ in range(2):
        ts_b.step(*slide)
    path = str(tmp_path / "lr0.pt")
    torch.save(ts_b.state_dict(), path)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    assert sd["lr"] == 0.0 and {g["lr"] for g in sd["optimizer"]["param_groups"]} == {0.0} and len({g["weight_decay"] for g in sd["optimizer"]["param_groups"]}) == 1
    want = ts_b.param_groups
    assert [g["lr_mult"] for g in want] == [1.0, 0.1, 0.0]
    eng_c, ts_c, _, _ = _fresh(monkeypatch, golden_dir, weights_seed=99, stochastic=4321, lr=LR)          # no param_groups
    ts_c.load_state_dict(sd)
    assert ts_c.param_groups == want and ts_c._grouped() and ts_c.lr == 0.0
    ts_c.set_lr(LR)
    for _ in range(2):
        ts_c.step(*slide)
    _assert_equal(end_a, _state(eng_c, ts_c), "uninterrupted against resumed from a checkpoint saved at lr 0")
    frozen = want[2]["names"][0]
    assert not torch.equal(eng_c.store.tensors[want[1]["names"][0]], eng_b.store.tensors[want[1]["names"][0]])      # (the run did move ...)
    assert torch.equal(eng_c.store.tensors[frozen], eng_b.store.tensors[frozen])                                    # ... but not the frozen group
    # a partition with uniform values survives: the default launch, and set_group still finds its group
    eng_d, ts_d, _, _ = _fresh(monkeypatch, golden_dir, stochastic=5, lr=LR, param_groups=[{"match": r"^gene_encoder\."}])
    eng_e, ts_e, _, _ = _fresh(monkeypatch, golden_dir, stochastic=5, lr=LR)
    ts_e.load_state_dict(ts_d.state_dict())
    assert len(ts_e.param_groups) == 2 and ts_e.param_groups == ts_d.param_groups and not ts_e._grouped()
    ts_e.set_group(1, lr_mult=0.1)
    assert ts_e._grouped() and all(k.startswith("gene_encoder.") for k in ts_e.param_groups[1]["names"])


def test_checkpoint_with_groups_resumes_bit_for_bit_and_loads_into_both_adamw_classes(golden_dir, monkeypatch, tmp_path):
    """Deterministic mode, accumulate = 2, clipping on, groups set: six calls uninterrupted against three calls (one micro-step of the
    second window held), a file, a FRESH TrainStep built WITHOUT param_groups on other weights, three calls.  The checkpoint's groups
    win over the constructor's.  The file's optimiser dict loads into torch.optim.AdamW and optim.AdamW built with the same groups."""
    _gpu()
    from modaltune_amd import checkpoint
    kw = dict(lr=LR, accumulate=2, max_grad_norm=1e-3, growth_interval=4)
    eng_a, ts_a, slide, _ = _fresh(monkeypatch, golden_dir, stochastic=77, param_groups=RULES, **kw)
    losses_a = []
    for _ in range(6):
        ts_a.step(*slide)
        losses_a.append(ts_a.loss.clone())
    end_a = _state(eng_a, ts_a)
    assert int(ts_a.step_dev) == 3 and float(ts_a.clip_coef) < 1.0          # (the clip was active)
    eng_b, ts_b, _, _ = _fresh(monkeypatch, golden_dir, stochastic=77, param_groups=RULES, **kw)
    for _ in range(3):
        ts_b.step(*slide)
    assert ts_b.window_pos == 1
    path = str(tmp_path / "groups.pt")
    torch.save(ts_b.state_dict(), path)
    sd = checkpoint.verify_file(path)
    assert sorted(sd) == sorted(checkpoint.REQUIRED_KEYS) and sd["format"] == 1
    want = ts_b.param_groups
    assert [(g["lr"], g["weight_decay"], g["lr_mult"], g["names"]) for g in sd["optimizer"]["param_groups"]] == \
        [(LR * g["lr_mult"], g["weight_decay"], g["lr_mult"], g["names"]) for g in want]
    names = list(eng_b.store.slots)
    assert [[names[i] for i in g["params"]] for g in sd["optimizer"]["param_groups"]] == [g["names"] for g in want]
    del eng_b, ts_b
    eng_c, ts_c, _, _ = _fresh(monkeypatch, golden_dir, weights_seed=99, stochastic=4321, **kw)          # no param_groups
    assert len(ts_c.param_groups) == 1 and not ts_c._grouped()
    ts_c.load_state_dict(sd)
    assert ts_c.param_groups == want and ts_c.window_pos == 1 and ts_c._grouped() and ts_c.group_of == {k: i for i, g in enumerate(want) for k in g["names"]}
    losses_c = []
    for _ in range(3):
        ts_c.step(*slide)
        losses_c.append(ts_c.loss.clone())
    _assert_equal(end_a, _state(eng_c, ts_c), "uninterrupted against resumed, with groups")
    assert torch.equal(torch.cat(losses_a[3:]), torch.cat(losses_c))
    # a uniform checkpoint loaded into a step built WITH groups: the checkpoint wins there too
    eng_d, ts_d, _, _ = _fresh(monkeypatch, golden_dir, stochastic=1, **kw)
    ts_c.load_state_dict(ts_d.state_dict())
    assert len(ts_c.param_groups) == 1 and not ts_c._grouped() and ts_c.wd == 0.01
    # the same file in both AdamW classes, built with the same groups
    slots = eng_c.store.slots
    m, v, step, hyper = checkpoint.unpack_optimizer(sd["optimizer"], slots, names, eng_c.store.n_flat, base_lr=sd["lr"])
    for cls in (optim.AdamW, torch.optim.AdamW):
        params = {k: torch.nn.Parameter(torch.zeros(slots[k][2], device="cuda")) for k in names}
        opt = cls([{"params": [params[k] for k in g["names"]]} for g in want], lr=5.0)
        opt.load_state_dict(sd["optimizer"])
        assert [(g["lr"], g["weight_decay"], g["lr_mult"]) for g in opt.param_groups] == [(LR * g["lr_mult"], g["weight_decay"], g["lr_mult"]) for g in want]
        for k in names:
            o, n, shape = slots[k]
            assert torch.equal(opt.state[params[k]]["exp_avg"].cpu().reshape(-1), m[o:o + n]), k
            assert torch.equal(opt.state[params[k]]["exp_avg_sq"].cpu().reshape(-1), v[o:o + n]), k
            assert float(opt.state[params[k]]["step"]) == 1.0
        # ... and its own state_dict comes back as the same groups
        back = checkpoint.unpack_optimizer(opt.state_dict(), slots, names, eng_c.store.n_flat, base_lr=sd["lr"])
        assert back[3]["groups"] == hyper["groups"] == want and torch.equal(back[0], m) and torch.equal(back[1], v)
    assert np.isfinite(float(torch.cat(losses_c).sum()))
