"""The loss-scale overflow path through the whole model: a step whose gradients come back non-finite is SKIPPED completely (parameters,
both moments, the step count and the fp16 weight caches stay put), the scale backs off, and nothing of the poisoned step -- inf / NaN in
workspaces, tape arenas, per-group gradient sets, atomically accumulated buffers, the static buffers of captured graphs -- reaches the
steps behind it.  The reference trainer starts its GradScaler at 2^15 (train_modaltune.py:107), so this branch runs in the first steps
of most trainings and again after every growth of the scale.

Recovery is judged against CONTROL twins (same weights, same clean steps, never the poisoned one); the bound is the spread between
such controls, measured in the same test: zero spread -> the victim must be bit-identical to a control, otherwise it may differ from a
control by at most twice that spread, per tensor, in relative max-norm.  The victim is never compared with itself.  The spread is the
LARGEST distance among CONTROLS (5; 4 for the big models) control twins, the victim's distance the one to its NEAREST control: with
one pair of controls the rule misfires on its own -- the max-norm distance of the moments is a few single roundings on a few
elements (L = 37: 1.2e-8 / 2.5e-8 / 3.3e-8, in steps) or dominated by rare large elements (second moment at L = 1500: 3.2e-7 ..
1.9e-6 from pair to pair).  Measured over every choice of victim and controls among 12 identical clean twins: 2 controls, 13 of 660
choices break the rule on v at L = 1500, 11 of 660 at L = 37; 3 controls: 1 resp. 3 of 1980; 4 and 5 controls: 0 of 3960 / 5544.

The clean steps of these comparisons run at lr = 0: the fp32-atomic weight-gradient reductions make two runs agree to rounding only,
and AdamW's normalised update turns the sign of a near-zero gradient into a +-lr step, so at lr > 0 the spread between two controls
is a handful of such flips (measured at lr = 1e-3: 6e-4 .. 1.2e-3 on the weights, 2e-5 .. 2.6e-4 on the moments and the loss, from
one pair of twins to the next) and hides anything below 1e-4.  At lr = 0 the weights stay, every clean step computes the same
gradient up to that rounding, and the moments, the loss and the logits expose a contamination of a later step at the 1e-7 level.
The POISONED step runs at lr = 1e-3 (the learning rate lives on the device), so a skip that is not one moves the weights; a last
step at lr = 1e-3 checks that training goes on."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from modaltune_amd import synth  # noqa: E402
from modaltune_amd.config import GIGAPATH_JSON, ModelConfig  # noqa: E402

NAN, INF = float("nan"), float("inf")
OVERFLOW_SCALE = 2.0 ** 40          # saturates the fp16 activation-gradient stream of both fixtures
CONTROLS, CONTROLS_BIG = 5, 4       # control twins per case (module docstring); _BIG: the TITAN configuration and the nn.Module models
POISON_LR = 1e-3                    # the learning rate of the poisoned step (the clean steps of the comparisons: 0, see above)


# ------------------------------------------------------------------------------------------ builders
def _longnet_twins(golden_dir, name, count, **ts_kw):
    """`count` engines + TrainSteps with the same state dict, built as test_model_gpu._build does, and the fixture's slide."""
    from modaltune_amd.engine import Engine
    from modaltune_amd.trainer import TrainStep
    g = np.load(os.path.join(golden_dir, f"model_{name}.npz"))
    L, depth, seed, ngrids = int(g["L"]), int(g["depth"]), int(g["seed"]), int(g["ngrids"])
    sizes = [int(s) for s in g["sizes"]]
    cfg = ModelConfig(depth=depth, interaction_indexes=tuple(tuple(int(i) for i in p) for p in g["inter"]), slide_ngrids=ngrids,
                      dropout=0.0, drop_path_rate=0.0, **(json.loads(str(g["extra_cfg"])) if "extra_cfg" in g.files else {}))
    state = synth.synth_state_dict(cfg, sizes, seed)
    twins = []
    for _ in range(count):
        eng = Engine(cfg, sizes, "cuda")
        eng.load_state_dict(state)
        assert not eng.stochastic            # dropout / DropPath off: two twins run the same arithmetic
        ts = TrainStep(eng, **ts_kw)
        ts.set_projector(synth.projector_state(seed))
        twins.append((eng, ts))
    inp = synth.synth_inputs(L, sizes, seed, grid=ngrids)
    x = torch.from_numpy(inp["x"]).cuda()
    slide = dict(x=x.reshape(-1, x.shape[-1]).contiguous(), coords=inp["coords"], genes=[torch.from_numpy(a).cuda() for a in inp["genes"]],
                 text=torch.from_numpy(inp["text"]))
    return twins, slide


def _titan_twins(count, L=900, **ts_kw):
    """The TITAN configuration on the stand-in backbone, as test_titan_gpu builds it (its gridding accumulates with atomics)."""
    import titan_standin
    from test_titan_cpu import TITAN_JSON
    from modaltune_amd.titan import NativeBackbone, TitanEngine, titan_model_config
    from modaltune_amd.trainer import TrainStep
    seed = 6
    sizes = synth.toy_group_sizes()
    twins = []
    for _ in range(count):
        vit = titan_standin.VisionTransformer()
        titan_standin.init_standin(vit, seed)
        cfg = titan_model_config(dict(TITAN_JSON, drop_path_rate=0.0), 3, False, 6)
        eng = TitanEngine(cfg, sizes, NativeBackbone(vit, "cuda"), "cuda")
        eng.load_state_dict(synth.synth_state_dict(cfg, sizes, seed))
        ts = TrainStep(eng, **ts_kw)
        ts.set_projector(synth.projector_state(seed))
        twins.append((eng, ts))
    inp = synth.synth_inputs_titan(L, sizes, seed, grid=40)
    slide = dict(x=torch.from_numpy(inp["x"]).cuda().reshape(L, -1).contiguous(), coords=torch.from_numpy(inp["coords"]).cuda().reshape(L, 2),
                 genes=[torch.from_numpy(a).cuda() for a in inp["genes"]], text=torch.from_numpy(inp["text"]).cuda())
    return twins, slide


# ------------------------------------------------------------------------------------------ the skip signature
def _caches(eng):
    return {k: (w.w.clone(), None if w.wt is None else w.wt.clone()) for k, w in eng._train16.items()}


def _snapshot(eng, ts):
    if not eng._caches_ready:
        eng._build_caches()
    torch.cuda.synchronize()
    assert len(eng._train16) > 0
    return dict(flat=eng.store.flat.clone(), m=ts.m.clone(), v=ts.v.clone(), step=int(ts.step_dev), scale=float(ts.scale),
                caches=_caches(eng))


def _assert_skipped(eng, ts, snap, what):
    torch.cuda.synchronize()
    assert torch.equal(eng.store.flat, snap["flat"]), (what, "parameters moved")
    assert torch.equal(ts.m, snap["m"]), (what, "first moment moved")
    assert torch.equal(ts.v, snap["v"]), (what, "second moment moved")
    assert int(ts.step_dev) == snap["step"], (what, int(ts.step_dev), snap["step"])
    assert float(ts.scale) == 0.5 * snap["scale"], (what, float(ts.scale), snap["scale"])
    assert int(ts.tracker) == 0 and int(ts.found_inf) == 0, (what, int(ts.tracker), int(ts.found_inf))
    now = _caches(eng)
    assert now.keys() == snap["caches"].keys()
    for k, (w, wt) in snap["caches"].items():
        assert torch.equal(now[k][0], w) and (wt is None or torch.equal(now[k][1], wt)), (what, "fp16 weight cache", k)
    assert bool(torch.isfinite(eng.store.flat).all())


def _relmax(a, b):
    a, b = a.detach().double().reshape(-1), b.detach().double().reshape(-1)
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def _state(eng, ts):
    torch.cuda.synchronize()
    return dict(flat=eng.store.flat, m=ts.m, v=ts.v, loss=ts.loss, logits=ts.last_logits)


def _judge(what, victim, controls):
    """The control-to-control rule of the module docstring on dicts of tensors.  Prints every figure before it asserts."""
    keys = list(victim)
    spread = {k: max(_relmax(a[k], b[k]) for i, a in enumerate(controls) for b in controls[i + 1:]) for k in keys}
    dist = {k: min(_relmax(victim[k], c[k]) for c in controls) for k in keys}
    print(what, "control-to-control", {k: f"{v:.2e}" for k, v in spread.items()}, "victim-to-control", {k: f"{v:.2e}" for k, v in dist.items()})
    for k in keys:
        assert bool(torch.isfinite(victim[k]).all()), (what, k, "not finite on the victim")
    if all(v == 0.0 for v in spread.values()):
        for k in keys:
            assert torch.equal(victim[k], controls[0][k]), (what, k, "deterministic schedule: the victim must be bit-identical to the control")
    else:
        for k in keys:
            assert dist[k] <= 2.0 * spread[k], (what, k, dist[k], spread[k])


def _assert_recovered(victim, controls, what):
    assert int(victim[1].found_inf) == 0
    assert all(int(victim[1].step_dev) == int(ts.step_dev) for _, ts in controls)
    _judge("overflow-recovery " + what, _state(*victim), [_state(*c) for c in controls])


# ------------------------------------------------------------------------------------------ schedules and poisons
# name -> (step_graphed?, pass groups forced?, per-bucket joins?, clean steps in front of the poisoned one)
# "replay": capture_after = 1 -> eager visit, capture + replay, replay; the poisoned step is the 4th visit: a replay of captured graphs.
# "eager_then_capture": the poisoned step is the eager visit in front of the capture, the clean steps are captured and replayed.
SCHEDULES = {
    "eager": (False, False, False, 1),
    "replay": (True, False, False, 3),
    "eager_then_capture": (True, False, False, 0),
    "groups_eager": (False, True, False, 1),
    "groups_replay": (True, True, False, 3),
    "groups_joined_eager": (False, True, True, 1),
    "groups_joined_replay": (True, True, True, 3),
}


def _configure(ts, schedule):
    graphed, groups, joins, pre = SCHEDULES[schedule]
    ts.split_min_patches = 0 if groups else 1 << 30
    ts.force_bucket_joins = joins
    ts.auto_split = False
    return graphed, groups, pre


def _step(ts, slide, graphed, x=None):
    x = slide["x"] if x is None else x
    if graphed:
        ts.step_graphed(x, slide["coords"], slide["genes"], slide["text"])
    else:
        ts.step(x, slide["coords"], slide["genes"], slide["text"], update=True)


def _poisoned_x(slide, poison):
    x = slide["x"].clone()
    L = x.shape[0]
    if poison == "nan_row":
        x[L // 2, :] = NAN
    elif poison == "inf_element":
        x[L // 3, 5] = INF
    else:
        return None
    return x


def _run_case(twins, slide, schedule, poison, what):
    victim, controls = twins[0], twins[1:]
    ctl_a = controls[0]
    for _, ts in twins:
        graphed, groups, pre = _configure(ts, schedule)
    eng, ts = victim
    for _ in range(pre):
        for _, t in twins:
            _step(t, slide, graphed)
    if groups and pre:
        assert ts._pass_streams is not None
    snap = _snapshot(eng, ts)
    replays, eager = ts.graph_replays, ts.eager_steps
    ts.set_lr(POISON_LR)
    # ---- the poisoned step, on the victim only
    onehots = ts.onehots.clone()
    if poison == "scale":
        ts.scale.fill_(OVERFLOW_SCALE)
        snap["scale"] = OVERFLOW_SCALE
        _step(ts, slide, graphed)
    elif poison == "one_group":
        ts.onehots[ts._groups[1][0], 0] = NAN          # reaches the passes of the SECOND group only
        _step(ts, slide, graphed)
        torch.cuda.synchronize()
        a = ts._groups[1][0]
        assert bool(torch.isfinite(ts.last_logits[:a]).all()) and not bool(torch.isfinite(ts.last_logits[a:]).any()), "the other group is clean"
        ts.onehots.copy_(onehots)
    else:
        _step(ts, slide, graphed, x=_poisoned_x(slide, poison))
    if schedule.endswith("replay"):
        assert (ts.graph_replays, ts.eager_steps) == (replays + 1, eager), "the poisoned step was a replay of captured graphs"
    else:
        assert (ts.graph_replays, ts.eager_steps) == (replays, eager + 1), "the poisoned step ran eagerly"
    _assert_skipped(eng, ts, snap, what)
    # ---- recovery: the control's scale, the clean slide, two clean steps on every twin
    ts.set_lr(0.0)
    ts.scale.copy_(ctl_a[1].scale)
    for _ in range(2):
        for _, t in twins:
            _step(t, slide, graphed)
    if graphed:
        assert ts.graph_replays >= replays + 2 and ctl_a[1].graph_replays >= 1
    assert int(ts.step_dev) == pre + 2
    eng.check_inputs()
    _assert_recovered(victim, controls, what)
    # ---- and training goes on: one step at a real learning rate
    before = eng.store.flat.clone()
    ts.set_lr(POISON_LR)
    _step(ts, slide, graphed)
    torch.cuda.synchronize()
    assert int(ts.step_dev) == pre + 3 and int(ts.found_inf) == 0
    assert bool(torch.isfinite(eng.store.flat).all()) and not torch.equal(eng.store.flat, before)
    moved = (eng.store.flat - before).abs().max()
    assert 0.1 * POISON_LR < float(moved) <= 2.0 * POISON_LR + ts.wd * POISON_LR * float(before.abs().max()), float(moved)      # (~lr per element + the decay)


CASES = ([(s, p) for s in ("eager", "replay", "eager_then_capture", "groups_eager", "groups_replay") for p in ("scale", "nan_row")]
         + [("eager", "inf_element"), ("replay", "inf_element"), ("groups_joined_eager", "scale"), ("groups_joined_replay", "nan_row"),
            ("groups_eager", "one_group"), ("groups_replay", "one_group"), ("groups_joined_eager", "one_group")])


@pytest.mark.parametrize("schedule,poison", CASES)
@pytest.mark.parametrize("name", ["L37_d3", "L1500_d3"])
def test_overflow_step_is_skipped_and_the_next_steps_recover(golden_dir, name, schedule, poison):
    """Skip signature + recovery under every schedule of the fused step.  Overflow provoked by the scale (2^40: the fp16
    activation-gradient stream saturates -- the case GradScaler exists for), by the data (a NaN patch-feature row, one inf element) and,
    with the pass groups, by a NaN in the one-hot row of ONE group's task (the other group's gradient set is finite: the sum in front of
    the optimiser must still skip).
    Measured control-to-control spread: see SPREAD_NOTE at the end of this file."""
    twins, slide = _longnet_twins(golden_dir, name, 1 + CONTROLS, lr=0.0, capture_after=1)
    _run_case(twins, slide, schedule, poison, f"{name}/{schedule}/{poison}")


@pytest.mark.parametrize("schedule,poison", [("eager", "nan_row"), ("replay", "nan_row"), ("replay", "inf_element")])
def test_overflow_titan_configuration_skips_and_recovers(schedule, poison):
    """The TITAN configuration (stand-in backbone; feature gridding by atomic scatter into grid cells): data-induced overflow, eager and
    as a replay.  Measured control-to-control spread: see SPREAD_NOTE."""
    twins, slide = _titan_twins(1 + CONTROLS_BIG, lr=0.0, capture_after=1)
    _run_case(twins, slide, schedule, poison, f"titan/{schedule}/{poison}")


# ------------------------------------------------------------------------------------------ a free-running sequence
def test_overflow_free_running_sequence_backs_off_and_trains(golden_dir):
    """init_scale 2^40, growth_interval 3, 30 step_graphed calls on one slide: the scale finds its level by itself.  A call is skipped
    iff step_dev did not move, and the parameters change iff it moved; the observed (scale, tracker) sequence is
    torch._amp_update_scale_ on the CPU fed the observed skip pattern; no step at a scale <= 2^24 is skipped (2^10 .. 2^24 all work on
    these fixtures: test_train_step_matches_reference_golden) and at least 8 of the 30 steps complete (from 2^40 at most 16 back-offs
    reach 2^24; from there the worst legal pattern is three clean steps and one skip) -- 'skips forever' cannot pass."""
    ((eng, ts),), slide = _longnet_twins(golden_dir, "L37_d3", 1, lr=1e-4, init_scale=2.0 ** 40, growth_interval=3, capture_after=1)
    ts.auto_split = False
    rs, rt = torch.full((1,), 2.0 ** 40), torch.zeros(1, dtype=torch.int32)
    done, log = 0, []
    for i in range(30):
        before, scale_in = eng.store.flat.clone(), float(ts.scale)
        _step(ts, slide, True)
        torch.cuda.synchronize()
        step = int(ts.step_dev)
        skipped = step == done
        assert step in (done, done + 1), (i, step, done)
        assert torch.equal(eng.store.flat, before) == skipped, (i, "the parameters change iff the step counted", skipped)
        torch._amp_update_scale_(rs, rt, torch.tensor([1.0 if skipped else 0.0]), 2.0, 0.5, 3)
        assert float(ts.scale) == float(rs) and int(ts.tracker) == int(rt), (i, float(ts.scale), float(rs), int(ts.tracker), int(rt))
        assert int(ts.found_inf) == 0, i
        assert not (skipped and scale_in <= 2.0 ** 24), (i, "skipped at a scale the fixtures are known to work at", scale_in)
        if not skipped:
            assert np.isfinite(float(ts.loss)) and bool(torch.isfinite(ts.last_logits).all()), i
        log.append((int(np.log2(scale_in)), int(skipped)))
        done = step
    print("overflow-free-running (log2 scale, skipped):", log)
    assert log[0][1] == 1, "2^40 does overflow"
    assert done >= 8, log
    assert ts.graph_replays >= 28 and bool(torch.isfinite(eng.store.flat).all())
    eng.check_inputs()


# ------------------------------------------------------------------------------------------ unscaled_grads()
def test_overflow_unscaled_grads_divide_by_the_scale_the_gradients_carry(golden_dir):
    """unscaled_grads() after an update=False step at scale S equals the same step at 2^12 (1 % on the norms, the bound
    test_train_step_matches_reference_golden uses between scales) -- and after update=True steps whose scaler update GREW or BACKED OFF
    the scale it still divides by the scale the gradients were produced with (TrainStep.grad_scale), not by the next step's."""
    ((eng, ts), (eng2, ts2)), slide = _longnet_twins(golden_dir, "L37_d3", 2, lr=0.0, weight_decay=0.0, growth_interval=1)
    for t in (ts, ts2):
        t.auto_split = False
        t.split_min_patches = 1 << 30

    def norms(grads):
        torch.cuda.synchronize()
        return {k: float(v.double().norm()) for k, v in grads.items()}

    def close(a, b, what):
        top = max(b.values())
        bad = [(k, a[k], b[k]) for k in b if abs(a[k] - b[k]) > 1e-2 * b[k] + 1e-6 * top]
        assert not bad, (what, bad[:5])

    ts2.scale.fill_(2.0 ** 12)
    ts2.step(slide["x"], slide["coords"], slide["genes"], slide["text"], update=False)
    ref = norms(ts2.unscaled_grads())
    assert all(np.isfinite(v) for v in ref.values()) and max(ref.values()) > 0
    for S in (2.0 ** 10, 2.0 ** 20):
        ts.scale.fill_(S)
        ts.step(slide["x"], slide["coords"], slide["genes"], slide["text"], update=False)
        close(norms(ts.unscaled_grads()), ref, f"update=False at {S}")
        assert float(ts.scale) == S == float(ts.grad_scale)
    # update=True, growth_interval = 1: the scaler doubles the scale behind the step (lr = 0, no decay: the weights stay)
    ts.scale.fill_(2.0 ** 14)
    ts.step(slide["x"], slide["coords"], slide["genes"], slide["text"], update=True)
    torch.cuda.synchronize()
    assert float(ts.scale) == 2.0 ** 15 and float(ts.grad_scale) == 2.0 ** 14 and int(ts.step_dev) == 1
    close(norms(ts.unscaled_grads()), ref, "after a growth")
    # ... and through step_graphed (eager visits, capture, replay), growing every time
    for i in range(4):
        s_in = float(ts.scale)
        ts.step_graphed(slide["x"], slide["coords"], slide["genes"], slide["text"])
        torch.cuda.synchronize()
        assert float(ts.scale) == 2.0 * s_in and float(ts.grad_scale) == s_in
        close(norms(ts.unscaled_grads()), ref, f"step_graphed visit {i}")
    assert ts.graph_replays >= 1
    # a back-off: the skipped step's gradients are not finite, and grad_scale still names the scale they were produced with
    ts.scale.fill_(OVERFLOW_SCALE)
    ts.step(slide["x"], slide["coords"], slide["genes"], slide["text"], update=True)
    torch.cuda.synchronize()
    assert float(ts.scale) == 0.5 * OVERFLOW_SCALE and float(ts.grad_scale) == OVERFLOW_SCALE and int(ts.step_dev) == 5
    assert not all(bool(torch.isfinite(v).all()) for v in ts.unscaled_grads().values())


# ------------------------------------------------------------------------------------------ nn.Module bridge + torch.amp.GradScaler
def _bridge_model():
    from modaltune_amd.aggregators import Aggregator
    seed, ngrids = 53, 64
    sizes = synth.toy_group_sizes()
    groups = {i: ["g"] * n for i, n in enumerate(sizes)}
    model = Aggregator.create("longnetvit_gene_adapter", gene_group_defination=groups, multi_task=3,
                              **dict(GIGAPATH_JSON, depth=3, slide_ngrids=ngrids, interaction_indexes=[[0, 0], [1, 1], [2, 2]], dropout=0.0,
                                     drop_path_rate=0.0))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(model.cfg, sizes, seed).items()}, strict=True)
    model.train()
    return model, sizes, seed, ngrids


@pytest.mark.parametrize("mode", ["eager_bridge", "graph_replay"])
def test_overflow_module_bridge_under_the_real_gradscaler(mode):
    """The reference trainer's loop -- three task calls, ONE scaler.scale(loss).backward(), scaler.step(opt), scaler.update() -- on the
    drop-in module with modaltune_amd.optim.AdamW and torch.amp.GradScaler(init_scale 2^15, growth_interval 2): one clean iteration, one
    with a NaN feature row, one whose loss has an inf gradient in one logit, three clean.  The poisoned iterations leave every trainable
    parameter bit-identical, halve the scale and do not advance the optimiser's step count; afterwards the gradients are finite, and
    after two more clean iterations the parameters and both moments equal control models that ran the clean iterations only
    (control-to-control rule; clean iterations at lr = 0 up to there, poisoned ones at 1e-3: module docstring; the loss scale is a
    power of two and the bridge rescales the incoming gradient to max |.| = 2^10 anyway, so the controls' different scale history
    changes nothing).  The last clean iteration runs at lr = 1e-3 and moves the parameters.
    Last: a loss scaled by 1e-42 -- every incoming dlogit below 3e-36 -- must return finite .grads (mt_absmax_scale's tiny maximum).
    Once on the eager bridge, once in the graph-replay steady state of module_graph.py."""
    from modaltune_amd.optim import AdamW
    replay = mode == "graph_replay"
    models = []
    for _ in range(1 + CONTROLS_BIG):
        model, sizes, seed, ngrids = _bridge_model()
        model._replay.enabled = replay
        train = [p for p in model.parameters() if p.requires_grad]
        opt = AdamW([{"params": train, "lr": 1e-3}], lr=1e-3, weight_decay=0.01, betas=(0.9, 0.999))
        scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 15, growth_interval=2)
        models.append((model, train, opt, scaler))
    inp = synth.synth_inputs(300, sizes, seed, grid=ngrids)
    x, c = torch.from_numpy(inp["x"]).cuda(), torch.from_numpy(inp["coords"]).cuda()
    x = x.reshape(-1, x.shape[-1]).contiguous()
    genes = {i: torch.from_numpy(a).cuda() for i, a in enumerate(inp["genes"])}
    eye = torch.eye(3, device="cuda")
    w = torch.randn(3, 256, generator=torch.Generator().manual_seed(1)).cuda()
    x_nan = x.clone()
    x_nan[150, :] = NAN

    def loss_of(model, kind):
        xs = (x_nan if kind == "nan_row" else x).clone()
        ys = [model(x=xs, coords=c, genes=genes, task_token=eye[t].clone()) for t in range(3)]
        loss = sum((y * w[t]).sum() for t, y in enumerate(ys))
        if kind == "inf_logit":
            loss = loss + ys[1].reshape(-1)[7] * INF          # d loss / d logit = inf in one logit
        if kind == "tiny":
            loss = loss * 1e-42
        return loss

    def steps_of(opt):
        return {float(s["step"]) for s in opt.state_dict()["state"].values()}

    def iteration(entry, kind, lr):
        model, train, opt, scaler = entry
        for grp in opt.param_groups:
            grp["lr"] = lr
        before = [p.detach().clone() for p in train]
        count, scale = steps_of(opt), scaler.get_scale()
        scaler.scale(loss_of(model, kind)).backward()
        finite = all(bool(torch.isfinite(p.grad).all()) for p in train)
        scaler.step(opt)
        scaler.update()
        opt.zero_grad()
        torch.cuda.synchronize()
        same = all(torch.equal(p.detach(), b) for p, b in zip(train, before))
        if kind == "clean":
            assert finite, "a clean iteration produces finite gradients"
            assert opt.last_step_fused is True and steps_of(opt) == {max(count, default=0.0) + 1.0}
            assert same == (lr == 0.0), "a clean iteration at lr > 0 moves the parameters"
        else:
            assert not finite
            assert same, (kind, "a parameter moved on a skipped iteration")
            assert scaler.get_scale() == 0.5 * scale, (kind, scaler.get_scale(), scale)
            assert steps_of(opt) == count, (kind, steps_of(opt), count)

    if replay:       # enter the steady state: eager visits, priming visits, capture (gradients thrown away: the weights stay)
        for entry in models:
            model, train, opt, scaler = entry
            for _ in range(6):
                loss_of(model, "clean").backward()
                opt.zero_grad()
            assert model._replay.captures == 1 and model._replay.replays >= 1
    victim, controls = models[0], models[1:]
    n0 = victim[0]._replay.replays
    # clean iterations at lr = 0, poisoned ones at 1e-3 (module docstring: why the comparisons run at lr = 0)
    for kind in ("clean", "nan_row", "inf_logit", "clean", "clean"):
        iteration(victim, kind, 0.0 if kind == "clean" else POISON_LR)
        if kind == "clean":
            for ctl in controls:
                iteration(ctl, kind, 0.0)
    assert all(steps_of(e[2]) == {3.0} for e in models)

    def tensors(entry):
        st = entry[2].state_dict()["state"]
        return dict(params=torch.cat([p.detach().reshape(-1) for p in entry[1]]),
                    exp_avg=torch.cat([st[i]["exp_avg"].reshape(-1) for i in sorted(st)]),
                    exp_avg_sq=torch.cat([st[i]["exp_avg_sq"].reshape(-1) for i in sorted(st)]))
    _judge("overflow-bridge " + mode, tensors(victim), [tensors(c) for c in controls])
    # ... and training goes on: one clean iteration at a real learning rate
    for entry in models:
        iteration(entry, "clean", POISON_LR)
    assert steps_of(victim[2]) == {4.0} and all(bool(torch.isfinite(p).all()) for p in victim[1])
    if replay:
        assert victim[0]._replay.replays == n0 + 6 and victim[0]._replay.captures == 1, "every iteration was served by graph replays"
    else:
        assert victim[0]._replay.replays == 0
    # a nearly converged loss: every incoming dlogit is below ~target / FLT_MAX
    model, train, opt, scaler = victim
    loss_of(model, "tiny").backward()
    torch.cuda.synchronize()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in train), "0 * inf in the bridge's loss scale"
    opt.zero_grad()


SPREAD_NOTE = """Measured on an MI355X when these tests first ran (largest relative max-norm distance among the control twins after the same
clean steps, lr = 0): parameters, loss and logits 0 (bit-identical) under every schedule; first moment 1.2e-8 .. 3.3e-8 at L = 37,
2.0e-6 .. 5.7e-6 at L = 1500, 1.2e-8 .. 2.2e-8 on the TITAN configuration, 1.9e-8 .. 2.6e-8 on the nn.Module bridge; second moment
2.4e-9 .. 9.4e-9, 3.2e-7 .. 2.1e-6, 7.5e-10 .. 1.5e-9 and 4.3e-9.  `pytest -s -k overflow` prints the figures of every case (lines
'overflow-recovery' / 'overflow-bridge').  2^40 overflows both fixtures; the free-running sequence settles between 2^29 and 2^30."""
