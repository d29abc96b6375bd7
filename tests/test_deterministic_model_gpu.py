"""GPU: the train step in the deterministic mode (Engine(deterministic=True) / MT_DETERMINISTIC=1): the reference golden's bars hold as
they do for the default path, and weights, moments, gradients and loss are comparable with torch.equal -- across runs, across the
eager step and its hipGraph replay, across interleavings of the two pass groups, and through the nn.Module bridge.  With the mode off
the step launches what it launched before."""
import os
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from modaltune_amd import ops, synth  # noqa: E402

from test_model_gpu import GRAD_TOL_NAMED, _build, _rel  # noqa: E402

GRAD_TOL = 1e-2       # test_model_gpu.py::test_train_step_matches_reference_golden: every gradient norm and full tensor (named exceptions aside)


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _build_det(monkeypatch, golden_dir, name, on=True):
    """test_model_gpu._build with the mode switched through the environment (its Engine(...) call passes no argument)."""
    monkeypatch.setenv("MT_DETERMINISTIC", "1" if on else "0")
    g, cfg, eng, ts, inp = _build(os.path.join(golden_dir, f"model_{name}.npz"))
    assert eng.deterministic is on and ts.deterministic is on
    x = torch.from_numpy(inp["x"]).cuda()
    genes = [torch.from_numpy(a).cuda() for a in inp["genes"]]
    return g, cfg, eng, ts, inp, x, genes, torch.from_numpy(inp["text"]).cuda()


def _state(eng, ts):
    torch.cuda.synchronize()
    return {"flat": eng.store.flat.clone(), "flat_grad": eng.store.flat_grad.clone(), "m": ts.m.clone(), "v": ts.v.clone(),
            "scale": ts.scale.clone(), "step_dev": ts.step_dev.clone(), "loss": ts.loss.clone()}


def _assert_same_bits(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k, float((a[k].double() - b[k].double()).abs().max()))


@pytest.mark.parametrize("name", ["L37_d3", "L1500_d3"])
def test_deterministic_step_matches_reference_golden(golden_dir, monkeypatch, name):
    """test_model_gpu.py::test_train_step_matches_reference_golden's checks and bars on the deterministic engine."""
    _gpu()
    g, cfg, eng, ts, inp, x, genes, text = _build_det(monkeypatch, golden_dir, name)
    loss = ts.step(x, inp["coords"], genes, text, update=False)
    torch.cuda.synchronize()
    assert _rel(ts.last_logits.cpu().numpy(), g["f64_logits"]) < 1e-3
    assert abs(float(loss) - float(g["f64_loss"])) / abs(float(g["f64_loss"])) < 1e-3
    assert int(ts.found_inf) == 0
    grads = ts.unscaled_grads()
    names = [str(n) for n in g["f64_grad_names"]]
    assert len(names) == 244
    ours = np.array([float(grads[n].double().norm()) for n in names])
    ref = g["f64_grad_norms"]
    bad = [(n, o, r) for n, o, r in zip(names, ours, ref) if abs(o - r) > GRAD_TOL_NAMED.get(n, GRAD_TOL) * r + 1e-6 * ref.max()]
    assert not bad, bad[:10]
    for k in g.files:
        if k.startswith("f64_grad/"):
            key = k[len("f64_grad/"):]
            err = np.linalg.norm(grads[key].double().cpu().numpy() - g[k]) / (np.linalg.norm(g[k]) + 1e-300)
            assert err < (GRAD_TOL_NAMED[key] if key == "gene_encoder.pathway_compression.weight" else GRAD_TOL), (k, err)


def test_two_fresh_engines_train_to_the_same_bits(golden_dir, monkeypatch):
    """Train mode (Dropout / DropPath on, same seed), three optimiser steps at L = 1500 on two engines built from scratch."""
    _gpu()
    runs = []
    for _ in range(2):
        g, cfg, eng, ts, inp, x, genes, text = _build_det(monkeypatch, golden_dir, "L1500_d3")
        eng.set_stochastic(True, seed=1234)
        losses = []
        for _ in range(3):
            ts.step(x, inp["coords"], genes, text, update=True)
            losses.append(ts.loss.clone())
        st = _state(eng, ts)
        st["losses"] = torch.cat(losses)
        assert int(ts.step_dev) == 3 and bool(torch.isfinite(st["flat"]).all())
        runs.append(st)
        del eng, ts
    _assert_same_bits(runs[0], runs[1], "run 0 against run 1")
    assert len(set(runs[0]["losses"].tolist())) == 3          # (the steps did move: three different losses)


def test_graph_replay_equals_the_eager_step_bit_for_bit(golden_dir, monkeypatch):
    """test_model_gpu.py::test_graph_replay_matches_eager needs 2.5 * 5 * lr on three tensors; here every parameter and both moments are
    torch.equal after five steps (two eager warm-ups, the capture, replays)."""
    _gpu()
    g, cfg, eng_a, ts_a, inp, x, genes, text = _build_det(monkeypatch, golden_dir, "L37_d3")
    _, _, eng_b, ts_b, _, _, _, _ = _build_det(monkeypatch, golden_dir, "L37_d3")
    la, lb = [], []
    for _ in range(5):
        ts_a.step(x, inp["coords"], genes, text, update=True)
        la.append(ts_a.loss.clone())
        ts_b.step_graphed(x, inp["coords"], genes, text)
        lb.append(ts_b.loss.clone())
    torch.cuda.synchronize()
    assert ts_b._graphs is not None and ts_b.graph_replays >= 2
    assert int(ts_a.step_dev) == int(ts_b.step_dev) == 5
    assert torch.equal(torch.cat(la), torch.cat(lb))
    _assert_same_bits(_state(eng_a, ts_a), _state(eng_b, ts_b), "eager against graph replay")


def test_pass_group_interleavings_give_the_same_gradient_bits(golden_dir, monkeypatch):
    """The two pass groups forced at L = 1500, the host pausing 0 / 2 / 10 ms between the groups' enqueues (so that the second group's
    kernels meet the first group's at different points), and the whole thing twice."""
    _gpu()
    g, cfg, eng, ts, inp, x, genes, text = _build_det(monkeypatch, golden_dir, "L1500_d3")
    ts.split_passes, ts.split_min_patches = True, 0
    assert ts._split_now(int(g["L"])) and not ts.auto_split
    seen = []
    for rep in range(2):
        for pause in (0.0, 0.002, 0.010):
            ts._group_hook = (lambda gi, p=pause: time.sleep(p)) if pause else None
            ts.step(x, inp["coords"], genes, text, update=False)
            torch.cuda.synchronize()
            seen.append((rep, pause, eng.store.flat_grad.clone(), ts.loss.clone()))
    ts._group_hook = None
    assert ts._pass_streams is not None and ts.split_decisions == {}
    assert float(seen[0][2].abs().max()) > 0
    for rep, pause, fg, loss in seen[1:]:
        assert torch.equal(fg, seen[0][2]) and torch.equal(loss, seen[0][3]), (rep, pause, float((fg - seen[0][2]).abs().max()))


def _module_run(sizes, inp, json_cfg, replay: bool, slides: int = 4):
    """The loop of test_model_gpu.py::test_fresh_constructor_trains_under_the_reference_loop (three model calls under autocast, KL loss,
    GradScaler) with the package's fused AdamW; returns (state_dict copy, replays)."""
    import torch.nn as nn
    import torch.nn.functional as F
    from modaltune_amd.aggregators import Aggregator
    from modaltune_amd.optim import AdamW
    groups = {i: ["g%d_%d" % (i, j) for j in range(n)] for i, n in enumerate(sizes)}
    model = Aggregator.create(subclass_name="longnetvit_gene_adapter", gene_group_defination=groups, **json_cfg, multi_task=3, init_seed=0,
                              deterministic=True).to("cuda")
    assert model.engine.deterministic
    rp = model._replay
    rp.enabled, rp.capture_after = bool(replay), 0        # (0: two priming visits, then the capture -- the fourth slide replays)
    opt = AdamW([{"params": [p for p in model.parameters() if p.requires_grad], "lr": 1e-3}], weight_decay=0.01, betas=(0.9, 0.999))
    scaler = torch.amp.GradScaler("cuda", enabled=True, init_scale=2.0 ** 15)
    images, coords = torch.from_numpy(inp["x"]).cuda(), torch.from_numpy(inp["coords"]).cuda()
    gene_data = {i: torch.from_numpy(a).cuda() for i, a in enumerate(inp["genes"])}
    text = torch.from_numpy(inp["text"]).cuda()[:, :256]
    text = text / text.norm(dim=-1, keepdim=True)
    target = F.softmax(text[[0, 1, 3], :], dim=1)
    loss_fn, eye = nn.KLDivLoss(reduction="sum"), torch.eye(3).cuda()
    model.train()
    for _ in range(slides):
        xs = images.clone()
        with torch.autocast("cuda", enabled=True):
            logit = torch.cat([model(x=xs, coords=coords, genes=gene_data, clinical=[], task_token=eye[t]) for t in (0, 1, 2)], dim=0)
            logit = logit / logit.norm(dim=-1, keepdim=True)
            loss = loss_fn(F.log_softmax(logit, dim=1), target) * 10
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        opt.zero_grad()
    torch.cuda.synchronize()
    assert np.isfinite(float(loss.detach()))
    return {k: v.detach().clone() for k, v in model.state_dict().items()}, rp.replays


def test_module_path_trains_to_the_same_bits_replayed_or_eager():
    """Aggregator.create(..., deterministic=True) + modaltune_amd.optim.AdamW + GradScaler under the reference loop, four slides: two
    runs give torch.equal state_dicts (stochastic layers as shipped), and -- with Dropout / DropPath at 0, because the eager bridge and
    the replay number their masks differently -- the run that reaches graph replay equals the run on the eager bridge."""
    _gpu()
    from test_init_cpu import SHIPPED_JSON
    sizes = synth.toy_group_sizes(6)
    inp = synth.synth_inputs(700, sizes, 5, grid=128)
    base = dict(SHIPPED_JSON, depth=3, interaction_indexes=[[0, 0], [1, 1], [2, 2]], slide_ngrids=128, pretrained=False)
    sd_a, rep_a = _module_run(sizes, inp, base, replay=True)
    sd_b, rep_b = _module_run(sizes, inp, base, replay=True)
    assert rep_a >= 1 and rep_b == rep_a
    _assert_same_bits(sd_a, sd_b, "module run 0 against run 1")
    plain = dict(base, dropout=0.0, drop_path_rate=0.0)
    sd_r, rep_r = _module_run(sizes, inp, plain, replay=True)
    sd_e, rep_e = _module_run(sizes, inp, plain, replay=False)
    assert rep_r >= 1 and rep_e == 0
    _assert_same_bits(sd_r, sd_e, "graph replay against the eager bridge")
    assert any(not torch.equal(sd_r[k], sd_a[k]) for k in sd_r)          # (the masks of the first pair did act)


def test_mode_off_launches_what_the_default_engine_launches(golden_dir, monkeypatch):
    """deterministic=False against the argument omitted (no switch set): the same launch names in the same order in ops.TIMELINE, none
    of them a `_det` one; the deterministic engine's step differs from it in exactly those names."""
    _gpu()
    from modaltune_amd.engine import Engine
    from modaltune_amd.trainer import TrainStep
    monkeypatch.delenv("MT_DETERMINISTIC", raising=False)
    g, cfg, eng0, ts0, inp = _build(os.path.join(golden_dir, "model_L1500_d3.npz"))
    assert eng0.deterministic is False
    x = torch.from_numpy(inp["x"]).cuda()
    genes = [torch.from_numpy(a).cuda() for a in inp["genes"]]
    text = torch.from_numpy(inp["text"]).cuda()
    sizes = [int(s) for s in g["sizes"]]

    def engine(det):
        eng = Engine(cfg, sizes, "cuda", deterministic=det)
        eng.load_state_dict(synth.synth_state_dict(cfg, sizes, int(g["seed"])))
        ts = TrainStep(eng)
        ts.set_projector(synth.projector_state(int(g["seed"])))
        return eng, ts

    def names(ts):
        ts.step(x, inp["coords"], genes, text, update=False)          # (first step: allocations)
        torch.cuda.synchronize()
        monkeypatch.setattr(ops, "TIMER", {})
        monkeypatch.setattr(ops, "TIMELINE", [])
        ts.step(x, inp["coords"], genes, text, update=False)
        torch.cuda.synchronize()
        out = [rec[0] for rec in ops.TIMELINE]
        monkeypatch.setattr(ops, "TIMER", None)
        monkeypatch.setattr(ops, "TIMELINE", None)
        return out
    omitted = names(ts0)
    off = names(engine(False)[1])
    on = names(engine(True)[1])
    assert len(omitted) > 100 and off == omitted
    assert not [n for n in omitted if "_det" in n]
    assert [n.replace("_det", "") for n in on] == omitted and sum("_det" in n for n in on) >= 20
