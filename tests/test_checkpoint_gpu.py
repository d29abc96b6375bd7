"""GPU: TrainStep.state_dict() / load_state_dict() and the replica canary at world size 1, on the model_L37_d3 golden's model
(L = 37, depth 3; test_model_gpu._build).  Every "equal" is torch.equal: a resumed run continues with the uninterrupted run's bits
(deterministic engine, MT_DETERMINISTIC=1, as test_deterministic_model_gpu._build_det switches it), and a load is a copy."""
import json
import os
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

from modaltune_amd import ops, synth  # noqa: E402

from test_model_gpu import _build  # noqa: E402

STATE = ("flat", "m", "v", "scale", "tracker", "step_dev", "rng")


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _other_trainables(cfg, sizes, seed, other_seed):
    """The frozen tensors of `seed` (a checkpoint without include_frozen leaves the backbone to the run that resumes, as the reference
    leaves it to slide_encoder.pth) with the TRAINABLE tensors of `other_seed`."""
    state = synth.synth_state_dict(cfg, sizes, seed)
    other = synth.synth_state_dict(cfg, sizes, other_seed)
    for k in synth.trainable_keys(cfg, sizes):
        state[k] = other[k]
    return state


def _fresh(monkeypatch, golden_dir, det=True, weights_seed=None, stochastic=None, **ts_kw):
    """_build on the L37_d3 golden; ts_kw: a TrainStep of its own on that engine; weights_seed: other trainable weights than the
    golden's (a load that does nothing then fails); stochastic: Dropout / DropPath on with that Philox seed."""
    from modaltune_amd.trainer import TrainStep
    if det:
        monkeypatch.setenv("MT_DETERMINISTIC", "1")
    else:
        monkeypatch.delenv("MT_DETERMINISTIC", raising=False)
    g, cfg, eng, ts, inp = _build(os.path.join(golden_dir, "model_L37_d3.npz"))
    assert eng.deterministic is det
    sizes = [int(s) for s in g["sizes"]]
    if weights_seed is not None:
        eng.load_state_dict(_other_trainables(cfg, sizes, int(g["seed"]), weights_seed))
    if ts_kw:
        ts = TrainStep(eng, **ts_kw)
        ts.set_projector(synth.projector_state(int(g["seed"])))
    if stochastic is not None:
        eng.set_stochastic(True, seed=stochastic)
    slide = (torch.from_numpy(inp["x"]).cuda(), inp["coords"], [torch.from_numpy(a).cuda() for a in inp["genes"]],
             torch.from_numpy(inp["text"]).cuda())
    return eng, ts, slide, (cfg, sizes, int(g["seed"]))


def _state(eng, ts):
    torch.cuda.synchronize()
    return {"flat": eng.store.flat.clone(), "m": ts.m.clone(), "v": ts.v.clone(), "scale": ts.scale.clone(), "tracker": ts.tracker.clone(),
            "step_dev": ts.step_dev.clone(), "rng": eng.rng.clone()}


def _assert_equal(a, b, what):
    for k in STATE:
        assert torch.equal(a[k], b[k]), (what, k, float((a[k].double() - b[k].double()).abs().max()))


def _through_a_file(sd, tmp_path, name="ck.pt"):
    path = str(tmp_path / name)
    torch.save(sd, path)
    return torch.load(path, map_location="cpu", weights_only=True)


def test_resumed_run_equals_the_uninterrupted_run(golden_dir, monkeypatch, tmp_path):
    """Train mode, growth_interval = 4 (the loss scale doubles at step 4, behind the cut): six eager steps against three steps, a
    checkpoint through torch.save / torch.load(weights_only=True), a FRESH engine on other weights and another Philox seed, three steps."""
    _gpu()
    from modaltune_amd import checkpoint
    eng_a, ts_a, slide, _ = _fresh(monkeypatch, golden_dir, stochastic=1234, growth_interval=4)
    losses_a = []
    for _ in range(6):
        ts_a.step(*slide)
        losses_a.append(ts_a.loss.clone())
    end_a = _state(eng_a, ts_a)
    assert int(ts_a.step_dev) == 6 and float(ts_a.scale) == 2.0 ** 16 and int(ts_a.tracker) == 2
    eng_b, ts_b, _, _ = _fresh(monkeypatch, golden_dir, stochastic=1234, growth_interval=4)
    for _ in range(3):
        ts_b.step(*slide)
    sd = ts_b.state_dict()
    path = str(tmp_path / "step3.pt")
    torch.save(sd, path)
    back = checkpoint.verify_file(path)          # (the device's checksums hold on the CPU)
    assert sorted(back) == sorted(checkpoint.REQUIRED_KEYS) and back["window"] is None and back["world"] == 1
    assert set(back["model"]) == set(eng_b.store.slots) and back["stochastic"] is True
    del eng_b, ts_b
    eng_c, ts_c, _, _ = _fresh(monkeypatch, golden_dir, weights_seed=99, stochastic=4321, growth_interval=4)
    assert not torch.equal(eng_c.store.flat, eng_a.store.flat)
    with warnings.catch_warnings():
        warnings.simplefilter("error")          # (same build: no warning)
        ts_c.load_state_dict(back)
    losses_c = []
    for _ in range(3):
        ts_c.step(*slide)
        losses_c.append(ts_c.loss.clone())
    _assert_equal(end_a, _state(eng_c, ts_c), "uninterrupted against resumed")
    assert torch.equal(torch.cat(losses_a[3:]), torch.cat(losses_c))
    assert len(set(torch.cat(losses_a).tolist())) == 6


def test_load_into_a_step_that_has_already_captured(golden_dir, monkeypatch):
    """A TrainStep that replays its geometry loads another run's checkpoint IN PLACE: no tensor is re-bound, the captured graphs stay
    and go on replaying, and its next replays equal that run's (eager) continuation -- which they can only do with the fp16 operand
    caches refreshed.  The stochastic layers stay ON: an eager step and a replayed step draw the same masks in train mode
    (test_deterministic_model_gpu.py::test_graph_replay_equals_the_eager_step_bit_for_bit's comparison run with set_stochastic(True, seed)
    on both engines gave equal losses, parameters, moments and Philox counters over five steps)."""
    _gpu()
    eng_r, ts_r, slide, _ = _fresh(monkeypatch, golden_dir, stochastic=55)
    for _ in range(3):
        ts_r.step(*slide)
    sd = ts_r.state_dict()
    losses_r = []
    for _ in range(2):
        ts_r.step(*slide)
        losses_r.append(ts_r.loss.clone())
    end_r = _state(eng_r, ts_r)
    eng_c, ts_c, _, _ = _fresh(monkeypatch, golden_dir, weights_seed=99, stochastic=66)
    for _ in range(4):
        ts_c.step_graphed(*slide)
    torch.cuda.synchronize()
    assert ts_c._graphs is not None and ts_c.graph_replays == 2
    tensors = (eng_c.store.flat, eng_c.store.flat_grad, ts_c.m, ts_c.v, ts_c.scale, ts_c.grad_scale, ts_c.tracker, ts_c.step_dev, ts_c.lr_dev,
               eng_c.rng, ts_c.found_inf)
    ptrs, gen, graphs = [t.data_ptr() for t in tensors], eng_c.generation, ts_c._graphs
    cache_ptrs = {k: w.w.data_ptr() for k, w in eng_c._train16.items()}
    ts_c.load_state_dict(sd)
    assert [t.data_ptr() for t in (eng_c.store.flat, eng_c.store.flat_grad, ts_c.m, ts_c.v, ts_c.scale, ts_c.grad_scale, ts_c.tracker,
                                   ts_c.step_dev, ts_c.lr_dev, eng_c.rng, ts_c.found_inf)] == ptrs
    assert eng_c.generation == gen and {k: w.w.data_ptr() for k, w in eng_c._train16.items()} == cache_ptrs
    losses_c = []
    for _ in range(2):
        ts_c.step_graphed(*slide)
        losses_c.append(ts_c.loss.clone())
    assert ts_c.graph_replays == 4 and ts_c.eager_steps == 2 and ts_c._graphs == graphs          # the same graphs went on replaying
    _assert_equal(end_r, _state(eng_c, ts_c), "eager continuation against replays behind a load")
    assert torch.equal(torch.cat(losses_r), torch.cat(losses_c))


def test_mid_window_checkpoint_resumes_the_window(golden_dir, monkeypatch, tmp_path):
    """accumulate = 3, saved after two micro-steps: the resumed boundary and the following window equal the uninterrupted run; a step
    with accumulate = 2 refuses the file."""
    _gpu()
    eng_a, ts_a, slide, _ = _fresh(monkeypatch, golden_dir, stochastic=7, accumulate=3)
    marks, losses_a = [], []
    for i in range(6):
        ts_a.step(*slide)
        losses_a.append(ts_a.loss.clone())
        if i in (2, 5):
            marks.append(_state(eng_a, ts_a))
    assert int(ts_a.step_dev) == 2 and ts_a.window_pos == 0
    eng_b, ts_b, _, _ = _fresh(monkeypatch, golden_dir, stochastic=7, accumulate=3)
    for _ in range(2):
        ts_b.step(*slide)
    assert ts_b.window_pos == 2
    sd = _through_a_file(ts_b.state_dict(), tmp_path)
    assert sd["window"]["pos"] == 2 and sd["window"]["accumulate"] == 3 and tuple(sd["window"]["grad"].shape) == (eng_b.store.n_flat,)
    del eng_b, ts_b
    eng_c, ts_c, _, _ = _fresh(monkeypatch, golden_dir, weights_seed=99, stochastic=8, accumulate=3)
    ts_c.load_state_dict(sd)
    assert ts_c.window_pos == 2
    losses_c = []
    for i in range(4):
        ts_c.step(*slide)
        losses_c.append(ts_c.loss.clone())
        if i in (0, 3):
            _assert_equal(marks[0 if i == 0 else 1], _state(eng_c, ts_c), f"window boundary behind resumed call {i}")
    assert torch.equal(torch.cat(losses_a[2:]), torch.cat(losses_c))
    eng_d, ts_d, _, _ = _fresh(monkeypatch, golden_dir, stochastic=7, accumulate=2)
    before = _state(eng_d, ts_d)
    with pytest.raises(ValueError, match="accumulate=3"):
        ts_d.load_state_dict(sd)
    _assert_equal(before, _state(eng_d, ts_d), "a refused load touches nothing")


def test_default_engine_round_trip_leaves_the_state_and_steps_on(golden_dir, monkeypatch):
    _gpu()
    eng, ts, slide, _ = _fresh(monkeypatch, golden_dir, det=False)
    for _ in range(2):
        ts.step(*slide)
    before = _state(eng, ts)
    sd = ts.state_dict(include_frozen=True)
    assert set(sd["model"]) == set(eng.store.tensors) and len(sd["model"]) > len(eng.store.slots)
    gen = eng.generation
    ts.load_state_dict(sd)
    _assert_equal(before, _state(eng, ts), "load_state_dict(state_dict())")
    assert eng.generation == gen          # (the frozen tensors did not change: their caches were not rebuilt)
    ts.step(*slide)
    assert int(ts.step_dev) == 3 and bool(torch.isfinite(ts.loss).all()) and bool(torch.isfinite(eng.store.flat).all())
    assert not torch.equal(eng.store.flat, before["flat"])


def test_interop_with_the_module_path_both_ways():
    """sd["optimizer"] / sd["scaler"] load into modaltune_amd.optim.AdamW, torch.optim.AdamW and torch's GradScaler over a drop-in
    model of the same configuration, and the dict assembled from those three loads into a TrainStep."""
    _gpu()
    from modaltune_amd.aggregators import Aggregator
    from modaltune_amd.engine import Engine
    from modaltune_amd.optim import AdamW
    from modaltune_amd.trainer import TrainStep
    from test_init_cpu import SHIPPED_JSON
    sizes = synth.toy_group_sizes(6)
    base = dict(SHIPPED_JSON, depth=3, interaction_indexes=[[0, 0], [1, 1], [2, 2]], slide_ngrids=128, pretrained=False)
    groups = {i: ["g%d_%d" % (i, j) for j in range(n)] for i, n in enumerate(sizes)}
    model = Aggregator.create(subclass_name="longnetvit_gene_adapter", gene_group_defination=groups, **base, multi_task=3, init_seed=0).to("cuda")

    def fused(seed):
        eng = Engine(model.cfg, sizes, "cuda")
        eng.load_state_dict(synth.synth_state_dict(model.cfg, sizes, seed))
        ts = TrainStep(eng, lr=1e-3, init_scale=2.0 ** 12, growth_interval=2)
        ts.set_projector(synth.projector_state(seed))
        return eng, ts
    eng, ts = fused(3)
    inp = synth.synth_inputs(150, sizes, 5, grid=128)
    slide = (torch.from_numpy(inp["x"]).cuda(), inp["coords"], [torch.from_numpy(a).cuda() for a in inp["genes"]], torch.from_numpy(inp["text"]).cuda())
    for _ in range(3):
        ts.step(*slide)
    sd = ts.state_dict(include_frozen=True)
    assert float(ts.scale) == 2.0 ** 13 and int(ts.step_dev) == 3
    # fused -> module path
    model.load_state_dict(sd["model"], strict=True)
    trainable = [(k, p) for k, p in model.named_parameters() if p.requires_grad]
    assert [k for k, _ in trainable] == list(eng.store.slots)
    for cls in (AdamW, torch.optim.AdamW):
        opt = cls([p for _, p in trainable], lr=5.0)
        opt.load_state_dict(sd["optimizer"])
        assert opt.param_groups[0]["lr"] == 1e-3 and opt.param_groups[0]["weight_decay"] == 0.01
        for k, p in trainable:
            o, n, shape = eng.store.slots[k]
            assert torch.equal(opt.state[p]["exp_avg"], ts.m[o:o + n].view(shape)), k
            assert torch.equal(opt.state[p]["exp_avg_sq"], ts.v[o:o + n].view(shape)), k
            assert float(opt.state[p]["step"]) == 3.0
    scaler = torch.amp.GradScaler("cuda", enabled=True, init_scale=2.0)
    scaler.load_state_dict(sd["scaler"])
    assert scaler.get_scale() == 2.0 ** 13 and scaler.get_growth_interval() == 2
    # module path -> fused: a TrainStep on other weights, from the dict a module-path trainer would assemble
    opt = AdamW([p for _, p in trainable], lr=5.0)
    opt.load_state_dict(sd["optimizer"])
    assembled = {"model": model.state_dict(), "optimizer": opt.state_dict(), "scaler": scaler.state_dict()}
    eng2, ts2 = fused(4)
    rng2 = eng2.rng.clone()
    assert not torch.equal(eng2.store.flat, eng.store.flat)
    ts2.load_state_dict(assembled)
    torch.cuda.synchronize()
    for a, b in ((ts2.m, ts.m), (ts2.v, ts.v), (ts2.scale, ts.scale), (ts2.step_dev, ts.step_dev), (ts2.tracker, ts.tracker),
                 (eng2.store.flat, eng.store.flat)):
        assert torch.equal(a, b)
    for k, t in eng.store.tensors.items():
        assert torch.equal(eng2.store.tensors[k], t), k          # (the frozen tensors came along)
    assert torch.equal(eng2.rng, rng2) and ts2.window_pos == 0 and ts2.lr == 1e-3          # the Philox state stays, the window is empty
    ts2.step(*slide)
    ts.step(*slide)
    assert bool(torch.isfinite(ts2.loss).all())
    # per-parameter step counts that disagree map to no single device counter
    assembled["optimizer"]["state"][3]["step"] = torch.tensor(9.0)
    with pytest.raises(ValueError, match="disagree"):
        ts2.load_state_dict(assembled)


def test_refusals(golden_dir, monkeypatch):
    _gpu()
    from modaltune_amd.engine import Engine
    from modaltune_amd.trainer import TrainStep
    eng, ts, slide, (cfg, sizes, seed) = _fresh(monkeypatch, golden_dir)
    ts.step(*slide)
    sd = ts.state_dict()
    before = _state(eng, ts)
    # another pathway grouping: the gene encoder's shapes differ
    sizes2 = [s + 1 for s in sizes]
    eng2 = Engine(cfg, sizes2, "cuda")
    eng2.load_state_dict(synth.synth_state_dict(cfg, sizes2, seed))
    other = TrainStep(eng2).state_dict()
    with pytest.raises(ValueError, match=r"gene_encoder\..* has shape"):
        ts.load_state_dict(other)
    with pytest.raises(ValueError, match="stochastic=True"):
        ts.load_state_dict(dict(sd, stochastic=True))
    with pytest.raises(ValueError, match="format"):
        ts.load_state_dict(dict(sd, format=7))
    with pytest.raises(KeyError, match="rng"):
        ts.load_state_dict({k: v for k, v in sd.items() if k != "rng"})
    _assert_equal(before, _state(eng, ts), "refused loads touch nothing")
    # one moved element of m: the device checksum behind the copy does not match the recorded one
    sd["optimizer"]["state"][5]["exp_avg"].view(-1)[0] += 1.0
    with pytest.raises(RuntimeError, match="checksum of `m`"):
        ts.load_state_dict(sd)
    ts.load_state_dict(sd, verify=False)          # (asked not to look)
    with pytest.warns(UserWarning, match="build"):
        ts.load_state_dict(dict(sd, build_id="f" * 64), verify=False)


def test_default_step_launches_what_the_parent_commit_launched(golden_dir, monkeypatch):
    """verify_every = 0 and no call of the new methods: the launch names of one update step (the recorder of
    test_deterministic_model_gpu.py::test_mode_off_launches_what_the_default_engine_launches) equal the list recorded from the commit
    before the checkpoint code existed (tests/golden/trainstep_launches_L37_d3.json), nothing was allocated for the canary, and the
    list is the same again behind a state_dict() / load_state_dict() pair and with verify_every set at world size 1."""
    _gpu()

    def names(ts, slide):
        monkeypatch.setattr(ops, "TIMER", {})
        monkeypatch.setattr(ops, "TIMELINE", [])
        ts.step(*slide)
        torch.cuda.synchronize()
        out = [rec[0] for rec in ops.TIMELINE]
        monkeypatch.setattr(ops, "TIMER", None)
        monkeypatch.setattr(ops, "TIMELINE", None)
        return out
    eng, ts, slide, _ = _fresh(monkeypatch, golden_dir, det=False)
    ts.step(*slide)          # (first step: allocations)
    torch.cuda.synchronize()
    first = names(ts, slide)
    parent = json.load(open(os.path.join(golden_dir, "trainstep_launches_L37_d3.json")))
    assert len(first) > 100 and first == parent["launches"]
    assert "checksum64" not in first and ts._cs_ws is None and ts.reducer.collectives == 0 and ts.verify_every == 0
    ts.load_state_dict(ts.state_dict())
    assert ts._cs_ws is not None
    assert names(ts, slide) == first
    eng2, ts2, _, _ = _fresh(monkeypatch, golden_dir, det=False, verify_every=1)
    ts2.step(*slide)
    torch.cuda.synchronize()
    assert names(ts2, slide) == first and ts2._cs_ws is None and ts2._boundaries == 2          # (world size 1: verify_replicas returns at once)


def test_param_checksum_is_the_reference_checksum_of_the_flat_buffer(golden_dir, monkeypatch):
    _gpu()
    from modaltune_amd.checkpoint import as_unsigned, checksum64_reference
    eng, ts, slide, _ = _fresh(monkeypatch, golden_dir)
    ts.step(*slide)
    cs = ts.param_checksum()
    assert cs.is_cuda and cs.dtype == torch.int64 and tuple(cs.shape) == (1,)
    assert as_unsigned(cs.item()) == checksum64_reference(eng.store.flat.cpu())
    assert as_unsigned(cs.item()) == ts.state_dict()["checksums"]["flat"]
    ts.verify_replicas()          # world size 1: returns at once


def test_titan_round_trip():
    """The TITAN TrainStep goes through the same code: save, load into a fresh engine on other weights, state equal, one step."""
    _gpu()
    import titan_standin
    from modaltune_amd.titan import NativeBackbone, TitanEngine, titan_model_config
    from modaltune_amd.trainer import TrainStep
    from test_titan_cpu import TITAN_JSON
    sizes = synth.toy_group_sizes()
    cfg = titan_model_config(dict(TITAN_JSON, drop_path_rate=0.0), 3, False, 6)

    def fused(seed):
        vit = titan_standin.VisionTransformer()
        titan_standin.init_standin(vit, 6)
        eng = TitanEngine(cfg, sizes, NativeBackbone(vit, "cuda"), "cuda")
        eng.load_state_dict(_other_trainables(cfg, sizes, 6, seed))
        ts = TrainStep(eng, lr=1e-5)
        ts.set_projector(synth.projector_state(6))
        return eng, ts
    L = 520
    inp = synth.synth_inputs_titan(L, sizes, 7, grid=40)
    slide = (torch.from_numpy(inp["x"]).cuda().reshape(L, -1), torch.from_numpy(inp["coords"]).cuda().reshape(L, 2),
             [torch.from_numpy(a).cuda() for a in inp["genes"]], torch.from_numpy(inp["text"]).cuda())
    eng, ts = fused(6)
    for _ in range(2):
        ts.step(*slide)
    sd = ts.state_dict()
    assert all(not k.startswith("backbone") for k in sd["model"]) and set(sd["model"]) == set(eng.store.slots)
    eng2, ts2 = fused(8)
    assert not torch.equal(eng2.store.flat, eng.store.flat)
    ts2.load_state_dict(sd)
    _assert_equal(_state(eng, ts), _state(eng2, ts2), "TITAN: state behind the load")
    ts2.step(*slide)
    assert int(ts2.step_dev) == 3 and bool(torch.isfinite(ts2.loss).all())
    eng2.check_inputs()
