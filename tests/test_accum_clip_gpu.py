"""GPU: gradient accumulation and global-norm clipping through TrainStep (accumulate, max_grad_norm) and the module path
(modaltune_amd.optim.clip_grad_norm_).

Model: the depth-3 synthetic one of test_ragged_lengths_through_one_trainstep; bags of 37, 129 and 300 patches; dropout off unless a
test says otherwise.  The EXPECTED gradient of a window is the float64 sum of its slides' own gradients, each from the existing
step(update=False) + unscaled_grads() on a twin engine with equal weights (the path the goldens pin).

Bars on the accumulated gradient (k = 3, lr = 0), per tensor: max |delta| <= bar * max |expected| of THAT tensor + FLOOR * the largest
entry of the whole expected gradient:
  deterministic engine  1e-5  a handful of fp32 `+=` per element against a float64 sum
  default engine        1e-3  25 x the run-to-run gradient noise DESIGN section 5 records (2.6e-7 on a largest entry of 7.0e-3), a tenth of
                              the goldens' 1 % bar; a dropped or doubled micro-step is off by >= 33 %
FLOOR = 1e-6, the absolute term the project's gradient comparisons carry (`+ 1e-6 * ref.max()` beside the 1 % bar of
test_train_step_matches_reference_golden): sixteen fp32 roundings of the largest entry.  It is there for tensors whose gradient is zero
up to rounding -- `gene_encoder.mlp_mixer.0.0.fn.3.bias`: ~1e-9 beside a largest entry ~1e-2, two evaluations of the REFERENCE differ
by more than its size -- where a bar relative to the tensor's own maximum measures nothing.  A micro-step dropped from or doubled in
any tensor whose own maximum is above ~3e-6 of the largest entry (1e-6 / 0.33) still fails.  Measured on an MI355X,
worst tensor: max |delta| against the tensor's own maximum, tensors above 1e-3 of the largest entry: 1.7e-6 (deterministic), 1.4e-6
(default; 4.4e-4 at L = 2048); max |delta| against the largest entry, all tensors: 7.5e-8, 1.1e-7 (6.2e-6 at L = 2048, on a tensor
whose own bar covers it).  Every case prints both figures.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from modaltune_amd import synth  # noqa: E402
from modaltune_amd.config import ModelConfig  # noqa: E402

SEED, NGRIDS = 41, 64
BAR = {True: 1e-5, False: 1e-3}          # deterministic engine / default engine
FLOOR = 1e-6                             # x the largest entry of the expected gradient (module docstring)
_cache = {}


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _cfg(dropout=False):
    kw = {} if dropout else dict(dropout=0.0, drop_path_rate=0.0)
    return ModelConfig(depth=3, interaction_indexes=((0, 0), (1, 1), (2, 2)), slide_ngrids=NGRIDS, **kw)


def _sizes():
    return synth.toy_group_sizes()


def _slide(L, variant=0, grid=NGRIDS):
    key = ("slide", L, variant)
    if key not in _cache:
        inp = synth.synth_inputs(L, _sizes(), SEED + L + 1000 * variant, grid=grid)
        _cache[key] = (torch.from_numpy(inp["x"]).cuda().half().reshape(L, -1), torch.from_numpy(inp["coords"]).cuda(),
                       [torch.from_numpy(a).cuda() for a in inp["genes"]], torch.from_numpy(inp["text"]).cuda())
    return _cache[key]


def _make(det=False, dropout=False, **ts_kw):
    from modaltune_amd.engine import Engine
    from modaltune_amd.trainer import TrainStep
    cfg = _cfg(dropout)
    if ("sd", dropout) not in _cache:
        _cache[("sd", dropout)] = synth.synth_state_dict(cfg, _sizes(), SEED)
    eng = Engine(cfg, _sizes(), "cuda", deterministic=det)
    eng.load_state_dict(_cache[("sd", dropout)])
    ts_kw.setdefault("lr", 0.0)
    ts_kw.setdefault("weight_decay", 0.0)
    ts = TrainStep(eng, **ts_kw)
    ts.set_projector(synth.projector_state(SEED))
    ts.auto_split = False
    ts.split_min_patches = 1 << 30
    return eng, ts


def _slide_grad(det, L, variant=0):
    """One slide's own gradient (float64, flat) on a twin engine: step(update=False) + unscaled_grads(); computed once per slide."""
    key = ("grad", det, L, variant)
    if key not in _cache:
        eng, ts = _make(det)
        ts.step(*_slide(L, variant), update=False)
        torch.cuda.synchronize()
        assert int(ts.found_inf) == 0
        _cache[key] = {k: v.double().clone() for k, v in ts.unscaled_grads().items()}
        del eng, ts
    return _cache[key]


def _expected(det, slides):
    parts = [_slide_grad(det, L, v) for L, v in slides]
    return {k: sum(p[k] for p in parts) for k in parts[0]}


def _check_grads(ts, want, bar, what, divide=1.0):
    torch.cuda.synchronize()
    got = ts.unscaled_grads()
    top = max(float(w.abs().max()) for w in want.values())
    worst, worst_own = (0.0, None), (0.0, None)
    for k, w in want.items():
        own = float(w.abs().max())
        d = float((got[k].double() / divide - w).abs().max())
        worst = max(worst, (d / top, k))
        if own > 1e-3 * top:
            worst_own = max(worst_own, (d / own, k))
    print(f"accum-clip {what}: worst max|delta| / largest entry = {worst[0]:.3e} ({worst[1]}); against the tensor's own maximum "
          f"(tensors above 1e-3 of the largest entry): {worst_own[0]:.3e} ({worst_own[1]}), bar {bar:g}")
    assert top > 0
    for k, w in want.items():
        d, own = float((got[k].double() / divide - w).abs().max()), float(w.abs().max())
        assert d <= bar * own + FLOOR * top, (what, k, d, own, top)


WINDOW_MIXED = [(37, 0), (129, 0), (300, 0)]
WINDOW_SAME = [(129, 0), (129, 1), (129, 2)]


@pytest.mark.parametrize("det", [True, False], ids=["deterministic", "default"])
@pytest.mark.parametrize("mode", ["eager", "eager_groups", "replay_same_geometry", "replay_three_lengths", "eager_and_replayed"])
def test_window_accumulates_the_sum_of_its_slides_gradients(monkeypatch, det, mode):
    """k = 3, lr = 0: after the boundary unscaled_grads() is the sum of the three slides' gradients (module docstring: reference and
    bars) -- eager batched; eager pass groups (MT_SPLIT_PASSES=force); step_graphed with the same geometry three times per window and
    with three different lengths per window, where every window position is a replay from the third window on; a window whose first
    micro-step is eager and whose others are replays.  The optimiser ran once per window, never inside one."""
    _gpu()
    slides = WINDOW_SAME if mode == "replay_same_geometry" else WINDOW_MIXED
    want = _expected(det, slides)
    if mode == "eager_groups":
        monkeypatch.setenv("MT_SPLIT_PASSES", "force")
    eng, ts = _make(det, accumulate=3, capture_after=2)
    if mode == "eager_groups":
        ts.split_min_patches = 0
        assert ts._split_now(37)
    windows = 1 if mode.startswith("eager_") or mode == "eager" else 4
    if mode == "eager_and_replayed":
        windows = 4
    for w in range(windows):
        for i, (L, v) in enumerate(slides):
            replays = ts.graph_replays
            graphed = mode.startswith("replay") or (mode == "eager_and_replayed" and i > 0)
            if graphed:
                ts.step_graphed(*_slide(L, v))
            else:
                ts.step(*_slide(L, v))
            if graphed and w >= 2:
                assert ts.graph_replays == replays + 1, (mode, w, i, "this window position was not a replay")
            assert ts.window_pos == (i + 1) % 3
            assert int(ts.step_dev) == w + (i == 2), (w, i, int(ts.step_dev))
        _check_grads(ts, want, BAR[det], f"{mode}/{'det' if det else 'default'}/window {w}")
    if mode == "eager_groups":
        assert ts._pass_streams is not None
    if mode == "replay_same_geometry":
        assert len(ts._gcache.entries) == 3          # one capture per role: first, middle, boundary
    eng.check_inputs()


def test_window_mechanics_norm_coefficient_and_clipped_update():
    """Deterministic engine, k = 3, lr = 1e-3.  step_dev, scale and tracker move only at the boundary.  max_grad_norm above the norm:
    grad_norm is the float64 norm of the expected MEAN gradient (1e-5 relative), clip_coef is 1 and the parameters and moments are
    torch.equal to a run without clipping.  max_grad_norm at half the norm: clip_coef is torch's min(1, max / (norm + 1e-6)) and p, m
    and v equal the float64 AdamW oracle fed the device's own pre-clip mean gradient times the float64 coefficient, rel < 1e-6."""
    _gpu()
    from oracle import modaltune_oracle as O
    want = _expected(True, WINDOW_MIXED)
    norm = float(np.sqrt(sum(float((w / 3.0).pow(2).sum()) for w in want.values())))
    runs = {}
    for name, mx in [("off", None), ("above", 10.0 * norm), ("below", 0.5 * norm)]:
        eng, ts = _make(True, accumulate=3, max_grad_norm=mx, lr=1e-3, weight_decay=0.01, growth_interval=1)
        p0 = eng.store.flat.double().clone()
        s0 = float(ts.scale)
        for i, (L, v) in enumerate(WINDOW_MIXED):
            assert (int(ts.step_dev), int(ts.tracker), float(ts.scale)) == (0, 0, s0), (name, i, "state moved inside the window")
            assert torch.equal(eng.store.flat.double(), p0)
            ts.step(*_slide(L, v))
        torch.cuda.synchronize()
        assert int(ts.step_dev) == 1 and float(ts.scale) == 2.0 * s0 and int(ts.found_inf) == 0      # (growth_interval 1: the scale grew ONCE)
        runs[name] = (eng, ts, p0)
    (e_off, t_off, _), (e_ab, t_ab, _), (e_be, t_be, p0) = runs["off"], runs["above"], runs["below"]
    for t in (t_ab, t_be):
        gn = float(t.grad_norm)
        print(f"accum-clip grad_norm {gn:.9g} against float64 {norm:.9g}: relative {abs(gn - norm) / norm:.3e}")
        assert abs(gn - norm) <= 1e-5 * norm
    assert float(t_ab.clip_coef) == 1.0
    assert torch.equal(e_ab.store.flat, e_off.store.flat) and torch.equal(t_ab.m, t_off.m) and torch.equal(t_ab.v, t_off.v)
    coef = min(1.0, 0.5 * norm / (float(t_be.grad_norm) + 1e-6))
    assert abs(float(t_be.clip_coef) - coef) <= 1e-6 * coef and coef < 0.51
    # the oracle: the device's own pre-clip mean gradient, the coefficient from float64
    g = e_be.store.flat_grad.double() / float(t_be.grad_scale) / 3.0
    c64 = min(1.0, 0.5 * norm / (float(g.norm()) + 1e-6))
    pr, mr, vr = O.adamw_update(p0, c64 * g, torch.zeros_like(g), torch.zeros_like(g), 1, float(t_be.lr_dev.cpu()))

    def rel(a, b):
        return float((a.double() - b).abs().max() / (b.abs().max() + 1e-300))
    print("accum-clip clipped update: rel p, m, v", rel(e_be.store.flat, pr), rel(t_be.m, mr), rel(t_be.v, vr))
    assert rel(e_be.store.flat, pr) < 1e-6 and rel(t_be.m, mr) < 1e-6 and rel(t_be.v, vr) < 1e-6
    assert not torch.equal(t_be.m, t_off.m)          # (the clip did act)


@pytest.mark.parametrize("max_grad_norm", [None, 1.0], ids=["noclip", "clip"])
def test_inf_in_a_micro_step_skips_the_whole_window(max_grad_norm):
    """test_overflow_gpu.py's injection (one inf patch feature) into the SECOND micro-step of a k = 3 window at lr = 1e-3: the
    parameters and moments stay bit-identical, the scale is halved once, the step count stays; the next window is clean and steps."""
    _gpu()
    eng, ts = _make(False, accumulate=3, max_grad_norm=max_grad_norm, lr=1e-3, weight_decay=0.01)
    before = (eng.store.flat.clone(), ts.m.clone(), ts.v.clone())
    s0 = float(ts.scale)
    for i, (L, v) in enumerate(WINDOW_MIXED):
        x, coords, genes, text = _slide(L, v)
        if i == 1:
            x = x.clone()
            x[L // 3, 5] = float("inf")
        ts.step(x, coords, genes, text)
    torch.cuda.synchronize()
    assert torch.equal(eng.store.flat, before[0]) and torch.equal(ts.m, before[1]) and torch.equal(ts.v, before[2])
    assert float(ts.scale) == 0.5 * s0 and int(ts.step_dev) == 0 and int(ts.found_inf) == 0 and int(ts.tracker) == 0
    if max_grad_norm is not None:
        assert float(ts.clip_coef) == 1.0 and not np.isfinite(float(ts.grad_norm))
    for L, v in WINDOW_MIXED:
        ts.step(*_slide(L, v))
    torch.cuda.synchronize()
    assert int(ts.step_dev) == 1 and float(ts.scale) == 0.5 * s0 and int(ts.found_inf) == 0
    assert bool(torch.isfinite(eng.store.flat).all()) and not torch.equal(eng.store.flat, before[0])
    eng.check_inputs()


def test_finish_window_applies_a_partial_window_and_update_false_raises():
    """Deterministic engines: two micro-steps of a k = 3 window + finish_window() equal a complete accumulate = 2 window bit for bit
    (the mean is over the micro-steps seen); a second finish_window() is a no-op; step(update=False) raises at k > 1."""
    _gpu()
    ea, ta = _make(True, accumulate=3, max_grad_norm=0.01, lr=1e-3, weight_decay=0.01)
    eb, tb = _make(True, accumulate=2, max_grad_norm=0.01, lr=1e-3, weight_decay=0.01)
    ta.finish_window()                             # an empty window: nothing happens
    assert int(ta.step_dev) == 0 and ta.window_pos == 0
    for L, v in WINDOW_MIXED[:2]:
        ta.step(*_slide(L, v))
        tb.step(*_slide(L, v))
    assert ta.window_pos == 2 and tb.window_pos == 0 and int(ta.step_dev) == 0
    ta.finish_window()
    torch.cuda.synchronize()
    assert ta.window_pos == 0 and int(ta.step_dev) == int(tb.step_dev) == 1
    assert torch.equal(ea.store.flat, eb.store.flat) and torch.equal(ta.m, tb.m) and torch.equal(ta.v, tb.v)
    assert torch.equal(ta.grad_norm, tb.grad_norm) and float(ta.clip_coef) < 1.0
    snap = ea.store.flat.clone()
    ta.finish_window()
    torch.cuda.synchronize()
    assert torch.equal(ea.store.flat, snap) and int(ta.step_dev) == 1
    with pytest.raises(ValueError):
        ta.step(*_slide(37), update=False)
    assert ta.window_pos == 0


def test_deterministic_dropout_windows_repeat_bit_for_bit_eager_and_replayed():
    """Deterministic engine, Dropout / DropPath on (same seed), k = 3 with clipping, three windows at lr = 1e-3: two fresh eager runs
    give torch.equal parameters, moments and losses, and so does a run through step_graphed (eager visit, capture, replay of every
    window position)."""
    _gpu()
    out = []
    for graphed in (False, False, True):
        eng, ts = _make(True, dropout=True, accumulate=3, max_grad_norm=1e-3, lr=1e-3, weight_decay=0.01, capture_after=1)
        eng.set_stochastic(True, seed=1234)
        losses = []
        for w in range(3):
            for L, v in WINDOW_SAME:
                (ts.step_graphed if graphed else ts.step)(*_slide(L, v))
                losses.append(ts.loss.clone())
        torch.cuda.synchronize()
        assert int(ts.step_dev) == 3 and (ts.graph_replays == 6) == graphed
        out.append(dict(flat=eng.store.flat.clone(), m=ts.m.clone(), v=ts.v.clone(), losses=torch.cat(losses), norm=ts.grad_norm.clone(),
                        coef=ts.clip_coef.clone()))
        del eng, ts
    print("accum-clip dropout windows: grad_norm", float(out[0]["norm"]), "clip_coef", float(out[0]["coef"]))
    assert float(out[0]["coef"]) < 1.0 and len(set(out[0]["losses"].tolist())) == 9
    for k in out[0]:
        assert torch.equal(out[0][k], out[1][k]), ("two eager runs", k)
        assert torch.equal(out[0][k], out[2][k]), ("eager against replayed", k)


def test_schedule_trial_inside_an_accumulating_run_leaves_the_window_alone():
    """L = 2048, three passes, k = 2, capture_after = 1: the schedule trial of the geometry falls due at the first position of the
    second window, replays real steps and restores what they touched; the window position is what it was, the optimiser ran once per
    window and the second window's gradient still is the sum of its two slides' (default-engine bar)."""
    _gpu()
    L = 2048
    want = _expected(False, [(L, 0), (L, 1)])
    eng, ts = _make(False, accumulate=2, capture_after=1, max_grad_norm=1e9)
    ts.auto_split, ts.split_min_patches = True, 7500
    for w in range(3):
        for i in range(2):
            ts.step_graphed(*_slide(L, i))
            assert ts.window_pos == (i + 1) % 2
            assert (L in ts.split_trials) == (w >= 1), (w, i)
        torch.cuda.synchronize()
        assert int(ts.step_dev) == w + 1
        _check_grads(ts, want, BAR[False], f"trial/window {w}")
    assert ts.graph_replays == 4 and np.isfinite(float(ts.grad_norm))
    eng.check_inputs()


def test_titan_engine_accumulates_a_window():
    """The TITAN configuration steps with both options wherever it steps today: accumulate = 2 with clipping, eager, on its smallest
    stand-in fixture -- the window's gradient is the sum of the slides' own (default-engine bar), the optimiser runs at the boundary."""
    _gpu()
    import titan_standin
    from test_titan_cpu import TITAN_JSON
    from modaltune_amd.titan import NativeBackbone, TitanEngine, titan_model_config
    from modaltune_amd.trainer import TrainStep
    seed, sizes, L = 6, synth.toy_group_sizes(), 170

    def make(**kw):
        vit = titan_standin.VisionTransformer()
        titan_standin.init_standin(vit, seed)
        cfg = titan_model_config(dict(TITAN_JSON, drop_path_rate=0.0), 3, False, 6)
        eng = TitanEngine(cfg, sizes, NativeBackbone(vit, "cuda"), "cuda")
        eng.load_state_dict(synth.synth_state_dict(cfg, sizes, seed))
        ts = TrainStep(eng, lr=0.0, weight_decay=0.0, **kw)
        ts.set_projector(synth.projector_state(seed))
        return eng, ts
    slides = []
    for s in (seed, seed + 1):
        inp = synth.synth_inputs_titan(L, sizes, s, grid=40)
        slides.append((torch.from_numpy(inp["x"]).cuda().reshape(L, -1).contiguous(), torch.from_numpy(inp["coords"]).cuda().reshape(L, 2),
                       [torch.from_numpy(a).cuda() for a in inp["genes"]], torch.from_numpy(inp["text"]).cuda()))
    e1, t1 = make()
    parts = []
    for s in slides:
        t1.step(*s, update=False)
        torch.cuda.synchronize()
        parts.append({k: v.double().clone() for k, v in t1.unscaled_grads().items()})
    want = {k: parts[0][k] + parts[1][k] for k in parts[0]}
    e2, t2 = make(accumulate=2, max_grad_norm=1e9)
    t2.step(*slides[0])
    assert int(t2.step_dev) == 0 and t2.window_pos == 1
    t2.step(*slides[1])
    _check_grads(t2, want, BAR[False], "titan")
    assert int(t2.step_dev) == 1 and t2.window_pos == 0 and float(t2.clip_coef) == 1.0 and float(t2.grad_norm) > 0


def test_module_path_clip_grad_norm_matches_torch(monkeypatch):
    """The reference-style loop on the drop-in module at L = 37: scaler.scale(loss).backward(); scaler.unscale_(opt);
    optim.clip_grad_norm_; scaler.step(opt).  Against torch.nn.utils.clip_grad_norm_ on cloned gradients: returned norm relative <=
    1e-5 (torch's is an fp32 norm of norms), clipped gradients rtol 1e-5; the fast path ran (torch's function is not called, the norm
    is a 0-d device tensor) and the AdamW.step behind it is the fused one."""
    _gpu()
    from modaltune_amd import optim
    from modaltune_amd.aggregators import Aggregator
    from modaltune_amd.config import GIGAPATH_JSON
    sizes = _sizes()
    groups = {i: ["g"] * n for i, n in enumerate(sizes)}
    model = Aggregator.create("longnetvit_gene_adapter", gene_group_defination=groups, multi_task=3,
                              **dict(GIGAPATH_JSON, depth=3, slide_ngrids=NGRIDS, interaction_indexes=[[0, 0], [1, 1], [2, 2]], dropout=0.0,
                                     drop_path_rate=0.0))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(model.cfg, sizes, 53).items()}, strict=True)
    model.train()
    train = [p for p in model.parameters() if p.requires_grad]
    opt = optim.AdamW(train, lr=1e-3, weight_decay=0.01)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 15)
    inp = synth.synth_inputs(37, sizes, 53, grid=NGRIDS)
    x, c = torch.from_numpy(inp["x"]).cuda(), torch.from_numpy(inp["coords"]).cuda()
    x = x.reshape(-1, x.shape[-1]).contiguous()
    genes = {i: torch.from_numpy(a).cuda() for i, a in enumerate(inp["genes"])}
    eye = torch.eye(3, device="cuda")
    w = torch.randn(3, 256, generator=torch.Generator().manual_seed(1)).cuda()
    torch_clip = torch.nn.utils.clip_grad_norm_

    def refuse(*a, **k):
        raise AssertionError("the fast path fell back to torch.nn.utils.clip_grad_norm_")
    for rnd, factor in enumerate((0.5, 3.0)):          # max_norm below the norm (clips) and above it (coefficient 1)
        xs = x.clone()                                 # (one slide: the three task calls are chained on the tensor they share)
        ys = [model(x=xs, coords=c, genes=genes, task_token=eye[t].clone()) for t in range(3)]
        scaler.scale(sum((y * w[t]).sum() for t, y in enumerate(ys))).backward()
        scaler.unscale_(opt)
        clones = [p.detach().clone().requires_grad_(True) for p in train]
        for q, p in zip(clones, train):
            q.grad = p.grad.detach().clone()
        total = float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(q.grad.double()) for q in clones])))
        want = torch_clip(clones, factor * total)
        monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", refuse)
        got = optim.clip_grad_norm_(train, factor * total)
        monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", torch_clip)
        assert got.is_cuda and got.dim() == 0
        print(f"accum-clip module path round {rnd}: norm {float(got):.9g} torch {float(want):.9g} float64 {total:.9g}")
        assert abs(float(got) - float(want)) <= 1e-5 * float(want)
        for q, p in zip(clones, train):
            assert torch.allclose(p.grad, q.grad, rtol=1e-5, atol=0.0), float((p.grad - q.grad).abs().max())
        if factor < 1.0:
            assert abs(float(torch.linalg.vector_norm(torch.stack([p.grad.double().norm() for p in train]))) / (factor * total) - 1.0) < 1e-4
        scaler.step(opt)
        scaler.update()
        assert opt.last_step_fused is True
        opt.zero_grad()
