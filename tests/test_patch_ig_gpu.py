"""GPU: Integrated Gradients over the patch embeddings (modaltune_amd.attribution with inputs = "patches" / "both", engine.PatchPoints,
csrc/gene.hip: mt_patch_points_fwd, mt_patch_ig_accumulate).

Kernel units against numpy in float64 (the arithmetic is fp32 throughout: 1e-6 of the tensor's largest value for the interpolation --
one subtraction and one fma per element -- and 1e-5 for the 768-term row dots, the project's token-side bar); the model level against the
float64 oracle under the SAME quadrature (tests/test_patch_ig_cpu.py: `_oracle_patch_ig`, `_oracle_joint_ig`) at the project's bar for
full gradient tensors, relative L2 <= 1e-2 (tests/test_ig_gpu.py); completeness; the exact properties on a deterministic engine; and
that a call leaves parameters, gradients, optimiser state, generation and captured graphs as they were."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from modaltune_amd import ops, synth  # noqa: E402
from test_ig_cpu import TARGET, _case  # noqa: E402
from test_patch_ig_cpu import _f_and_grads, _oracle_joint_ig, _oracle_patch_ig  # noqa: E402

D = 768
ALPHAS = {1: [0.37], 3: [0.0, 0.37, 1.0], 4: [1.0, 0.25, 0.0, 0.9]}
WEIGHTS = {1: [0.5], 3: [0.25, 0.0, 0.5], 4: [0.0, 0.3, 0.0, 0.2]}
TGT = torch.from_numpy(TARGET.astype(np.float32))


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _relmax(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / np.abs(ref).max())


def _l2(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(a - ref) / np.linalg.norm(ref))


# ---------------------------------------------------------------- kernel units
@pytest.mark.parametrize("B", [1, 3, 4])
@pytest.mark.parametrize("L", [1, 37, 300])
def test_patch_points_fwd_matches_float64_and_selects_the_endpoints(L, B):
    _gpu()
    dev = "cuda"
    rng = np.random.default_rng(10 * L + B)
    ex, eb = rng.standard_normal((L, D)).astype(np.float32), rng.standard_normal((L, D)).astype(np.float32)
    al = np.asarray(ALPHAS[B], np.float32)
    tex, teb = torch.from_numpy(ex).to(dev), torch.from_numpy(eb).to(dev)
    out = torch.full((B + 1, L, D), float("nan"), device=dev)          # (one spare pass behind the output: stays untouched)
    ops.patch_points_fwd(tex, teb, torch.from_numpy(al).to(dev), B, L, D, out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[B]).all())
    for b in range(B):
        if al[b] == 0.0:
            assert torch.equal(out[b], teb)
        elif al[b] == 1.0:
            assert torch.equal(out[b], tex)
        else:
            ref = eb.astype(np.float64) + float(al[b]) * (ex.astype(np.float64) - eb.astype(np.float64))
            assert _relmax(out[b].cpu().numpy(), ref) <= 1e-6
    assert torch.equal(tex, torch.from_numpy(ex).to(dev)) and torch.equal(teb, torch.from_numpy(eb).to(dev))


@pytest.mark.parametrize("B", [1, 3, 4])
@pytest.mark.parametrize("L", [1, 37, 300])
def test_patch_ig_accumulate_matches_float64_skips_dead_passes_and_repeats(L, B):
    _gpu()
    dev, N = "cuda", L + 1
    rng = np.random.default_rng(1000 + 10 * L + B)
    ex, eb = rng.standard_normal((L, D)).astype(np.float32), rng.standard_normal((L, D)).astype(np.float32)
    dh = rng.standard_normal((B, N, D)).astype(np.float32)
    w = np.asarray(WEIGHTS[B], np.float32)
    dh[:, 0] = np.nan                       # the cls row of every pass is never read
    dh[w == 0] = np.nan                     # ... nor any row of a weight-0 pass
    live = [b for b in range(B) if w[b] != 0]
    ref = sum(float(w[b]) * (dh[b, 1:].astype(np.float64) * (ex.astype(np.float64) - eb.astype(np.float64))).sum(1) for b in live)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tdh, tex, teb, tw = t(dh), t(ex), t(eb), t(w)
    one, again, twice, scaled = (torch.zeros(L + 1, device=dev) for _ in range(4))      # (one spare element: stays zero)
    ops.patch_ig_accumulate(tdh, N, tex, teb, tw, B, L, D, one)
    ops.patch_ig_accumulate(tdh, N, tex, teb, tw, B, L, D, again)
    for _ in range(2):
        ops.patch_ig_accumulate(tdh, N, tex, teb, tw, B, L, D, twice)
    ops.patch_ig_accumulate(tdh, N, tex, teb, tw, B, L, D, scaled, unscale_dev=torch.tensor([0.125], device=dev))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(one).all())
    err = _relmax(one[:L].cpu().numpy(), ref)
    print(L, B, f"relative error {err:.1e}")
    assert err <= 1e-5, err
    assert torch.equal(one, again)                          # the same bits on every launch
    assert torch.equal(twice, one + one)                    # a second accumulate adds
    assert torch.equal(scaled, one * 0.125)                 # unscale honoured (a power of two: exact)
    assert float(one[L]) == 0.0


# ---------------------------------------------------------------- model level
def _engine(name="L37_d3", deterministic=False):
    from modaltune_amd.engine import Engine
    cfg, sizes, _, _, _, _, _, inp = _case(name)
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"model_{name}.npz"))
    eng = Engine(cfg, sizes, "cuda", deterministic=deterministic)
    eng.load_state_dict(synth.synth_state_dict(cfg, sizes, int(g["seed"])))
    x, coords = torch.from_numpy(inp["x"]).cuda(), torch.from_numpy(inp["coords"]).cuda()
    genes = [torch.from_numpy(a).cuda() for a in inp["genes"]]
    clin = torch.from_numpy(inp["clinical"]).cuda() if cfg.clinical else None
    return cfg, eng, sizes, (x, coords, genes, clin), inp


def _relu_sides_of(eng, cfg, run):
    """{oracle prefix: bool [T, E]} -- which units of each Extractor FFN are ON in the engine's forward `run()`: the sign of the
    pre-activation that the fused linear1 + ReLU launch keeps for its backward (ops.sgemm_problem(act=ACT_RELU, pre_out=...)), in
    forward order."""
    pres, keep = [], ops.sgemm_problem

    def spy(*a, **k):
        if k.get("act") == ops.ACT_RELU and k.get("pre_out") is not None:
            pres.append(k["pre_out"])
        return keep(*a, **k)
    ops.sgemm_problem = spy
    try:
        run()
    finally:
        ops.sgemm_problem = keep
    n = len(cfg.interaction_indexes)
    prefixes = [f"interactions.{i}.extractor" for i in range(n)]
    if cfg.use_extra_extractor:
        prefixes += [f"interactions.{n - 1}.extra_extractors.{j}" for j in range(2)]
    assert len(pres) == len(prefixes), (len(pres), prefixes)
    torch.cuda.synchronize()
    return {p: (t[0] > 0).cpu().numpy() for p, t in zip(prefixes, pres)}


def test_one_patch_gradient_matches_oracle_autograd():
    """The engine-level call, one point at alpha = 1 from a zero bag: <e_x - e_base, dF_t/dx0> per patch against the oracle's
    sum_c (x - base)_c dF_t/dx_c (torch.autograd over the 1536 input channels) at the slide's own features.

    F is only piecewise smooth -- the Extractors' FFN has a ReLU -- and this point sits ON a kink for task 0: unit 40 of the first
    Extractor's FFN has a pre-activation of -1.3e-6 in the task-token row in float64 (tests/test_patch_ig_cpu.py pins it), which no fp32
    forward fed by fp16 operands can tell from zero, and the two one-sided derivatives differ by 2.66e-2 per patch.  The engine's
    forward lands on the other side: against the oracle's own side it measures 2.65e-2 / 1.55e-3 / 1.09e-3 for tasks 0 / 1 / 2 on an
    MI355X, with every other launch of the backward within 1e-3 of a float64 recomputation.  So the reference is
    the oracle's derivative on the side of each such kink where the engine's forward sits: for the units whose float64
    pre-activation is within KINK_TAU = 2^-11 (fp16's rounding) of zero relative to their row -- 16 of 62 400 here -- and for those
    only, the ReLU's side is read from the engine's forward; everywhere else the oracle keeps its own sign, and the bar stays 1e-2."""
    _gpu()
    from modaltune_amd.engine import PatchPoints
    cfg, eng, sizes, (x, coords, genes, clin), _ = _engine()
    dev = "cuda"
    L = x.reshape(-1, x.shape[-1]).shape[0]
    tgt = TGT.to(dev)
    scale = torch.empty(2, device=dev)
    ops.absmax_scale(tgt, scale, 1024.0)
    seed = (tgt * scale[0]).view(1, -1)
    base: dict = {}
    eng.prepare_shared(torch.zeros_like(x), coords, base)
    _, _, _, x64, _, genes64, _, _ = _case("L37_d3")
    report, plain = {}, {}
    for t in range(3):
        dp = torch.zeros(L, device=dev)
        pts = PatchPoints(base["x0"], torch.ones(1, device=dev), torch.ones(1, device=dev), dp, unscale=scale[1:2])
        sides = _relu_sides_of(eng, cfg, lambda: eng.forward(x, coords, genes, torch.eye(3, device=dev)[t:t + 1], need_grad=True, fresh=True,
                                                             patch_points=pts, stochastic=False))
        eng.backward(seed.clone(), call=eng.last_call)
        torch.cuda.synchronize()
        found = []
        _, dx, _ = _f_and_grads("L37_d3", t, TARGET, x64, genes64, relu_sides=sides, found=found)
        _, dx_own, _ = _f_and_grads("L37_d3", t, TARGET, x64, genes64)
        per_patch = lambda d: (x64.reshape(d.shape).numpy() * d).sum(1)
        report[t], plain[t] = _l2(dp.cpu().numpy(), per_patch(dx)), _l2(dp.cpu().numpy(), per_patch(dx_own))
        moved = [f for f in found if f[4] != (f[3] > 0)]
        print(f"task {t}: {len(found)} units within KINK_TAU of zero, the engine on the other side of {[(f[0], f[1], f[2], f'{f[3]:.1e}') for f in moved]}")
        assert len(found) <= 64          # (a handful of 62 400: the reference stays the oracle's)
    print("<e_x - e_base, dF/dx0> per patch, relative L2 against the oracle:", {k: f"{v:.2e}" for k, v in report.items()},
          "; against the oracle's own side of every kink:", {k: f"{v:.2e}" for k, v in plain.items()})
    assert max(report.values()) <= 1e-2, report


@pytest.mark.parametrize("name,tasks,m", [("L37_d3", (0, 1, 2), 16), ("L37_d3", (0,), 7), ("L37_d3_clin", (1,), 16)])
def test_patch_ig_matches_oracle_under_the_same_quadrature(name, tasks, m):
    """m = 16: sixteen points and the two endpoints are six passes of three exactly; m = 7: the last pass is mostly padding; the
    clinical geometry has one more token in front of the task token."""
    _gpu()
    from modaltune_amd.attribution import IntegratedGradients
    cfg, eng, sizes, (x, coords, genes, clin), _ = _engine(name)
    L = x.reshape(-1, x.shape[-1]).shape[0]
    res = IntegratedGradients(eng, tasks, steps=m, inputs="patches")(x, coords, genes, TGT, clinical=clin)
    torch.cuda.synchronize()
    assert res["patches"].shape == (len(tasks), L) and res["patches_total"].shape == (len(tasks),)
    assert res["patches"].dtype == torch.float32 and res["patches"].is_cuda and res["patches_total"].is_cuda and res["steps"] == m
    assert "attributions" not in res and "pathway" not in res
    report = {}
    for i, t in enumerate(tasks):
        ref = _oracle_patch_ig(name, t, TARGET, m)
        report[t] = (_l2(res["patches"][i].cpu().numpy(), ref["patches"]),
                     abs(float(res["patches_total"][i]) - ref["patches_total"]) / abs(ref["delta"]))
    print(name, m, "relative L2 of the patch attributions, |total - oracle| / |dF|:", {k: (f"{a:.2e}", f"{b:.2e}") for k, (a, b) in report.items()})
    assert max(a for a, _ in report.values()) <= 1e-2, report
    assert max(b for _, b in report.values()) <= 1e-2, report


@pytest.mark.parametrize("inputs", ["patches", "both"])
def test_completeness_on_the_gpu(inputs):
    """m = 32, task 0: |convergence_delta| / |delta| <= the oracle's own gap at m = 32 on the same path + 2e-2 (1e-2: the attribution
    bar, on their sum; 1e-2: delta, a difference of two logit rows that each carry the project's 1e-3 logits bar -- the bar of
    tests/test_ig_gpu.py::test_completeness_on_the_gpu).  f_input / f_baseline come out of the IG passes: against two plain
    forward-only passes of the engine."""
    _gpu()
    from modaltune_amd.attribution import IntegratedGradients
    cfg, eng, sizes, (x, coords, genes, clin), _ = _engine()
    res = IntegratedGradients(eng, (0,), steps=32, inputs=inputs)(x, coords, genes, TGT)
    oh = torch.eye(3, device="cuda")[0:1]
    gb = genes if inputs == "patches" else [torch.zeros_like(g) for g in genes]
    f_in = float((eng.forward(x, coords, genes, oh, need_grad=False).double().cpu().reshape(-1) * torch.from_numpy(TARGET)).sum())
    f_b = float((eng.forward(torch.zeros_like(x), coords, gb, oh, need_grad=False).double().cpu().reshape(-1) * torch.from_numpy(TARGET)).sum())
    torch.cuda.synchronize()
    gap = float(res["convergence_delta"].abs() / res["delta"].abs())
    ref = (_oracle_patch_ig if inputs == "patches" else _oracle_joint_ig)("L37_d3", 0, TARGET, 32)
    print(f"{inputs}: completeness gap on the GPU at m = 32: {gap:.2e} (oracle {ref['gap']:.2e}); f_input {float(res['f_input']):.6e} / plain "
          f"{f_in:.6e}; f_baseline {float(res['f_baseline']):.6e} / plain {f_b:.6e}")
    assert gap <= ref["gap"] + 2e-2, (gap, ref["gap"])
    assert abs(float(res["f_input"]) - f_in) <= 1e-6 * abs(f_in), (float(res["f_input"]), f_in)
    assert abs(float(res["f_baseline"]) - f_b) <= 1e-6 * abs(f_b), (float(res["f_baseline"]), f_b)
    assert torch.equal(res["delta"], res["f_input"] - res["f_baseline"])
    total = res["patches_total"] if inputs == "patches" else res["pathway"].sum(1) + res["patches_total"]
    assert torch.equal(res["patches_total"], res["patches"].sum(1))
    assert torch.equal(res["convergence_delta"], total - res["delta"])
    if inputs == "both":          # the split between the modalities, against the joint oracle path
        assert _l2(res["patches"][0].cpu().numpy(), ref["patches"]) <= 1e-2
        assert _l2(res["attributions"][0].cpu().numpy(), ref["attributions"]) <= 1e-2


PATCH_TENSORS = ("patches", "patches_total", "f_input", "f_baseline", "delta", "convergence_delta")
GENE_TENSORS = ("attributions", "pathway")


def test_exact_properties():
    _gpu()
    from test_ig_gpu import _module
    model, x, coords, genes = _module(deterministic=True)
    model.eval()
    kw = dict(task_ids=(0, 2), steps=4)
    a = model.integrated_gradients(x, coords, genes, TGT, inputs="patches", **kw)
    assert float(a["patches"].abs().min()) > 0
    # patch_baseline == x: nothing to attribute, exactly
    z = model.integrated_gradients(x, coords, genes, TGT, inputs="patches", patch_baseline=x.clone(), **kw)
    assert int(torch.count_nonzero(z["patches"])) == 0 and int(torch.count_nonzero(z["patches_total"])) == 0
    assert int(torch.count_nonzero(z["delta"])) == 0 and torch.equal(z["f_input"], z["f_baseline"])
    # target -> 2 target: the scaled seed and with it the whole gradient stream keep their bits and the reciprocal of the scale doubles
    # exactly (tests/test_ig_gpu.py::test_exact_properties): every output doubles bit for bit
    b = model.integrated_gradients(x, coords, genes, 2 * TGT, inputs="patches", **kw)
    for k in PATCH_TENSORS:
        assert torch.equal(b[k], 2 * a[k]), k
    # a repeated call: the same bits
    c = model.integrated_gradients(x, coords, genes, TGT, inputs="patches", **kw)
    for k in PATCH_TENSORS:
        assert torch.equal(c[k], a[k]), k
    # both modalities on the path, the patches standing still: the gene attributions of inputs="genes", bit for bit
    g = model.integrated_gradients(x, coords, genes, TGT, **kw)
    assert "patches" not in g
    bg = model.integrated_gradients(x, coords, genes, TGT, inputs="both", patch_baseline=x.clone(), **kw)
    for k in GENE_TENSORS:
        assert torch.equal(bg[k], g[k]), k
    assert int(torch.count_nonzero(bg["patches"])) == 0
    # ... and the genes standing still: the patch attributions of inputs="patches" (the pathway networks' first layer takes
    # alpha of one sum and 1 - alpha of an equal one there: a rounding apart)
    bp = model.integrated_gradients(x, coords, genes, TGT, inputs="both", baseline=[t.clone() for t in genes], **kw)
    assert float((bp["patches"] - a["patches"]).abs().max()) <= 1e-6 * float(a["patches"].abs().max())
    assert int(torch.count_nonzero(bp["attributions"])) == 0
    # the heatmap: evaluate.attention_to_grid takes a row as it is
    from modaltune_amd.evaluate import attention_to_grid
    grid = attention_to_grid(a["patches"][0], coords)
    assert np.isfinite(grid[~np.isnan(grid)]).all() and (~np.isnan(grid)).sum() >= 1


def test_patch_ig_leaves_training_state_and_captured_graphs_alone():
    _gpu()
    from modaltune_amd.attribution import IntegratedGradients
    from modaltune_amd.evaluate import EmbeddingExtractor
    from modaltune_amd.trainer import TrainStep
    cfg, eng, sizes, (x, coords, genes, clin), inp = _engine(deterministic=True)
    seed = int(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_L37_d3.npz"))["seed"])
    ts = TrainStep(eng, lr=0.0)
    ts.set_projector(synth.projector_state(seed))
    text = torch.from_numpy(inp["text"])
    losses = []
    for _ in range(6):
        ts.step_graphed(x, coords, genes, text)
        losses.append(ts.loss.clone())
        if ts.graph_replays >= 2:
            break
    assert ts.graph_replays >= 2
    ex = EmbeddingExtractor(eng, (0, 1, 2), capture_after=1)
    emb = [ex(x, coords, genes).clone() for _ in range(3)]
    assert ex.graph_replays >= 1
    torch.cuda.synchronize()
    st = eng.store
    snap = {"flat": st.flat.clone(), "flat_grad": st.flat_grad.clone(), "m": ts.m.clone(), "v": ts.v.clone(), "rng": eng.rng.clone(),
            "step": ts.step_dev.clone()}
    ptr, gen, replays, ex_replays, fresh_calls = st.flat_grad.data_ptr(), eng.generation, ts.graph_replays, ex.graph_replays, eng._fresh_calls
    for inputs in ("patches", "both"):
        IntegratedGradients(eng, (0, 1), steps=4, inputs=inputs)(x, coords, genes, TGT)
    torch.cuda.synchronize()
    assert eng.generation == gen and st.flat_grad.data_ptr() == ptr and eng._fresh_calls == fresh_calls
    now = {"flat": st.flat, "flat_grad": st.flat_grad, "m": ts.m, "v": ts.v, "rng": eng.rng, "step": ts.step_dev}
    for k in snap:
        assert torch.equal(snap[k], now[k]), k
    ts.step_graphed(x, coords, genes, text)
    torch.cuda.synchronize()
    assert ts.graph_replays == replays + 1 and torch.equal(ts.loss, losses[-1])
    again = ex(x, coords, genes)
    assert ex.graph_replays == ex_replays + 1 and torch.equal(again, emb[-1])


def test_requests_that_cannot_be_served_raise():
    _gpu()
    from modaltune_amd.aggregators import Aggregator
    from modaltune_amd.attribution import IntegratedGradients
    from modaltune_amd.engine import PatchPoints
    import modaltune_amd.titan  # noqa: F401
    from test_titan_cpu import TITAN_JSON
    cfg, eng, sizes, (x, coords, genes, clin), _ = _engine()
    dev = "cuda"
    L = x.reshape(-1, x.shape[-1]).shape[0]
    with pytest.raises(ValueError, match="inputs"):
        IntegratedGradients(eng, (0,), steps=4, inputs="pixels")
    ig = IntegratedGradients(eng, (0,), steps=4, inputs="patches")
    with pytest.raises(ValueError, match="patch_baseline"):
        ig(x, coords, genes, TGT, patch_baseline=torch.zeros(L - 1, x.shape[-1], device=dev))
    with pytest.raises(ValueError, match="patch_baseline"):
        ig(x, coords, genes, TGT, patch_baseline=torch.zeros(L, x.shape[-1] - 1, device=dev))
    with pytest.raises(ValueError, match="baseline"):
        ig(x, coords, genes, TGT, baseline=[torch.zeros_like(g) for g in genes])
    with pytest.raises(ValueError, match="patch_baseline"):
        IntegratedGradients(eng, (0,), steps=4)(x, coords, genes, TGT, patch_baseline=torch.zeros_like(x))
    oh = torch.eye(3, device=dev)[0:1]
    ok = lambda Lp=L: PatchPoints(torch.zeros(Lp, D, device=dev), torch.ones(1, device=dev), torch.ones(1, device=dev),
                                 torch.zeros(Lp, device=dev))
    with pytest.raises(ValueError, match="need_grad"):
        eng.forward(x, coords, genes, oh, need_grad=False, fresh=True, patch_points=ok(), stochastic=False)
    with pytest.raises(ValueError, match="patch_points.x0_base"):
        eng.forward(x, coords, genes, oh, need_grad=True, fresh=True, patch_points=ok(L + 1), stochastic=False)
    cpu = ok()
    cpu.alphas = torch.ones(1)
    with pytest.raises(ValueError, match="patch_points.alphas"):
        eng.forward(x, coords, genes, oh, need_grad=True, fresh=True, patch_points=cpu, stochastic=False)
    # the layers in front of a late first interaction run forward-only
    pcfg, peng, _, (px, pcoords, pgenes, _), _ = _engine("L37_d6_pre_gp")
    assert pcfg.first_interaction_layer > 0
    with pytest.raises(NotImplementedError, match="first_interaction_layer"):
        IntegratedGradients(peng, (0,), steps=4, inputs="both")
    with pytest.raises(NotImplementedError, match="first_interaction_layer"):
        peng.forward(px, pcoords, pgenes, oh, need_grad=True, fresh=True, patch_points=ok(), stochastic=False)
    tsizes = synth.toy_group_sizes()
    tm = Aggregator.create("titan_gene_adapter", gene_group_defination={i: ["g"] * n for i, n in enumerate(tsizes)}, **TITAN_JSON,
                           multi_task=3)
    with pytest.raises(NotImplementedError, match="TITAN"):
        IntegratedGradients(tm.engine, inputs="patches")
    with pytest.raises(NotImplementedError, match="TITAN"):
        tm.integrated_gradients(None, None, None, None, inputs="patches")
