"""GPU: Integrated Gradients over the gene inputs (modaltune_amd.attribution, csrc/gene.hip: mt_gene_snn_fwd_points,
mt_gene_snn_bwd_input, mt_ig_finalize).

Kernel units against torch on the CPU in float64 (1e-5 of the tensor's largest value: the arithmetic is fp32 throughout, the project's
token-side bar); the model level against the float64 oracle under the SAME quadrature (tests/test_ig_cpu.py: `_oracle_ig`) at the
project's bar for full gradient tensors, relative L2 <= 1e-2 (tests/test_model_gpu.py) -- the float64 oracle with only the patch-row
operands rounded to fp16 (oracle F16_PATCH_OPERANDS, no HIP kernel) deviates by 1.6e-3 on the m = 16 case; completeness; the exact
properties; and that a call leaves parameters, gradients, optimiser state, generation and captured graphs as they were."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from modaltune_amd import ops, synth  # noqa: E402
from modaltune_amd.config import GIGAPATH_JSON  # noqa: E402
from test_ig_cpu import TARGET, _case, _oracle_f_and_grad, _oracle_ig  # noqa: E402

F64 = torch.float64
GL = 256
SIZES = [1, 2, 31, 32, 33, 199, 300]      # one gene, below / at / above the 32-column chunk, and more than one 256-piece of the input


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ---------------------------------------------------------------- kernel units
def _unit_params(seed):
    """Random pathway networks of SIZES in one flat buffer, laid out as the engine's store does (16-byte aligned slots)."""
    rng = np.random.default_rng(seed)
    offs, chunks, off = [], [], 0
    for n in SIZES:
        row = []
        for shape, scale in (((GL, n), 1.0 / np.sqrt(n)), ((GL,), 0.5), ((GL, GL), 1.0 / 16), ((GL,), 0.5)):
            a = (rng.standard_normal(shape) * scale).astype(np.float32).reshape(-1)
            pad = (-a.size) % 4
            row.append(off)
            chunks.append(np.concatenate([a, np.zeros(pad, np.float32)]))
            off += a.size + pad
        offs.append(row)
    flat = np.concatenate(chunks)
    goff = np.concatenate([[0], np.cumsum(SIZES)[:-1]]).astype(np.int64)
    genes = rng.standard_normal(sum(SIZES)).astype(np.float32)
    base = (0.5 * rng.standard_normal(sum(SIZES))).astype(np.float32)
    return flat, np.asarray(offs, np.int64), goff, genes, base


def _unit_reference(flat, offs, goff, genes, base, alphas, dz=None, weights=None):
    """float64 on the CPU: a1, a2, z [G, P, 256] and (with dz, weights) sum_p d/dx_p of sum_p w_p <dz_p, z(x_p)> at the points x_p."""
    P = len(alphas)
    fl = torch.from_numpy(flat).to(F64)
    g, b = torch.from_numpy(genes).to(F64), torch.from_numpy(base).to(F64)
    a1s, a2s, zs, grad = [], [], [], torch.zeros_like(g)
    for i, n in enumerate(SIZES):
        o = offs[i]
        W1, b1 = fl[o[0]:o[0] + GL * n].view(GL, n), fl[o[1]:o[1] + GL]
        W2, b2 = fl[o[2]:o[2] + GL * GL].view(GL, GL), fl[o[3]:o[3] + GL]
        gi, bi = g[goff[i]:goff[i] + n], b[goff[i]:goff[i] + n]
        r1, r2, rz = [], [], []
        for p in range(P):
            xp = (bi + float(alphas[p]) * (gi - bi)).clone().requires_grad_(dz is not None)
            a1 = W1 @ xp + b1
            a2 = W2 @ torch.nn.functional.elu(a1) + b2
            z = torch.nn.functional.elu(a2)
            if dz is not None:
                (dx,) = torch.autograd.grad(float(weights[p]) * (torch.from_numpy(dz[i, p]).to(F64) * z).sum(), xp)
                grad[goff[i]:goff[i] + n] += dx
            r1.append(a1.detach()); r2.append(a2.detach()); rz.append(z.detach())
        a1s.append(torch.stack(r1)); a2s.append(torch.stack(r2)); zs.append(torch.stack(rz))
    return torch.stack(a1s).numpy(), torch.stack(a2s).numpy(), torch.stack(zs).numpy(), grad.numpy()


def _relmax(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / np.abs(ref).max())


UNIT_CASES = [(1, False, [0.625]), (3, True, [0.0, 0.37, 1.0]), (3, False, [1.0, 0.0, 0.5])]


@pytest.mark.parametrize("P,with_base,alphas", UNIT_CASES)
def test_point_kernels_match_float64(P, with_base, alphas):
    _gpu()
    dev, G, n = "cuda", len(SIZES), sum(SIZES)
    flat, offs, goff, genes, base = _unit_params(7 + P)
    if not with_base:
        base = np.zeros_like(base)
    rng = np.random.default_rng(100 + P)
    dz = rng.standard_normal((G, P, GL)).astype(np.float32)
    w = np.asarray([0.25, 0.0, 0.5][:P], np.float32)
    a1r, a2r, zr, dgr = _unit_reference(flat, offs, goff, genes, base, alphas, dz, w)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    fl, of, sz, go, ge = t(flat), t(offs), torch.tensor(SIZES, dtype=torch.int32, device=dev), t(goff), t(genes)
    bs = t(base) if with_base else None
    al = t(np.asarray(alphas, np.float32))
    a1, a2, z = (torch.full((G, P, GL), float("nan"), device=dev) for _ in range(3))
    ops.gene_snn_fwd_points(fl, of, sz, go, ge, bs, al, G, GL, a1, a2, z, P)
    torch.cuda.synchronize()
    errs = {"a1": _relmax(a1.cpu().numpy(), a1r), "a2": _relmax(a2.cpu().numpy(), a2r), "z": _relmax(z.cpu().numpy(), zr)}
    # backward: plain write, then accumulate twice more on top, then with unscale
    dzt, wt = t(dz), t(w)
    dg = torch.full((n,), float("nan"), device=dev)
    ops.gene_snn_bwd_input(fl, of, sz, go, G, GL, a1, a2, dzt, wt, dg, P, accumulate=False)
    one = dg.clone()
    acc = torch.zeros(n, device=dev)
    for _ in range(2):
        ops.gene_snn_bwd_input(fl, of, sz, go, G, GL, a1, a2, dzt, wt, acc, P, accumulate=True)
    us = torch.tensor([0.125], device=dev)
    scaled = torch.zeros(n, device=dev)
    ops.gene_snn_bwd_input(fl, of, sz, go, G, GL, a1, a2, dzt, wt, scaled, P, unscale_dev=us, accumulate=True)
    torch.cuda.synchronize()
    errs["dgenes"] = _relmax(one.cpu().numpy(), dgr)
    print(P, with_base, {k: f"{v:.1e}" for k, v in errs.items()})
    assert max(errs.values()) <= 1e-5, errs
    assert torch.equal(acc, one + one)                       # accumulate = 1 twice: twice the value
    assert torch.equal(scaled, one * 0.125)                  # unscale_dev honoured (a power of two: exact)
    if not with_base and alphas[0] == 1.0:
        # alpha = 1 from a null baseline is the plain forward: the bits of mt_gene_snn_fwd
        p1, p2, pz = torch.empty(G, GL, device=dev), torch.empty(G, 1, GL, device=dev), torch.empty(G, 1, GL, device=dev)
        ops.gene_snn_fwd(fl, of, sz, go, ge, G, GL, p1, p2, pz)
        assert torch.equal(pz[:, 0], z[:, 0]) and torch.equal(p1, a1[:, 0])
        assert torch.equal(a1[:, 1], t(flat)[of[:, 1:2] + torch.arange(GL, device=dev)])      # alpha = 0: a1 = b1 exactly


def test_ig_finalize_matches_numpy_and_repeats_bit_for_bit():
    _gpu()
    dev, G, n = "cuda", len(SIZES), sum(SIZES)
    rng = np.random.default_rng(5)
    genes, base, dg = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    goff = np.concatenate([[0], np.cumsum(SIZES)[:-1]]).astype(np.int64)
    t = lambda a: torch.from_numpy(a).to(dev)
    sz, go = torch.tensor(SIZES, dtype=torch.int32, device=dev), t(goff)
    for b in (base, None):
        attr, pw, pw2 = torch.empty(n, device=dev), torch.empty(G, device=dev), torch.empty(G, device=dev)
        ops.ig_finalize(t(genes), None if b is None else t(b), t(dg), sz, go, G, attr, pw)
        ops.ig_finalize(t(genes), None if b is None else t(b), t(dg), sz, go, G, torch.empty(n, device=dev), pw2)
        torch.cuda.synchronize()
        ref = (genes - (b if b is not None else np.float32(0))) * dg            # fp32: one rounding per operation, as the kernel
        assert np.array_equal(attr.cpu().numpy(), ref)
        sums = np.array([ref[goff[i]:goff[i] + SIZES[i]].astype(np.float64).sum() for i in range(G)])
        mags = np.array([np.abs(ref[goff[i]:goff[i] + SIZES[i]]).astype(np.float64).sum() for i in range(G)])
        assert (np.abs(pw.cpu().numpy() - sums) <= 1e-6 * mags).all()
        assert torch.equal(pw, pw2)


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


def _l2(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(a - ref) / np.linalg.norm(ref))


TGT = torch.from_numpy(TARGET.astype(np.float32))


def test_one_input_gradient_matches_oracle_autograd():
    """The engine-level call, one point at alpha = 1: dF_t/dgenes at the slide's own genes against torch.autograd through the oracle."""
    _gpu()
    from modaltune_amd.engine import GenePoints
    cfg, eng, sizes, (x, coords, genes, clin), _ = _engine()
    n, dev = sum(sizes), "cuda"
    tgt = TGT.to(dev)
    scale = torch.empty(2, device=dev)
    ops.absmax_scale(tgt, scale, 1024.0)
    seed = (tgt * scale[0]).view(1, -1)
    report = {}
    for t in range(3):
        dg = torch.zeros(n, device=dev)
        pts = GenePoints(None, torch.ones(1, device=dev), torch.ones(1, device=dev), dg, unscale=scale[1:2])
        eng.forward(x, coords, genes, torch.eye(3, device=dev)[t:t + 1], need_grad=True, fresh=True, points=pts, stochastic=False)
        eng.backward(seed.clone(), call=eng.last_call)
        torch.cuda.synchronize()
        _, ref = _oracle_f_and_grad("L37_d3", t, TARGET, _case("L37_d3")[5])
        report[t] = _l2(dg.cpu().numpy(), ref)
    print("dF/dgenes, relative L2 against the oracle:", {k: f"{v:.2e}" for k, v in report.items()})
    assert max(report.values()) <= 1e-2, report


@pytest.mark.parametrize("name,tasks,m", [("L37_d3", (0, 1, 2), 16), ("L37_d3", (0,), 7), ("L37_d3_clin", (1,), 16)])
def test_ig_matches_oracle_under_the_same_quadrature(name, tasks, m):
    """m = 16: sixteen points and the two endpoints are six passes of three exactly; m = 7: the last pass is mostly padding; the
    clinical geometry has one more token in front of the task token."""
    _gpu()
    from modaltune_amd.attribution import IntegratedGradients
    cfg, eng, sizes, (x, coords, genes, clin), _ = _engine(name)
    res = IntegratedGradients(eng, tasks, steps=m)(x, coords, genes, TGT, clinical=clin)
    torch.cuda.synchronize()
    assert res["attributions"].shape == (len(tasks), sum(sizes)) and res["pathway"].shape == (len(tasks), len(sizes))
    assert res["attributions"].dtype == torch.float32 and res["attributions"].is_cuda and res["steps"] == m
    assert res["offsets"].tolist() == np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
    report = {}
    for i, t in enumerate(tasks):
        ref = _oracle_ig(name, t, TARGET, m)
        pw = res["pathway"][i].cpu().numpy().astype(np.float64)
        report[t] = (_l2(res["attributions"][i].cpu().numpy(), ref["attributions"]),
                     float(np.abs(pw - ref["pathway"]).max() / np.linalg.norm(ref["pathway"])))
    print(name, m, "relative L2 of the attributions, pathway error / ||pathway||:", {k: (f"{a:.2e}", f"{b:.2e}") for k, (a, b) in report.items()})
    assert max(a for a, _ in report.values()) <= 1e-2, report
    assert max(b for _, b in report.values()) <= 1e-2, report


def test_completeness_on_the_gpu():
    """m = 32, task 0: |convergence_delta| / |delta| <= the oracle's own gap at m = 32 + 2e-2 (1e-2: the attribution bar above, on
    their sum; 1e-2: delta, a difference of two logit rows that each carry the project's 1e-3 logits bar).  f_input / f_baseline
    come out of the IG passes: against two plain forward-only passes of the engine."""
    _gpu()
    from modaltune_amd.attribution import IntegratedGradients
    cfg, eng, sizes, (x, coords, genes, clin), _ = _engine()
    res = IntegratedGradients(eng, (0,), steps=32)(x, coords, genes, TGT)
    oh = torch.eye(3, device="cuda")[0:1]
    f_in = float((eng.forward(x, coords, genes, oh, need_grad=False).double().cpu().reshape(-1) * torch.from_numpy(TARGET)).sum())
    f_b = float((eng.forward(x, coords, [torch.zeros_like(g) for g in genes], oh, need_grad=False).double().cpu().reshape(-1)
                 * torch.from_numpy(TARGET)).sum())
    torch.cuda.synchronize()
    gap = float(res["convergence_delta"].abs() / res["delta"].abs())
    ref = _oracle_ig("L37_d3", 0, TARGET, 32)
    print(f"completeness gap on the GPU at m = 32: {gap:.2e} (oracle {ref['gap']:.2e}); f_input {float(res['f_input']):.6e} / plain {f_in:.6e}; "
          f"f_baseline {float(res['f_baseline']):.6e} / plain {f_b:.6e}")
    assert gap <= ref["gap"] + 2e-2, (gap, ref["gap"])
    assert abs(float(res["f_input"]) - f_in) <= 1e-6 * abs(f_in), (float(res["f_input"]), f_in)
    assert abs(float(res["f_baseline"]) - f_b) <= 1e-6 * abs(f_b), (float(res["f_baseline"]), f_b)
    assert torch.equal(res["delta"], res["f_input"] - res["f_baseline"])
    assert torch.equal(res["convergence_delta"], res["pathway"].sum(1) - res["delta"])


def _module(deterministic=True):
    from modaltune_amd.aggregators import Aggregator
    cfg0, sizes, _, _, _, _, _, inp = _case("L37_d3")
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_L37_d3.npz"))
    groups = {i: ["g"] * n for i, n in enumerate(sizes)}
    model = Aggregator.create("longnetvit_gene_adapter", gene_group_defination=groups, multi_task=3, deterministic=deterministic,
                              **dict(GIGAPATH_JSON, depth=int(g["depth"]), slide_ngrids=int(g["ngrids"]),
                                     interaction_indexes=[list(map(int, p)) for p in g["inter"]], pretrained=False))
    sd = synth.synth_state_dict(model.cfg, sizes, int(g["seed"]))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    x, coords = torch.from_numpy(inp["x"]).cuda(), torch.from_numpy(inp["coords"]).cuda()
    genes = [torch.from_numpy(a).cuda() for a in inp["genes"]]
    return model, x, coords, genes


TENSORS = ("attributions", "pathway", "f_input", "f_baseline", "delta", "convergence_delta")


def test_exact_properties():
    _gpu()
    model, x, coords, genes = _module()
    assert model.cfg.dropout > 0 and model.cfg.drop_path_rate > 0          # (the shipped rates: train() switches the stochastic sites on)
    model.eval()
    a = model.integrated_gradients(x, coords, genes, TGT, task_ids=(0, 2), steps=4)
    # baseline == genes: nothing to attribute, exactly
    z = model.integrated_gradients(x, coords, genes, TGT, task_ids=(0, 2), steps=4, baseline=[g.clone() for g in genes])
    assert int(torch.count_nonzero(z["attributions"])) == 0 and int(torch.count_nonzero(z["pathway"])) == 0
    assert int(torch.count_nonzero(z["delta"])) == 0 and torch.equal(z["f_input"], z["f_baseline"])
    # target -> 2 target: the device scale 1024 / max |target| halves exactly (a power-of-two step), so the scaled seed and with it the
    # whole gradient stream keep their bits, and the reciprocal doubles exactly: every output doubles bit for bit
    b = model.integrated_gradients(x, coords, genes, 2 * TGT, task_ids=(0, 2), steps=4)
    for k in TENSORS:
        assert torch.equal(b[k], 2 * a[k]), k
    # the eval forward runs whatever model.training says (genes as the reference's dict, too)
    model.train()
    assert model.engine.stochastic
    c = model.integrated_gradients(x, coords, {i: g for i, g in enumerate(genes)}, TGT, task_ids=(0, 2), steps=4)
    for k in TENSORS:
        assert torch.equal(c[k], a[k]), k
    assert float(a["attributions"].abs().max()) > 0


def test_ig_leaves_training_state_and_captured_graphs_alone():
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
    ig = IntegratedGradients(eng, (0, 1), steps=4)
    r1 = ig(x, coords, genes, TGT)
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
    # reproducibility on the deterministic engine: a second call gives the same bits in every returned tensor
    r2 = ig(x, coords, genes, TGT)
    torch.cuda.synchronize()
    for k in TENSORS + ("offsets",):
        assert torch.equal(r1[k], r2[k]), k


def test_requests_that_cannot_be_served_raise():
    _gpu()
    from modaltune_amd.aggregators import Aggregator
    from modaltune_amd.attribution import IntegratedGradients
    import modaltune_amd.titan  # noqa: F401
    from test_titan_cpu import TITAN_JSON
    cfg, eng, sizes, (x, coords, genes, clin), _ = _engine()
    with pytest.raises(ValueError, match="steps"):
        IntegratedGradients(eng, (0, 1, 2), steps=0)
    ig = IntegratedGradients(eng, (0, 1, 2), steps=4)
    with pytest.raises(ValueError, match="target"):
        ig(x, coords, genes, torch.ones(2, 256))
    with pytest.raises(ValueError, match="target"):
        ig(x, coords, genes, torch.ones(255))
    with pytest.raises(ValueError, match="baseline"):
        ig(x, coords, genes, TGT, baseline=torch.zeros(sum(sizes) - 1))
    tsizes = synth.toy_group_sizes()
    tm = Aggregator.create("titan_gene_adapter", gene_group_defination={i: ["g"] * n for i, n in enumerate(tsizes)}, **TITAN_JSON,
                           multi_task=3)
    with pytest.raises(NotImplementedError, match="TITAN"):
        IntegratedGradients(tm.engine)
    with pytest.raises(NotImplementedError, match="TITAN"):
        tm.integrated_gradients(None, None, None, None)
