"""GPU: the full-width adapters, E = 768 -- `with_cffn=False`, nn.MultiheadAttention's packed in_proj_weight.

The adapter attention cores at 12 x 64, 24 x 32 and 48 x 16 against float64 at the bars tests/test_adapter_width_gpu.py carries up to
E = 576; the weight-gradient product at the two shapes the width creates, written into a row slice of a [2304, 768] destination; the
train step, the attention maps, the schedules (pass groups, graph replay, deterministic mode, an accumulation window with clipping),
the drop-in module, prompt_dropout and Integrated Gradients against reference goldens generated at the full width
(tests/golden/make_golden_full_width.py) and the float64 restatements of tests/full_width_ref.py; and the shipped configuration's
launch timeline, logits and loss against a recording made with the tree before the feature."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from modaltune_amd import ops, synth  # noqa: E402
from modaltune_amd.config import GIGAPATH_JSON, GeneConfig, ModelConfig, attention_sites, segment_lengths  # noqa: E402

import full_width_ref as R  # noqa: E402
from test_kernels_gpu import _mha_ref, rel, rng  # noqa: E402
from test_model_gpu import GRAD_TOL_NAMED, _build, _rel  # noqa: E402

DEV = "cuda"
PAIRS = [(768, 12), (768, 24), (768, 48)]          # head dims 64, 32, 16 at the full width
TAGS = ["nocffn", "nocffn_h24"]
INTER = [[0, 0], [1, 1], [2, 2]]
PD = 0.25


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ---------------------------------------------------------------- 1. the cores at AE = 768
@pytest.mark.parametrize("T,L", [(65, 301), (7, 129), (128, 513)])
@pytest.mark.parametrize("E,heads", PAIRS)
def test_inject_attention_at_full_width(E, heads, T, L):
    """tests/test_adapter_width_gpu.py::test_inject_attention_at_width's form and bars (a 2e-3, dq 3e-3, dk / dv 1e-3) at a 1536-byte
    row; the map kernel against its float64 recomputation from the kernel's own lse, 1e-5."""
    _gpu()
    hd = E // heads
    g = rng(T)
    B = 3
    q = torch.randn(B, L, E, generator=g).half()
    k = torch.randn(B, T, E, generator=g)
    v = torch.randn(B, T, E, generator=g)
    da = torch.randn(B, L, E, generator=g).half()
    qd, kd, vd = q.double().requires_grad_(True), k.double().requires_grad_(True), v.double().requires_grad_(True)
    ref = _mha_ref(qd, kd, vd, heads)
    ref.backward(da.double())
    M = B * L
    qg, kg, vg = q.to(DEV).view(M, E), k.to(DEV), v.to(DEV)
    a = torch.zeros(M, E, dtype=torch.float16, device=DEV)
    alse = torch.zeros(M, heads, device=DEV)
    ops.inject_attn_fwd(qg, kg, vg, a, M, L, T, lse=alse, heads=heads, head_dim=hd)
    dq = torch.zeros(M, E, dtype=torch.float16, device=DEV)
    dk = torch.zeros(B, T, E, device=DEV)
    dv = torch.zeros(B, T, E, device=DEV)
    ops.inject_attn_bwd(qg, a, alse, da.to(DEV).view(M, E), kg, vg, dq, dk, dv, M, L, T, heads=heads, head_dim=hd)
    w = torch.full((M, T), float("nan"), device=DEV)
    ops.inject_attn_probs(qg, kg, alse, w, M, L, T, heads=heads, head_dim=hd)
    torch.cuda.synchronize()
    kh = kg.half().double().view(B, T, heads, hd)
    s = torch.einsum("blhd,bthd->blht", qg.double().view(B, L, heads, hd), kh).reshape(M, heads, T)
    wref = torch.exp(float(np.float32(hd ** -0.5)) * s - alse.double()[..., None]).mean(dim=1)
    fig = dict(a=rel(a.view(B, L, E), ref), dq=rel(dq.view(B, L, E), qd.grad), dk=rel(dk, kd.grad), dv=rel(dv, vd.grad),
               map=float((w.double() - wref).abs().max()))
    print(f"inject {heads}x{hd} T={T} L={L}", {n: f"{x:.2e}" for n, x in fig.items()})
    assert fig["a"] < 2e-3, fig
    assert fig["dq"] < 3e-3, fig
    assert fig["dk"] < 1e-3 and fig["dv"] < 1e-3, fig
    assert fig["map"] <= 1e-5, fig
    assert float((w.double().sum(-1) - 1).abs().max()) <= 1e-4


@pytest.mark.parametrize("T,L,nsplit", [(65, 700, 4), (7, 129, 1), (128, 1000, 16)])
@pytest.mark.parametrize("E,heads", PAIRS)
def test_extract_attention_at_full_width(E, heads, T, L, nsplit):
    """tests/test_adapter_width_gpu.py::test_extract_attention_at_width's form and bars (out 1.5e-3, dq / dkv 3e-3); map 1e-5."""
    _gpu()
    hd = E // heads
    g = rng(T + L)
    B = 2
    q = torch.randn(B, T, E, generator=g)
    kv = torch.randn(B, L, 2 * E, generator=g).half()
    dout = torch.randn(B, T, E, generator=g)
    qd = q.double().requires_grad_(True)
    kvd = kv.double().requires_grad_(True)
    ref = _mha_ref(qd, kvd[..., :E], kvd[..., E:], heads)
    ref.backward(dout.double())
    qg, kvg = q.to(DEV), kv.to(DEV).view(B * L, 2 * E)
    out = torch.zeros(B, T, E, device=DEV)
    lse = torch.zeros(B, T, heads, device=DEV)
    pa = torch.zeros(B * heads * nsplit * T * hd, device=DEV)
    pm = torch.zeros(B * heads * nsplit * T * 2, device=DEV)
    ops.extract_attn_fwd(qg, kvg, out, lse, pa, pm, B, T, L, nsplit, heads=heads, head_dim=hd)
    dq = torch.zeros(B, T, E, device=DEV)
    dkv = torch.zeros(B * L, 2 * E, dtype=torch.float16, device=DEV)
    ops.extract_attn_bwd(qg, kvg, out, lse, dout.to(DEV), dq, dkv, B, T, L, heads=heads, head_dim=hd)
    w = torch.full((B, T, L), float("nan"), device=DEV)
    ops.extract_attn_probs(qg, kvg, lse, w, B, T, L, heads=heads, head_dim=hd)
    torch.cuda.synchronize()
    qh = (qg * np.float32(hd ** -0.5)).half().double().view(B, T, heads, hd)       # (the kernels scale in fp32, then round to fp16)
    kh = kvg[:, :E].double().view(B, L, heads, hd)
    wref = torch.exp(torch.einsum("bthd,blhd->bthl", qh, kh) - lse.double()[..., None]).mean(dim=2)
    fig = dict(out=rel(out, ref), dq=rel(dq, qd.grad), dkv=rel(dkv.view(B, L, 2 * E), kvd.grad), map=float((w.double() - wref).abs().max()))
    print(f"extract {heads}x{hd} T={T} L={L}", {n: f"{x:.2e}" for n, x in fig.items()})
    assert fig["out"] < 1.5e-3, fig
    assert fig["dq"] < 3e-3, fig
    assert fig["dkv"] < 3e-3, fig
    assert fig["map"] <= 1e-5, fig
    assert float((w.double().sum(-1) - 1).abs().max()) <= 1e-4


@pytest.mark.parametrize("T", [1, 7, 65, 128])
@pytest.mark.parametrize("E,heads", PAIRS)
def test_token_mha_at_full_width(E, heads, T):
    """tests/test_adapter_width_gpu.py::test_token_mha_at_width's form: fp32 throughout, 1e-4; the head-averaged map 1e-5."""
    _gpu()
    g = rng(T + 100)
    B = 3
    q, k, v, do = (torch.randn(B, T, E, generator=g) for _ in range(4))
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    ref = _mha_ref(qd, kd, vd, heads)
    ref.backward(do.double())
    out = torch.zeros(B, T, E, device=DEV)
    probs = torch.zeros(B, heads, T, T, device=DEV)
    ops.token_mha_fwd(q.to(DEV), k.to(DEV), v.to(DEV), out, probs, B, T, E, heads)
    dq, dk, dv = (torch.zeros(B, T, E, device=DEV) for _ in range(3))
    ops.token_mha_bwd(q.to(DEV), k.to(DEV), v.to(DEV), probs, do.to(DEV), dq, dk, dv, B, T, E, heads)
    mean = torch.full((B, T, T), float("nan"), device=DEV)
    ops.token_probs_mean(probs, mean, B, heads, T)
    torch.cuda.synchronize()
    hd = E // heads
    sp = lambda t: t.detach().view(B, T, heads, hd).transpose(1, 2)
    pref = torch.softmax(sp(qd) @ sp(kd).transpose(-1, -2) / hd ** 0.5, -1).mean(1)
    fig = dict(out=rel(out, ref), dq=rel(dq, qd.grad), dk=rel(dk, kd.grad), dv=rel(dv, vd.grad), map=float((mean.double().cpu() - pref).abs().max()))
    print(f"token {heads}x{hd} T={T}", {n: f"{x:.2e}" for n, x in fig.items()})
    assert max(fig[n] for n in ("out", "dq", "dk", "dv")) < 1e-4, fig
    assert fig["map"] <= 1e-5, fig
    assert float((probs.double().sum(-1) - 1).abs().max()) < 1e-5


# ---------------------------------------------------------------- 2. the weight-gradient product at the new shapes
@pytest.mark.parametrize("N1,N2,row0,M", [(n1, n2, r0, M) for n1, n2, r0 in [(768, 768, 0), (1536, 768, 768)] for M in (31, 333, 4100)]
                         + [(1536, 768, 768, 20000)])
def test_gemm_tn_into_a_row_slice_of_the_packed_gradient(N1, N2, row0, M):
    """The Injector's q product (768 x 768 -> rows [0, 768)) and the Extractor's k | v product (1536 x 768 -> rows [768, 2304)) of a
    [2304, 768] destination with the bias gradient into the matching slice of a [2304] vector: M below one 32-row step, a ragged tail,
    more rows than splits -- and, for the k | v product, the first M at which the atomic form launches 128 x 128 tiles (csrc/gemm.hip,
    TN_LARGE_MIN_ROWS; the deterministic form launches them at every M here).  Default form within 1e-3 of float64 over the fp16 operands; the deterministic form bit-identical over two
    calls and within the same bar; everything outside the slice untouched, bit for bit."""
    _gpu()
    g = rng(M + N1)
    A = torch.randn(M, N1, generator=g).half()
    B = torch.randn(M, N2, generator=g).half()
    C0 = torch.randn(2304, 768, generator=g)
    b0 = torch.randn(2304, generator=g)
    ref = C0.double().clone()
    ref[row0:row0 + N1] += A.double().t() @ B.double()
    refb = b0.double().clone()
    refb[row0:row0 + N1] += A.double().sum(0)
    Ad, Bd = A.to(DEV), B.to(DEV)
    outside = torch.ones(2304, dtype=torch.bool)
    outside[row0:row0 + N1] = False

    def run(det):
        C, b = C0.to(DEV).clone(), b0.to(DEV).clone()
        dst = C[row0:row0 + N1]
        assert dst.is_contiguous() and dst.stride(0) == 768 and dst.data_ptr() == C.data_ptr() + row0 * 768 * 4
        ops.gemm_tn(Ad, Bd, dst, M, N1, N2, ldc=768, colsum=b[row0:row0 + N1], det=det)
        torch.cuda.synchronize()
        return C.cpu(), b.cpu()

    need = ops.det_elems("gemm_tn_f16", M, N1, N2, 1)
    assert need % (N1 * (N2 + 1)) == 0 and 1 <= need // (N1 * (N2 + 1)) <= -(-M // 32)      # slots: the launched splits that hold rows
    results = {"default": run(None)}
    ws = torch.full((need,), float("nan"), device=DEV)
    results["det"] = run(ws)
    again = run(torch.full((need,), float("nan"), device=DEV))
    assert torch.equal(results["det"][0], again[0]) and torch.equal(results["det"][1], again[1])
    for what, (C, b) in results.items():
        fig = dict(C=rel(C[row0:row0 + N1], ref[row0:row0 + N1]), b=rel(b[row0:row0 + N1], refb[row0:row0 + N1]))
        print(f"gemm_tn {N1}x{N2} M={M} {what}", {n: f"{x:.2e}" for n, x in fig.items()})
        assert fig["C"] < 1e-3 and fig["b"] < 1e-3, (what, fig)
        assert torch.equal(C[outside], C0[outside]) and torch.equal(b[outside], b0[outside]), what


# ---------------------------------------------------------------- 3. train step and maps against the reference goldens
@pytest.mark.parametrize("tag", TAGS)
def test_train_step_matches_reference_golden_at_full_width(golden_dir, tag):
    """tests/test_model_gpu.py::test_train_step_matches_reference_golden's form and bars."""
    _gpu()
    g, cfg, eng, ts, inp = _build(os.path.join(golden_dir, f"model_L37_d3_{tag}.npz"))
    assert cfg.packed_in_proj and cfg.adapter_dim == 768 and not cfg.extractor_ffn
    eng.collect_taps = True
    x = torch.from_numpy(inp["x"]).cuda()
    genes = [torch.from_numpy(a).cuda() for a in inp["genes"]]
    loss = ts.step(x, inp["coords"], genes, torch.from_numpy(inp["text"]), update=False)
    torch.cuda.synchronize()
    logits = ts.last_logits.cpu().numpy()
    report = {}
    for i in range(len(cfg.interaction_indexes)):
        for t in range(logits.shape[0]):
            if f"f64_tap/task{t}/cls{i}" in g.files:
                report[f"cls{i}/t{t}"] = _rel(eng.taps[f"cls{i}"][t].cpu().numpy(), g[f"f64_tap/task{t}/cls{i}"].reshape(-1))
            if f"f64_tap/task{t}/c{i}" in g.files:
                report[f"c{i}/t{t}"] = _rel(eng.taps[f"c{i}"][t].cpu().numpy(), g[f"f64_tap/task{t}/c{i}"][0])
    report["logits"] = _rel(logits, g["f64_logits"])
    report["loss"] = abs(float(loss) - float(g["f64_loss"])) / abs(float(g["f64_loss"]))
    print(tag, {k: f"{v:.2e}" for k, v in report.items()})
    assert report["logits"] < 1e-3, report
    assert report["loss"] < 1e-3, report
    assert int(ts.found_inf) == 0
    grads = ts.unscaled_grads()
    names = [str(n) for n in g["f64_grad_names"]]
    assert sorted(names) == sorted(grads.keys())
    ours = np.array([float(grads[n].double().norm()) for n in names])
    ref = g["f64_grad_norms"]
    worst = sorted(((abs(o - r) / r, n) for n, o, r in zip(names, ours, ref) if r > 1e-6 * ref.max()), reverse=True)[:4]
    print(tag, "largest gradient-norm errors:", [(n, f"{e:.2e}") for e, n in worst])
    bad = [(n, o, r) for n, o, r in zip(names, ours, ref) if abs(o - r) > GRAD_TOL_NAMED.get(n, 1e-2) * r + 1e-6 * ref.max()]
    assert not bad, bad[:10]
    n = 0
    for k in g.files:
        if k.startswith("f64_grad/"):
            key = k[len("f64_grad/"):]
            err = np.linalg.norm(grads[key].double().cpu().numpy() - g[k]) / (np.linalg.norm(g[k]) + 1e-300)
            assert err < (3.5e-2 if key == "gene_encoder.pathway_compression.weight" else 1e-2), (k, err)
            n += 1
    assert n >= 5


def _engine(g, deterministic=None, **kw):
    from modaltune_amd.engine import Engine
    sizes = [int(s) for s in g["sizes"]]
    cfg = ModelConfig(depth=int(g["depth"]), interaction_indexes=tuple(tuple(int(i) for i in p) for p in g["inter"]),
                      slide_ngrids=int(g["ngrids"]), clinical=bool(int(g["clinical"])), token_agg=str(g["token_agg"]),
                      multi_task=int(g["multi_task"]), **dict(json.loads(str(g["extra_cfg"])), **kw))
    eng = Engine(cfg, sizes, "cuda", deterministic=deterministic)
    sd = synth.synth_state_dict(cfg, sizes, int(g["seed"]))
    eng.load_state_dict(sd)
    return cfg, eng, sizes, sd


def _inputs(sizes, L, seed, ngrids):
    inp = synth.synth_inputs(L, sizes, seed, grid=ngrids)
    return (torch.from_numpy(inp["x"]).cuda(), torch.from_numpy(inp["coords"]).cuda(), [torch.from_numpy(a).cuda() for a in inp["genes"]],
            torch.from_numpy(inp["text"]).cuda(), inp)


def test_maps_match_reference_golden_without_cffn(golden_dir):
    """tests/test_attn_maps_gpu.py::test_maps_match_reference_golden's form; the bar here: every map within 1e-3 of the reference's
    (max over the elements of every site), logits < 1e-3.  EmbeddingExtractor: eager == capture == replay bit for bit, maps included."""
    _gpu()
    from modaltune_amd.evaluate import EmbeddingExtractor
    g = np.load(os.path.join(golden_dir, "attn_maps_L37_d3_nocffn.npz"))
    cfg, eng, sizes, _ = _engine(g)
    L = int(g["L"])
    x, coords, genes, _, _ = _inputs(sizes, L, int(g["seed"]), int(g["ngrids"]))
    ex = EmbeddingExtractor(eng, (0, 1, 2), capture_after=1, attention=True)
    outs = [ex(x, coords, genes, None) for _ in range(3)]
    torch.cuda.synchronize()
    logits, maps = outs[0]
    assert ex.graph_replays >= 1
    for lg, mp in outs[1:]:
        assert torch.equal(lg, logits)
        for s in mp:
            assert torch.equal(mp[s], maps[s]), s
    assert sorted(maps) == sorted(attention_sites(cfg)) == sorted(k[4:] for k in g.files if k.startswith("map/"))
    assert _rel(logits.cpu().numpy(), g["f64_logits"]) < 1e-3
    T = cfg.num_tokens
    assert maps["interactions.0.injector.attn.multihead_attn"].shape == (3, L, T)
    assert maps["interactions.1.extractor.attn.multihead_attn"].shape == (3, T, L)
    assert maps["prompt_selfattention.2.self_attn"].shape == (3, T, T)
    report = {s: float(np.abs(maps[s].cpu().numpy().astype(np.float64) - g["map/" + s].astype(np.float64)).max()) for s in maps}
    print("nocffn maps", {k: f"{v:.1e}" for k, v in report.items()})
    assert max(report.values()) < 1e-3, report


# ---------------------------------------------------------------- 4. schedules at with_cffn=False, L = 37
def test_pass_groups_match_the_batched_step_without_cffn(golden_dir):
    """tests/test_adapter_width_gpu.py::test_pass_groups_match_the_batched_step_at_6x64's form and tolerances."""
    _gpu()
    g, cfg, eng, ts, inp = _build(os.path.join(golden_dir, "model_L37_d3_nocffn.npz"))
    x = torch.from_numpy(inp["x"]).cuda()
    genes = [torch.from_numpy(a).cuda() for a in inp["genes"]]
    text = torch.from_numpy(inp["text"])
    ts.split_min_patches = 1 << 30                    # batched
    ts.step(x, inp["coords"], genes, text, update=False)
    torch.cuda.synchronize()
    l0, loss0, g0 = ts.last_logits.clone(), float(ts.loss), {k: v.clone() for k, v in ts.unscaled_grads().items()}
    ts.split_min_patches = 0                          # two groups
    assert ts._split_now(int(g["L"]))
    ts.step(x, inp["coords"], genes, text, update=False)
    torch.cuda.synchronize()
    l1, loss1, g1 = ts.last_logits.clone(), float(ts.loss), ts.unscaled_grads()
    assert ts._pass_streams is not None and torch.equal(l0, l1) and abs(loss0 - loss1) <= 1e-6 * abs(loss0)
    top = max(float(v.norm()) for v in g0.values())
    for k in g0:
        assert float((g0[k] - g1[k]).norm()) <= 2e-3 * float(g0[k].norm()) + 1e-7 * top, k
    assert _rel(l1.cpu().numpy(), g["f64_logits"]) < 1e-3


def test_graph_replay_matches_eager_without_cffn(golden_dir):
    """tests/test_adapter_width_gpu.py::test_graph_replay_matches_eager_at_6x64's second half: training steps eager against
    step_graphed at that test's lr-scale tolerances, then with lr 0 the replayed forward against the eager one bit for bit."""
    _gpu()
    path = os.path.join(golden_dir, "model_L37_d3_nocffn.npz")
    g, cfg, eng_a, ts_a, inp = _build(path)
    _, _, eng_b, ts_b, _ = _build(path)
    x = torch.from_numpy(inp["x"]).cuda()
    genes = [torch.from_numpy(a).cuda() for a in inp["genes"]]
    text = torch.from_numpy(inp["text"]).cuda()
    la, lb = [], []
    for i in range(5):
        la.append(float(ts_a.step(x, inp["coords"], genes, text, update=True)))
        lb.append(float(ts_b.step_graphed(x, inp["coords"], genes, text)))     # 2 eager warm-ups, capture, replays
    torch.cuda.synchronize()
    assert ts_b._graphs is not None and int(ts_a.step_dev) == int(ts_b.step_dev) == 5
    assert np.allclose(la, lb, rtol=5e-4, atol=0), (la, lb)
    for k in ("interactions.0.injector.gamma", "final_project.weight", "gene_pe", "interactions.1.extractor.attn.multihead_attn.in_proj_weight"):
        a, b = eng_a.store.tensors[k], eng_b.store.tensors[k]
        assert float((a - b).abs().max()) <= 2.5 * 5 * ts_a.lr, k
    ts_b.set_lr(0.0); ts_b.wd = 0.0
    ts_b.step(x, inp["coords"], genes, text, update=False)
    torch.cuda.synchronize()
    lg0 = ts_b.last_logits.clone()
    n0 = ts_b.graph_replays
    for _ in range(3):
        ts_b.step_graphed(x, inp["coords"], genes, text)
        torch.cuda.synchronize()
        assert torch.equal(ts_b.last_logits, lg0)
    assert ts_b.graph_replays > n0


def _det_rig(golden_dir, **ts_kw):
    from modaltune_amd.trainer import TrainStep
    g = np.load(os.path.join(golden_dir, "model_L37_d3_nocffn.npz"))
    cfg, eng, sizes, sd = _engine(g, deterministic=True)
    ts = TrainStep(eng, **ts_kw)
    ts.set_projector(synth.projector_state(int(g["seed"])))
    ts.auto_split, ts.split_min_patches = False, 1 << 30
    x, coords, genes, text, _ = _inputs(sizes, int(g["L"]), int(g["seed"]), int(g["ngrids"]))
    return g, cfg, eng, ts, (x, coords, genes, text)


def test_deterministic_mode_repeats_bit_for_bit_without_cffn(golden_dir):
    """Two optimiser steps from the same state on two engines: loss, every gradient and every parameter torch.equal; and the
    deterministic gradients meet the golden's bars (the partial workspaces follow the width through the _det_elems queries)."""
    _gpu()
    runs = []
    for _ in range(2):
        g, cfg, eng, ts, slide = _det_rig(golden_dir)
        assert eng.deterministic and ts.deterministic
        need = max(ops.det_elems("gemm_tn_f16", 3 * 37, n1, 768, 1) for n1 in (768, 1536))
        assert eng._det_elems(3, 37) >= need
        losses = []
        for _ in range(2):
            ts.step(*slide, update=True)
            losses.append(ts.loss.clone())
        torch.cuda.synchronize()
        assert int(ts.step_dev) == 2 and int(ts.found_inf) == 0
        runs.append(dict(loss=torch.cat([l.reshape(1) for l in losses]), grad=eng.store.flat_grad.clone(), flat=eng.store.flat.clone(),
                         m=ts.m.clone(), v=ts.v.clone()))
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), (k, float((runs[0][k].double() - runs[1][k].double()).abs().max()))
    assert float(runs[0]["loss"][0]) != float(runs[0]["loss"][1])          # (the step did move the weights)
    g, cfg, eng, ts, slide = _det_rig(golden_dir)
    ts.step(*slide, update=False)
    torch.cuda.synchronize()
    grads = ts.unscaled_grads()
    names = [str(n) for n in g["f64_grad_names"]]
    ours, ref = np.array([float(grads[n].double().norm()) for n in names]), g["f64_grad_norms"]
    bad = [(n, o, r) for n, o, r in zip(names, ours, ref) if abs(o - r) > GRAD_TOL_NAMED.get(n, 1e-2) * r + 1e-6 * ref.max()]
    assert not bad, bad[:10]


def test_accumulation_window_with_clipping_without_cffn(golden_dir):
    """tests/test_accum_clip_gpu.py's bars on the deterministic engine, k = 2: the accumulated gradient is the sum of two eager
    micro-steps' gradients (1e-5 of the tensor's maximum + 1e-6 of the largest entry); grad_norm is the float64 norm of the mean
    gradient (1e-5); clip_coef is min(1, max / (norm + 1e-6)) (1e-6); parameters and moments equal the float64 AdamW oracle fed the
    device's own pre-clip mean gradient times the float64 coefficient (1e-6)."""
    _gpu()
    from oracle import modaltune_oracle as O
    g, cfg, eng_t, ts_t, slide = _det_rig(golden_dir, lr=0.0, weight_decay=0.0)
    x, coords, genes, text = slide
    slides = [slide, (x.flip(0).contiguous(), coords.flip(0).contiguous(), [-a for a in genes], text)]      # a second, different slide
    want = None
    for s in slides:                      # two eager micro-steps on the twin
        ts_t.step(*s, update=False)
        torch.cuda.synchronize()
        assert int(ts_t.found_inf) == 0
        part = {k: v.double().clone() for k, v in ts_t.unscaled_grads().items()}
        want = part if want is None else {k: want[k] + part[k] for k in part}
    assert any(float((want[k] - 2 * part[k]).abs().max()) > 0 for k in want)          # (the two slides' gradients differ)
    norm = float(np.sqrt(sum(float((w / 2.0).pow(2).sum()) for w in want.values())))
    g2, cfg2, eng, ts, _ = _det_rig(golden_dir, accumulate=2, max_grad_norm=0.5 * norm, lr=1e-3, weight_decay=0.01)
    p0 = eng.store.flat.double().clone()
    ts.step(*slides[0])
    assert int(ts.step_dev) == 0 and torch.equal(eng.store.flat.double(), p0) and ts.window_pos == 1
    ts.step(*slides[1])
    torch.cuda.synchronize()
    assert int(ts.step_dev) == 1 and int(ts.found_inf) == 0 and ts.window_pos == 0
    got = ts.unscaled_grads()
    top = max(float(w.abs().max()) for w in want.values())
    worst = max((float((got[k].double() - w).abs().max()) / top, k) for k, w in want.items())
    print(f"nocffn accumulate=2: worst max|delta| / largest entry {worst[0]:.3e} ({worst[1]})")
    for k, w in want.items():
        assert float((got[k].double() - w).abs().max()) <= 1e-5 * float(w.abs().max()) + 1e-6 * top, k
    gn = float(ts.grad_norm)
    assert abs(gn - norm) <= 1e-5 * norm, (gn, norm)
    coef = min(1.0, 0.5 * norm / (gn + 1e-6))
    assert abs(float(ts.clip_coef) - coef) <= 1e-6 * coef and coef < 0.51
    gd = eng.store.flat_grad.double() / float(ts.grad_scale) / 2.0
    c64 = min(1.0, 0.5 * norm / (float(gd.norm()) + 1e-6))
    pr, mr, vr = O.adamw_update(p0, c64 * gd, torch.zeros_like(gd), torch.zeros_like(gd), 1, float(ts.lr_dev.cpu()))

    def relf(a, b):
        return float((a.double() - b).abs().max() / (b.abs().max() + 1e-300))
    fig = (relf(eng.store.flat, pr), relf(ts.m, mr), relf(ts.v, vr))
    print("nocffn clipped update: rel p, m, v", fig)
    assert max(fig) < 1e-6, fig


# ---------------------------------------------------------------- 5. the module surface
def test_drop_in_module_without_cffn(golden_dir):
    """Aggregator.create(..., with_cffn=False): a reference-shaped state dict loads with strict=True and comes back under the same keys
    and shapes; the nn.Module bridge reaches graph replay, and its logits and loss match the reference golden (1e-3) and the fused
    TrainStep's logits (1e-4: the same fp32 forward kernels on one pass per call instead of three per launch)."""
    _gpu()
    from modaltune_amd.aggregators import Aggregator
    from oracle import modaltune_oracle as O
    layout = json.load(open(os.path.join(golden_dir, "full_width_layout.json")))["nocffn"]
    path = os.path.join(golden_dir, "model_L37_d3_nocffn.npz")
    g = np.load(path)
    L, seed, ngrids = int(g["L"]), int(g["seed"]), int(g["ngrids"])
    sizes = [int(s) for s in g["sizes"]]
    groups = {i: ["g"] * n for i, n in enumerate(sizes)}
    model = Aggregator.create("longnetvit_gene_adapter", gene_group_defination=groups, multi_task=3,
                              **dict(GIGAPATH_JSON, depth=3, slide_ngrids=ngrids, interaction_indexes=INTER, pretrained=False,
                                     dropout=0.0, drop_path_rate=0.0, **json.loads(str(g["extra_cfg"]))))
    cfg = model.cfg
    assert (cfg.adapter_dim, cfg.num_heads, cfg.packed_in_proj, cfg.extractor_ffn) == (768, 12, True, False)
    sd = synth.synth_state_dict(cfg, sizes, seed)
    assert list(sd.keys()) == list(layout["shapes"].keys())
    res = model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    back = model.state_dict()
    assert {k: list(v.shape) for k, v in back.items()} == layout["shapes"]
    assert torch.equal(back["interactions.2.extractor.attn.multihead_attn.in_proj_weight"].cpu(),
                       torch.from_numpy(sd["interactions.2.extractor.attn.multihead_attn.in_proj_weight"]))
    assert [k for k, p in model.named_parameters() if p.requires_grad] == layout["trainable"]
    inp = synth.synth_inputs(L, sizes, seed, grid=ngrids)
    x, coords = torch.from_numpy(inp["x"]).cuda(), torch.from_numpy(inp["coords"]).cuda()
    genes = {i: torch.from_numpy(a).cuda() for i, a in enumerate(inp["genes"])}
    psd = {k: torch.from_numpy(v).cuda() for k, v in synth.projector_state(seed).items()}
    text = O.projector_forward(torch.from_numpy(inp["text"]).cuda(), psd)
    eye = torch.eye(3).cuda()
    model.train()
    assert not model.engine.stochastic
    for i in range(8):
        xs = x.clone()
        logits = torch.cat([model(x=xs, coords=coords, genes=genes, clinical=[], task_token=eye[t]) for t in (0, 1, 2)])
        loss = O.distill_loss(logits, text)
        loss.backward()
        if i == 0:
            gw = dict(model.named_parameters())["interactions.0.injector.attn.multihead_attn.in_proj_weight"].grad
            assert tuple(gw.shape) == (2304, 768) and float(gw[:768].abs().max()) > 0 and float(gw[768:].abs().max()) > 0
        for p in model.parameters():
            p.grad = None
    torch.cuda.synchronize()
    assert model._replay.replays >= 1
    assert _rel(logits.detach().cpu().numpy(), g["f64_logits"]) < 1e-3
    assert abs(float(loss.detach()) - float(g["f64_loss"])) < 1e-3 * float(g["f64_loss"])
    _, _, eng, ts, _ = _build(path)
    ts.step(x, inp["coords"], [genes[i] for i in range(len(sizes))], torch.from_numpy(inp["text"]), update=False)
    torch.cuda.synchronize()
    fused = _rel(logits.detach().cpu().numpy(), ts.last_logits.cpu().numpy())
    print("module against the fused step's logits:", fused)
    assert fused < 1e-4, fused


# ---------------------------------------------------------------- 6. prompt_dropout at with_cffn=False
def _keep_mask(rng_, site, p, n):
    """tests/test_prompt_dropout_gpu.py::_keep_mask: the device's keep mask of the first n elements of an element-dropout site."""
    D = (int(n) + 3) // 4 * 4
    y = torch.empty(1, D, device=DEV)
    ops.dropout_f32(torch.ones(1, D, device=DEV), y, 1, D, ops.dropout_spec(rng_, site, p))
    return (y[0, :n] != 0).cpu()


def _pd_rig(golden_dir, pd, deterministic=None):
    from modaltune_amd.trainer import TrainStep
    g = np.load(os.path.join(golden_dir, "model_L37_d3_nocffn.npz"))
    kw = dict(dropout=0.0, drop_path_rate=0.0, gene=GeneConfig(dropout=0.0))
    if pd is not None:
        kw["prompt_dropout"] = pd
    cfg, eng, sizes, sd = _engine(g, deterministic=deterministic, **kw)
    ts = TrainStep(eng, split_passes=False)
    ts.set_projector(synth.projector_state(int(g["seed"])))
    x, coords, genes, text, inp = _inputs(sizes, int(g["L"]), int(g["seed"]), int(g["ngrids"]))
    return dict(g=g, cfg=cfg, eng=eng, ts=ts, sizes=sizes, sd=sd, inp=inp, slide=(x, inp["coords"], genes, text))


def _pd_step(r, step_no):
    r["eng"].rng[2] = step_no - 1          # (the step advances the counter first)
    r["ts"].step(*r["slide"], update=False)
    torch.cuda.synchronize()
    return r["ts"].loss.clone()


def test_prompt_dropout_matches_the_restatement_under_the_engines_masks(golden_dir, monkeypatch):
    """tests/test_prompt_dropout_gpu.py::test_train_step_matches_the_float64_oracle_under_the_engines_masks's form and bars with the
    prompt layer of tests/full_width_ref.py: mask 400 + 2 i on the probabilities, mask 401 + 2 i on out_proj's result."""
    _gpu()
    from oracle import modaltune_oracle as O
    r = _pd_rig(golden_dir, PD)
    eng, ts, cfg = r["eng"], r["ts"], r["cfg"]
    eng.set_stochastic(True, seed=4321)
    loss = _pd_step(r, 5)
    assert int(eng.rng[2]) == 5 and int(ts.found_inf) == 0
    logits = ts.last_logits.cpu().numpy()
    grads = ts.unscaled_grads()
    B, T, D, heads = 3, eng.T, cfg.embed_dim, cfg.num_heads
    nint = len(cfg.interaction_indexes)
    keep1 = {i: _keep_mask(eng.rng, 400 + 2 * i, PD, B * heads * T * T).view(B, heads, T, T) for i in range(1, nint)}
    keep2 = {i: _keep_mask(eng.rng, 401 + 2 * i, PD, B * T * D).view(B, T, D) for i in range(1, nint)}
    calls = []

    def masked(c, pe, sd, prefix, heads_):          # the oracle runs task pass by task pass
        n = len(calls)
        task, i = n // (nint - 1), int(prefix.rsplit(".", 1)[1])
        calls.append((task, i))
        return R.prompt_self_attention_nocffn_masked(c, pe, sd, prefix, heads_, keep1[i][task:task + 1], keep2[i][task:task + 1], PD)
    monkeypatch.setattr(O, "prompt_self_attention", masked)
    F64 = torch.float64
    sd = {k: torch.from_numpy(v).to(F64) for k, v in r["sd"].items()}
    psd = {k: torch.from_numpy(v).to(F64) for k, v in synth.projector_state(int(r["g"]["seed"])).items()}
    inp = r["inp"]
    ref_logits, ref_loss, ref_grads = R.train_step_loss_and_grads(
        sd, cfg, synth.trainable_keys(cfg, r["sizes"]), torch.from_numpy(inp["x"]).to(F64), torch.from_numpy(inp["coords"]).to(F64),
        [torch.from_numpy(a).to(F64) for a in inp["genes"]], torch.from_numpy(inp["text"]).to(F64), psd, segment_lengths())
    assert calls == [(t, i) for t in range(B) for i in range(1, nint)]
    fig = dict(logits=_rel(logits, ref_logits.numpy()), loss=abs(float(loss) - float(ref_loss)) / abs(float(ref_loss)),
               masks_matter=_rel(r["g"]["f64_logits"], ref_logits.numpy()))
    names = list(ref_grads)
    ours = np.array([float(grads[n].double().norm()) for n in names])
    ref = np.array([float(ref_grads[n].norm()) for n in names])
    fig["grad_norm_worst"] = float(np.max(np.abs(ours - ref) / (ref + 1e-6 * ref.max())))
    print("prompt_dropout nocffn engine step", {k: f"{v:.2e}" for k, v in fig.items()})
    assert fig["masks_matter"] > 4e-3
    assert fig["logits"] < 4e-4, fig
    assert fig["loss"] < 2e-4, fig
    bad = [(n, o, rr) for n, o, rr in zip(names, ours, ref) if abs(o - rr) > GRAD_TOL_NAMED.get(n, 1e-2) * rr + 1e-6 * ref.max()]
    assert not bad, bad[:10]


def test_zero_prompt_dropout_is_the_model_without_the_key(golden_dir):
    _gpu()
    ra, rb, rc = (_pd_rig(golden_dir, pd, deterministic=True) for pd in (None, 0.0, PD))
    for r in (ra, rb, rc):
        r["eng"].set_stochastic(True, seed=11)
    la, lb, lc = _pd_step(ra, 3), _pd_step(rb, 3), _pd_step(rc, 3)
    assert torch.equal(la, lb) and torch.equal(ra["eng"].store.flat_grad, rb["eng"].store.flat_grad)
    assert not torch.equal(la, lc)


# ---------------------------------------------------------------- 7. attribution
def test_integrated_gradients_completeness_without_cffn(golden_dir):
    """One integrated_gradients(..., inputs="both", steps=16) call at L = 37, task 0: tests/test_patch_ig_gpu.py::
    test_completeness_on_the_gpu's bar -- |convergence_delta| / |delta| <= the float64 oracle's own gap under the same midpoint rule on the
    same path + 2e-2."""
    _gpu()
    from modaltune_amd.attribution import IntegratedGradients
    from oracle import modaltune_oracle as O
    from test_ig_cpu import TARGET
    g = np.load(os.path.join(golden_dir, "model_L37_d3_nocffn.npz"))
    cfg, eng, sizes, sd = _engine(g)
    x, coords, genes, _, inp = _inputs(sizes, int(g["L"]), int(g["seed"]), int(g["ngrids"]))
    m = 16
    res = IntegratedGradients(eng, (0,), steps=m, inputs="both")(x, coords, genes, torch.from_numpy(TARGET.astype(np.float32)))
    torch.cuda.synchronize()
    gap = float(res["convergence_delta"].abs() / res["delta"].abs())
    # the oracle under the same quadrature (tests/test_patch_ig_cpu.py::_cached, through full_width_ref.oracle_state)
    F64 = torch.float64
    osd = R.oracle_state({k: torch.from_numpy(v).to(F64) for k, v in sd.items()}, cfg)
    x64, c64 = torch.from_numpy(inp["x"]).to(F64), torch.from_numpy(inp["coords"]).to(F64)
    g64 = [torch.from_numpy(a).to(F64) for a in inp["genes"]]
    tgt, tok = torch.from_numpy(TARGET), torch.eye(3, dtype=F64)[0]

    def f(xs, gs):
        return (O.model_forward(osd, cfg, xs, c64, gs, tok, segment_lengths()).reshape(-1) * tgt).sum()
    total = 0.0
    for k in range(m):
        a = (k + 0.5) / m
        xs, gs = (a * x64).requires_grad_(True), [(a * t).requires_grad_(True) for t in g64]
        grads = torch.autograd.grad(f(xs, gs), [xs] + gs)
        total += float((grads[0] * x64).sum() + sum((d * t).sum() for d, t in zip(grads[1:], g64))) / m
    with torch.no_grad():
        delta = float(f(x64, g64) - f(torch.zeros_like(x64), [torch.zeros_like(t) for t in g64]))
    ref_gap = abs(total - delta) / abs(delta)
    print(f"nocffn IG both, m = {m}: completeness gap on the GPU {gap:.2e} (oracle {ref_gap:.2e}); delta {float(res['delta']):.6e} / oracle {delta:.6e}")
    assert gap <= ref_gap + 2e-2, (gap, ref_gap)
    assert abs(float(res["delta"]) - delta) <= 1e-2 * abs(delta)
    assert torch.equal(res["convergence_delta"], res["pathway"].sum(1) + res["patches_total"] - res["delta"])


# ---------------------------------------------------------------- 8. the shipped width is untouched
def record_shipped_step():
    """{"timeline": [launch key, ...], "logits": [[bits]], "loss": bits} of one eager, batched train step (update=False, after one untimed
    step) of the shipped configuration on fixture model_L37_d3.  tests/golden/full_width_parent_timeline.json is this function's output
    on the tree before the full-width adapters existed."""
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    g, cfg, eng, ts, inp = _build(os.path.join(golden, "model_L37_d3.npz"))
    assert (cfg.adapter_dim, cfg.num_heads, cfg.with_cffn) == (192, 12, True)
    ts.auto_split, ts.split_min_patches = False, 1 << 30
    x = torch.from_numpy(inp["x"]).cuda()
    genes = [torch.from_numpy(a).cuda() for a in inp["genes"]]
    text = torch.from_numpy(inp["text"]).cuda()
    ts.step(x, inp["coords"], genes, text, update=False)
    torch.cuda.synchronize()
    ops.TIMER, ops.TIMELINE = {}, []
    try:
        ts.step(x, inp["coords"], genes, text, update=False)
        torch.cuda.synchronize()
    finally:
        timeline, ops.TIMER, ops.TIMELINE = ops.TIMELINE, None, None
    return {"timeline": [t[0] for t in timeline], "logits": ts.last_logits.cpu().view(torch.int32).tolist(),
            "loss": int(ts.loss.cpu().reshape(1).view(torch.int32)[0])}


def test_shipped_configuration_launches_what_the_parent_launched(golden_dir):
    want = json.load(open(os.path.join(golden_dir, "full_width_parent_timeline.json")))
    _gpu()
    got = record_shipped_step()
    assert len(want["timeline"]) > 100
    assert got["timeline"] == want["timeline"]
    assert got["logits"] == want["logits"] and got["loss"] == want["loss"]          # the same bits
