"""GPU: attention maps of the Modal-Adapter attentions (the need_weights output of the reference's nn.MultiheadAttention modules).

Kernels against a float64 recomputation from the same fp16-rounded operands and the same LSE; the model's maps against the reference
(tests/golden/attn_maps_*.npz, tests/golden/make_golden_attn_maps.py); the request changes nothing else (logits bit-identical, train
step unchanged); graph replay reproduces the eager maps bit for bit, for the batched pass and for the two pass groups."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from modaltune_amd import ops, synth  # noqa: E402
from modaltune_amd.config import GIGAPATH_JSON, ModelConfig, attention_sites, token_legend  # noqa: E402

AE, AH = 192, 12
INTER = [[0, 0], [1, 1], [2, 2]]


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ---------------------------------------------------------------- kernels
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("L", [1, 37, 1500, 10001])
@pytest.mark.parametrize("T", [7, 65, 128])
def test_extract_and_inject_maps_match_f64_recomputation(T, L, B):
    _gpu()
    g = torch.Generator(device="cuda").manual_seed(1000 * T + 10 * L + B)
    dev = "cuda"
    # extractor: q fp32 [B,T,192], kv fp16 [B*L,384]
    q = torch.randn(B, T, AE, device=dev, generator=g) * 2.0
    kv = (torch.randn(B * L, 2 * AE, device=dev, generator=g) * 1.5).half()
    out, lse = torch.empty(B, T, AE, device=dev), torch.empty(B, T, AH, device=dev)
    kps = -(-(-(-L // max(1, min(64, L // 256)))) // 64) * 64       # (the engine's split rule)
    nsplit = -(-L // kps)
    pa, pml = torch.empty(B * AH * nsplit * T * 16, device=dev), torch.empty(B * AH * nsplit * T * 2, device=dev)
    ops.extract_attn_fwd(q, kv, out, lse, pa, pml, B, T, L, nsplit)
    w = torch.full((B, T, L), float("nan"), device=dev)
    ops.extract_attn_probs(q, kv, lse, w, B, T, L)
    qh = (q * 0.25).half().double().view(B, T, AH, 16)
    kh = kv[:, :AE].double().view(B, L, AH, 16)
    s = torch.einsum("bthd,blhd->bthl", qh, kh)
    ref = torch.exp(s - lse.double()[..., None]).mean(dim=2)
    err = float((w.double() - ref).abs().max())
    assert err <= 1e-5, err
    assert float((w.double().sum(-1) - 1).abs().max()) <= 1e-4
    del s, ref
    # injector: q fp16 [M,192], k fp32 [B,T,192]
    M = B * L
    q2 = (torch.randn(M, AE, device=dev, generator=g) * 2.0).half()
    k = torch.randn(B, T, AE, device=dev, generator=g) * 1.5
    v = torch.randn(B, T, AE, device=dev, generator=g)
    a, alse = torch.empty(M, AE, dtype=torch.float16, device=dev), torch.empty(M, AH, device=dev)
    ops.inject_attn_fwd(q2, k, v, a, M, L, T, lse=alse)
    wi = torch.full((M, T), float("nan"), device=dev)
    ops.inject_attn_probs(q2, k, alse, wi, M, L, T)
    kh = k.half().double().view(B, T, AH, 16)
    s = torch.einsum("blhd,bthd->blht", q2.double().view(B, L, AH, 16), kh).reshape(M, AH, T)
    ref = torch.exp(0.25 * s - alse.double()[..., None]).mean(dim=1)
    err = float((wi.double() - ref).abs().max())
    assert err <= 1e-5, err
    assert float((wi.double().sum(-1) - 1).abs().max()) <= 1e-4


@pytest.mark.parametrize("T", [7, 65, 128])
def test_token_probs_mean(T):
    _gpu()
    g = torch.Generator(device="cuda").manual_seed(T)
    B = 3
    q, k, v = (torch.randn(B, T, AE, device="cuda", generator=g) for _ in range(3))
    out, probs = torch.empty(B, T, AE, device="cuda"), torch.empty(B, AH, T, T, device="cuda")
    ops.token_mha_fwd(q, k, v, out, probs, B, T, AE, AH)
    w = torch.full((B, T, T), float("nan"), device="cuda")
    ops.token_probs_mean(probs, w, B, AH, T)
    assert float((w.double() - probs.double().mean(1)).abs().max()) <= 1e-6
    assert float((w.double().sum(-1) - 1).abs().max()) <= 1e-4


# ---------------------------------------------------------------- model against the reference
def _engine(g):
    from modaltune_amd.engine import Engine
    sizes = [int(s) for s in g["sizes"]]
    cfg = ModelConfig(depth=int(g["depth"]), interaction_indexes=tuple(tuple(int(i) for i in p) for p in g["inter"]),
                      slide_ngrids=int(g["ngrids"]), clinical=bool(int(g["clinical"])), token_agg=str(g["token_agg"]),
                      multi_task=int(g["multi_task"]), **json.loads(str(g["extra_cfg"])))
    eng = Engine(cfg, sizes, "cuda")
    eng.load_state_dict(synth.synth_state_dict(cfg, sizes, int(g["seed"])))
    return cfg, eng, sizes


def _inputs(cfg, sizes, L, seed, ngrids):
    inp = synth.synth_inputs(L, sizes, seed, grid=ngrids)
    x = torch.from_numpy(inp["x"]).cuda()
    coords = torch.from_numpy(inp["coords"]).cuda()
    genes = [torch.from_numpy(a).cuda() for a in inp["genes"]]
    clin = torch.from_numpy(inp["clinical"]).cuda() if cfg.clinical else None
    return x, coords, genes, clin


def _row_l1(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).sum(-1).max())


@pytest.mark.parametrize("name", ["L37_d3", "L37_d3_cls_cat", "L37_d3_clin", "L1500_d3"])
def test_maps_match_reference_golden(golden_dir, name):
    _gpu()
    from modaltune_amd.evaluate import EmbeddingExtractor
    g = np.load(os.path.join(golden_dir, f"attn_maps_{name}.npz"))
    cfg, eng, sizes = _engine(g)
    x, coords, genes, clin = _inputs(cfg, sizes, int(g["L"]), int(g["seed"]), int(g["ngrids"]))
    ex = EmbeddingExtractor(eng, (0, 1, 2), graphed=False, attention=True)
    logits, maps = ex(x, coords, genes, clin)
    torch.cuda.synchronize()
    assert sorted(maps) == sorted(attention_sites(cfg))
    rel = float(np.abs(logits.cpu().numpy() - g["f64_logits"]).max() / np.abs(g["f64_logits"]).max())
    assert rel < 1e-3, rel
    report = {}
    for k in g.files:
        if not k.startswith("map/"):
            continue
        site = k[4:]
        if "/task" in site:
            site, t = site.rsplit("/task", 1)
            ours = maps[site][int(t)].cpu().numpy()
        else:
            ours = maps[site].cpu().numpy()
        assert ours.shape == g[k].shape, (k, ours.shape, g[k].shape)
        report[k] = _row_l1(ours, g[k])
    print(name, {k: f"{v:.1e}" for k, v in report.items()})
    assert len(report) >= 3
    bad = {k: v for k, v in report.items() if v > 5e-3}
    assert not bad, bad


# ---------------------------------------------------------------- non-interference and schedules
def _fixture_engine(golden_dir, name="L37_d3"):
    g = np.load(os.path.join(golden_dir, f"attn_maps_{name}.npz"))
    cfg, eng, sizes = _engine(g)
    return g, cfg, eng, sizes


def test_request_leaves_logits_and_train_step_unchanged(golden_dir):
    _gpu()
    from modaltune_amd.evaluate import EmbeddingExtractor
    from modaltune_amd.trainer import TrainStep
    g, cfg, eng, sizes = _fixture_engine(golden_dir)
    L, seed = int(g["L"]), int(g["seed"])
    x, coords, genes, clin = _inputs(cfg, sizes, L, seed, int(g["ngrids"]))
    ts = TrainStep(eng)
    ts.set_projector(synth.projector_state(seed))
    text = torch.from_numpy(synth.synth_inputs(L, sizes, seed, grid=int(g["ngrids"]))["text"])
    loss0 = float(ts.step(x, coords, genes, text, update=False, clinical=clin))
    lg0 = ts.last_logits.clone()
    for split in (False, True):                 # batched and the two pass groups (forced on at fixture size)
        plain = EmbeddingExtractor(eng, (0, 1, 2), capture_after=1)
        req = EmbeddingExtractor(eng, (0, 1, 2), capture_after=1, attention=True)
        for e in (plain, req):
            e.split_min_patches = 0 if split else 1 << 30
        pl = [plain(x, coords, genes, clin) for _ in range(3)]      # eager, then capture + replay
        rq = [req(x, coords, genes, clin) for _ in range(3)]
        torch.cuda.synchronize()
        assert plain.graph_replays >= 1 and req.graph_replays >= 1
        for a, (b, maps) in zip(pl, rq):
            assert torch.equal(a, b) and torch.equal(a, pl[0])
            for s in maps:
                assert torch.equal(maps[s], rq[0][1][s]), s
        site = attention_sites(cfg)[0]
        assert rq[1][1][site].data_ptr() != rq[2][1][site].data_ptr()     # fresh tensors per call
    loss1 = float(ts.step(x, coords, genes, text, update=False, clinical=clin))
    assert loss1 == loss0 and torch.equal(ts.last_logits, lg0)


def test_schedules_agree_at_full_bag_and_module_api(golden_dir):
    """L = 10 000, B = 3: graph replay reproduces the eager maps bit for bit, for the batched pass and for the two pass groups; the
    two schedules agree to rounding (their logits already differ in the last bits: the patch-side products run at M = 2 L + L
    instead of 3 L rows); the module API (LongNetGeneAdapter.attention_maps) gives the EmbeddingExtractor's maps."""
    _gpu()
    from modaltune_amd.aggregators import Aggregator
    from modaltune_amd.evaluate import EmbeddingExtractor
    g = np.load(os.path.join(golden_dir, "attn_maps_L37_d3.npz"))
    sizes, seed, ngrids = [int(s) for s in g["sizes"]], int(g["seed"]), 128
    groups = {i: ["g"] * n for i, n in enumerate(sizes)}
    model = Aggregator.create("longnetvit_gene_adapter", gene_group_defination=groups, multi_task=3,
                              **dict(GIGAPATH_JSON, depth=3, slide_ngrids=ngrids, interaction_indexes=INTER, pretrained=False))
    sd = synth.synth_state_dict(model.cfg, sizes, seed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    eng, L = model.engine, 10000
    x, coords, genes, _ = _inputs(model.cfg, sizes, L, seed, ngrids)
    res = {}
    for tag, split in (("batched", False), ("groups", True)):
        ex = EmbeddingExtractor(eng, (0, 1, 2), capture_after=1, attention=True)
        ex.split_min_patches = 7500 if split else 1 << 30
        res[tag] = ex(x, coords, genes)                                 # eager
        res[tag + "_replay"] = ex(x, coords, genes)                     # capture + replay
        assert ex.graph_replays == 1
    plain = EmbeddingExtractor(eng, (0, 1, 2), graphed=False, attention=True)(x, coords, genes)
    model.train()                                       # the module API runs the eval forward whatever the mode
    out = model.attention_maps(x, coords, {i: t for i, t in enumerate(genes)})
    torch.cuda.synchronize()
    lg, maps = res["batched"]
    T = model.cfg.num_tokens
    assert maps["interactions.0.injector.attn.multihead_attn"].shape == (3, L, T)
    assert maps["interactions.1.extractor.attn.multihead_attn"].shape == (3, T, L)
    assert maps["prompt_selfattention.2.self_attn"].shape == (3, T, T)
    for tag in ("batched", "groups"):
        assert torch.equal(res[tag + "_replay"][0], res[tag][0]), tag
        for s in maps:
            assert torch.equal(res[tag + "_replay"][1][s], res[tag][1][s]), (tag, s)
    diff = {s: float((res["groups"][1][s] - maps[s]).abs().max()) for s in maps}
    print("groups vs batched, max |diff|:", {s: f"{v:.1e}" for s, v in diff.items()})
    assert max(diff.values()) < 1e-4, diff
    for src in (plain, (out["logits"], out["maps"])):
        assert torch.equal(src[0], lg)
        for s in maps:
            assert torch.equal(src[1][s], maps[s]), s
    assert out["tokens"] == token_legend(model.cfg)
    for s in maps:
        assert float((maps[s].double().sum(-1) - 1).abs().max()) < 1e-4, s
    sub = model.attention_maps(x, coords, genes, task_ids=(2,), sites=["interactions.2.extractor.attn.multihead_attn"])
    assert list(sub["maps"]) == ["interactions.2.extractor.attn.multihead_attn"]
    one = sub["maps"]["interactions.2.extractor.attn.multihead_attn"]          # (a B = 1 pass: products at M = L rows)
    assert one.shape == (1, T, L)
    assert float((one[0] - maps["interactions.2.extractor.attn.multihead_attn"][2]).abs().max()) < 1e-4


def test_requests_that_cannot_be_served_raise(golden_dir):
    _gpu()
    from modaltune_amd.aggregators import Aggregator
    from modaltune_amd.evaluate import EmbeddingExtractor
    import modaltune_amd.titan  # noqa: F401
    from test_titan_cpu import TITAN_JSON
    g, cfg, eng, sizes = _fixture_engine(golden_dir)
    L = int(g["L"])
    x, coords, genes, clin = _inputs(cfg, sizes, L, int(g["seed"]), int(g["ngrids"]))
    maps = eng.new_attention_maps(attention_sites(cfg), 3, L)
    with pytest.raises(ValueError, match="need_grad=False"):
        eng.forward(x, coords, genes, torch.eye(3), need_grad=True, attn_maps=maps)
    with pytest.raises(ValueError, match="unknown attention site"):
        EmbeddingExtractor(eng, (0, 1, 2), attention=["interactions.0.injector.attn"])
    tsizes = synth.toy_group_sizes()
    tm = Aggregator.create("titan_gene_adapter", gene_group_defination={i: ["g"] * n for i, n in enumerate(tsizes)}, **TITAN_JSON,
                           multi_task=3)
    with pytest.raises(NotImplementedError, match="cell-to-coordinate"):
        EmbeddingExtractor(tm.engine, (0, 1, 2), attention=True)
    with pytest.raises(NotImplementedError, match="TITAN"):
        tm.attention_maps(None, None, None)
