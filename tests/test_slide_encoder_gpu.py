"""GPU: the plain slide encoder (modaltune_amd/slide_encoder.py) against the reference's own outcomes
(tests/golden/slide_encoder_L*.npz) and the oracle restatement (tests/slide_encoder_ref.py).

BAR is the bound tests/test_model_gpu.py::test_train_step_matches_reference_golden holds the logits of the depth-3 model goldens to
against fp64 (1e-3; fp16 operands, fp32 accumulation, fp32 residual stream), taken here as a relative L2 error per outcome.

Measured on an MI355X (this file's printout; relative L2 against fp64, worst outcome of each mode: single output | hidden states):
    L = 37 (N = 2)   cls 7.5e-4 | 7.6e-4    pool 4.4e-4 | 4.5e-4    return_feats rows 6.2e-4 | 6.1e-4
    L = 513          cls 8.1e-4 | 8.0e-4    pool 4.3e-4 | 4.3e-4    return_feats rows 6.4e-4 | 6.3e-4
    L = 1500         cls 8.2e-4 | 8.2e-4    pool 4.5e-4 | 4.5e-4    return_feats rows 6.5e-4 | 6.4e-4
    L = 1            cls 9.2e-4 | 9.1e-4    pool 6.8e-4 | 6.9e-4
    L = 2            cls 8.5e-4 | 8.5e-4    pool 6.0e-4 | 6.1e-4
The embedded input (hidden state 0) sits at 5e-8 (cls) and 1.5e-5 ... 8.5e-5 (pool); the cls row then takes 6e-4 ... 7e-4 in the first
layer: from there on it consists of branch outputs, which are products of fp16-stored operands.
"""
import os

import numpy as np
import pytest
import torch

import slide_encoder_ref as R
from modaltune_amd import synth
from modaltune_amd.config import GIGAPATH_JSON

pytestmark = pytest.mark.gpu

BAR = 1e-3
_built = {}


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _model(wseed, depth=3, ngrids=128, **kw):
    """One module per (weights, options), shared by the tests of this file (global_pool / return_feats are read per call)."""
    from modaltune_amd import slide_encoder as SE
    key = (wseed, depth, ngrids, tuple(sorted(kw.items())))
    if key not in _built:
        m = SE.gigapath_slide_enc12l768d(in_chans=1536, depth=depth, slide_ngrids=ngrids, init_seed=0, **kw)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in R.backbone_state(wseed, depth, ngrids).items()}, strict=True)
        _built[key] = m.eval()
    return _built[key]


def _fixture(golden_dir, L):
    g = np.load(os.path.join(golden_dir, f"slide_encoder_L{L}.npz"))
    x, coords = R.bags(L, g["iseeds"], int(g["ngrids"]), int(g["in_chans"]))
    return g, torch.from_numpy(x).cuda(), torch.from_numpy(coords).cuda()


@pytest.mark.parametrize("L", [37, 513, 1500])
def test_outcomes_match_the_reference_fixtures(golden_dir, L):
    """Every outcome of every (global_pool, all_layer_embed) mode against the reference's fp64 run, and the head of the return_feats
    state (single output: encoder.layer_norm applied)."""
    _gpu()
    g, x, coords = _fixture(golden_dir, L)
    m = _model(int(g["wseed"]), graphed=False, return_feats=True)
    report = {}
    for gp in (0, 1):
        m.global_pool = bool(gp)
        for al in (0, 1):
            outs, feats = m(x, coords, all_layer_embed=bool(al))
            ref = g[f"f64/gp{gp}_al{al}"]
            assert len(outs) == ref.shape[0] == (4 if al else 1)
            for k, o in enumerate(outs):
                assert o.dtype == torch.float32 and tuple(o.shape) == (x.shape[0], 768)
                report[f"gp{gp}/al{al}/{k}"] = _l2(o.cpu().numpy(), ref[k])
            assert tuple(feats.shape) == (x.shape[0], L + 1, 768)
            report[f"gp{gp}/al{al}/feats"] = _l2(feats[:, :8].cpu().numpy(), g[f"f64/feats_al{al}"])
    print(f"slide encoder L={L}:", {k: f"{v:.2e}" for k, v in report.items()})
    worst = max(report, key=report.get)
    assert report[worst] < BAR, (worst, report)


@pytest.mark.parametrize("L", [1, 2])
def test_small_bags_against_the_oracle(L):
    """L = 1 and L = 2 (N = 2 and 3 token rows: every dilated branch is one short segment) against tests/slide_encoder_ref.py in fp64,
    every outcome of every mode, at BAR.

    The cls row is the 0.02-sigma cls token plus branch outputs, i.e. almost entirely the product of fp16-stored operands, and two
    token rows average nothing out: these bags sit closest to the bar (L = 1: 9.2e-4).  With the branches added to the stream through
    fp16 copies, as the adapter path adds them, L = 1 measured 1.02e-3; the module keeps the stream fp32 (slide_encoder._launch)."""
    _gpu()
    wseed = 61
    sd = {k: torch.from_numpy(v).double() for k, v in R.backbone_state(wseed).items()}
    m = _model(wseed, graphed=False, return_feats=True)
    report = {}
    x, coords = R.bags(L, (81 + L,))
    for gp in (False, True):
        m.global_pool = gp
        for al in (False, True):
            want, _ = R.forward(sd, torch.from_numpy(x).double(), torch.from_numpy(coords).double(), 3, gp, al)
            outs, _ = m(torch.from_numpy(x).cuda(), torch.from_numpy(coords).cuda(), all_layer_embed=al)
            assert len(outs) == len(want)
            report[(L, gp, al)] = [_l2(o.cpu().numpy(), w.numpy()) for o, w in zip(outs, want)]
            print(f"L={L} pool={gp} all={al}:", [f"{e:.2e}" for e in report[(L, gp, al)]])
    assert max(max(v) for v in report.values()) < BAR, report


def test_encoder_layer_norm_is_applied_and_before_the_mean(golden_dir):
    """Pool mode, synth's random LayerNorm affines: the last all-layer outcome (no encoder.layer_norm) differs from the single output
    (encoder.layer_norm on every row, THEN the mean) by far more than BAR, and each sits at its own reference."""
    _gpu()
    g, x, coords = _fixture(golden_dir, 513)
    m = _model(int(g["wseed"]), graphed=False, return_feats=True)
    m.global_pool = True
    single = m(x, coords)[0][0].cpu().numpy()
    last = m(x, coords, all_layer_embed=True)[0][-1].cpu().numpy()
    assert _l2(last, single) > 10 * BAR
    assert _l2(single, g["f64/gp1_al0"][0]) < BAR and _l2(last, g["f64/gp1_al1"][-1]) < BAR
    # LN(mean(x)) -- encoder.layer_norm AFTER the mean -- is not what the reference computes either
    sd = {k: torch.from_numpy(v).double() for k, v in R.backbone_state(int(g["wseed"])).items()}
    _, state = R.forward(sd, x.double().cpu(), coords.double().cpu(), 3, True, True)
    from oracle import modaltune_oracle as O
    wrong = O._ln(O._ln(state[:, 1:].mean(dim=1), sd, "encoder.layer_norm"), sd, "norm", R.NORM_EPS).numpy()
    assert _l2(wrong, g["f64/gp1_al0"][0]) > 10 * BAR and _l2(single, wrong) > 10 * BAR


def test_batching_and_input_shapes(golden_dir):
    """N = 2 on the pass axis equals the two N = 1 calls within BAR; [L, C] equals [1, L, C]; chunks of the pass axis change nothing."""
    _gpu()
    from modaltune_amd import slide_encoder as SE
    g, x, coords = _fixture(golden_dir, 37)
    m = _model(int(g["wseed"]), graphed=False, return_feats=True)
    for gp in (False, True):
        m.global_pool = gp
        for al in (False, True):
            both, fb = m(x, coords, all_layer_embed=al)
            ones = [m(x[i:i + 1], coords[i:i + 1], all_layer_embed=al) for i in range(2)]
            for k in range(len(both)):
                for i in range(2):
                    assert _l2(both[k][i].cpu().numpy(), ones[i][0][k][0].cpu().numpy()) < BAR
            flat, ff = m(x[0], coords[0], all_layer_embed=al)
            assert all(torch.equal(a, b) for a, b in zip(flat, ones[0][0])) and torch.equal(ff, ones[0][1])
    old = SE.MAX_CHUNK_ROWS
    try:
        SE.MAX_CHUNK_ROWS = 38                  # one bag (38 token rows) per chunk
        chunked, fc = m(x, coords, all_layer_embed=True)
    finally:
        SE.MAX_CHUNK_ROWS = old
    assert all(torch.equal(a[i], ones[i][0][k][0]) for k, a in enumerate(chunked) for i in range(2)) and tuple(fc.shape) == (2, 38, 768)


def test_replay_equals_eager(golden_dir):
    """A recurring (N, L, all_layer_embed) is captured after `capture_after` visits and replayed: torch.equal with the eager run, for
    new inputs of the same geometry too."""
    _gpu()
    g, x, coords = _fixture(golden_dir, 513)
    eager = _model(int(g["wseed"]), graphed=False, return_feats=True)
    rep = _model(int(g["wseed"]), graphed=True, capture_after=1, return_feats=True)
    x2, c2 = (torch.from_numpy(a).cuda() for a in R.bags(513, (99,)))
    for gp in (False, True):
        eager.global_pool = rep.global_pool = gp
        for al in (False, True):
            want, wf = eager(x, coords, all_layer_embed=al)
            before = rep.graph_replays
            first = rep(x, coords, all_layer_embed=al)                      # eager visit (counted)
            second = rep(x, coords, all_layer_embed=al)                     # captured and replayed
            third = rep(x2, c2, all_layer_embed=al)                         # replay, other slide
            again = rep(x, coords, all_layer_embed=al)
            assert rep.graph_replays == before + 3
            for got in (first, second, again):
                assert all(torch.equal(a, b) for a, b in zip(got[0], want)) and torch.equal(got[1], wf)
            w2, wf2 = eager(x2, c2, all_layer_embed=al)
            assert all(torch.equal(a, b) for a, b in zip(third[0], w2)) and torch.equal(third[1], wf2)


def test_adapter_shares_its_frozen_tensors_and_features_are_collected(golden_dir):
    """LongNetGeneAdapter.slide_encoder(): the same storage (no second backbone copy), the same outcomes as a stand-alone module with
    those weights, bitwise unchanged by an adapter train step; evaluate.get_features collects [cases, 768] through BaselineFeatures."""
    _gpu()
    from modaltune_amd import optim
    from modaltune_amd.aggregators import Aggregator
    from modaltune_amd.evaluate import get_features
    from modaltune_amd.slide_encoder import BaselineFeatures
    sizes = synth.toy_group_sizes()
    groups = {i: ["g"] * n for i, n in enumerate(sizes)}
    model = Aggregator.create("longnetvit_gene_adapter", gene_group_defination=groups, multi_task=3,
                              **dict(GIGAPATH_JSON, depth=3, slide_ngrids=128, interaction_indexes=[[0, 0], [1, 1], [2, 2]], dropout=0.0,
                                     drop_path_rate=0.0, pretrained=False))
    wseed = 61
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(model.cfg, sizes, wseed).items()}, strict=True)
    enc = model.slide_encoder()
    assert not enc.training and enc.engine is model.engine
    theirs = dict(model.named_parameters())
    for k, p in enc.named_parameters():
        assert p.data_ptr() == theirs[k].data_ptr() and not p.requires_grad, k
    assert sorted(enc.state_dict()) == sorted(R.backbone_state(wseed))
    g, x, coords = _fixture(golden_dir, 37)
    alone = _model(wseed, graphed=False, return_feats=True)
    alone.global_pool = False
    before = enc(x, coords, all_layer_embed=True)
    assert all(torch.equal(a, b) for a, b in zip(before, alone(x, coords, all_layer_embed=True)[0]))
    assert _l2(torch.stack(before).cpu().numpy(), g["f64/gp0_al1"]) < BAR
    # one train step of the adapter on the same slide: the trainable tensors move, the baseline embedding does not
    inp = synth.synth_inputs(37, sizes, 71, grid=128)
    genes = {i: torch.from_numpy(a).cuda() for i, a in enumerate(inp["genes"])}
    opt = optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=1e-3)
    moved = model.state_dict()["final_project.weight"].clone()
    eye = torch.eye(3, device="cuda")
    model.train()
    logits = torch.cat([model(x=x[0], coords=coords[0], genes=genes, task_token=eye[t]) for t in range(3)])
    logits.square().sum().backward()
    opt.step()
    torch.cuda.synchronize()
    assert not torch.equal(moved, model.state_dict()["final_project.weight"])
    after = enc(x, coords, all_layer_embed=True)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    # the collector: same slide dicts as EmbeddingExtractor's, genes ignored
    slides = [{"x": x[i], "coords": coords[i], "genes": [torch.from_numpy(a).cuda() for a in inp["genes"]], "case_id": f"c{i}"} for i in range(2)]
    feats, ids = get_features(BaselineFeatures(enc), slides)
    assert feats.shape == (2, 768) and ids == ["c0", "c1"]
    assert _l2(feats, g["f64/gp0_al0"][0]) < BAR
    pooled = get_features(BaselineFeatures(model.slide_encoder(global_pool=True)), slides)[0]
    assert _l2(pooled, g["f64/gp1_al0"][0]) < BAR
