"""GPU: prompt_dropout in the prompt self-attention (train mode).

1. mt_token_mha_fwd_drop / _bwd_drop against float64 under the DEVICE's own mask (exported with mt_dropout_f32 over a flat row of ones:
   the same MtDropout, element index ((b heads + h) T + i) T + j), at test_token_mha's bar (1e-4 relative, fp32 throughout), at every
   head dim and at every T where the backward changes form -- with the keep-bit image in LDS the forms change at 126 | 127 (head dim 16),
   113 | 114 (32), 92 | 93 and 110 | 111 (64); the thresholds of the plain kernels (127 | 128, 114 | 115, 111 | 112) are kept as cases.
2. Properties of the mask.  3. Off means off: bit for bit the plain entries.
4. The train step of fixture model_L37_d3 with prompt_dropout = 0.25 (every other rate 0) against the float64 oracle with its
   prompt_self_attention replaced by tests/prompt_dropout_ref.py under the engine's own masks.  5. Engine invariants.  6. TITAN."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from modaltune_amd import synth  # noqa: E402
from modaltune_amd.config import GIGAPATH_JSON, GeneConfig, ModelConfig  # noqa: E402

import prompt_dropout_ref as R  # noqa: E402
from test_model_gpu import GRAD_TOL_NAMED, _rel  # noqa: E402

DEV = "cuda"
PD = 0.25


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from modaltune_amd import ops
    return ops


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _rng(seed, step=0):
    return torch.tensor([seed & 0x7FFFFFFF, (seed >> 31) & 0x7FFFFFFF, step, 0], dtype=torch.int32, device=DEV)


def _keep_mask(ops, rng, site, p, n):
    """The device's keep mask of the first n elements of an element-dropout site: mt_dropout_f32 over one flat row of ones."""
    D = R.flat_row_len(n)
    y = torch.empty(1, D, device=DEV)
    ops.dropout_f32(torch.ones(1, D, device=DEV), y, 1, D, ops.dropout_spec(rng, site, p))
    vals = torch.unique(y)
    assert all(float(v) == 0.0 or abs(float(v) - 1.0 / (1.0 - p)) < 1e-6 for v in vals), vals      # 0 or 1 / (1 - p), nothing else
    return (y[0, :n] != 0).cpu()


def _run(ops, q, k, v, do, heads, drop):
    B, T, E = q.shape
    out, probs = torch.zeros(B, T, E, device=DEV), torch.zeros(B, heads, T, T, device=DEV)
    dq, dk, dv = (torch.zeros(B, T, E, device=DEV) for _ in range(3))
    ops.token_mha_fwd(q, k, v, out, probs, B, T, E, heads, drop=drop)
    ops.token_mha_bwd(q, k, v, probs, do, dq, dk, dv, B, T, E, heads, drop=drop)
    torch.cuda.synchronize()
    return out, probs, dq, dk, dv


# ---------------------------------------------------------------- 1. kernels against float64 under the device's mask
SHAPES = [(12, 16, T) for T in (1, 5, 65, 126, 127, 128)] + [(6, 32, T) for T in (7, 113, 114, 115)] + \
         [(6, 64, T) for T in (7, 92, 93, 110, 111, 112)]


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("heads,hd,T", SHAPES)
def test_kernels_match_float64_under_the_devices_mask(heads, hd, T, p):
    ops = _gpu()
    B, E, site = 3, heads * hd, 400
    g = torch.Generator().manual_seed(1000 * hd + T)
    q, k, v, do = (torch.randn(B, T, E, generator=g) for _ in range(4))
    rng = _rng(77, step=3)
    keep = _keep_mask(ops, rng, site, p, B * heads * T * T).view(B, heads, T, T)
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    ref, P = R.attention_core(qd, kd, vd, heads, keep, p)
    ref.backward(do.double())
    dev = [t.to(DEV) for t in (q, k, v, do)]
    out, probs, dq, dk, dv = _run(ops, *dev, heads, ops.dropout_spec(rng, site, p))
    _, probs0, _, _, _ = _run(ops, *dev, heads, None)
    fig = dict(out=rel(out, ref), dq=rel(dq, qd.grad), dk=rel(dk, kd.grad), dv=rel(dv, vd.grad), probs=rel(probs, P))
    print(f"token drop {heads}x{hd} T={T} p={p}", {n: f"{x:.2e}" for n, x in fig.items()})
    assert max(fig.values()) < 1e-4, fig
    assert torch.equal(probs, probs0)          # the saved probabilities are the PRE-dropout softmax
    if T > 1:
        assert not torch.equal(out, _run(ops, *dev, heads, None)[0])


# ---------------------------------------------------------------- 2. the mask
def test_mask_properties_at_the_shipped_shape():
    ops = _gpu()
    B, heads, T, E, p, site = 3, 12, 65, 192, 0.1, 402
    g = torch.Generator().manual_seed(5)
    q, k, do = (torch.randn(B, T, E, generator=g).to(DEV) for _ in range(3))
    ones = torch.ones(B, T, E, device=DEV)
    rng = _rng(1234, step=7)
    spec = ops.dropout_spec(rng, site, p)
    out, probs, _, _, _ = _run(ops, q, k, ones, do, heads, spec)
    n = B * heads * T * T
    keep = _keep_mask(ops, rng, site, p, n).view(B, heads, T, T)
    # all-ones V: out[b, i, h * 16 + d] = row sum of P~[b, h, i, :] for every d
    rows = (probs.double().cpu() * keep / (1.0 - p)).sum(-1)                   # [B, heads, T]
    got = out.view(B, T, heads, 16).permute(0, 2, 1, 3).double().cpu()
    assert float((got - rows.unsqueeze(-1)).abs().max()) < 1e-5
    frac = float(keep.double().mean())
    sigma = math.sqrt(p * (1 - p) / n)
    print("kept fraction", frac, "sigma", sigma)
    assert n == 152100 and abs(frac - (1 - p)) < 4 * sigma
    # same (seed, step, site): the same bits; another step (mt_rng_advance) or another site: another mask
    out2 = _run(ops, q, k, ones, do, heads, spec)[0]
    assert torch.equal(out, out2)
    out_site = _run(ops, q, k, ones, do, heads, ops.dropout_spec(rng, site + 2, p))[0]
    ops.rng_advance(rng)
    out_step = _run(ops, q, k, ones, do, heads, spec)[0]
    assert int(rng[2]) == 8 and not torch.equal(out_step, out) and not torch.equal(out_site, out) and not torch.equal(out_site, out_step)


def test_backward_uses_the_forwards_mask_dv_of_a_dropped_entry_is_exactly_zero():
    ops = _gpu()
    B, heads, T, E, p, site = 3, 12, 65, 192, 0.1, 404
    g = torch.Generator().manual_seed(6)
    q, k, v = (torch.randn(B, T, E, generator=g).to(DEV) for _ in range(3))
    rng = _rng(99, step=1)
    keep = _keep_mask(ops, rng, site, p, B * heads * T * T).view(B, heads, T, T)
    b, h = 1, 7
    i, j = [int(t) for t in torch.nonzero(~keep[b, h])[3]]                       # a dropped (i, j) ...
    i2 = int(torch.nonzero(keep[b, h, :, j])[0])                                  # ... and a kept entry of the same column
    for row, dropped in ((i, True), (i2, False)):
        do = torch.zeros(B, T, E, device=DEV)
        do[b, row, h * 16:(h + 1) * 16] = 1.0                                     # one-hot dA: dV[j] = P~[row, j] dA[row]
        _, probs, _, _, dv = _run(ops, q, k, v, do, heads, ops.dropout_spec(rng, site, p))
        got = dv[b, j, h * 16:(h + 1) * 16]
        if dropped:
            assert float(got.abs().max()) == 0.0
        else:
            want = float(probs[b, h, row, j]) / (1.0 - p)
            assert float((got - want).abs().max()) < 1e-6 * max(want, 1e-30) + 1e-12 and want > 0


# ---------------------------------------------------------------- 3. off means off
@pytest.mark.parametrize("T", [65, 128])
def test_off_is_the_plain_entry_bit_for_bit(T):
    ops = _gpu()
    from modaltune_amd import _lib
    lib, p_, s_ = _lib.load(), ops._p, ops._s
    B, heads, E = 3, 12, 192
    g = torch.Generator().manual_seed(T)
    q, k, v, do = (torch.randn(B, T, E, generator=g).to(DEV) for _ in range(4))
    plain = _run(ops, q, k, v, do, heads, None)
    rng = _rng(3, step=2)
    null_rng = ops.dropout_spec(rng, 400, 0.3)
    null_rng.rng = None
    for what, spec in (("p = 0", ops.dropout_spec(rng, 400, 0.0)), ("null rng", null_rng)):
        got = _run(ops, q, k, v, do, heads, spec)
        for a, b2 in zip(got, plain):
            assert torch.equal(a, b2), what
    # drop == NULL through the new entries themselves
    out, probs = torch.zeros(B, T, E, device=DEV), torch.zeros(B, heads, T, T, device=DEV)
    dq, dk, dv = (torch.zeros(B, T, E, device=DEV) for _ in range(3))
    assert lib.mt_token_mha_fwd_drop(p_(q), p_(k), p_(v), B, T, E, heads, p_(out), p_(probs), None, s_()) == 0
    assert lib.mt_token_mha_bwd_drop(p_(q), p_(k), p_(v), p_(probs), p_(do), B, T, E, heads, p_(dq), p_(dk), p_(dv), None, s_()) == 0
    torch.cuda.synchronize()
    for a, b2 in zip((out, probs, dq, dk, dv), plain):
        assert torch.equal(a, b2)
    # refused: p outside [0, 1), DropPath at this site, a head dim that is none of 16 / 32 / 64
    for bad in (ops.dropout_spec(rng, 400, 1.0), ops.dropout_spec(rng, 400, -0.1), ops.dropout_spec(rng, 400, float("nan")),
                ops.dropout_spec(rng, 400, 0.1, 401, 0.1)):
        with pytest.raises(RuntimeError, match="bad argument"):
            ops.token_mha_fwd(q, k, v, out, probs, B, T, E, heads, drop=bad)
        with pytest.raises(RuntimeError, match="bad argument"):
            ops.token_mha_bwd(q, k, v, probs, do, dq, dk, dv, B, T, E, heads, drop=bad)
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.token_mha_fwd(q, k, v, out, torch.zeros(B, 4, T, T, device=DEV), B, T, E, 4, drop=ops.dropout_spec(rng, 400, 0.1))      # head dim 48


# ---------------------------------------------------------------- 4. / 5. the engine
def _cfg(g, pd, **kw):
    base = dict(depth=int(g["depth"]), interaction_indexes=tuple(tuple(int(i) for i in p) for p in g["inter"]), slide_ngrids=int(g["ngrids"]),
                dropout=0.0, drop_path_rate=0.0, gene=GeneConfig(dropout=0.0))
    if pd is not None:
        base["prompt_dropout"] = pd
    base.update(kw)
    return ModelConfig(**base)


def _rig(golden_dir, pd, deterministic=None, name="model_L37_d3", **ts_kw):
    from modaltune_amd.engine import Engine
    from modaltune_amd.trainer import TrainStep
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    cfg = _cfg(g, pd)
    cfg.validate()
    sizes, seed = [int(s) for s in g["sizes"]], int(g["seed"])
    eng = Engine(cfg, sizes, DEV, deterministic=deterministic)
    sd = synth.synth_state_dict(cfg, sizes, seed)
    eng.load_state_dict(sd)
    ts = TrainStep(eng, split_passes=False, **ts_kw)          # the batched pass, B = 3
    ts.set_projector(synth.projector_state(seed))
    inp = synth.synth_inputs(int(g["L"]), sizes, seed, grid=int(g["ngrids"]))
    x = torch.from_numpy(inp["x"]).cuda()
    genes = [torch.from_numpy(a).cuda() for a in inp["genes"]]
    return dict(g=g, cfg=cfg, sizes=sizes, seed=seed, eng=eng, ts=ts, inp=inp, x=x, genes=genes, text=torch.from_numpy(inp["text"]).cuda(), sd=sd)


def _step(r, step_no=None, graphed=False, update=False):
    if step_no is not None:
        r["eng"].rng[2] = step_no - 1          # (the step advances the counter first)
    ts = r["ts"]
    if graphed:
        ts.step_graphed(r["x"], r["inp"]["coords"], r["genes"], r["text"])
    else:
        ts.step(r["x"], r["inp"]["coords"], r["genes"], r["text"], update=update)
    torch.cuda.synchronize()
    return ts.loss.clone()


def test_train_step_matches_the_float64_oracle_under_the_engines_masks(golden_dir, monkeypatch):
    ops = _gpu()
    from modaltune_amd.config import segment_lengths
    from oracle import modaltune_oracle as O
    r = _rig(golden_dir, PD)
    eng, ts, cfg = r["eng"], r["ts"], r["cfg"]
    eng.set_stochastic(True, seed=4321)
    loss = _step(r, step_no=5)
    assert int(eng.rng[2]) == 5 and int(ts.found_inf) == 0
    logits = ts.last_logits.cpu().numpy()
    grads = ts.unscaled_grads()
    # the masks of every (site, pass): sites 400 + 2 i (probabilities, [B, heads, T, T]) and 401 + 2 i (residual, [B T, D]), i = 1, 2
    B, T, D, heads = 3, eng.T, cfg.embed_dim, cfg.num_heads
    nint = len(cfg.interaction_indexes)
    keep1 = {i: _keep_mask(ops, eng.rng, 400 + 2 * i, PD, B * heads * T * T).view(B, heads, T, T) for i in range(1, nint)}
    keep2 = {i: _keep_mask(ops, eng.rng, 401 + 2 * i, PD, B * T * D).view(B, T, D) for i in range(1, nint)}
    calls = []

    def masked(c, pe, sd, prefix, heads_):          # the oracle runs task pass by task pass: call n is (pass n // (nint - 1), layer of the prefix)
        n = len(calls)
        task, i = n // (nint - 1), int(prefix.rsplit(".", 1)[1])
        calls.append((task, i))
        assert c.shape[0] == 1 and i == 1 + n % (nint - 1)
        return R.prompt_self_attention_masked(c, pe, sd, prefix, heads_, keep1[i][task:task + 1], keep2[i][task:task + 1], PD)
    monkeypatch.setattr(O, "prompt_self_attention", masked)
    F64 = torch.float64
    sd = {k: torch.from_numpy(v).to(F64) for k, v in r["sd"].items()}
    psd = {k: torch.from_numpy(v).to(F64) for k, v in synth.projector_state(r["seed"]).items()}
    inp = r["inp"]
    ref_logits, ref_loss, ref_grads = O.train_step_loss_and_grads(
        sd, cfg, synth.trainable_keys(cfg, r["sizes"]), torch.from_numpy(inp["x"]).to(F64), torch.from_numpy(inp["coords"]).to(F64),
        [torch.from_numpy(a).to(F64) for a in inp["genes"]], torch.from_numpy(inp["text"]).to(F64), psd, segment_lengths())
    assert calls == [(t, i) for t in range(B) for i in range(1, nint)]
    fig = dict(logits=_rel(logits, ref_logits.numpy()), loss=abs(float(loss) - float(ref_loss)) / abs(float(ref_loss)),
               masks_matter=_rel(r["g"]["f64_logits"], ref_logits.numpy()))
    names = list(ref_grads)
    ours = np.array([float(grads[n].double().norm()) for n in names])
    ref = np.array([float(ref_grads[n].norm()) for n in names])
    fig["grad_norm_worst"] = float(np.max(np.abs(ours - ref) / (ref + 1e-6 * ref.max())))
    print("prompt_dropout engine step", {k: f"{v:.2e}" for k, v in fig.items()})
    assert fig["masks_matter"] > 4e-3                     # (ten times the logits bar: the p = 0 golden is another model output)
    assert fig["logits"] < 4e-4, fig
    assert fig["loss"] < 2e-4, fig
    bad = [(n, o, rr) for n, o, rr in zip(names, ours, ref) if abs(o - rr) > GRAD_TOL_NAMED.get(n, 1e-2) * rr + 1e-6 * ref.max()]
    assert not bad, bad[:10]


def test_zero_rate_is_the_model_without_the_key_and_eval_draws_no_mask(golden_dir):
    _gpu()
    ra, rb, rc = _rig(golden_dir, None, deterministic=True), _rig(golden_dir, 0.0, deterministic=True), _rig(golden_dir, PD, deterministic=True)
    for r in (ra, rb, rc):
        r["eng"].set_stochastic(True, seed=11)
    la, lb, lc = _step(ra, 3), _step(rb, 3), _step(rc, 3)
    assert torch.equal(la, lb) and torch.equal(ra["eng"].store.flat_grad, rb["eng"].store.flat_grad)
    assert not torch.equal(la, lc)
    oh = torch.eye(3, device=DEV)
    with torch.no_grad():
        ev = [r["eng"].forward(r["x"], r["inp"]["coords"], r["genes"], oh, need_grad=False).clone() for r in (rb, rc)]
    assert torch.equal(ev[0], ev[1])


def test_deterministic_mode_same_seed_same_bits_eager_and_graphed(golden_dir):
    """Two engines from scratch, same seed: five optimiser steps eagerly on one, through step_graphed (two eager warm-ups, the capture,
    replays) on the other -- the same loss bits at every counter value, the same weights at the end; consecutive replays draw fresh masks;
    and a third engine repeats the eager run bit for bit."""
    _gpu()
    runs = []
    for graphed in (False, True, False):
        r = _rig(golden_dir, PD, deterministic=True)
        r["eng"].set_stochastic(True, seed=2024)
        losses = [(_step(r, graphed=True) if graphed else _step(r, update=True)) for _ in range(5)]
        if graphed:
            assert r["ts"].graph_replays >= 2
        assert int(r["eng"].rng[2]) == 5
        runs.append((torch.cat(losses), r["eng"].store.flat.clone()))
    (le, we), (lg, wg), (le2, we2) = runs
    assert bool(torch.isfinite(le).all())
    assert torch.equal(le, le2) and torch.equal(we, we2)          # same seed, inputs, schedule: same bits
    assert torch.equal(le, lg) and torch.equal(we, wg)            # eager and replayed steps at the same counter
    assert float(lg[3]) != float(lg[4])                           # two consecutive replays: fresh masks


def test_replays_draw_fresh_masks_with_frozen_weights(golden_dir):
    """lr = 0: nothing but the device's Philox counter moves between the steps, so different losses ARE different masks; the eager step at
    a replay's counter value gives the replay's loss bits."""
    _gpu()
    r = _rig(golden_dir, PD, deterministic=True, lr=0.0, weight_decay=0.0)
    r["eng"].set_stochastic(True, seed=5)
    w0 = r["eng"].store.flat.clone()
    losses = [_step(r, graphed=True) for _ in range(5)]
    assert r["ts"].graph_replays >= 2 and torch.equal(r["eng"].store.flat, w0)
    assert float(losses[3]) != float(losses[4])
    assert torch.equal(_step(r, step_no=5), losses[4]) and torch.equal(_step(r, step_no=4), losses[3])


def test_forward_only_paths_draw_no_mask(golden_dir):
    """EmbeddingExtractor, attention maps and Integrated Gradients: torch-equal to the p = 0 model's, with the engine in train mode."""
    _gpu()
    from modaltune_amd.attribution import IntegratedGradients
    from modaltune_amd.config import attention_sites
    from modaltune_amd.evaluate import EmbeddingExtractor
    r0, r1 = _rig(golden_dir, 0.0, deterministic=True), _rig(golden_dir, PD, deterministic=True)
    outs = []
    for r in (r0, r1):
        eng = r["eng"]
        eng.set_stochastic(True, seed=8)
        _step(r, 2)                                                        # (a train step first: the mode is live)
        emb = EmbeddingExtractor(eng, graphed=False)(r["x"], r["inp"]["coords"], r["genes"]).clone()
        L = int(r["g"]["L"])
        maps = eng.new_attention_maps(attention_sites(r["cfg"]), 3, L)
        with torch.no_grad():
            lg = eng.forward(r["x"], r["inp"]["coords"], r["genes"], torch.eye(3, device=DEV), need_grad=False, attn_maps=maps).clone()
        ig = IntegratedGradients(eng, steps=4)(r["x"], r["inp"]["coords"], r["genes"], torch.ones(r["cfg"].output_dim))
        torch.cuda.synchronize()
        outs.append((emb, lg, {k: v.clone() for k, v in maps.items()}, ig["attributions"].clone(), ig["pathway"].clone()))
    a, b = outs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])
    assert any(k.startswith("prompt_selfattention.") for k in a[2])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


def test_accumulation_window_and_pass_groups_run_and_repeat(golden_dir):
    """TrainStep(accumulate=2): one window (a micro-step and the boundary) twice from the same seed; and the step as two pass groups
    (site groups 1 and 2: masks of their own) twice at the same counter.  Deterministic mode: torch.equal."""
    _gpu()
    seen = []
    for _ in range(2):
        r = _rig(golden_dir, PD, deterministic=True, accumulate=2)
        r["eng"].set_stochastic(True, seed=31)
        l1, l2 = _step(r, update=True), _step(r, update=True)
        assert int(r["ts"].step_dev) == 1 and float(l1) != float(l2) and bool(torch.isfinite(r["eng"].store.flat).all())
        seen.append((l1, l2, r["eng"].store.flat.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*seen))
    r = _rig(golden_dir, PD, deterministic=True)
    r["eng"].set_stochastic(True, seed=31)
    batched = _step(r, 4)
    r["ts"].split_passes, r["ts"].split_min_patches = True, 0
    assert r["ts"]._split_now(int(r["g"]["L"]))
    g1 = _step(r, 4)
    grad1 = r["eng"].store.flat_grad.clone()
    g2 = _step(r, 4)
    assert torch.equal(g1, g2) and torch.equal(grad1, r["eng"].store.flat_grad) and bool(torch.isfinite(g1).all())
    assert not torch.equal(g1, batched)                 # the groups' sites are offset: other masks than the batched pass's


def test_module_api_trains_with_prompt_dropout_and_replays_draw_fresh_masks():
    _gpu()
    from modaltune_amd.aggregators import Aggregator
    sizes = synth.toy_group_sizes()
    groups = {i: ["g"] * n for i, n in enumerate(sizes)}
    inp = synth.synth_inputs(120, sizes, 3, grid=32)
    x, coords = torch.from_numpy(inp["x"]).cuda(), torch.from_numpy(inp["coords"]).cuda()
    genes = {i: torch.from_numpy(a).cuda() for i, a in enumerate(inp["genes"])}
    eye = torch.eye(3).cuda()
    runs = []
    for _ in range(2):
        model = Aggregator.create("longnetvit_gene_adapter", gene_group_defination=groups, multi_task=3, init_seed=0, deterministic=True,
                                  **dict(GIGAPATH_JSON, depth=3, slide_ngrids=32, interaction_indexes=[[0, 0], [1, 1], [2, 2]], pretrained=False,
                                         dropout=0.0, drop_path_rate=0.0, prompt_dropout=PD))
        model.cfg.gene.dropout = model.engine.cfg.gene.dropout = 0.0          # the prompt sites are the only stochastic ones
        model.eval()
        assert not model.engine.stochastic
        model.train()
        assert model.engine.stochastic
        outs = []
        for _ in range(8):
            xs = x.clone()                       # (a new slide tensor per step, as a loader hands them over)
            ys = torch.cat([model(x=xs, coords=coords, genes=genes, clinical=[], task_token=eye[t]) for t in (0, 1, 2)])
            ys.square().sum().backward()
            gn = torch.cat([q.grad.reshape(-1) for q in model.parameters() if q.grad is not None])
            assert bool(torch.isfinite(ys).all()) and bool(torch.isfinite(gn).all()) and float(gn.norm()) > 0
            for q in model.parameters():
                q.grad = None
            outs.append(ys.detach().clone())
        assert model._replay.replays >= 2
        assert not torch.equal(outs[-1], outs[-2]) and not torch.equal(outs[-2], outs[-3])      # replays: fresh masks each
        runs.append(torch.stack(outs))
        del model
    assert torch.equal(runs[0], runs[1])          # reproducible: the same model, the same calls, the same bits


# ---------------------------------------------------------------- 6. TITAN
def test_titan_train_step_runs_and_repeats_from_the_seed(golden_dir):
    """The TITAN engine shares Engine._prompt_self_attention.  Its forward sums the feature grid with fp32 atomics, so "the same" is not
    bitwise there: the same (seed, counter) repeats the loss to 1e-5 relative -- atomic-order noise is ~1e-7 per sum --, while other masks
    (p = 0.25 on the probabilities and the residual of two layers) move it by far more than that."""
    _gpu()
    import titan_standin
    from modaltune_amd.titan import NativeBackbone, TitanEngine, titan_model_config
    from modaltune_amd.trainer import TrainStep
    from test_titan_cpu import TITAN_JSON, _case
    g, _, sizes, inp, seed, clinical = _case(golden_dir, "titan_L300")
    assert not clinical
    vit = titan_standin.VisionTransformer()
    titan_standin.init_standin(vit, seed)
    cfg = titan_model_config(dict(TITAN_JSON, prompt_dropout=PD), 3, False, depth=6)
    assert cfg.prompt_dropout == PD
    eng = TitanEngine(cfg, sizes, NativeBackbone(vit, DEV), DEV)
    eng.load_state_dict(synth.synth_state_dict(cfg, sizes, seed))
    ts = TrainStep(eng)
    ts.set_projector(synth.projector_state(seed))
    L = int(g["L"])
    x, coords = torch.from_numpy(inp["x"]).cuda().reshape(L, -1), torch.from_numpy(inp["coords"]).cuda().reshape(L, 2)
    genes, text = [torch.from_numpy(a).cuda() for a in inp["genes"]], torch.from_numpy(inp["text"]).cuda()
    base = float(ts.step(x, coords, genes, text, update=False))          # eval-like: the engine's stochastic mode is off
    eng.set_stochastic(True, seed=77)

    def run(step_no):
        eng.rng[2] = step_no - 1
        v = float(ts.step(x, coords, genes, text, update=False))
        torch.cuda.synchronize()
        assert int(ts.found_inf) == 0 and bool(torch.isfinite(eng.store.flat_grad).all()) and float(eng.store.flat_grad.abs().max()) > 0
        return v
    l3, l3b, l4 = run(3), run(3), run(4)
    print("titan prompt_dropout losses", base, l3, l3b, l4)
    assert np.isfinite([l3, l3b, l4]).all()
    assert abs(l3 - l3b) <= 1e-5 * abs(l3)
    assert abs(l3 - l4) > 1e-4 * abs(l3) and abs(l3 - base) > 1e-4 * abs(base)
