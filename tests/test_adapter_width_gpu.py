"""GPU: the Modal-Adapter at widths other than the shipped 12 heads x 16 (`cffn_ratio`, `num_heads`: head dims 16 / 32 / 64 with a
run-time head count).

Kernels against the float64 reference of tests/test_kernels_gpu.py with the bars those tests carry at 12 x 16; the width-aware entry
points against their fixed-width twins at 12 x 16 (same bits); the attention-map kernels against a float64 recomputation; the train
step, the attention maps, the schedules (graph replay, pass groups, the drop-in module) and the TITAN engine against reference goldens
generated at 6 x 64, 6 x 32, 24 x 16 and 9 x 64 (tests/golden/make_golden_adapter_width.py)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from modaltune_amd import _lib, ops, synth  # noqa: E402
from modaltune_amd.config import GIGAPATH_JSON, ModelConfig, attention_sites  # noqa: E402

from test_kernels_gpu import _mha_ref, rel, rng  # noqa: E402
from test_model_gpu import GRAD_TOL_NAMED, _build, _rel  # noqa: E402

DEV = "cuda"
# (E, heads): head dims 16, 32, 64 at E = 192 and 384, and the widest supported adapter, 9 x 64
PAIRS = [(192, 12), (192, 6), (192, 3), (384, 24), (384, 12), (384, 6), (576, 9)]
WIDTH_TAGS = ["h6x64", "h6x32", "h24x16", "h9x64"]
INTER = [[0, 0], [1, 1], [2, 2]]


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ---------------------------------------------------------------- 4. kernels against float64
@pytest.mark.parametrize("T,L", [(65, 301), (7, 301), (66, 1100), (33, 513)])
@pytest.mark.parametrize("E,heads", PAIRS)
def test_inject_attention_at_width(E, heads, T, L):
    """tests/test_kernels_gpu.py::test_inject_attention at (E, heads), its bars unchanged."""
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
    a = torch.zeros(B * L, E, dtype=torch.float16, device=DEV)
    alse = torch.zeros(B * L, heads, device=DEV)
    ops.inject_attn_fwd(q.to(DEV), k.to(DEV), v.to(DEV), a, B * L, L, T, lse=alse, heads=heads, head_dim=hd)
    dq = torch.zeros(B * L, E, dtype=torch.float16, device=DEV)
    dk = torch.zeros(B, T, E, device=DEV)
    dv = torch.zeros(B, T, E, device=DEV)
    ops.inject_attn_bwd(q.to(DEV), a, alse, da.to(DEV), k.to(DEV), v.to(DEV), dq, dk, dv, B * L, L, T, heads=heads, head_dim=hd)
    torch.cuda.synchronize()
    fig = dict(a=rel(a.view(B, L, E), ref), dq=rel(dq.view(B, L, E), qd.grad), dk=rel(dk, kd.grad), dv=rel(dv, vd.grad))
    print(f"inject {heads}x{hd} T={T} L={L}", {n: f"{x:.2e}" for n, x in fig.items()})
    assert fig["a"] < 2e-3, fig
    assert fig["dq"] < 3e-3, fig
    assert fig["dk"] < 1e-3 and fig["dv"] < 1e-3, fig


@pytest.mark.parametrize("T,L,nsplit", [(65, 700, 4), (7, 129, 1), (66, 1000, 16)])
@pytest.mark.parametrize("E,heads", PAIRS)
def test_extract_attention_at_width(E, heads, T, L, nsplit):
    """tests/test_kernels_gpu.py::test_extract_attention at (E, heads), its bars unchanged."""
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
    out = torch.zeros(B, T, E, device=DEV)
    lse = torch.zeros(B, T, heads, device=DEV)
    pa = torch.zeros(B * heads * nsplit * T * hd, device=DEV)
    pm = torch.zeros(B * heads * nsplit * T * 2, device=DEV)
    ops.extract_attn_fwd(q.to(DEV), kv.to(DEV), out, lse, pa, pm, B, T, L, nsplit, heads=heads, head_dim=hd)
    dq = torch.zeros(B, T, E, device=DEV)
    dkv = torch.zeros(B * L, 2 * E, dtype=torch.float16, device=DEV)
    ops.extract_attn_bwd(q.to(DEV), kv.to(DEV), out, lse, dout.to(DEV), dq, dkv, B, T, L, heads=heads, head_dim=hd)
    torch.cuda.synchronize()
    fig = dict(out=rel(out, ref), dq=rel(dq, qd.grad), dkv=rel(dkv.view(B, L, 2 * E), kvd.grad))
    print(f"extract {heads}x{hd} T={T} L={L}", {n: f"{x:.2e}" for n, x in fig.items()})
    assert fig["out"] < 1.5e-3, fig
    assert fig["dq"] < 3e-3, fig
    assert fig["dkv"] < 3e-3, fig


@pytest.mark.parametrize("T", [65, 7, 64, 127, 128, 1])
@pytest.mark.parametrize("E,heads", PAIRS)
def test_token_mha_at_width(E, heads, T):
    """tests/test_kernels_gpu.py::test_token_mha at (E, heads): fp32 throughout, 1e-4 (T = 127 / 128 reach the backward's forms
    that read P -- and at head dim 64 Q and K -- from global memory)."""
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
    torch.cuda.synchronize()
    fig = dict(out=rel(out, ref), dq=rel(dq, qd.grad), dk=rel(dk, kd.grad), dv=rel(dv, vd.grad))
    print(f"token {heads}x{E // heads} T={T}", {n: f"{x:.2e}" for n, x in fig.items()})
    assert max(fig.values()) < 1e-4, fig
    assert float((probs.double().sum(-1) - 1).abs().max()) < 1e-5


def test_unsupported_head_dims_are_refused():
    _gpu()
    B, T, E = 1, 4, 96
    q, k, v, out = (torch.zeros(B, T, E, device=DEV) for _ in range(4))
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.token_mha_fwd(q, k, v, out, torch.zeros(B, 2, T, T, device=DEV), B, T, E, 2)          # head dim 48
    a = torch.zeros(8, E, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.inject_attn_fwd(a, k, v, torch.zeros_like(a), 8, 8, T, lse=torch.zeros(8, 2, device=DEV), heads=2, head_dim=48)


# ---------------------------------------------------------------- 5. same bits at the shipped width; maps at the new ones
def _close(a, b, tol):
    return float((a.double() - b.double()).abs().max()) <= tol * float(b.double().abs().max())


def test_width_aware_entry_points_equal_their_twins_at_12x16():
    """Every `_hd` entry point at (12, 16) against the entry point that takes no width: forward outputs and the backward outputs
    written without atomics bit for bit, the atomically accumulated dk / dv / dq to 1e-6 relative."""
    _gpu()
    lib, p, s = _lib.load(), ops._p, ops._s
    E, H, D, B, T, L = 192, 12, 16, 3, 65, 700
    g = torch.Generator(device=DEV).manual_seed(5)
    M = B * L
    # injector
    q = torch.randn(M, E, device=DEV, generator=g).half()
    k, v = torch.randn(B, T, E, device=DEV, generator=g), torch.randn(B, T, E, device=DEV, generator=g)
    da = torch.randn(M, E, device=DEV, generator=g).half()
    res = []
    for hd in (False, True):
        a, lse = torch.zeros(M, E, dtype=torch.float16, device=DEV), torch.zeros(M, H, device=DEV)
        dq, dk, dv = torch.zeros_like(a), torch.zeros_like(k), torch.zeros_like(v)
        w = torch.zeros(M, T, device=DEV)
        if hd:
            _lib.check(lib.mt_inject_attn_fwd_hd(p(q), M, L, p(k), p(v), T, H, D, p(a), p(lse), s()))
            _lib.check(lib.mt_inject_attn_bwd_hd(p(q), p(a), p(lse), p(da), M, L, p(k), p(v), T, H, D, p(dq), p(dk), p(dv), None, s()))
            _lib.check(lib.mt_inject_attn_probs_hd(p(q), M, L, p(k), p(lse), T, H, D, p(w), s()))
        else:
            _lib.check(lib.mt_inject_attn_fwd(p(q), M, L, p(k), p(v), T, p(a), p(lse), s()))
            _lib.check(lib.mt_inject_attn_bwd(p(q), p(a), p(lse), p(da), M, L, p(k), p(v), T, p(dq), p(dk), p(dv), s()))
            _lib.check(lib.mt_inject_attn_probs(p(q), M, L, p(k), p(lse), T, p(w), s()))
        res.append((a, lse, dq, w, dk, dv))
    torch.cuda.synchronize()
    for x, y in zip(res[0][:4], res[1][:4]):
        assert torch.equal(x, y)
    for x, y in zip(res[0][4:], res[1][4:]):
        assert _close(x, y, 1e-6)
    # extractor
    q = torch.randn(B, T, E, device=DEV, generator=g)
    kv = torch.randn(M, 2 * E, device=DEV, generator=g).half()
    dout = torch.randn(B, T, E, device=DEV, generator=g)
    nsplit = 4
    res = []
    for hd in (False, True):
        out, lse = torch.zeros(B, T, E, device=DEV), torch.zeros(B, T, H, device=DEV)
        pa, pm = torch.zeros(B * H * nsplit * T * D, device=DEV), torch.zeros(B * H * nsplit * T * 2, device=DEV)
        dq, dkv = torch.zeros(B, T, E, device=DEV), torch.zeros(M, 2 * E, dtype=torch.float16, device=DEV)
        w = torch.zeros(B, T, L, device=DEV)
        if hd:
            _lib.check(lib.mt_extract_attn_fwd_hd(p(q), p(kv), B, T, L, H, D, p(out), p(lse), p(pa), p(pm), nsplit, s()))
            _lib.check(lib.mt_extract_attn_bwd_hd(p(q), p(kv), p(out), p(lse), p(dout), B, T, L, H, D, p(dq), p(dkv), None, s()))
            _lib.check(lib.mt_extract_attn_probs_hd(p(q), p(kv), p(lse), B, T, L, H, D, p(w), s()))
        else:
            _lib.check(lib.mt_extract_attn_fwd(p(q), p(kv), B, T, L, p(out), p(lse), p(pa), p(pm), nsplit, s()))
            _lib.check(lib.mt_extract_attn_bwd(p(q), p(kv), p(out), p(lse), p(dout), B, T, L, p(dq), p(dkv), s()))
            _lib.check(lib.mt_extract_attn_probs(p(q), p(kv), p(lse), B, T, L, p(w), s()))
        res.append((out, lse, dkv, w, pa, pm, dq))
    torch.cuda.synchronize()
    for x, y in zip(res[0][:6], res[1][:6]):
        assert torch.equal(x, y)
    assert _close(res[0][6], res[1][6], 1e-6)


@pytest.mark.parametrize("L", [37, 1500])
@pytest.mark.parametrize("T", [7, 65, 128])
@pytest.mark.parametrize("E,heads", PAIRS)
def test_maps_match_f64_recomputation_at_width(E, heads, T, L):
    """tests/test_attn_maps_gpu.py::test_extract_and_inject_maps_match_f64_recomputation's form at (E, heads): 1e-5 on the map, rows
    sum to 1 within 1e-4 (24 x 16 and 9 x 64 at T = 128 run the kernels' head-group loop)."""
    _gpu()
    B, hd, dev = 3, E // heads, DEV
    scale = hd ** -0.5
    g = torch.Generator(device=dev).manual_seed(1000 * T + 10 * L + heads)
    q = torch.randn(B, T, E, device=dev, generator=g) * 2.0
    kv = (torch.randn(B * L, 2 * E, device=dev, generator=g) * 1.5).half()
    out, lse = torch.empty(B, T, E, device=dev), torch.empty(B, T, heads, device=dev)
    kps = -(-(-(-L // max(1, min(64, L // 256)))) // 64) * 64       # (the engine's split rule)
    nsplit = -(-L // kps)
    pa, pml = torch.empty(B * heads * nsplit * T * hd, device=dev), torch.empty(B * heads * nsplit * T * 2, device=dev)
    ops.extract_attn_fwd(q, kv, out, lse, pa, pml, B, T, L, nsplit, heads=heads, head_dim=hd)
    w = torch.full((B, T, L), float("nan"), device=dev)
    ops.extract_attn_probs(q, kv, lse, w, B, T, L, heads=heads, head_dim=hd)
    qh = (q * np.float32(scale)).half().double().view(B, T, heads, hd)       # (the kernels scale in fp32, then round to fp16)
    kh = kv[:, :E].double().view(B, L, heads, hd)
    s = torch.einsum("bthd,blhd->bthl", qh, kh)
    ref = torch.exp(s - lse.double()[..., None]).mean(dim=2)
    err = float((w.double() - ref).abs().max())
    assert err <= 1e-5, err
    assert float((w.double().sum(-1) - 1).abs().max()) <= 1e-4
    del s, ref
    M = B * L
    q2 = (torch.randn(M, E, device=dev, generator=g) * 2.0).half()
    k = torch.randn(B, T, E, device=dev, generator=g) * 1.5
    v = torch.randn(B, T, E, device=dev, generator=g)
    a, alse = torch.empty(M, E, dtype=torch.float16, device=dev), torch.empty(M, heads, device=dev)
    ops.inject_attn_fwd(q2, k, v, a, M, L, T, lse=alse, heads=heads, head_dim=hd)
    wi = torch.full((M, T), float("nan"), device=dev)
    ops.inject_attn_probs(q2, k, alse, wi, M, L, T, heads=heads, head_dim=hd)
    kh = k.half().double().view(B, T, heads, hd)
    s = torch.einsum("blhd,bthd->blht", q2.double().view(B, L, heads, hd), kh).reshape(M, heads, T)
    ref = torch.exp(float(np.float32(scale)) * s - alse.double()[..., None]).mean(dim=1)
    err = float((wi.double() - ref).abs().max())
    assert err <= 1e-5, err
    assert float((wi.double().sum(-1) - 1).abs().max()) <= 1e-4


def _tile_positions(n):
    """Where a row can sit in a launch of n rows: lane 0, the last row of the first wave tile, the first row of the second wave tile,
    the last row of the first workgroup, the first row of the second workgroup, the last row (the tail mask)."""
    return sorted({r for r in (0, 31, 32, 127, 128, n - 1) if r < n})


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


@pytest.mark.parametrize("T", [33, 65])
@pytest.mark.parametrize("E,heads", [(192, 12), (192, 6), (192, 3)])
def test_adapter_rows_do_not_depend_on_their_tile(E, heads, T):
    """A patch row's injector output, LSE and map row, and a key's column of the extractor map, are functions of the row's own operand
    and of the token-side LDS image only: the same row gives the same BITS as the only row of a launch and as row 0 / 31 / 32 / 127 /
    128 / last of launches of 127, 129 and 513 rows (every lane position, wave tile and workgroup, and the tail masks, of the shared
    accumulator-row, tile-store and staging helpers).  The reference is the 1-row launch.  Holds for the library before the kernels'
    stages were stated once as well (run there through MODALTUNE_HIP_LIB: 6 passed), no exception to record."""
    _gpu()
    hd = E // heads
    g = torch.Generator(device=DEV).manual_seed(100 * T + heads)
    k, v = torch.randn(1, T, E, device=DEV, generator=g), torch.randn(1, T, E, device=DEV, generator=g)
    qrow = torch.randn(E, device=DEV, generator=g).half()
    tq = torch.randn(1, T, E, device=DEV, generator=g)                           # the extractor's tokens, their lse fixed and passed in
    tlse = 3.0 + torch.rand(1, T, heads, device=DEV, generator=g)
    kvrow = torch.randn(2 * E, device=DEV, generator=g).half()
    ref = None
    for n in (1, 127, 129, 513):
        pos = _tile_positions(n)
        q = torch.randn(n, E, device=DEV, generator=g).half()
        kv = torch.randn(n, 2 * E, device=DEV, generator=g).half()
        q[pos], kv[pos] = qrow, kvrow
        a = torch.full((n, E), float("nan"), dtype=torch.float16, device=DEV)
        lse = torch.full((n, heads), float("nan"), device=DEV)
        wi = torch.full((n, T), float("nan"), device=DEV)
        we = torch.full((1, T, n), float("nan"), device=DEV)
        ops.inject_attn_fwd(q, k, v, a, n, n, T, lse=lse, heads=heads, head_dim=hd)
        ops.inject_attn_probs(q, k, lse, wi, n, n, T, heads=heads, head_dim=hd)
        ops.extract_attn_probs(tq, kv, tlse, we, 1, T, n, heads=heads, head_dim=hd)
        torch.cuda.synchronize()
        for t in (a, lse, wi, we):
            assert not bool(torch.isnan(t).any()), "an element was not written"
        if ref is None:
            ref = [_bits(x).clone() for x in (a[0], lse[0], wi[0], we[0, :, 0])]
        for r in pos:
            got = (a[r], lse[r], wi[r], we[0, :, r])
            for name, x, y in zip(("a", "lse", "inject map", "extract map"), got, ref):
                assert torch.equal(_bits(x), y), (name, n, r)


# ---------------------------------------------------------------- 6. train step against the reference goldens
@pytest.mark.parametrize("tag", WIDTH_TAGS)
def test_train_step_matches_reference_golden_at_width(golden_dir, tag):
    """tests/test_model_gpu.py::test_train_step_matches_reference_golden's form and bars (the fixture keeps two of the token taps)."""
    _gpu()
    g, cfg, eng, ts, inp = _build(os.path.join(golden_dir, f"model_L37_d3_{tag}.npz"))
    assert f"h{cfg.num_heads}x{cfg.adapter_head_dim}" == tag
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
    ours = np.array([float(grads[n].double().norm()) for n in names])
    ref = g["f64_grad_norms"]
    worst = sorted(((abs(o - r) / r, n) for n, o, r in zip(names, ours, ref) if r > 1e-6 * ref.max()), reverse=True)[:4]
    print(tag, "largest gradient-norm errors:", [(n, f"{e:.2e}") for e, n in worst])
    bad = [(n, o, r) for n, o, r in zip(names, ours, ref) if abs(o - r) > GRAD_TOL_NAMED.get(n, 1e-2) * r + 1e-6 * ref.max()]
    assert not bad, bad[:10]
    for k in g.files:
        if k.startswith("f64_grad/"):
            key = k[len("f64_grad/"):]
            err = np.linalg.norm(grads[key].double().cpu().numpy() - g[k]) / (np.linalg.norm(g[k]) + 1e-300)
            assert err < (3.5e-2 if key == "gene_encoder.pathway_compression.weight" else 1e-2), (k, err)


# ---------------------------------------------------------------- 7. attention maps against the reference goldens
def _engine(g):
    from modaltune_amd.engine import Engine
    sizes = [int(s) for s in g["sizes"]]
    cfg = ModelConfig(depth=int(g["depth"]), interaction_indexes=tuple(tuple(int(i) for i in p) for p in g["inter"]),
                      slide_ngrids=int(g["ngrids"]), clinical=bool(int(g["clinical"])), token_agg=str(g["token_agg"]),
                      multi_task=int(g["multi_task"]), **json.loads(str(g["extra_cfg"])))
    eng = Engine(cfg, sizes, "cuda")
    eng.load_state_dict(synth.synth_state_dict(cfg, sizes, int(g["seed"])))
    return cfg, eng, sizes


def _inputs(sizes, L, seed, ngrids):
    inp = synth.synth_inputs(L, sizes, seed, grid=ngrids)
    return (torch.from_numpy(inp["x"]).cuda(), torch.from_numpy(inp["coords"]).cuda(), [torch.from_numpy(a).cuda() for a in inp["genes"]],
            torch.from_numpy(inp["text"]))


@pytest.mark.parametrize("tag", WIDTH_TAGS)
def test_maps_match_reference_golden_at_width(golden_dir, tag):
    """tests/test_attn_maps_gpu.py::test_maps_match_reference_golden's bars: row-L1 <= 5e-3 per site, logits < 1e-3."""
    _gpu()
    from modaltune_amd.evaluate import EmbeddingExtractor
    g = np.load(os.path.join(golden_dir, f"attn_maps_L37_d3_{tag}.npz"))
    cfg, eng, sizes = _engine(g)
    L = int(g["L"])
    x, coords, genes, _ = _inputs(sizes, L, int(g["seed"]), int(g["ngrids"]))
    logits, maps = EmbeddingExtractor(eng, (0, 1, 2), graphed=False, attention=True)(x, coords, genes, None)
    torch.cuda.synchronize()
    assert sorted(maps) == sorted(attention_sites(cfg))
    r = float(np.abs(logits.cpu().numpy() - g["f64_logits"]).max() / np.abs(g["f64_logits"]).max())
    assert r < 1e-3, r
    T = cfg.num_tokens
    assert maps["interactions.0.injector.attn.multihead_attn"].shape == (3, L, T)
    assert maps["interactions.1.extractor.attn.multihead_attn"].shape == (3, T, L)
    assert maps["prompt_selfattention.2.self_attn"].shape == (3, T, T)
    report = {}
    for k in g.files:
        if k.startswith("map/"):
            ours = maps[k[4:]].cpu().numpy()
            assert ours.shape == g[k].shape, (k, ours.shape, g[k].shape)
            report[k] = float(np.abs(ours.astype(np.float64) - g[k].astype(np.float64)).sum(-1).max())
    print(tag, {k: f"{v:.1e}" for k, v in report.items()})
    assert len(report) == len(attention_sites(cfg))
    bad = {k: v for k, v in report.items() if v > 5e-3}
    assert not bad, bad


# ---------------------------------------------------------------- 8. schedules at 6 x 64
def test_graph_replay_matches_eager_at_6x64(golden_dir):
    """TrainStep.step_graphed in tests/test_model_gpu.py::test_graph_replay_matches_eager's form (training steps: the fp32-atomic
    weight-gradient reductions make two runs agree to rounding, hence that test's lr-scale tolerances), then with lr 0 the replayed
    forward against the eager one bit for bit; EmbeddingExtractor: eager == capture == replay bit for bit, maps included."""
    _gpu()
    from modaltune_amd.evaluate import EmbeddingExtractor
    path = os.path.join(golden_dir, "model_L37_d3_h6x64.npz")
    g, cfg, eng_a, ts_a, inp = _build(path)
    _, _, eng_b, ts_b, _ = _build(path)
    assert (cfg.adapter_dim, cfg.num_heads, cfg.adapter_head_dim) == (384, 6, 64)
    x = torch.from_numpy(inp["x"]).cuda()
    genes = [torch.from_numpy(a).cuda() for a in inp["genes"]]
    text = torch.from_numpy(inp["text"]).cuda()
    ex = EmbeddingExtractor(eng_a, (0, 1, 2), capture_after=1, attention=True)
    coords = torch.from_numpy(inp["coords"]).cuda()
    outs = [ex(x, coords, genes, None) for _ in range(3)]           # eager, capture, replay -- before any weight moves
    torch.cuda.synchronize()
    assert ex.graph_replays >= 1
    for lg, maps in outs[1:]:
        assert torch.equal(lg, outs[0][0])
        for s in maps:
            assert torch.equal(maps[s], outs[0][1][s]), s
    assert _rel(outs[0][0].cpu().numpy(), g["f64_logits"]) < 1e-3
    la, lb = [], []
    for i in range(5):
        la.append(float(ts_a.step(x, inp["coords"], genes, text, update=True)))
        lb.append(float(ts_b.step_graphed(x, inp["coords"], genes, text)))     # 2 eager warm-ups, capture, replays
    torch.cuda.synchronize()
    assert ts_b._graphs is not None
    assert int(ts_a.step_dev) == int(ts_b.step_dev) == 5
    assert np.allclose(la, lb, rtol=5e-4, atol=0), (la, lb)
    for k in ("interactions.0.injector.gamma", "final_project.weight", "gene_pe"):
        a, b = eng_a.store.tensors[k], eng_b.store.tensors[k]
        assert float((a - b).abs().max()) <= 2.5 * 5 * ts_a.lr, k
    # lr 0: the weights stay -- the replayed step's forward is the eager step's, bit for bit
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


def test_pass_groups_match_the_batched_step_at_6x64(golden_dir):
    """tests/test_model_gpu.py::test_pass_groups_on_two_streams_match_the_batched_step's form and tolerances."""
    _gpu()
    g, cfg, eng, ts, inp = _build(os.path.join(golden_dir, "model_L37_d3_h6x64.npz"))
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
    for k in g0:
        n = float(g0[k].norm())
        assert float((g0[k] - g1[k]).norm()) <= 2e-3 * n + 1e-7 * max(float(v.norm()) for v in g0.values()), k
    assert _rel(l1.cpu().numpy(), g["f64_logits"]) < 1e-3
    names = [str(n) for n in g["f64_grad_names"]]
    ours = np.array([float(g1[n].double().norm()) for n in names])
    ref = g["f64_grad_norms"]
    bad = [(n, o, r) for n, o, r in zip(names, ours, ref) if abs(o - r) > GRAD_TOL_NAMED.get(n, 1e-2) * r + 1e-6 * ref.max()]
    assert not bad, bad[:5]
    ts.set_lr(0.0); ts.wd = 0.0
    losses = []
    for _ in range(5):
        ts.step_graphed(x, inp["coords"], genes, text)
        torch.cuda.synchronize()
        losses.append(float(ts.loss))
    assert ts.graph_replays >= 2 and max(losses) - min(losses) <= 1e-6 * abs(loss0) and abs(losses[-1] - loss0) <= 1e-6 * abs(loss0)


def test_drop_in_module_reaches_replay_at_6x64(golden_dir):
    """The nn.Module bridge built from the constructor kwargs (cffn_ratio=0.5, num_heads=6): its forward / backward reach graph
    replay, and the replayed logits and loss match the reference golden."""
    _gpu()
    from modaltune_amd.aggregators import Aggregator
    from oracle import modaltune_oracle as O
    g = np.load(os.path.join(golden_dir, "model_L37_d3_h6x64.npz"))
    L, seed, ngrids = int(g["L"]), int(g["seed"]), int(g["ngrids"])
    sizes = [int(s) for s in g["sizes"]]
    groups = {i: ["g"] * n for i, n in enumerate(sizes)}
    model = Aggregator.create("longnetvit_gene_adapter", gene_group_defination=groups, multi_task=3,
                              **dict(GIGAPATH_JSON, depth=3, slide_ngrids=ngrids, interaction_indexes=INTER, pretrained=False,
                                     dropout=0.0, drop_path_rate=0.0, **json.loads(str(g["extra_cfg"]))))
    cfg = model.cfg
    assert (cfg.adapter_dim, cfg.num_heads) == (384, 6)
    sd = synth.synth_state_dict(cfg, sizes, seed)
    assert sd["interactions.0.injector.attn.multihead_attn.q_proj_weight"].shape == (384, 384)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    inp = synth.synth_inputs(L, sizes, seed, grid=ngrids)
    x, coords = torch.from_numpy(inp["x"]).cuda(), torch.from_numpy(inp["coords"]).cuda()
    genes = {i: torch.from_numpy(a).cuda() for i, a in enumerate(inp["genes"])}
    psd = {k: torch.from_numpy(v).cuda() for k, v in synth.projector_state(seed).items()}
    text = O.projector_forward(torch.from_numpy(inp["text"]).cuda(), psd)
    eye = torch.eye(3).cuda()
    model.train()
    assert not model.engine.stochastic
    for i in range(8):
        xs = x.clone()                           # (a new slide tensor per step, as a loader hands them over)
        logits = torch.cat([model(x=xs, coords=coords, genes=genes, clinical=[], task_token=eye[t]) for t in (0, 1, 2)])
        loss = O.distill_loss(logits, text)
        loss.backward()
        for p in model.parameters():
            p.grad = None
    torch.cuda.synchronize()
    assert model._replay.replays >= 1
    assert _rel(logits.detach().cpu().numpy(), g["f64_logits"]) < 1e-3
    assert abs(float(loss.detach()) - float(g["f64_loss"])) < 1e-3 * float(g["f64_loss"])


# ---------------------------------------------------------------- 9. TITAN engine at 6 x 32
@pytest.mark.parametrize("impl", ["native", "torch"])
def test_titan_train_step_matches_reference_golden_at_6x32(golden_dir, impl):
    """tests/test_titan_gpu.py::test_titan_adapter_train_step_matches_reference_golden's form and bars."""
    _gpu()
    import titan_standin
    from modaltune_amd.aggregators import Aggregator
    import modaltune_amd.titan  # noqa: F401
    from oracle import modaltune_oracle as O
    from test_titan_cpu import TITAN_JSON
    g = np.load(os.path.join(golden_dir, "model_titan_L300_h6x32.npz"))
    L, seed, grid = int(g["L"]), int(g["seed"]), int(g["grid"])
    sizes = [int(s) for s in g["sizes"]]
    inp = synth.synth_inputs_titan(L, sizes, seed, grid=grid)
    vit = titan_standin.VisionTransformer()
    titan_standin.init_standin(vit, seed)
    groups = {i: ["g"] * n for i, n in enumerate(sizes)}
    model = Aggregator.create("titan_gene_adapter", gene_group_defination=groups, **dict(TITAN_JSON, **json.loads(str(g["extra_cfg"]))),
                              multi_task=3, backbone=vit, backbone_impl=impl)
    assert (model.cfg.adapter_dim, model.cfg.num_heads, model.cfg.adapter_head_dim) == (192, 6, 32)
    sd = synth.synth_state_dict(model.cfg, sizes, seed)
    state = {k: torch.from_numpy(v) for k, v in sd.items() if k in dict(model._params)}
    state.update(vit.state_dict())
    model.load_state_dict(state, strict=True)
    x = torch.from_numpy(inp["x"]).cuda()
    coords = torch.from_numpy(inp["coords"]).cuda()
    genes = {i: torch.from_numpy(a).cuda() for i, a in enumerate(inp["genes"])}
    model.train()
    assert len([p for p in model.parameters() if p.requires_grad]) == len(g["f64_grad_names"])
    logits = torch.cat([model(x=x, coords=coords, genes=genes, task_token=torch.eye(3)[t].cuda()) for t in (0, 1, 2)], dim=0)
    assert _rel(logits.detach().cpu().numpy(), g["f64_logits"]) < 1e-3
    psd = {k: torch.from_numpy(v).cuda() for k, v in synth.projector_state(seed).items()}
    loss = O.distill_loss(logits, O.projector_forward(torch.from_numpy(inp["text"]).cuda(), psd))
    assert abs(float(loss.detach()) - float(g["f64_loss"])) < 1e-3 * float(g["f64_loss"])
    loss.backward()
    torch.cuda.synchronize()
    names = [str(n) for n in g["f64_grad_names"]]
    params = dict(model.named_parameters())
    ours = np.array([float(params[n].grad.double().norm()) for n in names])
    ref = g["f64_grad_norms"]
    bad = [(n, o, r) for n, o, r in zip(names, ours, ref) if abs(o - r) > 2e-2 * r + 1e-6 * ref.max()]
    assert not bad, bad[:10]
    for k in g.files:
        if k.startswith("f64_grad/"):
            ours_k = params[k[len("f64_grad/"):]].grad.double().cpu().numpy()
            err = np.linalg.norm(ours_k - g[k]) / (np.linalg.norm(g[k]) + 1e-300)
            assert err < 4e-2, (k, err)


# ---------------------------------------------------------------- 10. the torch ops
def test_torch_ops_take_the_head_count():
    _gpu()
    import modaltune_amd.torch_ops  # noqa: F401
    B, T, L, E, heads = 2, 65, 300, 384, 6
    g = torch.Generator(device=DEV).manual_seed(3)
    q = torch.randn(B * L, E, device=DEV, generator=g).half()
    k, v = torch.randn(B, T, E, device=DEV, generator=g), torch.randn(B, T, E, device=DEV, generator=g)
    a, lse = torch.ops.modaltune_hip.inject_attention_fwd(q, k, v, L, heads)
    am, lm = torch.ops.modaltune_hip.inject_attention_fwd(q.to("meta"), k.to("meta"), v.to("meta"), L, heads)
    assert a.shape == am.shape == (B * L, E) and lse.shape == lm.shape == (B * L, heads) and a.dtype == am.dtype and lse.dtype == lm.dtype
    ref = _mha_ref(q.double().view(B, L, E), k.double(), v.double(), heads)
    assert rel(a.view(B, L, E).cpu(), ref.cpu()) < 2e-3
    tq = torch.randn(B, T, E, device=DEV, generator=g)
    kv = torch.randn(B * L, 2 * E, device=DEV, generator=g).half()
    out, lse = torch.ops.modaltune_hip.extract_attention_fwd(tq, kv, L, heads)
    om, lm = torch.ops.modaltune_hip.extract_attention_fwd(tq.to("meta"), kv.to("meta"), L, heads)
    assert out.shape == om.shape == (B, T, E) and lse.shape == lm.shape == (B, T, heads)
    kvd = kv.double().view(B, L, 2 * E)
    assert rel(out.cpu(), _mha_ref(tq.double(), kvd[..., :E], kvd[..., E:], heads).cpu()) < 1.5e-3
    # the default is the shipped 12 heads
    q12 = torch.randn(B * L, 192, device=DEV, generator=g).half()
    k12 = torch.randn(B, T, 192, device=DEV, generator=g)
    assert torch.ops.modaltune_hip.inject_attention_fwd(q12, k12, k12, L)[1].shape == (B * L, 12)
    with pytest.raises(RuntimeError, match="heads of dim 16, 32 or 64"):
        torch.ops.modaltune_hip.inject_attention_fwd(q12, k12, k12, L, 4)
