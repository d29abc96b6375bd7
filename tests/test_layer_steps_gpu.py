"""The `steps` mask of the four composite launchers (mt_longnet_layer_fwd / _bwd, mt_vit_block_fwd / _bwd; csrc/layer.hip holds the
only launch list of a frozen backbone layer) and the timed pass that walks it (ops.TIMER: one single-step call per kernel).

1. At the C boundary: one call with MT_LAYER_ALL and the bits one call at a time, in order, from identical inputs leave every buffer
   bit-identical -- under both `pend` forms, defer, dh16_valid, feeds_lower and (LongNet) live dropout specs.  The lists hold no
   atomics (frozen weights: no dw / db), so exact equality is the bar.
2. The timed pass files every launch under the key the launch-by-launch Python schedule used: tests/golden/layer_step_keys.json was
   recorded with that schedule, before it was deleted (TIMER launch counts and the TIMELINE key sequence of one train step).
3. The timed step computes what the shipped step computes: logits and loss bit-identical, gradients within twice the spread of
   untimed repeats of the same seeded step (the control-to-control rule of test_overflow_gpu.py; zero spread -> bit-identical)."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from modaltune_amd import synth  # noqa: E402
from modaltune_amd.config import DILATED_RATIOS, ModelConfig, branch_table  # noqa: E402

KEYS_JSON = "layer_step_keys.json"
CONTROLS = 5       # untimed repeats per case (test_overflow_gpu.py's docstring: with one pair of controls the rule misfires on its own)


# ------------------------------------------------------------------------------------------ 1. step by step == all at once
def _bits(ops, entry):
    return [1 << i for i in range(len(ops.LAYER_STEPS[entry]))]      # every bit of the entry's list, applicable or not


def _compare(bufs, run_all, run_steps, what):
    """Both runs from the same contents of every buffer; every buffer bit-identical afterwards."""
    init = {k: v.clone() for k, v in bufs.items()}
    run_all()
    torch.cuda.synchronize()
    want = {k: v.clone() for k, v in bufs.items()}
    for k, v in bufs.items():
        v.copy_(init[k])
    run_steps()
    torch.cuda.synchronize()
    for k in bufs:
        assert torch.equal(bufs[k], want[k]), (what, k)
    return want


def test_longnet_layer_bits_one_at_a_time_equal_one_call():
    from modaltune_amd import ops
    from modaltune_amd.engine import Engine
    cfg = ModelConfig(depth=1, interaction_indexes=((0, 0),), dropout=0.25, drop_path_rate=0.1)
    sizes = synth.toy_group_sizes()
    eng = Engine(cfg, sizes, "cuda")
    eng.load_state_dict(synth.synth_state_dict(cfg, sizes, seed=31))
    eng._build_caches()
    eng.set_stochastic(True, seed=77)
    B, L, D, Fd = 2, 700, cfg.embed_dim, cfg.ffn_dim
    N = L + 1
    M = B * N
    plan = ops.make_plan(branch_table(N, eng.seg_lengths, DILATED_RATIOS), N, B)
    g = torch.Generator().manual_seed(5)
    spec = eng._ws_spec(B, L)
    names = dict(hin="hin0", hmid="hmid0", qkv="qkv0", o_br="obr0", lse_br="lsebr0", lse_tot="lsetot0", a1="a1_0", st1="st1_0", stin="stin_0",
                 st2="st2_0", stf="stf_0", u16="u16", br16="br16", t16="t16", dh="dh", dy16="dy16", dh16="dh16", dt16="dt16", da1="da1",
                 dmixed="dmixed", dqkv16="dqkv16", delta="delta", attn_ws="attn_ws")
    bufs = {}
    for field, nm in names.items():
        dt, shape = spec[nm]
        bufs[field] = (0.1 * torch.randn(shape, generator=g)).to(dt).cuda()
    bufs["hin"] = torch.randn(M, D, generator=g).cuda()
    bufs["out"] = torch.randn(M, D, generator=g).cuda()
    bufs["pend_x"] = torch.randn(M, D, generator=g).cuda()
    bufs["pend_branch"] = (0.3 * torch.randn(M, D, generator=g)).half().cuda()
    cb = ops.struct_of(ops.MtLongNetLayerBuffers, **{f: bufs[f] for f in names})
    lw = eng._layer_w[0]
    drop = lambda site: ops.dropout_spec(eng.rng, site, 0.25, site + 1, 0.1, N)
    d_attn, d_ffn, d_pend, d_lower = drop(16), drop(18), drop(40), drop(42)
    for pend in (None, (bufs["pend_x"], bufs["pend_branch"], d_pend)):
        for defer in (False, True):
            def fwd(steps):
                ops.longnet_layer_fwd(lw, cb, plan, M, D, Fd, bufs["out"], pend=pend, defer=defer, drop_attn=d_attn, drop_ffn=d_ffn, steps=steps)
            got = _compare(bufs, lambda: fwd(ops.LAYER_ALL), lambda: [fwd(b) for b in _bits(ops, "longnet_layer_fwd")],
                           ("longnet fwd", pend is not None, defer))
            assert bool(torch.isfinite(got["br16" if defer else "out"]).all()) and bool(torch.isfinite(got["hmid"]).all())
    # the backward reads what the last forward above saved (and writes none of it: every case starts from the same activations)
    bufs["dh"].copy_(64.0 * torch.randn(M, D, generator=g))
    bufs["dh16"].copy_(bufs["dh"])
    for dh16_valid in (False, True):
        for feeds_lower in (False, True):
            def bwd(steps):
                ops.longnet_layer_bwd(lw, cb, plan, M, D, Fd, dh16_valid, feeds_lower, drop_attn=d_attn, drop_ffn=d_ffn, drop_lower_ffn=d_lower,
                                      steps=steps)
            got = _compare(bufs, lambda: bwd(ops.LAYER_ALL), lambda: [bwd(b) for b in _bits(ops, "longnet_layer_bwd")],
                           ("longnet bwd", dh16_valid, feeds_lower))
            assert bool(torch.isfinite(got["dh"]).all()) and bool(torch.isfinite(got["dh16"].float()).all())
            bufs["dh"].copy_(64.0 * torch.randn(M, D, generator=g))
            bufs["dh16"].copy_(bufs["dh"])


def test_vit_block_bits_one_at_a_time_equal_one_call():
    import titan_standin
    from modaltune_amd import ops
    from modaltune_amd.titan import NativeBackbone, device_tokens
    vit = titan_standin.VisionTransformer()
    titan_standin.init_standin(vit, 6)
    bb = NativeBackbone(vit, "cuda")
    x, coords, psz = bb._probe_inputs()
    _, cells, dims, Lv = device_tokens(x, coords, psz)
    B, N, D, Fd = 2, Lv + 1, bb.D, bb.F
    M = B * N
    plan, keep = bb.make_plan(cells, dims, N, B)
    g = torch.Generator().manual_seed(9)
    spec = bb.ws_spec(B, Lv)
    names = dict(hmid="hmid0", qkv="qkv0", o16="o0", lse="lse0", a1="a1_0", st1="st1_0", st2="st2_0", u16="u16", br16="br16", t16="t16",
                 dy16="dy16", dh16="dh16", dt16="dt16", da1="da1", dqkv16="dqkv16", delta="delta")
    bufs = {}
    for field, nm in names.items():
        dt, shape = spec[nm]
        bufs[field] = (0.1 * torch.randn(shape, generator=g)).to(dt).cuda()
    for nm in ("hin", "out", "pend_x", "dh"):
        bufs[nm] = torch.randn(M, D, generator=g).cuda()
    bufs["pend_branch"] = (0.3 * torch.randn(M, D, generator=g)).half().cuda()
    cb = ops.struct_of(ops.MtVitBlockBuffers, hin=bufs["hin"], dh=bufs["dh"], **{f: bufs[f] for f in names})
    cw = bb.blocks[0]["cw"]
    for pend in (None, (bufs["pend_x"], bufs["pend_branch"])):
        for defer in (False, True):
            def fwd(steps):
                ops.vit_block_fwd(cw, cb, plan, M, D, Fd, bufs["out"], pend=pend, defer=defer, steps=steps)
            got = _compare(bufs, lambda: fwd(ops.LAYER_ALL), lambda: [fwd(b) for b in _bits(ops, "vit_block_fwd")],
                           ("vit fwd", pend is not None, defer))
            assert bool(torch.isfinite(got["br16" if defer else "out"]).all()) and bool(torch.isfinite(got["hmid"]).all())
    bufs["dh"].copy_(64.0 * torch.randn(M, D, generator=g))
    bufs["dh16"].copy_(bufs["dh"])
    for dh16_valid in (False, True):
        for feeds_lower in (False, True):
            def bwd(steps):
                ops.vit_block_bwd(cw, cb, plan, M, D, Fd, dh16_valid, feeds_lower, steps=steps)
            got = _compare(bufs, lambda: bwd(ops.LAYER_ALL), lambda: [bwd(b) for b in _bits(ops, "vit_block_bwd")],
                           ("vit bwd", dh16_valid, feeds_lower))
            assert bool(torch.isfinite(got["dh"]).all()) and bool(torch.isfinite(got["dh16"].float()).all())
            bufs["dh"].copy_(64.0 * torch.randn(M, D, generator=g))
            bufs["dh16"].copy_(bufs["dh"])
    assert keep is not None


# ------------------------------------------------------------------------------------------ the configurations of 2. and 3.
def _longnet(L):
    """Depth 2, one interaction block over both layers (layer 0 defers its fc2 add, layer 1 takes it as `pend` and leaves fp16(dh) to
    layer 0), train mode with Dropout / DropPath; 3 task passes: M = 3 (L + 1) rows."""
    from modaltune_amd.engine import Engine
    from modaltune_amd.trainer import TrainStep
    seed = 12
    cfg = ModelConfig(depth=2, interaction_indexes=((0, 1),), slide_ngrids=64, dropout=0.25, drop_path_rate=0.1)
    sizes = synth.toy_group_sizes()
    eng = Engine(cfg, sizes, "cuda")
    eng.load_state_dict(synth.synth_state_dict(cfg, sizes, seed))
    ts = TrainStep(eng, lr=0.0, weight_decay=0.0)
    ts.set_projector(synth.projector_state(seed))
    inp = synth.synth_inputs(L, sizes, seed, grid=64)
    x = torch.from_numpy(inp["x"]).cuda()
    return eng, ts, (x.reshape(-1, x.shape[-1]).contiguous(), inp["coords"], [torch.from_numpy(a).cuda() for a in inp["genes"]],
                     torch.from_numpy(inp["text"]).cuda())


def _titan(L=900):
    """The TITAN configuration on the stand-in backbone (6 dense blocks, three interaction blocks of two), train mode."""
    import titan_standin
    from test_titan_cpu import TITAN_JSON
    from modaltune_amd.titan import NativeBackbone, TitanEngine, titan_model_config
    from modaltune_amd.trainer import TrainStep
    seed = 6
    sizes = synth.toy_group_sizes()
    vit = titan_standin.VisionTransformer()
    titan_standin.init_standin(vit, seed)
    cfg = titan_model_config(TITAN_JSON, 3, False, 6)
    eng = TitanEngine(cfg, sizes, NativeBackbone(vit, "cuda"), "cuda")
    eng.load_state_dict(synth.synth_state_dict(cfg, sizes, seed))
    ts = TrainStep(eng, lr=0.0, weight_decay=0.0)
    ts.set_projector(synth.projector_state(seed))
    inp = synth.synth_inputs_titan(L, sizes, seed, grid=40)
    return eng, ts, (torch.from_numpy(inp["x"]).cuda().reshape(L, -1).contiguous(), torch.from_numpy(inp["coords"]).cuda().reshape(L, 2),
                     [torch.from_numpy(a).cuda() for a in inp["genes"]], torch.from_numpy(inp["text"]).cuda())


CASES = {"longnet_M_above_1024": lambda: _longnet(400), "longnet_M_up_to_1024": lambda: _longnet(100), "titan": _titan}


def _seeded_step(eng, ts, slide, update):
    """One eager, batched step whose dropout masks are those of (seed 2026, step 1) whenever it is called."""
    ts.auto_split, ts.split_min_patches = False, 1 << 30
    eng.set_stochastic(True, seed=2026)
    ts.step(*slide, update=update)
    torch.cuda.synchronize()


def record_keys(case):
    """{"timer": {key: launches}, "timeline": [key, ...]} of one timed train step of CASES[case] (after one untimed step: workspaces
    and weight caches exist).  The fixture is this function's output at the last commit that had the Python launch lists."""
    from modaltune_amd import ops
    eng, ts, slide = CASES[case]()
    _seeded_step(eng, ts, slide, True)
    ops.TIMER, ops.TIMELINE = {}, []
    try:
        _seeded_step(eng, ts, slide, True)
    finally:
        timer, timeline, ops.TIMER, ops.TIMELINE = ops.TIMER, ops.TIMELINE, None, None
    return {"timer": {k: len(v) for k, v in sorted(timer.items())}, "timeline": [t[0] for t in timeline]}


@pytest.mark.parametrize("case", list(CASES))
def test_timed_pass_files_every_launch_under_the_recorded_key(golden_dir, case):
    want = json.load(open(os.path.join(golden_dir, KEYS_JSON)))[case]
    got = record_keys(case)
    assert got["timer"] == want["timer"]
    # launches the recorded schedule timed but left out of its TIMELINE (the dense attention backward's three phases): listed in the
    # fixture; they now appear there, each as often as TIMER counts it, and nothing else moved
    added = want["timeline_added"]
    assert [k for k in got["timeline"] if k not in added] == want["timeline"]
    for k in added:
        assert got["timeline"].count(k) == want["timer"][k], k
    at = [i for i, k in enumerate(got["timeline"]) if added and k == added[0]]
    assert all(got["timeline"][i:i + len(added)] == added for i in at)      # ... as one run in launch order per block
    assert want["timer"]["dense_attn_bwd_kv" if case == "titan" else "dilated_attn_bwd_kv"] > 0, "the case runs the backbone's backward"


# ------------------------------------------------------------------------------------------ 3. the timed step is the shipped step
def _relmax(a, b):
    a, b = a.detach().double().reshape(-1), b.detach().double().reshape(-1)
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


@pytest.mark.parametrize("case", ["longnet_M_above_1024", "titan"])
def test_timed_step_computes_what_the_untimed_step_computes(case):
    from modaltune_amd import ops
    eng, ts, slide = CASES[case]()

    def run(timed):
        ops.TIMER = {} if timed else None
        try:
            _seeded_step(eng, ts, slide, False)
        finally:
            n, ops.TIMER = (len(ops.TIMER) if timed else 0), None
        assert int(ts.found_inf) == 0
        return n, ts.last_logits.clone(), ts.loss.clone(), {k: v.clone() for k, v in ts.unscaled_grads().items()}

    run(False)      # (workspaces, weight caches)
    controls = [run(False) for _ in range(CONTROLS)]
    n, logits, loss, grads = run(True)
    assert n > 10, "the timed pass did time launches"
    assert bool(torch.isfinite(logits).all()) and float(loss) > 0
    for _, lg, ls, _ in controls:
        assert torch.equal(logits, lg) and torch.equal(loss, ls)
    spread = {k: max(_relmax(a[3][k], b[3][k]) for i, a in enumerate(controls) for b in controls[i + 1:]) for k in grads}
    dist = {k: min(_relmax(grads[k], c[3][k]) for c in controls) for k in grads}
    top = sorted(grads, key=lambda k: -dist[k])[:5]
    print(f"timed-vs-untimed {case}: largest control-to-control spread {max(spread.values()):.2e}; largest timed-to-control distances",
          {k: f"{dist[k]:.2e} (spread {spread[k]:.2e})" for k in top})
    assert any(float(v.abs().max()) > 0 for v in grads.values())
    for k in grads:
        if spread[k] == 0.0:
            assert torch.equal(grads[k], controls[0][3][k]), (k, dist[k])
        else:
            assert dist[k] <= 2.0 * spread[k], (k, dist[k], spread[k])
