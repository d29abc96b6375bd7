"""GPU: the backbone kernels leave out the task passes DropPath dropped (Engine.droppath_skip / MT_DROPPATH_SKIP, the live table of
mt_droppath_live) -- and nothing changes: the device table is the numpy restatement's, and a deterministic train step with the skip
on has the loss, logits and gradient bits of the same step with it off, eagerly and under one captured graph whose draws change from
replay to replay, from a workspace that was NaN before the first step too.  depth 3 with DropPath rates 0 / 0.3 / 0.6 and N = 301 rows
per pass (a multiple of no tile height); the seeds come from the restatement so that every case of dropped passes occurs."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from modaltune_amd import ops, synth  # noqa: E402
from modaltune_amd.config import ModelConfig  # noqa: E402

import test_droppath_live_cpu as R  # noqa: E402

DEPTH, RATE, L, DATA_SEED = 3, 0.6, 300, 5
N = L + 1
KINDS = ("attn", "ffn")


def _want(B):
    return {(k, c) for k in KINDS for c in R.possible_cases(B)}


# seeds per schedule, picked on the CPU at collection time (12 at the most over the four schedules); the step that runs draws with
# the rng's step word = 1 (set_stochastic zeroes it, the step advances it once)
SEEDS = {
    1: R.pick_seeds(_want(1), lambda s: R.cases_seen(s, 1, DEPTH, RATE, 1), 2),
    2: R.pick_seeds(_want(2), lambda s: R.cases_seen(s, 1, DEPTH, RATE, 2), 3),
    3: R.pick_seeds(_want(3), lambda s: R.cases_seen(s, 1, DEPTH, RATE, 3), 4),
    # two pass groups: B = 2 with site group 1 and B = 1 with site group 2 (site offsets 1024 and 2048)
    "groups": R.pick_seeds({(g,) + kc for g, B in ((0, 2), (1, 1)) for kc in _want(B)},
                           lambda s: {(0,) + kc for kc in R.cases_seen(s, 1, DEPTH, RATE, 2, 1024)}
                           | {(1,) + kc for kc in R.cases_seen(s, 1, DEPTH, RATE, 1, 2048)}, 3),
}
assert sum(len(v) for v in SEEDS.values()) <= 12


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


class _Rig:
    def __init__(self, B):
        from modaltune_amd.engine import Engine
        from modaltune_amd.trainer import TrainStep
        self.cfg = ModelConfig(depth=DEPTH, interaction_indexes=((0, 2),), slide_ngrids=64, drop_path_rate=RATE, dropout=0.25)
        sizes = synth.toy_group_sizes()
        inp = synth.synth_inputs(L, sizes, DATA_SEED, grid=64)
        self.eng = Engine(self.cfg, sizes, "cuda")
        assert self.eng.deterministic and self.eng.droppath_skip
        self.eng.load_state_dict(synth.synth_state_dict(self.cfg, sizes, DATA_SEED))
        self.ts = TrainStep(self.eng, task_ids=(0, 1, 2)[:B], text_rows=(0, 1, 3)[:B])
        self.ts.set_projector(synth.projector_state(DATA_SEED))
        self.B = B
        self.args = (torch.from_numpy(inp["x"]).cuda(), inp["coords"], [torch.from_numpy(a).cuda() for a in inp["genes"]],
                     torch.from_numpy(inp["text"]).cuda())

    def schedule(self, groups):
        self.ts.split_passes, self.ts.split_min_patches = bool(groups), 0
        assert self.ts._split_now(L) is bool(groups)

    def step(self, seed, skip):
        self.eng.droppath_skip = skip
        self.eng.set_stochastic(True, seed=seed)
        self.ts.step(*self.args, update=False)
        torch.cuda.synchronize()
        return {"loss": self.ts.loss.clone(), "logits": self.ts.last_logits.clone(), "grad": self.eng.store.flat_grad.clone()}

    def tables(self, groups):
        """The live tables the last step wrote, one per workspace store."""
        ws = self.ts._group_workspaces(L, bool(groups))
        return [w["live"].cpu().numpy().copy() for w in ws]


@pytest.fixture(scope="module")
def det_env():
    mp = pytest.MonkeyPatch()
    mp.setenv("MT_DETERMINISTIC", "1")
    mp.delenv("MT_DROPPATH_SKIP", raising=False)
    mp.delenv("MT_SPLIT_PASSES", raising=False)
    yield
    mp.undo()


@pytest.fixture(scope="module")
def rigs(det_env):
    _gpu()
    made = {}

    def get(B):
        if B not in made:
            made[B] = _Rig(B)
        return made[B]
    yield get
    made.clear()


def _same(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k, float((a[k].double() - b[k].double()).abs().max()))
        assert bool(torch.isfinite(a[k]).all()), (what, k)


def _cases_of_table(t, B):
    """{(kind, case)} a live table shows; a hull hides a dead middle pass, so "middle" is read off the restatement by the callers."""
    seen = set()
    for i in range(2, 2 * DEPTH):          # (layer 0 has rate 0)
        b0, b1 = int(t[i, 0]), int(t[i, 1])
        pattern = [b0 <= b < b1 for b in range(B)]
        seen |= {(KINDS[i & 1], c) for c in R.case_of(pattern) if c != "middle"}
    return seen


@pytest.mark.parametrize("B", [1, 2, 3])
def test_device_table_equals_the_restatement(rigs, B):
    _gpu()
    rng = torch.zeros(4, dtype=torch.int32, device="cuda")
    table = torch.full((2 * DEPTH, 2), -7, dtype=torch.int32, device="cuda")
    for seed in list(range(1, 40)) + [2 ** 31 + 5, 2 ** 40 + 3]:
        for step, base in ((1, 0), (3, 1024), (70000, 2048)):
            words = R.rng_words(seed, step)
            rng.copy_(torch.tensor(words, dtype=torch.int64).to(torch.int32))
            sites, ps = R.layer_sites(DEPTH, base), R.layer_ps(DEPTH, RATE)
            ops.droppath_live(sites, ps, B, rng, table)
            assert np.array_equal(table.cpu().numpy(), R.live_table(words, sites, ps, B)), (seed, step, base)


@pytest.mark.parametrize("sched", [1, 2, 3, "groups"])
def test_skip_on_has_the_bits_of_skip_off(rigs, sched):
    """Eager steps, every seed of the schedule: loss, logits and the flat gradient with the skip on torch.equal the skip-off step from
    the same state and rng; the tables read back show every case the schedule can have."""
    B, groups = (3, True) if sched == "groups" else (sched, False)
    rig = rigs(B)
    rig.schedule(groups)
    seen = set()
    for seed in SEEDS[sched]:
        off = rig.step(seed, False)
        on = rig.step(seed, True)
        _same(on, off, (sched, seed))
        assert float(on["grad"].abs().max()) > 0
        tabs = rig.tables(groups)
        words = R.rng_words(seed, 1)
        geo = [(2, 1024), (1, 2048)] if groups else [(B, 0)]
        for g, (t, (gb, base)) in enumerate(zip(tabs, geo)):
            assert np.array_equal(t, R.live_table(words, R.layer_sites(DEPTH, base), R.layer_ps(DEPTH, RATE), gb)), (sched, seed, g)
            got = _cases_of_table(t, gb)
            if gb == 3:      # (the hull of live-dead-live is {0, 3}: that case is the restatement's word, the table agreeing with it above)
                got |= {kc for kc in R.cases_seen(seed, 1, DEPTH, RATE, 3, base) if kc[1] == "middle"}
            seen |= {(g,) + kc for kc in got} if groups else got
    want = {(g,) + kc for g, gb in ((0, 2), (1, 1)) for kc in _want(gb)} if groups else _want(B)
    assert seen >= want, sorted(want - seen)


@pytest.mark.parametrize("sched", [1, 2, 3, "groups"])
def test_skip_under_one_captured_graph(det_env, sched):
    """Two trainers from the same state, skip off / on, the same step_graphed calls: two eager visits and the capture, then for every
    seed of the schedule the rng is re-seeded IN PLACE (the captured graph reads the same device words) and the graph is replayed four
    times (rng step words 1 .. 4) -- the draws change under the one captured graph and the tables follow on the device.  Every replay's
    loss and the final weights, moments and gradients are torch.equal; the tables read back after the replays equal the restatement
    and show every case the schedule can have ("groups": the two concurrent tables of the B = 2 | 1 groups on their forked streams)."""
    _gpu()
    B, groups = (3, True) if sched == "groups" else (sched, False)
    geo = [(2, 1024), (1, 2048)] if groups else [(B, 0)]
    runs = []
    for skip in (False, True):
        rig = _Rig(B)
        rig.schedule(groups)
        rig.eng.droppath_skip = skip
        rig.eng.set_stochastic(True, seed=11)
        for _ in range(3):                       # two eager visits, the capture
            rig.ts.step_graphed(*rig.args)
        before, losses, seen = rig.ts.graph_replays, [], set()
        assert before == 1
        for seed in SEEDS[sched]:
            rig.eng.set_stochastic(True, seed=seed)
            for k in range(1, 5):
                rig.ts.step_graphed(*rig.args)
                torch.cuda.synchronize()
                losses.append(rig.ts.loss.clone())
                if not skip:
                    continue
                for g, (t, (gb, base)) in enumerate(zip(rig.tables(groups), geo)):
                    assert np.array_equal(t, R.live_table(R.rng_words(seed, k), R.layer_sites(DEPTH, base), R.layer_ps(DEPTH, RATE), gb)), \
                        (sched, seed, k, g)
                    got = _cases_of_table(t, gb)
                    if gb == 3:      # (a hull hides a dead middle pass: the restatement's word, the table agreeing with it above)
                        got |= {kc for kc in R.cases_seen(seed, k, DEPTH, RATE, 3, base) if kc[1] == "middle"}
                    seen |= {(g,) + kc for kc in got} if groups else got
        assert rig.ts.graph_replays - before == 4 * len(SEEDS[sched])
        if skip:
            want = {(g,) + kc for g, gb in ((0, 2), (1, 1)) for kc in _want(gb)} if groups else _want(B)
            assert seen >= want, sorted(want - seen)
        runs.append({"losses": torch.cat([v.reshape(-1) for v in losses]), "flat": rig.eng.store.flat.clone(),
                     "grad": rig.eng.store.flat_grad.clone(), "m": rig.ts.m.clone(), "v": rig.ts.v.clone()})
        del rig
    _same(runs[1], runs[0], ("graphed", sched))
    assert len(set(runs[0]["losses"].tolist())) == len(runs[0]["losses"])


def test_poisoned_workspace(rigs, det_env):
    """Every floating-point buffer of the workspace store is NaN before the first step of a fresh engine (skip on): all outputs are
    finite and torch.equal the skip-off step of an unpoisoned engine -- no dropped pass's stale bytes reach a result."""
    ref = rigs(3)
    ref.schedule(False)
    rig = _Rig(3)
    rig.schedule(False)
    rig.eng.set_stochastic(True, seed=1)          # (the store of a stochastic engine has one buffer more: allocate it as the steps will)
    ws = rig.eng._workspace(3, L)
    store = rig.eng._ws_store[(3, 0)]
    for t in store["flat"].values():
        if t.is_floating_point():
            t.fill_(float("nan"))
    assert bool(torch.isnan(ws["br16"]).all()) and bool(torch.isnan(ws["t16"]).all())
    for seed in SEEDS[3]:
        on = rig.step(seed, True)
        for t in store["flat"].values():          # ... and again before every further step: whatever a skipped kernel left is poison
            if t.is_floating_point():
                t.fill_(float("nan"))
        _same(on, ref.step(seed, False), ("poisoned", seed))


# ---------------------------------------------------------------------------------------------------------------- per kernel
SENT = 7.0


@pytest.mark.parametrize("b0,b1", [(0, 3), (1, 3), (0, 2), (1, 2), (0, 0), (2, 3)])
def test_attention_forward_live_rows(rigs, b0, b1):
    """mt_dilated_attn_fwd with a live entry: rows of the passes in [b0, b1) equal the full launch, every other row keeps the sentinel."""
    rig = rigs(3)
    plan = rig.eng._attention_plan(N, 3)
    nb, M = plan.nbranch, 3 * N
    g = torch.Generator(device="cuda").manual_seed(11)
    qkv = (torch.randn(M, 2304, device="cuda", generator=g) * 0.5).half()
    full_o = torch.full((nb, M, 768), SENT, dtype=torch.float16, device="cuda")
    full_l = torch.full((nb, M, 16), SENT, dtype=torch.float32, device="cuda")
    ops.dilated_attn_fwd(qkv, plan, full_o, full_l)
    o = torch.full_like(full_o, SENT)
    lse = torch.full_like(full_l, SENT)
    live = torch.tensor([b0, b1], dtype=torch.int32, device="cuda")
    ops.dilated_attn_fwd(qkv, plan, o, lse, live=live)
    torch.cuda.synchronize()
    assert bool((full_o != SENT).any())
    r0, r1 = b0 * N, b1 * N
    assert torch.equal(o[:, r0:r1], full_o[:, r0:r1]) and torch.equal(lse[:, r0:r1], full_l[:, r0:r1])
    for lo, hi in ((0, r0), (r1, M)):
        assert bool((o[:, lo:hi] == SENT).all()) and bool((lse[:, lo:hi] == SENT).all())


@pytest.mark.parametrize("b0,b1", [(0, 3), (1, 2), (0, 0), (2, 3)])
def test_ffn_layernorm_live_rows(rigs, b0, b1):
    """The FFN's sub-LayerNorm (fp16 GELU form, D = 3072), forward and backward, over the live rows only."""
    _gpu()
    M, F = 3 * N, 3072
    g = torch.Generator(device="cuda").manual_seed(12)
    x = torch.randn(M, F, device="cuda", generator=g).half()
    dy = (torch.randn(M, F, device="cuda", generator=g) * 0.1).half()
    w = torch.rand(F, device="cuda", generator=g) + 0.5
    b = torch.randn(F, device="cuda", generator=g) * 0.1
    live = torch.tensor([b0, b1], dtype=torch.int32, device="cuda")
    y_full, st_full = torch.empty_like(x), torch.empty(M, 2, device="cuda")
    ops.layernorm_fwd(x, w, b, y_full, st_full, M, F, gelu_in=True)
    y, st = torch.full_like(x, SENT), torch.full((M, 2), SENT, device="cuda")
    ops.layernorm_fwd(x, w, b, y, st, M, F, gelu_in=True, live=live, live_rows=N)
    dx_full = torch.empty_like(x)
    ops.layernorm_bwd(dy, x, w, st_full, dx_full, M, F, gelu_in=True)
    dx = torch.full_like(x, SENT)
    ops.layernorm_bwd(dy, x, w, st_full, dx, M, F, gelu_in=True, live=live, live_rows=N)
    torch.cuda.synchronize()
    r0, r1 = b0 * N, b1 * N
    for got, full in ((y, y_full), (st, st_full), (dx, dx_full)):
        assert torch.equal(got[r0:r1], full[r0:r1])
        assert bool((got[:r0] == SENT).all()) and bool((got[r1:] == SENT).all())


def test_ffn_layernorm_live_rows_with_an_explicit_eps():
    """A live entry and an epsilon in one call (one MtLaunchOpts; the fp16 GELU form, D = 3072, 3 passes of 5 rows): the live rows have
    the bits of the same call without a table, the other rows keep the sentinel, and the epsilon is the one given -- inputs of standard
    deviation 1e-3 leave a row variance of about 2.5e-7 behind the GELU, so rstd at 1e-6 is about 3 times that at 1e-5."""
    _gpu()
    rows, F = 5, 3072
    M = 3 * rows
    g = torch.Generator(device="cuda").manual_seed(15)
    x = (torch.randn(M, F, device="cuda", generator=g) * 1e-3).half()
    w = torch.rand(F, device="cuda", generator=g) + 0.5
    b = torch.randn(F, device="cuda", generator=g) * 0.1
    y_full, st_full = torch.empty_like(x), torch.empty(M, 2, device="cuda")
    ops.layernorm_fwd(x, w, b, y_full, st_full, M, F, gelu_in=True, eps=1e-6)
    y_ref, st_ref = torch.empty_like(x), torch.empty(M, 2, device="cuda")
    ops.layernorm_fwd(x, w, b, y_ref, st_ref, M, F, gelu_in=True)          # eps = 1e-5
    torch.cuda.synchronize()
    ratio = st_full[:, 1] / st_ref[:, 1]
    assert float(ratio.min()) > 2.0 and not torch.equal(y_full, y_ref), ratio
    for b0, b1 in ((1, 3), (0, 3), (0, 0)):
        live = torch.tensor([b0, b1], dtype=torch.int32, device="cuda")
        y, st = torch.full_like(x, SENT), torch.full((M, 2), SENT, device="cuda")
        ops.layernorm_fwd(x, w, b, y, st, M, F, gelu_in=True, eps=1e-6, live=live, live_rows=rows)
        torch.cuda.synchronize()
        r0, r1 = b0 * rows, b1 * rows
        for got, full, other in ((y, y_full, y_ref), (st, st_full, st_ref)):
            assert torch.equal(got[r0:r1], full[r0:r1]), (b0, b1)
            assert bool((got[:r0] == SENT).all()) and bool((got[r1:] == SENT).all()), (b0, b1)
            assert r0 == r1 or not torch.equal(got[r0:r1], other[r0:r1]), (b0, b1)


@pytest.mark.parametrize("b0,b1", [(0, 3), (1, 2), (0, 0), (0, 1)])
def test_residual_layernorm_backward_counts_dead_dy_as_zero(rigs, b0, b1):
    """mt_layernorm_bwd with a live entry on the residual stream (D = 768, accumulating, with the fp16 copy): NaN dy rows outside the live passes give
    what exact-zero dy rows give -- dh unchanged there, dx_f16 written."""
    _gpu()
    M, D = 3 * N, 768
    g = torch.Generator(device="cuda").manual_seed(13)
    x = torch.randn(M, D, device="cuda", generator=g)
    dy = (torch.randn(M, D, device="cuda", generator=g) * 0.1).half()
    w = torch.rand(D, device="cuda", generator=g) + 0.5
    st = torch.stack([x.mean(1), (x.var(1, unbiased=False) + 1e-5).rsqrt()], 1).contiguous()
    dh0 = torch.randn(M, D, device="cuda", generator=g)
    dead = torch.ones(M, dtype=torch.bool, device="cuda")
    dead[b0 * N:b1 * N] = False
    dy_zero, dy_nan = dy.clone(), dy.clone()
    dy_zero[dead] = 0
    dy_nan[dead] = float("nan")
    live = torch.tensor([b0, b1], dtype=torch.int32, device="cuda")
    dh_ref, d16_ref = dh0.clone(), torch.empty(M, D, dtype=torch.float16, device="cuda")
    ops.layernorm_bwd(dy_zero, x, w, st, dh_ref, M, D, accumulate=True, dx16=d16_ref)
    dh, d16 = dh0.clone(), torch.full((M, D), SENT, dtype=torch.float16, device="cuda")
    ops.layernorm_bwd(dy_nan, x, w, st, dh, M, D, accumulate=True, dx16=d16, live=live, live_rows=N)
    torch.cuda.synchronize()
    assert torch.equal(dh, dh_ref) and torch.equal(d16, d16_ref)
    assert torch.equal(dh[dead], dh0[dead])


# (shape, epilogue, bias) -> the kernel that serves it on a 256-CU device: the 128 x 128 tile kernel at 3 x 301 rows (the engine tests'
# size), and at 3 x 2753 rows (a multiple of no tile height either) the persistent kernel with / without bias and with the head-major
# q|k|v epilogue, the ping-pong kernel's 256-row tiles (N = 3072: the persistent kernel's last round would be too empty) and its
# 128-row tiles (K = 3072)
GEMM_CASES = [
    (301, 768, 768, "bias", True), (301, 2304, 768, "qkv_hm", True), (301, 768, 3072, "bias", False),
    (2753, 2304, 768, "qkv_hm", True), (2753, 2304, 768, "bias", True), (2753, 2304, 768, "bias", False),
    (2753, 3072, 768, "bias", True), (2753, 768, 3072, "bias", False),
]


@pytest.mark.parametrize("rows,Nn,K,epi,with_bias", GEMM_CASES)
def test_gemm_live_rows(rows, Nn, K, epi, with_bias):
    """mt_gemm_nt_f16 with a live entry: rows of the passes in [b0, b1) are torch.equal to the full launch -- the row tiles are laid from row
    b0 * rows on, a row's bits do not depend on that, and the head-major epilogue places it by its global row -- and every other row of
    C keeps the sentinel."""
    _gpu()
    M = 3 * rows
    g = torch.Generator(device="cuda").manual_seed(14)
    A = (torch.randn(M, K, device="cuda", generator=g) * 0.5).half()
    W = (torch.randn(Nn, K, device="cuda", generator=g) * 0.05).half()
    bias = torch.randn(Nn, device="cuda", generator=g) if with_bias else None
    epilogue = ops.EPI_QKV_HM if epi == "qkv_hm" else ops.EPI_BIAS
    shape = (Nn // 48, M, 48) if epi == "qkv_hm" else (1, M, Nn)          # [slab][row][column]
    full = torch.full(shape, SENT, dtype=torch.float16, device="cuda")
    ops.gemm_nt(A, W, full, M, Nn, K, epilogue=epilogue, bias=bias, ldc=Nn)
    ref = (A.float() @ W.float().t() + (bias if with_bias else 0)).half()
    ref = ref.view(M, Nn // 48, 48).transpose(0, 1) if epi == "qkv_hm" else ref.view(1, M, Nn)
    assert float((full.float() - ref.float()).abs().max()) < 0.05          # (the full launch is a product: the sentinel is gone)
    for b0, b1 in ((0, 3), (1, 3), (0, 2), (1, 2), (0, 0), (2, 3)):
        out = torch.full(shape, SENT, dtype=torch.float16, device="cuda")
        live = torch.tensor([b0, b1], dtype=torch.int32, device="cuda")
        ops.gemm_nt(A, W, out, M, Nn, K, epilogue=epilogue, bias=bias, ldc=Nn, live=live, live_rows=rows)
        torch.cuda.synchronize()
        r0, r1 = b0 * rows, b1 * rows
        assert torch.equal(out[:, r0:r1], full[:, r0:r1]), (b0, b1)
        assert bool((out[:, :r0] == SENT).all()) and bool((out[:, r1:] == SENT).all()), (b0, b1)


def test_gemm_live_takes_no_residual_epilogue():
    """The products that carry the residual stream run over every row: a table with them is refused, not ignored."""
    _gpu()
    A = torch.zeros(256, 64, dtype=torch.float16, device="cuda")
    W = torch.zeros(64, 64, dtype=torch.float16, device="cuda")
    out, resid = torch.zeros(256, 64, device="cuda"), torch.zeros(256, 64, device="cuda")
    live = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    with pytest.raises(Exception):
        ops.gemm_nt(A, W, out, 256, 64, 64, epilogue=ops.EPI_BIAS_RESID, resid=resid, ldr=64, live=live, live_rows=128)
