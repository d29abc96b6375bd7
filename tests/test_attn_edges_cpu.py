"""CPU: what tests/test_attn_edges_gpu.py relies on, checked without a kernel.

1. The closed form of tests/attn_edge_ref.py IS the gradient: branch b's share of the oracle's mixed output (w_b detached, times O_b,
   contracted with dmixed) differentiated by autograd for q, k and v equals it to 1e-9 per sequence, for every branch on its own, and
   the branches sum to the gradient of dilated_attention_core itself.
2. The per-sequence metric discriminates: four defects of ONE ratio-16 sequence push it over the bars, the clean fp16-staged emulation
   stays under them; the global max|a - b| / max|b| of the combined gradient that the older tests use stays under their 2e-2 for
   several of them (which, and the figures of those that do not, in the test's docstring).
3. The bars are 4 x the rounding floor (re-derived here over every plan and regime) and lie below the older tests' bars.
4. The plans produce the nvalid values they were chosen for, and the planted pairs of the "peaked" regime dominate from the last key
   tile."""
import pytest
import torch

import attn_edge_ref as R

H, HD = R.H, R.HD


def _autograd_setup(plan):
    """Float64 leaves (q = q' / MT_QK_SCALE_LOG2, k, v) of the case's own fp16 inputs, the oracle's branch outputs with a graph, the
    branch weights, lse_tot and delta in float64 (not rounded to fp32: the comparison is to 1e-9)."""
    from oracle import modaltune_oracle as O
    c = R.make_case(plan, "soft")
    tok = lambda t: t.double().permute(1, 0, 2).reshape(c.B, c.N, H, HD)
    q, k, v = (tok(c.qkv[0]) / R.QK).requires_grad_(True), tok(c.qkv[1]).requires_grad_(True), tok(c.qkv[2]).requires_grad_(True)
    mixed, outs, lses = O.dilated_attention_core(q, k, v, c.segs, c.ratios, return_branches=True)
    L = torch.stack(lses).detach()
    lse_tot = torch.logsumexp(L, dim=0)
    w = torch.exp(L - lse_tot)
    dm = tok(c.dmixed)
    delta = (dm[None] * torch.stack(outs).detach()).sum(-1)
    return c, (q, k, v), mixed, outs, w, dm, lse_tot.view(c.M, H), delta.view(len(c.bt), c.M, H)


def _dense_grads(c, loss, leaves, retain=True):
    """autograd's dq | dk | dv as [M, 3, 16, 48], dq for q' (the leaf is q = q' / QK, so dL/dq' = dL/dq / QK)."""
    gq, gk, gv = torch.autograd.grad(loss, leaves, retain_graph=retain)
    return torch.stack([gq / R.QK, gk, gv], dim=2).view(c.M, 3, H, HD)


@pytest.mark.parametrize("plan,use_qlimit", [("tail3", False), ("qlim", False), ("qlim", True)])
def test_closed_form_equals_autograd_per_branch_and_sums_to_the_core_gradient(plan, use_qlimit):
    """With qlimit, branch b's share is contracted with dmixed only on the rows that are its queries (i < qlimit): every real entry
    stays a key.  The oracle knows no qlimit, so the sum over branches is compared with the core's gradient without it only."""
    c, leaves, mixed, outs, w, dm, lse_tot, delta = _autograd_setup(plan)
    qlimit = c.qlimit if use_qlimit else None
    geoms = R.geometry(c.bt, c.N, c.B, qlimit)
    ref = R.bwd_reference(c.qkv, c.dmixed, lse_tot, delta, c.bt, c.N, c.B, qlimit)
    total = torch.zeros(c.M, 3, H, HD, dtype=torch.float64)
    for b, gm in enumerate(geoms):
        isq = torch.zeros(c.M, H, dtype=torch.bool).scatter_(1, gm.heads, gm.is_query).view(c.B, c.N, H, 1)
        got = _dense_grads(c, (w[b].unsqueeze(-1) * outs[b] * dm * isq).sum(), leaves)
        comp = torch.stack([R.compact(got[:, i], gm) for i in range(3)], dim=1)
        assert torch.equal(R.spread(comp, gm), got)                 # nothing outside the heads of the covering group
        errors = R.bwd_errors([comp], [ref[b]], [gm])
        for (_, name), (e, at) in errors.items():
            assert e < 1e-9, (plan, b, name, e, at)
        assert float(comp[:, 0][~gm.is_query].abs().max() if (~gm.is_query).any() else 0.0) == 0.0
        total += got
    if not use_qlimit:
        core = _dense_grads(c, (mixed.view(c.B, c.N, H, HD) * dm).sum(), leaves, retain=False)
        assert float((total - core).abs().max() / core.abs().max()) < 1e-9


def _old_rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _combined(parts, geoms):
    return sum(R.spread(p, gm) for p, gm in zip(parts, geoms))


# (plan, pass, segment, head) of the mutated ratio-16 sequence: nvalid 65 (two query tiles, the second with one entry) / 25 / 16
MUTATED = {"n1025": (0, 0, 0), "n385": (1, 0, 0), "tail3": (1, 0, 5)}
# mutation -> (plans, quantities it must push over the bar)
EXPECT = {
    "drop_last_key": (("n1025",), ("dq", "dk", "dv")),
    "neighbour_delta": (("n1025", "n385", "tail3"), ("dq", "dk")),
    "residue_shift": (("n1025", "n385", "tail3"), ("dq", "dk", "dv")),
    "skip_query_tile_2": (("n1025",), ("dk", "dv")),
}
# (mutation, plan, quantity) whose defect the older tests' metric does NOT see: the global rel of the combined gradient stays under 2e-2
OLD_METRIC_BLIND = {("neighbour_delta", "n1025", "dk"), ("neighbour_delta", "n385", "dk"),
                    ("skip_query_tile_2", "n1025", "dk"), ("skip_query_tile_2", "n1025", "dv")}


@pytest.mark.parametrize("mutation", list(EXPECT))
def test_metric_catches_a_defect_of_one_ratio16_sequence(mutation):
    """One sequence of the ratio-16 branch computed wrong, in the fp16-staged emulation (what a kernel with that defect would leave):
    (a) drop_last_key -- the last key of a sequence with nvalid 65 (a key tile of its own) takes no part; (b) neighbour_delta -- delta
    read from head h ^ 1, which belongs to another head group, so the branch does not visit it (0 in these inputs; dV does not depend
    on delta); (c) residue_shift -- the sequence walks the rows of the next residue; (d) skip_query_tile_2 -- the dK / dV sweep leaves
    out the queries 64 .. 127 (one query here).  The per-sequence metric must exceed the bar AT THAT SEQUENCE and nowhere else.
    The metric of the older tests -- one maximum over the whole combined [M, 3, 768] slab, bar 2e-2 -- is computed for the same
    defects (got: the sum of the staged branches rounded to fp16; want: the float64 sum).  Measured at these inputs, soft regime
    (per-sequence error of the mutated sequence -> global rel of the combined gradient; the ratio is scale-free in dmixed):
      (a) n1025  dq 2.2e-1 -> 2.2e-2   dk 5.3e-1 -> 4.4e-2   dv 5.4e-1 -> 3.6e-2
      (b) n1025  dq 2.2e-1 -> 2.2e-2   dk 1.5e-1 -> 1.2e-2;  n385  dq 4.7e-1 -> 3.7e-2   dk 1.8e-1 -> 1.8e-2;
          tail3  dq 2.7e-1 -> 3.5e-2   dk 2.2e-1 -> 2.6e-2
      (c) all three plans  1.4 .. 3.0 -> 1.3e-1 .. 3.2e-1
      (d) n1025  dk 1.8e-1 -> 1.5e-2   dv 1.8e-1 -> 1.2e-2
    So a sequence of the ratio-16 branch that is wrong by 15 .. 20 % stays UNDER the old bar for dk of (b) on n1025 and n385 and for
    dk and dv of (d): those are asserted (OLD_METRIC_BLIND) and show the gap.  (a) does NOT stay under the old bar at this input scale
    -- dropping the last of 65 keys zeroes that key's dK / dV outright, an error of 50 % of the sequence, and the ratio-16 branch
    carries about a fifth of the combined gradient's maximum here, more than its branch weight suggests, since P~ per key is of the
    same size in every branch -- nor do dq of (b) (2.2e-2 .. 3.7e-2) and dk of (b) on tail3; (c) replaces the whole sequence by
    unrelated values and is far over it.  For those the old figure is printed, not asserted; the inputs were not tuned until it held.
    In every case the per-sequence metric is 10 to 15 times more sensitive than the global one, with a bar 4 to 6 times lower."""
    plans, over = EXPECT[mutation]
    for plan in plans:
        c = R.make_case(plan, "soft")
        b = len(c.bt) - 1
        assert c.bt[b].ratio == 16
        gm, at = c.geoms[b], MUTATED[plan]
        if mutation in ("drop_last_key", "skip_query_tile_2"):
            assert int(gm.nv[gm.number(*at)]) == 65
        clean = R.bwd_errors(c.emu, c.ref, c.geoms)
        R.check(clean, R.BARS, f"{plan} clean emulation")
        emu = list(c.emu)
        emu[b] = R.bwd_reference(c.qkv, c.dmixed, c.lse_tot, c.delta, c.bt, c.N, c.B, c.qlimit, staged=True,
                                 mutate={(b,) + at: mutation}, branches=(b,))[b]
        for w, name in enumerate(R.QUANTITIES):
            err = R.seq_errors(emu[b][:, w], c.ref[b][:, w], gm)
            e, where = R.worst(err, gm)
            others = err.clone()
            others[gm.number(*at)] = float("nan")
            print(f"{mutation} {plan} {name}: mutated sequence {float(err[gm.number(*at)]):.3e}, worst other {R.worst(others, gm)[0]:.3e}")
            assert R.worst(others, gm)[0] < R.BARS[name]
            if name in over:
                assert e > R.BARS[name] and where == at, (plan, name, e, where)
                with pytest.raises(AssertionError, match=rf"branch {b} {name}.*\({at[0]}, {at[1]}, {at[2]}\)"):
                    R.check(R.bwd_errors(emu, c.ref, c.geoms), R.BARS, plan)
            else:
                assert e < R.BARS[name]
        got = _combined(emu, c.geoms).half().double()
        want = _combined(c.ref, c.geoms)
        for w, name in enumerate(R.QUANTITIES):
            r = _old_rel(got[:, w], want[:, w])
            print(f"{mutation} {plan} {name}: global rel of the combined gradient {r:.3e}")
            if (mutation, plan, name) in OLD_METRIC_BLIND:
                assert r < 2e-2, (plan, name, r)


def test_bars_are_four_times_the_rounding_floor():
    """The floor: the worst per-sequence error of the fp16-staged emulation against float64 over every plan and both regimes -- it
    comes from the reference alone.  The constants are 4 x that (the margin covers what the emulation does not carry: the fp32
    accumulation order of the MFMA chains, the hardware exp2, the fp32 rounding of lse_tot and delta) and must lie below the bars the
    older tests use for the same quantities: 2e-2 (dq, dk, dv), 3e-3 (branch outputs), 2e-3 (LSE)."""
    floor = {q: 0.0 for q in R.BARS}
    for plan in R.PLANS:
        for regime in R.REGIMES:
            f = R.floors(R.make_case(plan, regime))
            print(plan, regime, {q: f"{e:.3e}" for q, e in f.items()})
            for q, e in f.items():
                assert e < R.BARS[q], (plan, regime, q, e)          # the clean emulation sits under the bar
                floor[q] = max(floor[q], e)
    print("floors", {q: f"{e:.3e}" for q, e in floor.items()})
    for q, e in floor.items():
        assert 3.0 * e <= R.BARS[q] <= 5.0 * e, (q, e, R.BARS[q])
    assert max(R.BARS["dq"], R.BARS["dk"], R.BARS["dv"]) < 2e-2 and R.BARS["o"] < 3e-3 and R.BARS["lse"] < 2e-3


# plan -> per branch the set of nvalid over (segment, head group)
EDGES = {
    "n385": [{385}, {193, 192}, {97, 96}, {49, 48}, {25, 24}],
    "n1023": [{1023}, {512, 511}, {256, 255}, {128, 127}, {64, 63}],
    "n1025": [{1024, 1}, {513, 512}, {257, 256}, {129, 128}, {65, 64}],
    "tail3": [{64, 3}, {64, 2, 1}, {64, 1, 0}, {32, 1, 0}, {16, 1, 0}],
    "qlim": [{257}, {129, 128}, {65, 64}],
}


@pytest.mark.parametrize("plan", list(R.PLANS))
def test_edge_table(plan):
    """nvalid per (branch, segment, head group), computed here from the plan, is what the plans were chosen for -- an edit of the
    shapes cannot quietly lose an edge -- and agrees with a count of the rows that walk each sequence."""
    B, N, segs, ratios, qlimit = R.PLANS[plan]
    bt = R.branch_table(N, list(segs) if segs else R.segment_lengths(), ratios)
    table = R.edge_table(bt, N)
    for b, br in enumerate(bt):
        assert {n for (bb, _, _), n in table.items() if bb == b} == EDGES[plan][b], (plan, b)
    for b, gm in enumerate(R.geometry(bt, N, B, qlimit)):
        count = torch.bincount(gm.seq_id.reshape(-1), minlength=gm.nseq)
        assert torch.equal(count, gm.nv)                            # the row walk and Seq::nvalid's formula agree
        for s in range(gm.nseq):
            p, j, h = gm.name(s)
            assert int(gm.nv[s]) == table[b, j, h // gm.hb]
    tiles = lambda n: (n + 63) // 64
    if plan == "n385":          # 7 key tiles and a fourth 128-block with one live lane; 4 against 3 tiles
        assert tiles(385) == 7 and 385 - 3 * 128 == 1 and (tiles(193), tiles(192)) == (4, 3)
    if plan == "n1025":         # two segments in the dense branch, the second of ONE row; 65 and 513: a last key tile of one entry
        assert table[0, 0, 0] == 1024 and table[0, 1, 0] == 1 and tiles(65) == 2 and tiles(1025 // 2 + 1) == 9
    if plan == "tail3":
        assert N % 2 == 1 and bt[0].nseg == 5 and bt[1].nseg == 3 and bt[2].nseg == 2      # full segments; the second pass starts odd
        assert [table[0, 4, 0], table[1, 2, 0], table[1, 2, 1]] == [3, 2, 1]
        for b in (2, 3, 4):     # the last segment holds 3 rows: one entry for the residues 0 .. 2, NONE for every other head group
            assert [table[b, 1, g] for g in range(bt[b].ratio)] == [1, 1, 1] + [0] * (bt[b].ratio - 3)
    if plan == "qlim":          # queries: a prefix that ends on a tile edge, just past one, inside one; every real entry is a key
        gms = R.geometry(bt, N, B, qlimit)
        assert [sorted(set(gm.nq.tolist())) for gm in gms] == [[64], [65], [33]]
        assert all(int((~gm.is_query).sum()) > 0 for gm in gms)


@pytest.mark.parametrize("plan", list(R.PLANS))
def test_planted_pairs_dominate_from_the_last_key_tile(plan):
    c = R.make_case(plan, "peaked")
    assert len(c.planted) == len(c.bt)
    for b, p, g, qrow, krow in c.planted:
        gm = c.geoms[b]
        nv = int(gm.nv[gm.number(p, 0, g * gm.hb)])
        assert int(gm.sidx[krow]) // 64 == (nv - 1) // 64 and bool(gm.is_query[qrow].all())
        hs = slice(g * gm.hb, (g + 1) * gm.hb)
        s = (c.qkv[0][hs, qrow].double() * c.qkv[1][hs, krow].double()).sum(-1) / R.LOG2E      # the planted logit, natural units
        assert float(s.min()) > 30.0
        assert float((c.lse_ref[b, qrow, hs] - s).abs().max()) < 1e-6                          # ... carries the row's whole softmax
