"""GPU: the three MFMA kernels of the dilated attention (csrc/attn.hip forward, attn_bwd_kv.hip dK / dV, attn_bwd_q.hip dQ) against
float64 PER BRANCH AND PER SPARSE SEQUENCE, at the shapes where nvalid() and the tile counts change what is computed.

The kernels' values are read where the kernels leave them -- the backward's per-branch workspace regions (and, in the in-place form,
the dense branch in dqkv) before any combine, the forward's o_br / lse_br before any mix -- and compared with tests/attn_edge_ref.py,
which evaluates the formula of include/modaltune_hip.h from exactly the tensors the kernels read.  The metric is
max|got - ref| / max|ref| over ONE sequence's [nvalid, 48] slab (the LSE: max|got - ref|), so a ratio-16 sequence that is wrong by a
few percent fails although it is invisible in the combined gradient; a failure names (branch, quantity, pass, segment, head).  The
bars are 4 x the rounding floor of the fp16 staging (attn_edge_ref.BARS; tests/test_attn_edges_cpu.py re-derives them).

Plans (H = 16, d = 48; nvalid per head group -- tests/test_attn_edges_cpu.py::test_edge_table asserts them):
  n385   B 2, shipped segments: 385 (7 key tiles, a fourth 128-block with one live lane); 193 | 192 (4 | 3 tiles); 97 | 96; 49 | 48; 25 | 24
  n1023  B 1: 1023; 512 | 511; 256 | 255; 128 | 127; 64 | 63
  n1025  B 1: dense segments of 1024 and ONE row; 513 | 512; 257 | 256; 129 | 128; 65 | 64
  tail3  B 2, N 259, segments (64, 128, 256, 256, 256): last segments of 3 rows -- nvalid 3 (dense), 2 | 1 (ratio 2), 1 for the head
         groups 0 .. 2 and 0 for every other one (ratios 4, 8, 16: those workgroups exit and write nothing); several full segments per
         pass; the second pass starts at an odd row
  qlim   B 2, N 257, ratios (1, 2, 4), one segment each, qlimit (64, 65, 33): the queries are a prefix that ends on / just past a tile
         edge, every real entry is a key.  dK and dV are compared on all keys, dQ' on the rows i < qlimit; what the dQ kernel leaves in
         the other rows' slots is not asserted.  The FORWARD honours qlimit too (attn.hip: nvq = min(nv, p.qlimit[br]); workgroups
         past it exit, lanes past it store nothing), so its o_br / lse_br are compared on the rows i < qlimit and the other rows must
         keep the pre-fill.
Regimes: "soft" (logits of spread about 0.5) and "peaked" (about 3, with one planted pair per branch whose dominant key sits in the
last key tile of the sequence: the forward's deferred rescale fires there); q, k, v and dmixed are fp16 randn, dmixed of spread 1.
The rows of a sequence that is mostly padding (the ragged last segments of tail3 and n1025) keep the soft scale in both regimes
(attn_edge_ref.make_case says why).  Per case: lse_br, O_b and lse_tot come from the float64 oracle on the fp16-rounded inputs,
delta_b = sum_d dmixed O_b rounded to fp32; workspace, dqkv, o_br and lse_br are pre-filled with NaN.

Measured on the MI355X: the table in tests/README.md, row "dilated attention at the tile edges, per sequence"."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_edge_ref as R  # noqa: E402

DEV = "cuda"
CASES = [(p, r) for p in R.PLANS for r in R.REGIMES]
H, HD = R.H, R.HD


def _nan16(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float16, device=DEV)


_cache = {}


def _run(plan, regime):
    """The kernels' outputs of one case, computed once: workspace form and in-place form of the backward (phases KV | Q only), forward."""
    if (plan, regime) in _cache:
        return _cache[plan, regime]
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from modaltune_amd import ops
    c = R.make_case(plan, regime)
    g = R.Case()
    g.c = c
    nb, M = len(c.bt), c.M
    p = ops.make_plan(c.bt, c.N, c.B, qlimit=c.qlimit)
    qkv, dmixed, lse_tot, delta = (t.to(DEV).contiguous() for t in (c.qkv, c.dmixed, c.lse_tot, c.delta))
    halves = ops.dilated_attn_bwd_workspace_bytes(p) // 2
    g.off = [0]
    for br in c.bt:
        g.off.append(g.off[-1] + M * 3 * (H // br.ratio) * HD)
    assert g.off[-1] == halves
    phases = ops.ATTN_BWD_KV | ops.ATTN_BWD_Q
    ws, dqkv = _nan16(halves), _nan16(M, 2304)
    ops.dilated_attn_bwd_phases(qkv, dmixed, lse_tot, delta, p, ws, dqkv, phases)
    ws_i, dqkv_i = _nan16(halves), _nan16(M, 2304)
    ops.dilated_attn_bwd_inplace_phases(qkv, dmixed, lse_tot, delta, p, ws_i, dqkv_i, phases)
    o_br = _nan16(nb, M, R.DM)
    lse_br = torch.full((nb, M, H), float("nan"), device=DEV)
    ops.dilated_attn_fwd(qkv, p, o_br, lse_br)
    torch.cuda.synchronize()
    g.ws, g.dqkv, g.ws_i, g.dqkv_i = ws.cpu(), dqkv.cpu(), ws_i.cpu(), dqkv_i.cpu()
    g.o_br, g.lse_br = o_br.cpu().view(nb, M, H, HD), lse_br.cpu()
    g.db = max(i for i, br in enumerate(c.bt) if br.ratio == 1)
    _cache[plan, regime] = g
    return g


def _regions(g, ws):
    return [ws[g.off[b]:g.off[b + 1]].view(g.c.M, 3, H // br.ratio, HD) for b, br in enumerate(g.c.bt)]


def _report(tag, errors, c):
    for (b, q), (e, at) in sorted(errors.items()):
        print(f"{tag} {c.plan} {c.regime} branch {b} (ratio {c.bt[b].ratio}) {q}: {e:.3e} at (pass, segment, head) = {at}")


@pytest.mark.parametrize("plan,regime", CASES)
def test_backward_workspace_regions_per_sequence(plan, regime):
    """dK / dV / dQ' of every branch, as the two kernels leave them in the workspace, against float64 per sequence."""
    g = _run(plan, regime)
    c = g.c
    got = _regions(g, g.ws)
    errors = R.bwd_errors(got, c.ref, c.geoms)
    _report("bwd", errors, c)
    assert torch.isnan(g.dqkv).all()                                   # no combine ran: dqkv keeps its pre-fill
    for b, gm in enumerate(c.geoms):                                   # finite exactly where a sequence has an entry
        assert torch.isfinite(got[b][:, 1:]).all(), f"branch {b}: dk / dv"
        fin = torch.isfinite(got[b][:, 0]).all(-1)
        assert bool(fin[gm.is_query].all()), f"branch {b}: dq"
        if c.qlimit is None:
            assert bool(gm.is_query.all())
    R.check(errors, R.BARS, f"{plan} {regime}")


@pytest.mark.parametrize("plan,regime", CASES)
def test_backward_inplace_dense_branch_per_sequence(plan, regime):
    """The in-place form: the dense branch goes straight into dqkv (its region of the workspace stays untouched), the sparse branches
    into the workspace as before -- the same values, and the dense branch in dqkv against float64 per sequence."""
    g = _run(plan, regime)
    c = g.c
    db, gm = g.db, c.geoms[g.db]
    dense = g.dqkv_i.view(c.M, 3, H, HD)
    errors = {(db, q): R.worst(R.seq_errors(dense[:, w], c.ref[db][:, w], gm, gm.is_query if w == 0 else None), gm)
              for w, q in enumerate(R.QUANTITIES)}
    _report("inplace", errors, c)
    assert torch.isnan(g.ws_i[g.off[db]:g.off[db + 1]]).all()
    assert torch.isfinite(dense[:, 1:]).all()
    assert bool(torch.isfinite(dense[:, 0]).all(-1)[gm.is_query].all())
    for b in range(len(c.bt)):
        if b != db:
            assert torch.equal(g.ws_i[g.off[b]:g.off[b + 1]].view(torch.int16), g.ws[g.off[b]:g.off[b + 1]].view(torch.int16))
    R.check(errors, R.BARS, f"{plan} {regime} in place")


@pytest.mark.parametrize("plan,regime", CASES)
def test_forward_branch_outputs_per_sequence(plan, regime):
    """o_br / lse_br of every branch against the oracle's branch outputs per sequence; (row, head) pairs that are no query of a branch
    (heads of other groups; with qlimit the rows past it) keep the pre-fill."""
    g = _run(plan, regime)
    c = g.c
    errors = R.fwd_errors(g.o_br, g.lse_br, c.o_ref, c.lse_ref, c.geoms)
    _report("fwd", errors, c)
    for b, gm in enumerate(c.geoms):
        query = torch.zeros(c.M, H, dtype=torch.bool).scatter_(1, gm.heads, gm.is_query)
        assert c.qlimit is not None or torch.equal(query, c.cov[b])       # (the oracle visits the same pairs)
        assert torch.equal(torch.isfinite(g.lse_br[b]), query), f"branch {b}: lse_br written exactly at the branch's queries"
        assert torch.equal(torch.isfinite(g.o_br[b]).all(-1), query) and torch.equal(torch.isnan(g.o_br[b]).all(-1), ~query), f"branch {b}"
    R.check(errors, R.BARS, f"{plan} {regime} forward")
