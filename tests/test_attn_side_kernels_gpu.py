"""GPU: the memory-bound side kernels of the dilated attention -- branch mix + inner LayerNorm (forward, backward) and the backward's
combine -- and the in-place form of the backward (dense branch written straight into dqkv, the combine adds the sparse branches only)
against the workspace form, a torch restatement of the sum, and fp64.

Shapes: B = 2, N = 333 with a small segment table (every branch but the last has several segments, N is a multiple of no segment
length, every (branch, residue) pair occurs) and B = 2, N = 1203 with the shipped table (two 1024-segments in the dense branch).  Both
have an even number of rows (666, 2406), so a third case, B = 3 with the small table (999 rows), is the one whose last row pair of the
mix kernels is half-live.  Two more plans move the dense branch: ratios (2, 1, 4) put it at index 1 (its workspace region starts at
a non-zero offset, and the combine adds it between two sparse branches), and a six-branch plan runs the kernels' instantiations for
more than five branches.  A plan with no ratio-1 branch has nothing to write in place: both entries must then do the same."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from modaltune_amd.config import branch_table, segment_lengths  # noqa: E402

DEV = "cuda"
RATIOS = (1, 2, 4, 8, 16)
SMALL = (48, 80, 144, 272, 333)
CASES = {"small": (2, 333, SMALL, RATIOS), "shipped": (2, 1203, None, RATIOS), "small_odd": (3, 333, SMALL, RATIOS),
         "dense_mid": (2, 333, (48, 80, 144), (2, 1, 4)), "six": (2, 333, SMALL + (112,), RATIOS + (2,))}
H, HD, DM = 16, 48, 768
QK = 0.14433756729740643 * 1.4426950408889634


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _nan16(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float16, device=DEV)


def _bits(t):
    return t.view(torch.int16)


class Case:
    pass


_cache = {}


def _case(name):
    """Everything the tests of one shape share, computed once and left unchanged."""
    if name in _cache:
        return _cache[name]
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from modaltune_amd import ops
    B, N, segs, ratios = CASES[name]
    segs = list(segs) if segs else segment_lengths()
    c = Case()
    c.ops, c.B, c.N, c.M = ops, B, N, B * N
    M = c.M
    c.bt = branch_table(N, segs, ratios)
    c.plan = ops.make_plan(c.bt, N, B)
    nb = len(c.bt)
    c.db = max(i for i, b in enumerate(c.bt) if b.ratio == 1)      # the dense branch
    g = torch.Generator().manual_seed(1234 + N)
    qkv = (torch.randn(M, 2304, generator=g) * 0.7)
    qkv[:, :768] *= QK
    c.qkv = qkv.half().to(DEV).view(M, 3, H, HD).permute(1, 2, 0, 3).contiguous()      # head-major
    c.ln_w = (1 + 0.1 * torch.randn(DM, generator=g)).to(DEV)
    c.ln_b = (0.1 * torch.randn(DM, generator=g)).to(DEV)
    c.dy = (torch.randn(M, DM, generator=g) * 0.1).half().to(DEV)
    c.o_br = torch.zeros(nb, M, DM, dtype=torch.float16, device=DEV)
    c.lse_br = torch.zeros(nb, M, H, device=DEV)
    ops.dilated_attn_fwd(c.qkv, c.plan, c.o_br, c.lse_br)
    # cov[b][m, h]: branch b visits (row, head) -- head group h // (16 / r) is the position's residue inside its segment
    pos = torch.arange(M, device=DEV) % N
    heads = torch.arange(H, device=DEV)
    c.res = [(pos % b.seg) % b.ratio for b in c.bt]
    c.cov = torch.stack([(heads[None, :] // (H // b.ratio)) == r[:, None] for b, r in zip(c.bt, c.res)])      # [nb, M, H]

    def mix_fwd(grid):
        y = _nan16(M, DM)
        stats = torch.full((M, 2), float("nan"), device=DEV)
        lse_tot = torch.full((M, H), float("nan"), device=DEV)
        ops.dilated_mix_ln_fwd_grid(c.o_br, c.lse_br, c.plan, c.ln_w, c.ln_b, y, stats, lse_tot, grid)
        return y, stats, lse_tot
    c.mix_fwd = mix_fwd
    c.y, c.stats, c.lse_tot = mix_fwd(0)

    def mix_bwd(grid):
        dmixed = _nan16(H, M, HD)
        delta = torch.zeros(nb, M, H, device=DEV)      # (entries of branches that do not visit a (row, head) are left alone)
        ops.dilated_mix_ln_bwd_grid(c.dy, c.o_br, c.lse_br, c.lse_tot, c.plan, c.ln_w, c.stats, dmixed, delta, grid)
        return dmixed, delta
    c.mix_bwd = mix_bwd
    c.dmixed, c.delta = mix_bwd(0)

    # attention backward, both forms, outputs and workspaces pre-filled with NaN patterns
    c.ws_halves = ops.dilated_attn_bwd_workspace_bytes(c.plan) // 2
    c.ws_off = [0]
    for b in c.bt:
        c.ws_off.append(c.ws_off[-1] + M * 3 * (H // b.ratio) * HD)
    assert c.ws_off[-1] == c.ws_halves
    c.dqkv_w, c.ws_w = _nan16(M, 2304), _nan16(c.ws_halves)
    ops.dilated_attn_bwd_phases(c.qkv, c.dmixed, c.lse_tot, c.delta, c.plan, c.ws_w, c.dqkv_w, ops.ATTN_BWD_ALL)
    c.dqkv_i, c.ws_i = _nan16(M, 2304), _nan16(c.ws_halves)
    ops.dilated_attn_bwd_inplace_phases(c.qkv, c.dmixed, c.lse_tot, c.delta, c.plan, c.ws_i, c.dqkv_i, ops.ATTN_BWD_ALL)
    # the dense branch alone, as the two kernels leave it in dqkv before the in-place combine
    c.dense, ws_d = _nan16(M, 2304), _nan16(c.ws_halves)
    ops.dilated_attn_bwd_inplace_phases(c.qkv, c.dmixed, c.lse_tot, c.delta, c.plan, ws_d, c.dense, ops.ATTN_BWD_KV | ops.ATTN_BWD_Q)
    torch.cuda.synchronize()
    _cache[name] = c
    return c


def _sparse_full(c, i):
    """Branch i's compact workspace region of the in-place run spread over the dense layout: ([M, 3, 16, 48] values, [M, 16] mask)."""
    b = c.bt[i]
    hb = H // b.ratio
    comp = c.ws_i[c.ws_off[i]:c.ws_off[i + 1]].view(c.M, 3, hb, HD)
    idx = c.res[i][:, None] * hb + torch.arange(hb, device=DEV)[None, :]                 # [M, hb] heads of the covering group
    full = torch.zeros(c.M, 3, H, HD, dtype=torch.float16, device=DEV)
    full.scatter_(2, idx[:, None, :, None].expand(c.M, 3, hb, HD), comp)
    return full, c.cov[i]


@pytest.mark.parametrize("name", list(CASES))
def test_inplace_form_equals_workspace_form(name):
    c = _case(name)
    assert torch.isfinite(c.dqkv_w).all() and torch.isfinite(c.dqkv_i).all()      # nothing left untouched, nothing added to a NaN
    assert torch.equal(c.dqkv_i, c.dqkv_w)
    lo, hi = c.ws_off[c.db], c.ws_off[c.db + 1]                                   # the dense region of the workspace
    assert hi - lo == c.dense.numel()
    for a, b in ((0, lo), (hi, c.ws_halves)):                                     # the sparse regions, bit for bit
        assert torch.equal(_bits(c.ws_i[a:b]), _bits(c.ws_w[a:b]))
    assert torch.isfinite(c.ws_w[lo:hi]).all()
    assert torch.isnan(c.ws_i[lo:hi]).all()                                       # the in-place form leaves the dense region alone
    assert torch.isfinite(c.dense).all()                                          # the dense branch covers every (row, which, head)
    assert torch.equal(c.dense.view(-1), c.ws_w[lo:hi])                           # ... and is what the workspace form puts in its region


@pytest.mark.parametrize("name", list(CASES))
def test_inplace_combine_sums_dense_plus_covering_sparse_branches(name):
    c = _case(name)
    acc32 = torch.zeros(c.M, 3, H, HD, device=DEV)                                # from +0, as the kernels
    acc64 = acc32.double()
    anyc = torch.zeros(c.M, H, dtype=torch.bool, device=DEV)
    for i in range(len(c.bt)):                                                    # ascending branch index, the dense value at its own
        if i == c.db:
            acc32 = acc32 + c.dense.float().view(c.M, 3, H, HD)
            acc64 = acc64 + c.dense.double().view(c.M, 3, H, HD)
            continue
        full, cov = _sparse_full(c, i)
        m = cov[:, None, :, None]
        acc32 = torch.where(m, acc32 + full.float(), acc32)
        acc64 = torch.where(m, acc64 + full.double(), acc64)
        anyc |= cov
    frac = float(anyc.float().mean())
    print(f"{name}: (row, head) covered by a sparse branch: {frac:.4f}")
    assert 0.3 < frac < 0.9                                                       # both kinds of entry occur
    want = torch.where(anyc[:, None, :, None], acc32.half(), c.dense.view(c.M, 3, H, HD)).view(c.M, 2304)
    assert torch.equal(c.dqkv_i, want)
    # against the fp64 sum: one rounding of a sum whose fp32 partial sums are exact to well below half an fp16 ulp
    a = acc64.abs().clamp(min=2.0 ** -14)
    ulp = torch.pow(2.0, torch.floor(torch.log2(a)) - 10)
    err = ((c.dqkv_i.double().view(c.M, 3, H, HD) - acc64).abs() / ulp).max()
    print(f"{name}: in-place combine against the fp64 sum: {float(err):.3f} fp16 ulp")
    assert float(err) <= 1.0


def _mix_reference(c):
    """fp64 restatement of branch mix + LayerNorm and their backward from the SAME fp16 branch outputs / fp32 LSEs the kernels read."""
    o = c.o_br.double().view(len(c.bt), c.M, H, HD)
    lse = torch.where(c.cov, c.lse_br.double(), torch.full_like(c.lse_br, float("-inf"), dtype=torch.float64))
    tot = torch.logsumexp(lse, dim=0)                                             # [M, H]
    wgt = torch.exp(lse - tot[None])                                              # 0 where a branch does not visit
    mixed = (wgt[..., None] * torch.where(c.cov[..., None], o, torch.zeros_like(o))).sum(0).view(c.M, DM).requires_grad_(True)
    y = torch.nn.functional.layer_norm(mixed, (DM,), c.ln_w.double(), c.ln_b.double(), 1e-5)
    y.backward(c.dy.double())
    dmixed = mixed.grad.view(c.M, H, HD)
    delta = (dmixed[None] * o).sum(-1)                                            # [nb, M, H]
    return tot, y.detach(), dmixed, torch.where(c.cov, delta, torch.zeros_like(delta))


@pytest.mark.parametrize("name", list(CASES))
def test_mix_kernels_vs_fp64(name):
    c = _case(name)
    tot, y, dmixed, delta = _mix_reference(c)
    r_y = rel(c.y, y)
    e_tot = float((c.lse_tot.double() - tot).abs().max())
    got_dm = c.dmixed.view(H, c.M, HD).permute(1, 0, 2)
    r_dm, r_dl = rel(got_dm, dmixed), rel(c.delta, delta)
    print(f"{name}: y {r_y:.2e} lse_tot {e_tot:.2e} dmixed {r_dm:.2e} delta {r_dl:.2e}")
    assert torch.isfinite(c.y).all() and torch.isfinite(c.dmixed).all() and torch.isfinite(c.stats).all()
    assert r_y < 4e-3                  # bars of test_dilated_attention_fwd_mix_vs_reference_golden
    assert e_tot < 2e-3
    assert r_dm < 2e-2                 # bar of test_dilated_attention_bwd_vs_oracle_autograd
    assert r_dl < 2e-2


@pytest.mark.parametrize("grid", [1, 7])
@pytest.mark.parametrize("name", list(CASES))
def test_mix_kernels_do_not_depend_on_the_grid(name, grid):
    """One workgroup (a wave walks every fourth row pair to the end of the rows) and a grid that does not divide the rows give the
    bits of the default launch, in which at these sizes every wave handles one pair."""
    c = _case(name)
    y, stats, lse_tot = c.mix_fwd(grid)
    dmixed, delta = c.mix_bwd(grid)
    torch.cuda.synchronize()
    for got, want in ((y, c.y), (stats, c.stats), (lse_tot, c.lse_tot), (dmixed, c.dmixed), (delta, c.delta)):
        assert torch.isfinite(got).all()
        assert torch.equal(got, want)


def test_plan_without_dense_branch_takes_workspace_form():
    """No ratio-1 branch: nothing can be written in place, so the in-place entry runs the workspace form -- same dqkv, same
    workspace, bit for bit (NaN pre-fill included where nothing is written).  The inputs are made with torch: the mix kernels are
    not the subject here, and with this plan half of the (row, head) entries are visited by no branch."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from modaltune_amd import ops
    B, N = 2, 333
    M = B * N
    bt = branch_table(N, [48, 80], (2, 4))
    plan = ops.make_plan(bt, N, B)
    g = torch.Generator().manual_seed(77)
    qkv = torch.randn(M, 2304, generator=g) * 0.7
    qkv[:, :768] *= QK
    qkv = qkv.half().to(DEV).view(M, 3, H, HD).permute(1, 2, 0, 3).contiguous()
    o_br = torch.zeros(len(bt), M, DM, dtype=torch.float16, device=DEV)
    lse_br = torch.zeros(len(bt), M, H, device=DEV)
    ops.dilated_attn_fwd(qkv, plan, o_br, lse_br)
    pos = torch.arange(M, device=DEV) % N
    heads = torch.arange(H, device=DEV)
    cov = torch.stack([(heads[None, :] // (H // b.ratio)) == ((pos % b.seg) % b.ratio)[:, None] for b in bt])
    lse_tot = torch.logsumexp(torch.where(cov, lse_br, torch.full_like(lse_br, float("-inf"))), dim=0)
    lse_tot = torch.where(cov.any(0), lse_tot, torch.zeros_like(lse_tot)).contiguous()
    dmixed = (torch.randn(H, M, HD, generator=g) * 0.1).half().to(DEV)
    delta = (torch.randn(len(bt), M, H, generator=g) * 0.01).to(DEV)
    n = ops.dilated_attn_bwd_workspace_bytes(plan) // 2
    dqkv_w, ws_w, dqkv_i, ws_i = _nan16(M, 2304), _nan16(n), _nan16(M, 2304), _nan16(n)
    ops.dilated_attn_bwd_phases(qkv, dmixed, lse_tot, delta, plan, ws_w, dqkv_w, ops.ATTN_BWD_ALL)
    ops.dilated_attn_bwd_inplace_phases(qkv, dmixed, lse_tot, delta, plan, ws_i, dqkv_i, ops.ATTN_BWD_ALL)
    torch.cuda.synchronize()
    assert torch.isfinite(dqkv_w).all() and torch.isfinite(ws_w).all()
    assert torch.equal(_bits(dqkv_i), _bits(dqkv_w))
    assert torch.equal(_bits(ws_i), _bits(ws_w))
