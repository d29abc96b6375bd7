"""Helper (not a test module): the dilated attention per branch and per sparse sequence, in float64, at the kernels' tile edges.

A sparse sequence is one (branch, pass, segment, head): head h of a branch with dilation r belongs to head group g = h // (16 / r) and
walks, inside the segment, the rows seg_base + g + i r for i < nvalid (csrc/attn_common.h: Seq::nvalid; the entries nvalid .. n are
zero padding).  Everything here works FROM EXACTLY THE TENSORS THE KERNELS READ -- fp16 head-major q' | k | v with
q' = MT_QK_SCALE_LOG2 q, fp16 head-major dmixed, fp32 lse_tot, fp32 delta_br -- and evaluates the formula of
include/modaltune_hip.h (mt_dilated_attn_bwd):

    P~[i,k] = exp2(q'_i . k_k - lse_tot[row_i, h] log2 e)        dP[i,k] = dmixed[h, row_i] . v_k        dS = P~ (dP - delta[b, row_i, h])
    dV_k = sum_i P~[i,k] dmixed_i        dK_k = ln 2 sum_i dS[i,k] q'_i        dQ'_i = ln 2 sum_k dS[i,k] k_k

with the queries i < min(nvalid, qlimit) and the keys k < nvalid (padded entries are neither in the backward).  Results come in the
compact workspace layout of the kernels, per branch [M, 3 = dq | dk | dv, 16 / r, 48] with the heads of the row's covering group
(tests/test_attn_side_kernels_gpu.py: _sparse_full), next to a Geom that maps every (row, head-in-group) to its sequence.

* bwd_reference(..., staged=False): the formula in float64.
* bwd_reference(..., staged=True): the same with the roundings the kernels stage their MFMA operands and results through: P' = ln 2 P~
  and dS' = P' (dP - delta) to fp16 before the second product (dV = P'^T dmixed / ln 2, dK = dS'^T q', dQ' = dS' k), the three results to
  fp16.  Everything else stays float64: no fp32 accumulation order, no hardware exp2.  Its distance from the float64 formula is the
  rounding floor of the method.
* fwd_staged: the forward the same way (P = exp2(s' - max) to fp16 before P V and before the row sum, O to fp16, the LSE to fp32).
* seq_errors / worst: the metric -- for every sequence max|got - ref| / max|ref| over its [nvalid, 48] slab (the LSE: max|got - ref|,
  the absolute error the existing tests bound), exact zeros where the reference is all zero; worst() names the sequence.
* make_case(plan, regime): the inputs, the oracle's branch outputs and the references of one test case, computed once.
* BARS: 4 x the rounding floor, the worst staged-against-float64 error over every plan and regime (test_attn_edges_cpu re-derives it)."""
import functools

import torch

from modaltune_amd.config import branch_table, segment_lengths

H, HD, DM = 16, 48, 768
QK = 0.14433756729740643 * 1.4426950408889634      # MT_QK_SCALE_LOG2
LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453
RATIOS = (1, 2, 4, 8, 16)

# name -> (B, N, segment table (None = the shipped one), ratios, qlimit)
PLANS = {
    "n385": (2, 385, None, RATIOS, None),
    "n1023": (1, 1023, None, RATIOS, None),
    "n1025": (1, 1025, None, RATIOS, None),
    "tail3": (2, 259, (64, 128, 256, 256, 256), RATIOS, None),
    "qlim": (2, 257, (257, 257, 257), (1, 2, 4), (64, 65, 33)),
}
# name -> (standard deviation of q and k: the logits q.k / sqrt(48) then have standard deviation sd^2, planted pairs)
REGIMES = {"soft": (0.5 ** 0.5, False), "peaked": (3.0 ** 0.5, True)}
# dmixed of spread 1: dS' = ln 2 P~ (dP - delta) is staged in fp16, and the one-row dense segment of n1025 has P~ of about 3e-4 (one
# real key among 1023 padded ones): at a spread of 0.1 its dS' is subnormal in fp16 and the sequence's dq / dk are rounding (6e-3,
# 1.4e-2 in the emulation) whatever the kernel does.  The per-sequence metric is scale-free in dmixed otherwise.
DMIXED_SD = 1.0
PLANT_GAIN = 4.0      # k[key] = 4 q[query]: a logit of 4 |q_h|^2 / sqrt(48), about 80 at this scale, against a spread of 3

QUANTITIES = ("dq", "dk", "dv")
# 4 x the rounding floors (worst per-sequence error of the staged emulation against float64 over PLANS x REGIMES), written once;
# tests/test_attn_edges_cpu.py::test_bars_are_four_times_the_rounding_floor recomputes the floors and holds these within [3x, 5x].
BARS = {"dq": 3.1e-3, "dk": 5.5e-3, "dv": 3.2e-3, "o": 2.6e-3, "lse": 8.1e-4}


def nvalid(br, N, j, g):
    """Real entries of the sparse sequence of segment j, head group g (csrc/attn_common.h: Seq::nvalid)."""
    lim = min(br.seg, N - j * br.seg) - g
    return 0 if lim <= 0 else min(br.n, -(-lim // br.ratio))


def edge_table(bt, N):
    """{(branch, segment, head group): nvalid}."""
    return {(b, j, g): nvalid(br, N, j, g) for b, br in enumerate(bt) for j in range(br.nseg) for g in range(br.ratio)}


class Geom:
    """One branch: seq_id [M, hb] (row, head-in-group) -> sequence number (pass nseg + segment) 16 + head; sidx [M] the row's index i
    inside its sequences; heads [M, hb] the heads of the row's covering group; nv / nq [S] real entries / queries per sequence."""

    def __init__(self, br, N, B, qlimit=0):
        self.br, self.N, self.B, self.hb = br, N, B, H // br.ratio
        M = B * N
        pos = torch.arange(M) % N
        loc = pos % br.seg
        self.res = loc % br.ratio
        self.sidx = loc // br.ratio
        self.heads = self.res[:, None] * self.hb + torch.arange(self.hb)[None, :]
        self.seq_id = ((torch.arange(M) // N) * br.nseg + pos // br.seg)[:, None] * H + self.heads
        self.nseq = B * br.nseg * H
        self.nv = torch.tensor([nvalid(br, N, j, h // self.hb) for _ in range(B) for j in range(br.nseg) for h in range(H)])
        self.nq = torch.clamp(self.nv, max=qlimit if qlimit else br.n)
        self.is_query = self.sidx[:, None] < self.nq[self.seq_id]                      # [M, hb]

    def name(self, s):
        """(pass, segment, head) of sequence number s."""
        return (s // (self.br.nseg * H), (s // H) % self.br.nseg, s % H)

    def number(self, p, j, h):
        return (p * self.br.nseg + j) * H + h

    def rows(self, p, j, g, shift=0):
        """Token rows of the entries i < nvalid of (pass, segment, head group); shift: the residue moved by that much (a mutation:
        rows past the end of the pass are clamped the way Seq::row_clamped clamps them)."""
        n = nvalid(self.br, self.N, j, g)
        r = p * self.N + j * self.br.seg + (g + shift) % self.br.ratio + torch.arange(n) * self.br.ratio
        return torch.clamp(r, max=(p + 1) * self.N - 1)


def geometry(bt, N, B, qlimit=None):
    return [Geom(br, N, B, qlimit[b] if qlimit else 0) for b, br in enumerate(bt)]


def _r16(t):
    return t.to(torch.float16).to(torch.float64)


def _chunks(hb, nv):
    step = max(1, min(hb, (1 << 22) // max(1, nv * nv)))      # at most 4 M scores (32 MB of float64) per temporary
    return [(a, min(hb, a + step)) for a in range(0, hb, step)]


MUTATIONS = ("drop_last_key", "neighbour_delta", "residue_shift", "skip_query_tile_2")


def bwd_reference(qkv, dmixed, lse_tot, delta_br, bt, N, B, qlimit=None, staged=False, mutate=None, branches=None):
    """qkv [3, 16, M, 48], dmixed [16, M, 48], lse_tot [M, 16], delta_br [nb, M, 16] (any float dtype: read as they are, in float64)
    -> per branch a float64 [M, 3, 16 / ratio, 48] (zeros where nothing is defined: dq of the rows that are no queries).
    mutate: {(branch, pass, segment, head): one of MUTATIONS} -- that sequence is computed WRONG in the named way (what a kernel with
    that defect would leave in the sequence's slots); for tests of the metric only.  branches: compute only these (None elsewhere)."""
    qkv, dmixed = qkv.detach().cpu().double(), dmixed.detach().cpu().double()
    lse_tot, delta_br = lse_tot.detach().cpu().double(), delta_br.detach().cpu().double()
    mutate = mutate or {}
    out = []
    for b, (br, gm) in enumerate(zip(bt, geometry(bt, N, B, qlimit))):
        hb = gm.hb
        if branches is not None and b not in branches:
            out.append(None)
            continue
        comp = torch.zeros(B * N, 3, hb, HD, dtype=torch.float64)
        one_by_one = any(k[0] == b for k in mutate)
        for p in range(B):
            for j in range(br.nseg):
                for g in range(br.ratio):
                    nv = nvalid(br, N, j, g)
                    if nv == 0:
                        continue
                    rows = gm.rows(p, j, g)
                    nq = int(gm.nq[gm.number(p, j, g * hb)])
                    for a, e in ([(x, x + 1) for x in range(hb)] if one_by_one else _chunks(hb, nv)):
                        hs = torch.arange(g * hb + a, g * hb + e)
                        mut = mutate.get((b, p, j, g * hb + a)) if one_by_one else None
                        dq, dk, dv = _sequence_bwd(qkv, dmixed, lse_tot, delta_br[b], gm, p, j, g, hs, rows, nq, staged, mut)
                        comp[rows[:nq], 0, a:e] = dq.transpose(0, 1)
                        comp[rows, 1, a:e] = dk.transpose(0, 1)
                        comp[rows, 2, a:e] = dv.transpose(0, 1)
        out.append(comp)
    return out


def _sequence_bwd(qkv, dmixed, lse_tot, delta, gm, p, j, g, hs, rows, nq, staged, mut):
    """The sequences (pass p, segment j, heads hs of group g) -> dq [G, nq, 48], dk, dv [G, nv, 48]."""
    src = gm.rows(p, j, g, shift=1) if mut == "residue_shift" else rows      # where the inputs are read
    hx = hs[:, None]
    qp, k, v, do = qkv[0][hx, src[None, :nq]], qkv[1][hx, src[None]], qkv[2][hx, src[None]], dmixed[hx, src[None, :nq]]
    lt = lse_tot[src[:nq]][:, hs].transpose(0, 1)                                                   # [G, nq]
    dl = delta[src[:nq]][:, hs ^ 1 if mut == "neighbour_delta" else hs].transpose(0, 1)
    nv = rows.numel()
    nk = nv - 1 if mut == "drop_last_key" else nv                                                    # keys [0, nk)
    pt = torch.exp2(qp @ k[:, :nk].transpose(1, 2) - lt[..., None] * LOG2E)                          # P~ [G, nq, nk]
    dsc = pt * (do @ v[:, :nk].transpose(1, 2) - dl[..., None])                                      # dS
    if staged:
        pt, dsc = _r16(pt * LN2) / LN2, _r16(dsc * LN2) / LN2
    dq = (dsc @ k[:, :nk]) * LN2
    keep = torch.ones(nq, dtype=torch.float64)
    if mut == "skip_query_tile_2":
        keep[64:128] = 0.0                                                                            # (dK / dV kernel: queries 64 .. 127)
    dk = ((dsc * keep[None, :, None]).transpose(1, 2) @ qp) * LN2
    dv = (pt * keep[None, :, None]).transpose(1, 2) @ do
    if nk < nv:                                                                                       # the dropped key gets nothing
        z = torch.zeros(hs.numel(), nv - nk, HD, dtype=torch.float64)
        dk, dv = torch.cat([dk, z], 1), torch.cat([dv, z], 1)
    if staged:
        dq, dk, dv = _r16(dq), _r16(dk), _r16(dv)
    return dq, dk, dv


def fwd_staged(qkv, bt, N, B, qlimit=None):
    """The forward with the kernel's roundings and nothing else of it: per sequence s' = q' . k over the real keys, the n - nvalid
    padded keys at logit 0 and value 0, P = exp2(s' - max) to fp16 before P V and before the row sum, O = P V / sum to fp16, the LSE
    to fp32.  -> per branch (o [M, hb, 48], lse [M, hb]) in the compact layout, float64, zeros where a row is no query."""
    qkv = qkv.detach().cpu().double()
    out = []
    for br, gm in zip(bt, geometry(bt, N, B, qlimit)):
        hb = gm.hb
        o, lse = torch.zeros(B * N, hb, HD, dtype=torch.float64), torch.zeros(B * N, hb, dtype=torch.float64)
        for p in range(B):
            for j in range(br.nseg):
                for g in range(br.ratio):
                    nv = nvalid(br, N, j, g)
                    if nv == 0:
                        continue
                    rows = gm.rows(p, j, g)
                    nq = int(gm.nq[gm.number(p, j, g * hb)])
                    for a, e in _chunks(hb, nv):
                        hx = torch.arange(g * hb + a, g * hb + e)[:, None]
                        s = qkv[0][hx, rows[None, :nq]] @ qkv[1][hx, rows[None]].transpose(1, 2)      # [G, nq, nv], log2 units
                        m = s.max(-1).values
                        if br.n > nv:
                            m = m.clamp(min=0.0)
                        pr = _r16(torch.exp2(s - m[..., None]))
                        l = pr.sum(-1) + (br.n - nv) * torch.exp2(-m)
                        o[rows[:nq], a:e] = _r16((pr @ qkv[2][hx, rows[None]]) / l[..., None]).transpose(0, 1)
                        lse[rows[:nq], a:e] = ((m + torch.log2(l)) * LN2).float().double().transpose(0, 1)
        out.append((o, lse))
    return out


# ------------------------------------------------------------------------------------------------ the metric
def seq_errors(got, ref, gm, mask=None, absolute=False):
    """got, ref [M, hb, ...] (trailing dimensions: the sequence's slab per row), mask [M, hb] or None (entries outside it are not
    compared, whatever they hold) -> float64 [S]: per sequence max|got - ref| / max|ref| (absolute: max|got - ref|); a sequence whose
    reference is all zero gives 0 when got is all zero too and inf otherwise; nan where a sequence has no entry."""
    got, ref = got.detach().cpu().double().reshape(*ref.shape[:2], -1), ref.detach().cpu().double().reshape(*ref.shape[:2], -1)
    diff = (got - ref).abs().amax(-1)
    diff = torch.where(torch.isnan(diff), torch.full_like(diff, float("inf")), diff)      # a NaN where a value belongs is a miss
    mag = ref.abs().amax(-1)
    live = torch.ones_like(gm.seq_id, dtype=torch.bool) if mask is None else mask
    idx = gm.seq_id[live]
    num = torch.zeros(gm.nseq, dtype=torch.float64).scatter_reduce_(0, idx, diff[live], "amax", include_self=True)
    den = torch.zeros(gm.nseq, dtype=torch.float64).scatter_reduce_(0, idx, mag[live], "amax", include_self=True)
    cnt = torch.zeros(gm.nseq, dtype=torch.float64).scatter_reduce_(0, idx, torch.ones(idx.numel(), dtype=torch.float64), "sum")
    if absolute:
        err = num
    else:
        err = torch.where(den > 0, num / den.clamp(min=1e-300), torch.where(num > 0, torch.full_like(num, float("inf")), num))
    return torch.where(cnt > 0, err, torch.full_like(err, float("nan")))


def worst(err, gm):
    """(worst error, (pass, segment, head)) of a seq_errors() result."""
    e = torch.where(torch.isnan(err), torch.full_like(err, -1.0), err)
    s = int(e.argmax())
    return float(e[s]), gm.name(s)


def bwd_errors(got, ref, geoms):
    """got, ref: per branch [M, 3, hb, 48] -> {(branch, "dq" | "dk" | "dv"): (worst per-sequence error, (pass, segment, head))}; dq
    only over the rows that are queries."""
    res = {}
    for b, gm in enumerate(geoms):
        for w, name in enumerate(QUANTITIES):
            res[b, name] = worst(seq_errors(got[b][:, w], ref[b][:, w], gm, gm.is_query if w == 0 else None), gm)
    return res


def fwd_errors(got_o, got_lse, ref_o, ref_lse, geoms):
    """got_o / ref_o: per branch [M, 16, 48] dense, got_lse / ref_lse [M, 16] -> {(branch, "o" | "lse"): (worst, (pass, segment, head))}
    over the (row, head) pairs that are queries of the branch."""
    res = {}
    for b, gm in enumerate(geoms):
        go, ro = (compact(t[b], gm) for t in (got_o, ref_o))
        gl, rl = (compact(t[b], gm) for t in (got_lse, ref_lse))
        res[b, "o"] = worst(seq_errors(go, ro, gm, gm.is_query), gm)
        res[b, "lse"] = worst(seq_errors(gl[..., None], rl[..., None], gm, gm.is_query, absolute=True), gm)
    return res


def compact(dense, gm):
    """dense [M, 16, ...] -> [M, hb, ...]: the heads of every row's covering group."""
    dense = dense.detach().cpu()
    idx = gm.heads.reshape(*gm.heads.shape, *([1] * (dense.dim() - 2))).expand(*gm.heads.shape, *dense.shape[2:])
    return dense.gather(1, idx)


def spread(comp, gm):
    """[M, 3, hb, 48] compact -> [M, 3, 16, 48] dense, zeros at the heads the branch does not visit."""
    full = torch.zeros(comp.shape[0], 3, H, HD, dtype=comp.dtype)
    return full.scatter_(2, gm.heads[:, None, :, None].expand(comp.shape[0], 3, gm.hb, HD), comp)


def check(errors, bars, what):
    """Assert every (branch, quantity) of an errors dict under its bar; the message names the failing sequences."""
    bad = [f"{what}: branch {b} {q}: {e:.3e} >= {bars[q]:.3e} at (pass, segment, head) = {at}"
           for (b, q), (e, at) in sorted(errors.items()) if not e < bars[q]]
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ the cases
class Case:
    pass


@functools.lru_cache(maxsize=None)
def make_case(plan, regime):
    """Inputs and references of one (plan, regime), computed once and left unchanged: the fp16 tensors the kernels read, the oracle's
    float64 branch outputs from those same rounded inputs, lse_tot and delta_br rounded to fp32, and both backward references."""
    from oracle import modaltune_oracle as O
    c = Case()
    c.plan, c.regime = plan, regime
    c.B, c.N, segs, c.ratios, c.qlimit = PLANS[plan]
    c.segs = list(segs) if segs else segment_lengths()
    c.M = M = c.B * c.N
    c.bt = branch_table(c.N, c.segs, c.ratios)
    c.geoms = geometry(c.bt, c.N, c.B, c.qlimit)
    sd, plant = REGIMES[regime]
    gen = torch.Generator().manual_seed(7919 * list(PLANS).index(plan) + list(REGIMES).index(regime) + 1)
    # Rows of a sequence that is mostly padding (fewer real entries than padded ones: the ragged last segments) keep the soft scale in
    # every regime.  With logits of spread 3, P~ of one real key among up to 1023 padded keys at logit 0 falls below 2^-14, where the
    # fp16 the kernels stage P' in has no relative precision left: the sequence's whole (tiny) gradient is then rounding, for any
    # kernel, and a per-sequence relative error says nothing about the tiling.
    tail = torch.zeros(M, dtype=torch.bool)
    for br, gm in zip(c.bt, c.geoms):
        tail |= gm.nv[gm.seq_id[:, 0]] * 2 < br.n
    c.tail_rows = int(tail.sum())
    scale = torch.where(tail, torch.tensor(REGIMES["soft"][0]), torch.tensor(sd))[:, None, None]
    q = (torch.randn(M, H, HD, generator=gen) * scale).half()
    k = (torch.randn(M, H, HD, generator=gen) * scale).half()
    v = torch.randn(M, H, HD, generator=gen).half()
    c.planted = []
    if plant:      # per branch one query whose dominant key sits in the LAST key tile of their sequence
        for b, (br, gm) in enumerate(zip(c.bt, c.geoms)):
            p, g = b % c.B, b % br.ratio
            rows = gm.rows(p, 0, g)
            nv = rows.numel()
            iq = min(5, nv - 2)
            used = {t[4] for t in c.planted}      # (a key row planted for one branch stays that branch's)
            ik = next(i for i in range(nv - 1, max(iq, 64 * ((nv - 1) // 64) - 1), -1) if int(rows[i]) not in used)
            assert iq < int(gm.nq[gm.number(p, 0, g * gm.hb)])
            k[rows[ik]] = (q[rows[iq]].float() * PLANT_GAIN).half()
            c.planted.append((b, p, g, int(rows[iq]), int(rows[ik])))
    qs = (q.float() * QK).half()                                                     # q' as the QKV GEMM's epilogue leaves it
    c.qkv = torch.stack([qs, k, v]).permute(0, 2, 1, 3).contiguous()                 # head-major [3, 16, M, 48]
    f = lambda t: t.double().view(c.B, c.N, H, HD)
    with torch.no_grad():
        _, outs, lses = O.dilated_attention_core(f(qs) / QK, f(k), f(v), c.segs, c.ratios, return_branches=True)
    c.o_ref = torch.stack(outs).view(len(c.bt), M, H, HD)                            # zeros where a branch does not visit
    c.lse_ref = torch.stack(lses).view(len(c.bt), M, H)                              # -1e8 there
    c.cov = c.lse_ref > -1e7
    c.lse_tot = torch.logsumexp(c.lse_ref, dim=0).float()
    dm = (torch.randn(M, H, HD, generator=gen) * DMIXED_SD).half()
    c.dmixed = dm.permute(1, 0, 2).contiguous()                                      # head-major [16, M, 48]
    c.delta = (dm.double()[None] * c.o_ref).sum(-1).float()                          # [nb, M, 16]; 0 where a branch does not visit
    args = (c.qkv, c.dmixed, c.lse_tot, c.delta, c.bt, c.N, c.B, c.qlimit)
    c.ref = bwd_reference(*args)
    c.emu = bwd_reference(*args, staged=True)
    c.fwd_emu = fwd_staged(c.qkv, c.bt, c.N, c.B, c.qlimit)
    return c


def floors(c):
    """{quantity: worst per-sequence error of the staged emulation against float64} of one case."""
    res = {q: 0.0 for q in BARS}
    for (b, q), (e, _) in bwd_errors(c.emu, c.ref, c.geoms).items():
        res[q] = max(res[q], e)
    emu_o = [spread_fwd(o, gm) for (o, _), gm in zip(c.fwd_emu, c.geoms)]
    emu_l = [spread_fwd(l, gm) for (_, l), gm in zip(c.fwd_emu, c.geoms)]
    for (b, q), (e, _) in fwd_errors(emu_o, emu_l, c.o_ref, c.lse_ref, c.geoms).items():
        res[q] = max(res[q], e)
    return res


def spread_fwd(comp, gm):
    """[M, hb, ...] compact -> [M, 16, ...] dense, zeros elsewhere."""
    full = torch.zeros(comp.shape[0], H, *comp.shape[2:], dtype=comp.dtype)
    idx = gm.heads.reshape(*gm.heads.shape, *([1] * (comp.dim() - 2))).expand(*gm.heads.shape, *comp.shape[2:])
    return full.scatter_(1, idx, comp)
