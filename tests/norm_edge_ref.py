"""Helper (not a test module): the LayerNorm family of csrc/norm.hip per element, in float64, at its row, grid and dispatch edges.

Four launchers (include/modaltune_hip.h), the `kind` of a case:

    fwd   mt_layernorm_fwd       y = LN(x | gelu(x)) w + b (+ add_rows[m % period]), stats = {mean, rstd} per row
    add   mt_add_layernorm_fwd   h = x + drop(branch) ; y = fp16(LN(h) w + b), stats
    bwd   mt_layernorm_bwd       dx (+)= rstd (g - mean(g) - xh mean(g xh)) [gelu'(x)], g = dy w, xh = (x - mean) rstd ; dx16 ; dw, db
    inj   mt_inject_resid_bwd    dx (+)= (1 + g) dy ; dproj = fp16(g dy) ; dgamma += sum_m dy (x + proj)

Everything works FROM EXACTLY THE TENSORS THE KERNELS READ: fp16 / fp32 inputs widened to float64; the backward takes the `stats` tensor the
kernel is given, so its reference is the closed form above with THOSE statistics, not autograd through a fresh LayerNorm.  The GELU is
the exact erf one.

* make_case(kind, M, D, ...): one seeded call per key.  Buffers with ld > D and the row maps of the case, NaN wherever the kernel must not
  read (padding columns, cls rows, stale dy and statistics of dead rows), every output buffer and the statistics NaN-prefilled with two
  rows behind M (dw / db / dgamma: four elements behind D).
* reference(c, mask): {output: (float64 value, bound)} in the logical layout.  u = 2^-24, gamma = (D / 64 + 10) u: a lane's serial
  additions, the six shuffle additions, the cross-wave addition and the product with the rounded 1 / D.

      rounding term   2^-11 |ref| + 2^-25 (fp16)  |  2^-24 |ref| + 2^-150 (fp32)            (the second addend: the subnormal floor)
      forward         d_mean = gamma mean|v| + mean(d_v)                                     (d_v: what v itself may be off by, below)
                      d_var  = gamma var + 2 d_mean mean|d| + d_mean^2 + 2 u var + 2 mean(|d| d_v) + mean(d_v^2)
                      e_rstd = d_var / (2 (var + eps)) + 2 u
                      b_y    = |w| rstd (d_mean + d_v + u |d|) + |w d| rstd (e_rstd + 3 u) + u (|y| + |b|) (+ u (|y| + |add|)) + rounding
                      the stored mean within d_mean, the stored rstd within e_rstd rstd
      backward        d_xh = 2 u |xh| + rstd d_v (+ u |mean| rstd: the packed form folds -mean rstd into one rounded addend)
                      d_c1 = (gamma + u) mean|g|         d_c2 = (gamma + 2 u) mean|g xh| + mean(|g| d_xh)
                      d_t  = u |g| + d_c1 + |xh| d_c2 + |c2| d_xh + u (|xh c2| + |g - c1| + |t|)        t = g - c1 - xh c2
                      b_dx = rstd d_t + u |rstd t| ; with GELU |gelu'| b_dx + |rstd t| d_gelu' + u |dx| ; accumulating + u |dx + old|
      dw / db / dgamma  (M + 8) u (|initial| + sum_m |terms|) + sum_m |dy| d_xh: holds whatever the order of the atomics (at most M
                      additions of rows, three across the waves, one atomic, two roundings inside a term; the second addend is what
                      xh itself is off by, dw only)
      add form        b_h = u |drop(branch)| + rounding ; d_v = b_h ;  inj  b_dx = 2 u |(1 + g) dy| (+ u |total|), b_dproj = u |g dy| + rounding

  GELU input (A&S 7.1.26, csrc/common.h): |erf error| <= 1.5e-7 as common.h states it (tests/test_norm_edges_cpu.py confirms the figure
  by evaluating the polynomial in float64), plus ONE ULP (2^-23) EACH FOR THE HARDWARE RECIPROCAL AND EXP2 -- THAT FIGURE IS AN
  ASSUMPTION, nothing here has measured v_rcp_f32 / v_exp_f32 -- carried through the polynomial: d_erf = 1.5e-7 + e (A1 rel_t + A0
  (rel_e + 6 u)) + u with A0 = sum |a_k| t^k, A1 = sum k |a_k| t^k, rel_t = 2^-23 + 3 u, rel_e = 2^-23 + 5 u z^2; d_v = |x| d_erf / 2
  + 3 u |gelu|, d_gelu' = d_erf / 2 + |x phi| (rel_e + 3 u) + 2 u (Phi + |x phi|).
  The bounds are derived, not tuned: the measured worst ratios are a record, nothing here was adjusted to them.
* errors(got, ref, bound): worst |got - ref| / bound and its (row, column); a NaN where a value belongs is inf.  where(name, at, c) names the row,
  the 256-column chunk and the lane that owns the element in the kernel the case enters (the packed pair has its own layout).
* check_untouched(before, after, written): canaries, bit for bit.
* cpu_emulation(c, fault): the same operation in plain float32 torch (two passes, biased variance, eps inside the root, A&S GELU in
  fp32, outputs rounded to their type) and the planted FAULTS.
* MATRIX / REFUSED: the cases of tests/test_norm_edges_gpu.py by name; run_gpu(ops, c): one call on the device, measured.
"""
import functools
import zlib

import torch

DT = {"f16": torch.float16, "f32": torch.float32}
U = 2.0 ** -24
U_OUT = {"f16": 2.0 ** -11, "f32": 2.0 ** -24}
FLOOR = {"f16": 2.0 ** -25, "f32": 2.0 ** -150}
ULP = 2.0 ** -23            # ASSUMPTION: v_rcp_f32 and v_exp_f32 are within one ulp
ERF_ERR = 1.5e-7            # csrc/common.h for A&S 7.1.26
AS_P = 0.3275911
AS_A = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)
SQRT1_2, INV_SQRT_2PI = 0.70710678118654752440, 0.39894228040143267794
REGIMES = ("plain", "mean1000", "nearconst", "const", "outlier")      # + "tails" for fp16 GELU inputs
KINDS = ("fwd", "add", "bwd", "inj")
NAN = float("nan")


def gamma(D):
    return (D / 64 + 10) * U


def rounding(ref, dt):
    return U_OUT[dt] * ref.abs() + FLOOR[dt]


def as_erf(z):
    """A&S 7.1.26 for z >= 0 in z's dtype (float64: the approximation itself; float32: what the kernels evaluate)."""
    t = 1.0 / (1.0 + AS_P * z)
    poly = AS_A[4]
    for a in AS_A[3::-1]:
        poly = poly * t + a
    return 1.0 - poly * t * torch.exp(-z * z)


def as_gelu(x, grad=False):
    """gelu / gelu' through the polynomial, in x's dtype."""
    er = torch.copysign(as_erf(x.abs() * SQRT1_2), x)
    phi = 0.5 * (1.0 + er)
    return phi + x * INV_SQRT_2PI * torch.exp(-0.5 * x * x) if grad else x * phi


def gelu_terms(x):
    """x float64 -> gelu, its bound d_v, gelu', its bound (module docstring)."""
    z = x.abs() * SQRT1_2
    t, e = 1.0 / (1.0 + AS_P * z), torch.exp(-z * z)
    a0 = sum(abs(a) * t ** (k + 1) for k, a in enumerate(AS_A))
    a1 = sum((k + 1) * abs(a) * t ** (k + 1) for k, a in enumerate(AS_A))
    rel_t, rel_e = ULP + 3 * U, ULP + 5 * U * z * z
    derf = ERF_ERR + e * (a1 * rel_t + a0 * (rel_e + 6 * U)) + U
    Phi = 0.5 * (1.0 + torch.erf(x * SQRT1_2))
    xphi = x * e * INV_SQRT_2PI
    g = x * Phi
    return g, 0.5 * x.abs() * derf + 3 * U * g.abs(), Phi + xphi, 0.5 * derf + xphi.abs() * (rel_e + 3 * U) + 2 * U * (Phi + xphi.abs())


class Case:
    pass


def _phys(M, kind, L, device):
    """-> (physical row of every logical row, physical rows) of a row map: None | "patch" rowmap(L, L + 1, 1) | "bcast" rowmap(L, 0, 0)."""
    m = torch.arange(M, device=device)
    if kind == "patch":
        return (m // L) * (L + 1) + 1 + m % L, -(-M // L) * (L + 1)
    if kind == "bcast":
        return m % L, min(L, M)
    assert kind is None
    return m, M


def _ld(D, dt, pad):
    return D if not pad else D + 4 if (dt == "f32" or pad == 4) else D + 8


def _values(regime, M, D, rn, ru):
    if regime == "plain":
        return rn(M, D) * 2 + 0.5
    if regime == "mean1000":
        return rn(M, D) + 1000.0
    if regime == "nearconst":
        return rn(M, D) * 1e-3 + 3.0
    if regime == "const":
        return (rn(M, 1) * 2 + 0.5).expand(M, D).clone()
    if regime == "outlier":
        v = rn(M, D) * 0.01
        m = torch.arange(M, device=v.device)
        v[m, (m * 37 + 5) % D] = 300.0
        return v
    assert regime == "tails"
    return ru(M, D) * 16 - 8


def _inbuf(vals, row, phys, ld, dt):
    buf = torch.full((phys, ld), NAN, dtype=DT[dt], device=vals.device)
    buf[row, :vals.shape[1]] = vals.to(DT[dt])
    return buf


def _outbuf(M, D, row, phys, ld, dt, device, old=None, rows=None):
    """NaN-prefilled output buffer with two rows behind the last one, `old` where an accumulating kernel reads it; the written mask
    (rows: the logical rows that are written, all by default)."""
    buf = torch.full((phys + 2, ld), NAN, dtype=DT[dt], device=device)
    written = torch.zeros(phys + 2, ld, dtype=torch.bool, device=device)
    if old is not None:
        buf[row, :D] = old.to(DT[dt])
    written[row if rows is None else row[rows[0]:rows[1]], :D] = True
    return buf, written


@functools.lru_cache(maxsize=None)
def make_case(kind, M, D, xdt="f32", odt="f32", dydt="f32", gelu=False, regime="plain", xmap=None, ymap=None, dymap=None, dxmap=None,
              L=5, pad=True, inplace=False, add_period=0, stats=True, param=False, det=False, live=None, accumulate=False, dx16=False,
              drop=None, eps=1e-5, device="cpu"):
    """xdt: dtype of x; odt: of y (fwd) / dx (bwd); dydt: of dy.  pad: ld = D + 4 (fp32) | D + 8 (fp16); pad = 4: D + 4 for fp16 too
    (8-byte rows: off the packed kernels); pad = False: dense.  live = (b0, b1, live_rows): the rows [b0, b1) * live_rows.
    drop = (p, path_p, rows_per_pass) (add form).  inplace: y is x (fwd)."""
    assert kind in KINDS
    c = Case()
    c.kind, c.M, c.D, c.xdt, c.odt, c.dydt, c.gelu, c.regime, c.device = kind, M, D, xdt, odt, dydt, gelu, regime, device
    c.maps = dict(x=xmap, y=ymap, dy=dymap, dx=dxmap)
    c.L, c.pad, c.inplace, c.add_period, c.stats, c.param, c.det, c.live = L, pad, inplace, add_period, stats, param, det, live
    c.accumulate, c.dx16, c.drop, c.eps = accumulate, dx16, drop, eps
    c.eps32 = float(torch.tensor(eps, dtype=torch.float32))
    key = repr((kind, M, D, xdt, odt, dydt, gelu, regime, xmap, ymap, dymap, dxmap, L, pad, inplace, add_period, stats, param, det, live,
                accumulate, dx16, drop, eps))
    gen = torch.Generator(device=device).manual_seed(zlib.crc32(key.encode()))
    rn = lambda *s: torch.randn(*s, generator=gen, device=device)
    ru = lambda *s: torch.rand(*s, generator=gen, device=device)
    c.first, c.end = 0, M
    if live:
        c.first = min(max(live[0], 0) * live[2], M)
        c.end = max(c.first, min(max(live[1], 0) * live[2], M))
    # the packed ln_gelu_* pair: D % 1024 == 0, fp16 everywhere, rows 16-byte aligned (csrc/norm.hip: ln_fwd_types / ln_bwd_types)
    c.packed = (kind in ("fwd", "bwd") and gelu and D % 1024 == 0 and xdt == odt == "f16" and (kind == "fwd" or dydt == "f16")
                and not add_period and not param and _ld(D, "f16", pad) % 8 == 0)
    c.cmp = (c.first, c.end) if (live and c.packed) else None      # the rows that are compared: all, but for the packed pair's live range
    c.bufs, c.init, c.written = {}, {}, {}
    c.w = 1 + 0.1 * rn(D)
    c.b = 0.1 * rn(D)
    xv = _values(regime, M, D, rn, ru)
    c.xrow, xphys = _phys(M, xmap, L, device)
    if xmap == "bcast":
        xv = xv[c.xrow]
    dead = torch.ones(M, dtype=torch.bool, device=device)
    dead[c.first:c.end] = False
    if kind in ("fwd", "add"):
        if kind == "add":
            xdt, odt, pad = "f32", "f16", False
            c.xdt, c.odt, c.pad = xdt, odt, pad
        ldx = _ld(D, xdt, pad)
        c.ldx = ldx
        if live and c.packed:
            xv[dead] = NAN
        c.bufs["x"] = _inbuf(xv, c.xrow, xphys, ldx, xdt)
        if kind == "add":
            c.bufs["branch"] = rn(M, D).half()
            c.init["h"], c.written["h"] = _outbuf(M, D, c.xrow, M, D, "f32", device)
            c.yrow, c.ldy = c.xrow, D
            c.init["y"], c.written["y"] = _outbuf(M, D, c.yrow, M, D, "f16", device)
        elif inplace:
            assert xdt == odt and ymap == xmap
            c.yrow, c.ldy = c.xrow, ldx
            c.init["y"] = c.bufs["x"]
            c.written["y"] = torch.zeros(xphys, ldx, dtype=torch.bool, device=device)
            c.written["y"][c.yrow, :D] = True
        else:
            c.yrow, yphys = _phys(M, ymap, L, device)
            c.ldy = _ld(D, odt, pad)
            c.init["y"], c.written["y"] = _outbuf(M, D, c.yrow, yphys, c.ldy, odt, device, rows=c.cmp)
        c.add_rows = rn(add_period, D) if add_period else None
        if stats:
            c.init["stats"] = torch.full((M + 2, 2), NAN, device=device)
            c.written["stats"] = torch.zeros(M + 2, 2, dtype=torch.bool, device=device)
            c.written["stats"][c.first:c.end if c.cmp else M] = True
        return c
    # the backward kinds
    c.ldx = _ld(D, xdt, pad)
    dyv = rn(M, D)
    c.dyrow, dyphys = _phys(M, dymap, L, device)
    c.dxrow, dxphys = _phys(M, dxmap, L, device)
    c.lddy, c.lddx = _ld(D, dydt, pad), _ld(D, odt, pad)
    old = rn(M, D) if accumulate else None
    if kind == "bwd":
        v = xv.to(DT[xdt]).double()
        if gelu:
            v = gelu_terms(v)[0]
        mean = v.mean(1, keepdim=True)
        rstd = ((v - mean).pow(2).mean(1, keepdim=True) + c.eps32).rsqrt()
        c.bufs["stats"] = torch.cat([mean, rstd], 1).float()
        if live:      # stale bytes of the dead rows: dy for the generic kernel (which reads x and statistics), everything for the packed one
            dyv[dead] = NAN
            if c.packed:
                xv[dead] = NAN
                c.bufs["stats"][dead] = NAN
        c.bufs["x"] = _inbuf(xv, c.xrow, xphys, c.ldx, xdt)
        c.bufs["dy"] = _inbuf(dyv, c.dyrow, dyphys, c.lddy, dydt)
        c.init["dx"], c.written["dx"] = _outbuf(M, D, c.dxrow, dxphys, c.lddx, odt, device, old=old, rows=c.cmp)
        if dx16:
            c.init["dx16"], c.written["dx16"] = _outbuf(M, D, torch.arange(M, device=device), M, D, "f16", device)
        if param:
            for n in ("dw", "db"):
                c.init[n] = torch.cat([rn(D), torch.full((4,), NAN, device=device)])
                c.written[n] = torch.arange(D + 4, device=device) < D
        return c
    assert kind == "inj" and D == 768 and xdt == odt == dydt == "f32" and not gelu
    c.bufs["x"] = _inbuf(xv, c.xrow, xphys, c.ldx, "f32")
    c.bufs["dy"] = _inbuf(dyv, c.dyrow, dyphys, c.lddy, "f32")
    c.bufs["proj"] = rn(M, D).half()
    c.bufs["gamma"] = 0.1 * rn(D)
    c.init["dx"], c.written["dx"] = _outbuf(M, D, c.dxrow, dxphys, c.lddx, "f32", device, old=old)
    c.init["dproj"], c.written["dproj"] = _outbuf(M, D, torch.arange(M, device=device), M, D, "f16", device)
    c.init["dgamma"] = torch.cat([rn(D), torch.full((4,), NAN, device=device)])
    c.written["dgamma"] = torch.arange(D + 4, device=device) < D
    return c


# ------------------------------------------------------------------------------------------------ the float64 reference and its bound
def _x(c, dtype=torch.float64):
    return c.bufs["x"][c.xrow, :c.D].to(dtype)


def _fwd_core(c, v, dv, extra=None):
    """LN(v) w + b (+ extra) in float64, v off by at most dv elementwise -> {y, mean, rstd: (ref, bound without the output rounding)}."""
    D, kd = c.D, dict(dim=1, keepdim=True)
    w, b = c.w.double(), c.b.double()
    mean = v.mean(**kd)
    d = v - mean
    var = (d * d).mean(**kd)
    rstd = (var + c.eps32).rsqrt()
    y = d * rstd * w + b
    g = gamma(D)
    dmean = g * v.abs().mean(**kd) + dv.mean(**kd)
    dvar = g * var + 2 * dmean * d.abs().mean(**kd) + dmean ** 2 + 2 * U * var + 2 * (d.abs() * dv).mean(**kd) + (dv * dv).mean(**kd)
    erstd = 0.5 * dvar / (var + c.eps32) + 2 * U
    by = w.abs() * rstd * (dmean + dv + U * d.abs()) + (w * d).abs() * rstd * (erstd + 3 * U) + U * (y.abs() + b.abs())
    if extra is not None:
        y = y + extra
        by = by + U * (y.abs() + extra.abs())
    return dict(y=(y, by), mean=(mean[:, 0], dmean[:, 0]), rstd=(rstd[:, 0], (erstd * rstd)[:, 0]))


def reference(c, mask=None):
    """{output name: (float64 reference, bound)} in the logical layout ([M, D], [M] for mean / rstd, [D] for dw / db / dgamma).
    mask [M, D] (add form with dropout): the factor of every element as ops.dropout_f32 reads it from the device."""
    M, D = c.M, c.D
    zero = torch.zeros((), dtype=torch.float64, device=c.device)
    out = {}
    if c.kind == "fwd":
        x = _x(c)
        v, dv = (gelu_terms(x)[:2]) if c.gelu else (x, zero.expand(M, D))
        extra = c.add_rows.double()[torch.arange(M, device=c.device) % c.add_period] if c.add_period else None
        out = _fwd_core(c, v, dv, extra)
        out["y"] = (out["y"][0], out["y"][1] + rounding(out["y"][0], c.odt))
        if not c.stats:
            del out["mean"], out["rstd"]
    elif c.kind == "add":
        br = c.bufs["branch"].double()
        if mask is not None:      # (a dropped element is SELECTED to 0: its branch bytes may be stale)
            br = torch.where(mask != 0, br * mask.double(), torch.zeros_like(br))
        h = _x(c) + br
        bh = U * br.abs() + rounding(h, "f32")
        out = _fwd_core(c, h, bh)
        out["y"] = (out["y"][0], out["y"][1] + rounding(out["y"][0], "f16"))
        out["h"] = (h, bh)
    elif c.kind == "bwd":
        x = _x(c)
        kd = dict(dim=1, keepdim=True)
        if c.gelu:
            v, dv, gp, dgp = gelu_terms(x)
        else:
            v, dv = x, zero.expand(M, D)
        st = c.bufs["stats"].double()
        mean, rstd = st[:, 0:1], st[:, 1:2]
        dy = c.bufs["dy"][c.dyrow, :D].double()
        if c.live and not c.packed:      # dy of a dead row counts as zero
            dy = dy.clone()
            dy[:c.first] = 0.0
            dy[c.end:] = 0.0
        w = c.w.double()
        xh = (v - mean) * rstd
        g = dy * w
        c1, c2 = g.mean(**kd), (g * xh).mean(**kd)
        t = g - c1 - xh * c2
        dx = rstd * t
        gm = gamma(D)
        dxh = 2 * U * xh.abs() + rstd * dv + (U * mean.abs() * rstd if c.packed else 0.0)
        dc1 = (gm + U) * g.abs().mean(**kd)
        dc2 = (gm + 2 * U) * (g * xh).abs().mean(**kd) + (g.abs() * dxh).mean(**kd)
        dt = U * g.abs() + dc1 + xh.abs() * dc2 + c2.abs() * dxh + U * ((xh * c2).abs() + (g - c1).abs() + t.abs())
        bdx = rstd * dt + U * dx.abs()
        if c.gelu:
            bdx = gp.abs() * bdx + dx.abs() * dgp
            dx = dx * gp
            bdx = bdx + U * dx.abs()
        if c.accumulate:
            dx = dx + c.init["dx"][c.dxrow, :D].double()
            bdx = bdx + U * dx.abs()
        out["dx"] = (dx, bdx + rounding(dx, c.odt))
        if c.dx16:
            out["dx16"] = (dx, bdx + rounding(dx, "f16"))
        if c.param:
            tw, tb = dy * xh, dy
            out["dw"] = (c.init["dw"][:D].double() + tw.sum(0),
                         (M + 8) * U * (c.init["dw"][:D].double().abs() + tw.abs().sum(0)) + (dy.abs() * dxh).sum(0) + FLOOR["f32"])
            out["db"] = (c.init["db"][:D].double() + tb.sum(0), (M + 8) * U * (c.init["db"][:D].double().abs() + tb.abs().sum(0)) + FLOOR["f32"])
    else:
        dy, x = c.bufs["dy"][c.dyrow, :D].double(), _x(c)
        p, g = c.bufs["proj"].double(), c.bufs["gamma"].double()
        dx = (1 + g) * dy
        bdx = 2 * U * dx.abs()
        if c.accumulate:
            dx = dx + c.init["dx"][c.dxrow, :D].double()
            bdx = bdx + U * dx.abs()
        out["dx"] = (dx, bdx + rounding(dx, "f32"))
        q = g * dy
        out["dproj"] = (q, U * q.abs() + rounding(q, "f16"))
        tg, g0 = dy * (x + p), c.init["dgamma"][:D].double()
        out["dgamma"] = (g0 + tg.sum(0), (M + 8) * U * (g0.abs() + (dy.abs() * (x.abs() + p.abs())).sum(0)) + FLOOR["f32"])
    return out


# ------------------------------------------------------------------------------------------------ the metric
def errors(got, ref, bound):
    """-> (worst |got - ref| / bound, (row, column)); [N] vectors count as one row.  A NaN (or inf) where a value belongs counts as inf."""
    r = (got.to(ref.device).double() - ref).abs() / bound
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
    if r.numel() == 0:
        return 0.0, (0, 0)
    i = int(r.argmax())
    n = ref.shape[-1]
    return float(r.reshape(-1)[i]), (i // n, i % n) if ref.dim() == 2 else (i, 0)


def where(name, at, c=None):
    """Row, 256-column chunk and owner of an element, for messages.  c: the case -- the packed ln_gelu_* pair (a lane owns 8 columns per
    512-column chunk; forward: two rows per workgroup, two waves per row; backward: one row per workgroup, three waves) differs from
    the generic layout (four rows per workgroup, one wave per row, a lane owns 4 columns per 256-column chunk)."""
    m, n = at
    packed = c is not None and c.packed
    if name in ("mean", "rstd"):
        if packed:
            return f"{name} of row {m} (row {(m - c.first) % 2} of its two-row workgroup, counted from the first live row {c.first})"
        return f"{name} of row {m} (workgroup {m // 4} of four rows, wave {m % 4})"
    if name in ("dw", "db", "dgamma"):
        n = m
        return f"{name}[{n}]: 256-column chunk {n // 256}, lane {(n % 256) // 4}, element {n % 4}"
    if packed:
        per_wave = c.D // 2 if c.kind == "fwd" else c.D // 3
        off = n % per_wave
        rows = f"row {(m - c.first) % 2} of its two-row workgroup" if c.kind == "fwd" else "one row per workgroup"
        return (f"{name} row {m} ({rows}, counted from the first live row {c.first}), column {n}: 256-column chunk {n // 256}; packed layout: "
                f"wave {n // per_wave} of the row, its 512-column chunk {off // 512}, lane {(off % 512) // 8}, element {off % 8}")
    return f"{name} row {m} (wave {m % 4} of a four-row workgroup), column {n}: 256-column chunk {n // 256}, lane {(n % 256) // 4}, element {n % 4}"


def check_untouched(before, after, written):
    """Every element outside `written` (bool, the buffer's shape) must be bit-identical in `before` and `after`.
    -> (number of changed elements, flat index of the first or None)."""
    it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[before.element_size()]
    bad = ((before.view(it) != after.view(it)) & ~written.to(before.device)).reshape(-1)
    n = int(bad.sum())
    return n, (int(bad.nonzero()[0]) if n else None)


def measure(c, got, ref=None, mask=None):
    """got: {name: logical tensor}.  -> {name: (ratio, at)} over the rows that are compared."""
    ref = reference(c, mask) if ref is None else ref
    res = {}
    for name, (r, bd) in ref.items():
        g = got[name]
        if c.cmp and r.dim() >= 1 and r.shape[0] == c.M and name not in ("dw", "db", "dgamma"):
            g, r, bd = g[c.cmp[0]:c.cmp[1]], r[c.cmp[0]:c.cmp[1]], bd[c.cmp[0]:c.cmp[1]]
            ratio, at = errors(g, r, bd)
            at = (at[0] + c.cmp[0], at[1])
        else:
            ratio, at = errors(g, r, bd)
        res[name] = (ratio, at)
    return res


# ------------------------------------------------------------------------------------------------ float32 emulation and planted faults
FAULTS = ("onepass_var", "bessel", "no_eps", "chunk_w", "lane_shift", "swap_c1c2", "no_gelu_grad", "ignore_accumulate", "stale_stats",
          "last_row_unwritten", "wave_missing_dw")


def fault_applies(c, fault):
    """Whether the planted fault changes anything the case computes."""
    fwd = c.kind in ("fwd", "add")
    return {"onepass_var": fwd, "bessel": fwd, "no_eps": fwd, "chunk_w": c.kind != "inj" and c.D >= 512, "lane_shift": True,
            "swap_c1c2": c.kind == "bwd", "no_gelu_grad": c.kind == "bwd" and c.gelu, "ignore_accumulate": c.accumulate,
            "stale_stats": c.kind in ("fwd", "add", "bwd") and c.M > 1 and (c.stats or c.kind != "fwd"),
            "last_row_unwritten": fwd and c.M % 2 == 1, "wave_missing_dw": (c.param or c.kind == "inj") and c.M >= 2}[fault]


def _shift_lane(t):
    t[:, 8:12] = t[:, 4:8].clone()      # lane 2's four columns of chunk 0 taken from lane 1
    return t


def cpu_emulation(c, fault=None, mask=None):
    """{name: logical tensor in the output's dtype}: float32 torch on the CPU; fault: one of FAULTS -- what a kernel with that defect
    would leave."""
    M, D = c.M, c.D
    f32 = torch.float32
    w, b = c.w.clone(), c.b
    if fault == "chunk_w":
        w[256:512] = c.w[0:256]
    kd = dict(dim=1, keepdim=True)
    out = {}
    if c.kind in ("fwd", "add"):
        if c.kind == "add":
            br = c.bufs["branch"].float()
            if mask is not None:
                br = torch.where(mask != 0, br * mask, torch.zeros_like(br))
            v = _x(c, f32) + br
            out["h"] = v.clone()
        else:
            v = _x(c, f32)
            if c.gelu:
                v = as_gelu(v)
        if fault == "lane_shift":
            v = _shift_lane(v.clone())
        mean = v.mean(**kd)
        d = v - mean
        var = (v * v).mean(**kd) - mean * mean if fault == "onepass_var" else (d * d).mean(**kd)
        if fault == "bessel":
            var = var * (D / (D - 1.0))
        rstd = torch.rsqrt(var if fault == "no_eps" else var + c.eps32).to(f32)
        y = d * rstd * w + b
        if c.kind == "fwd" and c.add_period:
            y = y + c.add_rows[torch.arange(M) % c.add_period]
        y = y.to(DT[c.odt])
        mean, rstd = mean[:, 0].clone(), rstd[:, 0].clone()
        if fault == "stale_stats":
            mean[1:], rstd[1:] = mean[:-1].clone(), rstd[:-1].clone()
        if fault == "last_row_unwritten":
            y[M - 1] = NAN
            mean[M - 1] = rstd[M - 1] = NAN
        out["y"] = y
        if c.stats or c.kind == "add":
            out["mean"], out["rstd"] = mean, rstd
        return out
    dy = c.bufs["dy"][c.dyrow, :D].float()
    x = _x(c, f32)
    old = c.init["dx"][c.dxrow, :D].float()
    lost = torch.arange(M) % 4 == 1      # wave 1's rows
    if c.kind == "bwd":
        if c.live and not c.packed:
            dy[:c.first] = 0.0
            dy[c.end:] = 0.0
        st = c.bufs["stats"].clone()
        if fault == "stale_stats":
            st[1:] = c.bufs["stats"][:-1]
        mean, rstd = st[:, 0:1], st[:, 1:2]
        v = as_gelu(x) if c.gelu else x
        if fault == "lane_shift":
            v = _shift_lane(v.clone())
        xh = (v - mean) * rstd
        g = dy * w
        c1, c2 = g.mean(**kd), (g * xh).mean(**kd)
        if fault == "swap_c1c2":
            c1, c2 = c2, c1
        dx = rstd * (g - c1 - xh * c2)
        if c.gelu and fault != "no_gelu_grad":
            dx = dx * as_gelu(x, grad=True)
        if c.accumulate and fault != "ignore_accumulate":
            dx = dx + old
        out["dx"] = dx.to(DT[c.odt])
        if c.dx16:
            out["dx16"] = dx.half()
        if c.param:
            keep = ~lost if fault == "wave_missing_dw" else torch.ones(M, dtype=torch.bool)
            out["dw"] = c.init["dw"][:D] + (dy * xh)[keep].sum(0)
            out["db"] = c.init["db"][:D] + dy[keep].sum(0)
        return out
    g = c.bufs["gamma"]
    dx = (1 + g) * dy
    if c.accumulate and fault != "ignore_accumulate":
        dx = dx + old
    out["dx"] = _shift_lane(dx) if fault == "lane_shift" else dx
    out["dproj"] = (g * dy).half()
    keep = ~lost if fault == "wave_missing_dw" else torch.ones(M, dtype=torch.bool)
    out["dgamma"] = c.init["dgamma"][:D] + (dy * (x + c.bufs["proj"].float()))[keep].sum(0)
    return out


# ------------------------------------------------------------------------------------------------ the cases of the GPU matrix
SMALL_M = (1, 2, 3, 4, 5, 7, 8, 9, 67)
PARAM_M = (2047, 2048, 2049, 2053, 4101)      # around the 512-workgroup cap of the PARAM / DET forms and inject_resid_bwd (4 rows each)
GRID_M = (16383, 16384, 16385, 16389, 32771)  # around ln_grid's 4096 x 4, ln_gelu_grid's 8192 x 2 and ln_gelu_bwd's 16384 x 1
H = dict(xdt="f16", odt="f16", dydt="f16")
# form -> the keyword arguments that select it (the instantiation it enters is named in tests/README.md)
FORMS = {
    "fwd-f32": dict(kind="fwd", D=256),
    "fwd-f32-f16": dict(kind="fwd", D=768, odt="f16"),
    "fwd-f16": dict(kind="fwd", D=2304, xdt="f16", odt="f16"),
    "fwd-gelu-generic": dict(kind="fwd", D=768, gelu=True, **H),
    "fwd-gelu-packed": dict(kind="fwd", D=3072, gelu=True, **H),
    "add": dict(kind="add", D=768),
    "bwd-f32": dict(kind="bwd", D=256),
    "bwd-h-f-f": dict(kind="bwd", D=768, dydt="f16", accumulate=True, dx16=True),
    "bwd-h-f-h": dict(kind="bwd", D=768, dydt="f16", odt="f16"),
    "bwd-gelu-generic": dict(kind="bwd", D=768, gelu=True, **H),
    "bwd-gelu-packed": dict(kind="bwd", D=3072, gelu=True, **H),
    "bwd-param": dict(kind="bwd", D=256, param=True),
    "bwd-param-patch": dict(kind="bwd", D=768, dydt="f16", param=True, accumulate=True, dx16=True, xmap="patch", dxmap="patch"),
    "bwd-det": dict(kind="bwd", D=768, param=True, det=True),
    "bwd-det-patch": dict(kind="bwd", D=768, dydt="f16", param=True, det=True, accumulate=True, xmap="patch", dxmap="patch"),
    "bwd-live": dict(kind="bwd", D=768, dydt="f16", accumulate=True),
    "inj": dict(kind="inj", D=768),
    "inj-engine": dict(kind="inj", D=768, dymap="patch", dxmap="patch", xmap="bcast", accumulate=True),
    "inj-det": dict(kind="inj", D=768, det=True),
    "inj-det-engine": dict(kind="inj", D=768, det=True, dymap="patch", dxmap="patch", xmap="bcast"),
}


def _live_for(M):
    """A live range that starts and ends on odd pass boundaries, an odd number of rows per pass."""
    rows = 3 if M < 40 else 7 if M < 1000 else 1023
    return (1, max(2, (M // rows) | 1), rows)


def _matrix():
    cs = {}

    def add(name, form, **kw):
        k = dict(FORMS[form], **kw)
        if k.get("live", "auto" if form == "bwd-live" else None) == "auto":
            k["live"] = _live_for(k["M"])
        assert name not in cs, name
        cs[name] = k

    for M in SMALL_M:      # every form at the small and odd row counts (idle waves, the clamp of the last workgroup)
        for form in FORMS:
            add(f"rows-{form}-M{M}", form, M=M)
    for M in PARAM_M:      # a wave's second row into gw / gb / gg
        for form in ("bwd-param", "bwd-param-patch", "bwd-det", "bwd-det-patch", "inj", "inj-engine", "inj-det", "inj-det-engine"):
            add(f"cap512-{form}-M{M}", form, M=M, L=33)
    for M in GRID_M:       # the grid-stride loops (references on the device)
        add(f"grid-fwd-f32-M{M}", "fwd-f32", M=M)
        add(f"grid-bwd-f32-M{M}", "bwd-f32", M=M)
        add(f"grid-add-M{M}", "add", M=M)
        add(f"grid-fwd-gelu-packed-M{M}", "fwd-gelu-packed", M=M)
        add(f"grid-bwd-gelu-packed-M{M}", "bwd-gelu-packed", M=M)
    add("grid-bwd-live-M16389", "bwd-live", M=16389)
    add("grid-fwd-gelu-packed-live-M32771", "fwd-gelu-packed", M=32771, live=(1, 19, 1723))
    add("grid-bwd-gelu-packed-live-M32771", "bwd-gelu-packed", M=32771, live=(1, 19, 1723))
    # the numerical regimes
    for regime in REGIMES:
        for D in (256, 768, 2304, 3072):
            add(f"regime-{regime}-fwd-f32-D{D}", "fwd-f32", M=9, D=D, regime=regime)
            add(f"regime-{regime}-fwd-f32-f16-D{D}", "fwd-f32-f16", M=9, D=D, regime=regime)
            add(f"regime-{regime}-bwd-f32-D{D}", "bwd-f32", M=9, D=D, regime=regime)
        add(f"regime-{regime}-add", "add", M=9, regime=regime)
        add(f"regime-{regime}-inj", "inj", M=9, regime=regime)
    for regime in REGIMES + ("tails",):
        for form in ("fwd-gelu-generic", "fwd-gelu-packed", "bwd-gelu-generic", "bwd-gelu-packed"):
            add(f"regime-{regime}-{form}", form, M=9, regime=regime)
    # dispatch: every (D, dtypes, gelu) the launchers accept
    for D in (256, 768, 2304, 3072):
        for tn, t in (("f32-f32", dict()), ("f32-f16", dict(odt="f16")), ("f16-f16", dict(xdt="f16", odt="f16"))):
            for ge in (False, True):
                add(f"dispatch-fwd-{tn}-{'gelu-' if ge else ''}D{D}", "fwd-f32", M=9, D=D, gelu=ge, **t)
        for tn, t in (("f-f-f", dict()), ("h-f-f", dict(dydt="f16")), ("h-f-h", dict(dydt="f16", odt="f16"))):
            add(f"dispatch-bwd-{tn}-D{D}", "bwd-f32", M=9, D=D, **t)
            add(f"dispatch-bwd-{tn}-acc-D{D}", "bwd-f32", M=9, D=D, accumulate=True, **t)
            add(f"dispatch-bwd-{tn}-live-D{D}", "bwd-f32", M=9, D=D, live="auto", **t)
            if tn == "f-f-f" or D <= 768:      # dw / db: fp32 dy at every D (72 and 96 KB of LDS at 2304 and 3072), fp16 dy up to 768
                add(f"dispatch-bwd-{tn}-param-D{D}", "bwd-f32", M=9, D=D, param=True, **t)
                add(f"dispatch-bwd-{tn}-det-D{D}", "bwd-f32", M=9, D=D, param=True, det=True, **t)
        add(f"dispatch-bwd-gelu-D{D}", "bwd-gelu-generic", M=9, D=D)
        add(f"dispatch-bwd-gelu-acc-D{D}", "bwd-gelu-generic", M=9, D=D, accumulate=True)
    add("dispatch-fwd-gelu-ld+4-D3072", "fwd-gelu-packed", M=9, pad=4)      # rows 8-byte aligned only: off the packed kernels
    add("dispatch-bwd-gelu-ld+4-D3072", "bwd-gelu-packed", M=9, pad=4)
    add("dispatch-fwd-gelu-dense-D3072", "fwd-gelu-packed", M=9, pad=False)
    add("dispatch-bwd-gelu-dense-D3072", "bwd-gelu-packed", M=9, pad=False)
    add("dispatch-fwd-gelu-packed-nostats", "fwd-gelu-packed", M=9, stats=False)
    add("dispatch-fwd-f32-nostats", "fwd-f32", M=9, stats=False)
    add("dispatch-fwd-f16-inplace", "fwd-f16", M=9, D=768, inplace=True)
    add("dispatch-fwd-f32-inplace-patch", "fwd-f32", M=9, D=768, inplace=True, xmap="patch", ymap="patch")
    add("dispatch-fwd-add-rows-period5", "fwd-f32", M=9, D=768, add_period=5)
    add("dispatch-fwd-add-rows-period5-f16", "fwd-f32-f16", M=67, add_period=5)
    add("dispatch-fwd-x-bcast", "fwd-f32-f16", M=9, xmap="bcast", L=5)
    add("dispatch-bwd-x-bcast", "bwd-h-f-f", M=9, xmap="bcast", L=5)
    add("dispatch-fwd-eps", "fwd-f32", M=9, D=768, eps=1e-6, regime="nearconst")
    # maps and strides: the patch map alone and combined, a pass boundary inside a workgroup's four rows
    for L in (5, 33):
        for M in (67,):
            add(f"maps-fwd-x-L{L}", "fwd-f32-f16", M=M, L=L, xmap="patch")
            add(f"maps-fwd-y-L{L}", "fwd-f32-f16", M=M, L=L, ymap="patch")
            add(f"maps-fwd-xy-L{L}", "fwd-f32", M=M, D=768, L=L, xmap="patch", ymap="patch")
            add(f"maps-fwd-gelu-packed-xy-L{L}", "fwd-gelu-packed", M=M, L=L, xmap="patch", ymap="patch")
            add(f"maps-bwd-dy-L{L}", "bwd-h-f-f", M=M, L=L, dymap="patch")
            add(f"maps-bwd-x-L{L}", "bwd-h-f-f", M=M, L=L, xmap="patch")
            add(f"maps-bwd-dx-L{L}", "bwd-h-f-f", M=M, L=L, dxmap="patch")
            add(f"maps-bwd-all-L{L}", "bwd-h-f-f", M=M, L=L, dymap="patch", xmap="patch", dxmap="patch")
            add(f"maps-bwd-gelu-packed-all-L{L}", "bwd-gelu-packed", M=M, L=L, dymap="patch", xmap="patch", dxmap="patch")
            add(f"maps-inj-engine-L{L}", "inj-engine", M=M, L=L)
    # the add form under its masks (read from the device)
    for M, rpp in ((67, 20), (9, 3)):
        add(f"add-dropout-M{M}", "add", M=M, drop=(0.25, 0.0, rpp))
        add(f"add-dropout-droppath-M{M}", "add", M=M, drop=(0.25, 0.5, rpp))
        add(f"add-droppath-M{M}", "add", M=M, drop=(0.0, 0.5, rpp))
    # LIVE: the range starts and ends on odd pass boundaries, live_rows is odd
    for M in (9, 67):
        add(f"live-fwd-gelu-packed-M{M}", "fwd-gelu-packed", M=M, live="auto")
        add(f"live-bwd-gelu-packed-M{M}", "bwd-gelu-packed", M=M, live="auto")
        add(f"live-bwd-gelu-packed-acc-M{M}", "bwd-gelu-packed", M=M, live="auto", accumulate=True)
        add(f"live-bwd-h-f-f-patch-M{M}", "bwd-live", M=M, xmap="patch", dxmap="patch", L=5)
    add("live-bwd-empty-range", "bwd-live", M=9, live=(3, 3, 3))
    for lv, tag in (((1, 2, 3), "3rows"), ((1, 2, 5), "5rows"), ((0, 1, 1), "1row")):      # an odd number of live rows: the second row of the
        add(f"live-fwd-gelu-packed-odd-{tag}", "fwd-gelu-packed", M=11, live=lv)             # last pair joins the barriers and stores nothing
        add(f"live-bwd-gelu-packed-odd-{tag}", "bwd-gelu-packed", M=11, live=lv)
    add("live-fwd-gelu-packed-clamped", "fwd-gelu-packed", M=9, live=(1, 99, 3))
    return cs


MATRIX = _matrix()

# what the launchers refuse: MT_ERR_UNSUPPORTED (-3), the NaN-prefilled outputs bit-identical
REFUSED = {
    "fwd-D512": dict(kind="fwd", M=9, D=512),
    "bwd-D512": dict(kind="bwd", M=9, D=512),
    "add-D256": dict(kind="add", M=9, D=256),
    "fwd-f16-to-f32": dict(kind="fwd", M=9, D=768, xdt="f16", odt="f32"),
    "fwd-live-generic": dict(kind="fwd", M=9, D=768, live=(1, 3, 3)),
    "fwd-live-gelu-ld+4": dict(kind="fwd", M=9, D=3072, gelu=True, pad=4, live=(1, 3, 3), **H),
    "fwd-live-gelu-D768": dict(kind="fwd", M=9, D=768, gelu=True, live=(1, 3, 3), **H),
    "bwd-f-f-h": dict(kind="bwd", M=9, D=768, odt="f16"),
    "bwd-f-h-f": dict(kind="bwd", M=9, D=768, xdt="f16"),
    "bwd-h-h-h-nogelu": dict(kind="bwd", M=9, D=768, **H),
    "bwd-f-h-h": dict(kind="bwd", M=9, D=768, xdt="f16", odt="f16"),
    "bwd-h-h-f": dict(kind="bwd", M=9, D=768, dydt="f16", xdt="f16"),
    "bwd-live-param": dict(kind="bwd", M=9, D=768, param=True, live=(1, 3, 3)),            # (dw / db sum over every row: no table)
    "bwd-live-det": dict(kind="bwd", M=9, D=768, param=True, det=True, live=(1, 3, 3)),    # (live and partials: not both)
    "bwd-gelu-f32": dict(kind="bwd", M=9, D=768, gelu=True),
    "bwd-gelu-h-f-f": dict(kind="bwd", M=9, D=3072, gelu=True, dydt="f16"),
    "bwd-gelu-param": dict(kind="bwd", M=9, D=768, gelu=True, param=True, **H),
    "bwd-gelu-det": dict(kind="bwd", M=9, D=3072, gelu=True, param=True, det=True, **H),
    "bwd-gelu-dx16": dict(kind="bwd", M=9, D=768, gelu=True, dx16=True, **H),
    "bwd-gelu-live-generic": dict(kind="bwd", M=9, D=768, gelu=True, live=(1, 3, 3), **H),
    "bwd-gelu-live-ld+4": dict(kind="bwd", M=9, D=3072, gelu=True, pad=4, live=(1, 3, 3), **H),
    "bwd-h-f-f-param-D2304": dict(kind="bwd", M=9, D=2304, dydt="f16", param=True),
    "bwd-h-f-h-det-D3072": dict(kind="bwd", M=9, D=3072, dydt="f16", odt="f16", param=True, det=True),
}


def case_of(kw, device="cpu"):
    return make_case(**kw, device=device)


def on_device(M):
    """Cases above the grid caps build their inputs and float64 references on the device."""
    return M > 16000


# ------------------------------------------------------------------------------------------------ one call on the device
def _rowmap(kind, L):
    from modaltune_amd._lib import rowmap
    return None if kind is None else rowmap(L, L + 1, 1) if kind == "patch" else rowmap(L, 0, 0)


def device_buffers(c, dev="cuda"):
    """The inputs and the (NaN-prefilled) outputs of the case on the device; an in-place forward shares one buffer."""
    t = {k: v.to(dev).clone() for k, v in c.bufs.items()}
    for k, v in c.init.items():
        t[k] = t["x"] if (c.inplace and k == "y") else v.to(dev).clone()
    for k in ("w", "b", "add_rows"):
        v = getattr(c, k, None)
        t[k] = None if v is None else v.to(dev)
    return t


def launch(ops, c, t, spec=None):
    """The one call of the case on the buffers `t`.  Raises what the launcher's status raises."""
    M, D = c.M, c.D
    mp = {k: _rowmap(v, c.L) for k, v in c.maps.items()}
    t["_keep"] = [mp, spec]
    live = None
    if c.live:
        live = torch.tensor(c.live[:2], dtype=torch.int32, device=t["x"].device)
        t["_keep"].append(live)
    lk = dict(live=live, live_rows=c.live[2]) if c.live else {}
    det = None
    if c.det:
        name = "layernorm_bwd" if c.kind == "bwd" else "inject_resid_bwd"
        det = torch.full((ops.det_elems(name, M, D),), NAN, device=t["x"].device)
        t["_keep"].append(det)
    if c.kind == "fwd":
        ops.layernorm_fwd(t["x"], t["w"], t["b"], t["y"], t.get("stats"), M, D, ldx=c.ldx, xmap=mp["x"], ldy=c.ldy, ymap=mp["y"],
                          gelu_in=c.gelu, add_rows=t["add_rows"], add_period=c.add_period, eps=c.eps, **lk)
    elif c.kind == "add":
        ops.add_layernorm_fwd(t["x"], t["branch"], t["w"], t["b"], t["h"], t["y"], t["stats"], M, D, drop=spec, eps=c.eps)
    elif c.kind == "bwd" and c.live and c.param:
        # ops.layernorm_bwd raises ValueError for a live table with dw / db before it calls: the launcher's own answer through the C entry
        from modaltune_amd import _lib
        _lib.check(_lib.load().mt_layernorm_bwd(
            t["dy"].data_ptr(), c.lddy, ops._rm(mp["dy"]), ops._dt(t["dy"]), t["x"].data_ptr(), c.ldx, ops._rm(mp["x"]), ops._dt(t["x"]),
            int(c.gelu), t["w"].data_ptr(), t["stats"].data_ptr(), t["dx"].data_ptr(), c.lddx, ops._rm(mp["dx"]), ops._dt(t["dx"]),
            int(c.accumulate), t["dw"].data_ptr(), t["db"].data_ptr(), None, None, M, D,
            ops._opts("layernorm_bwd", live=live, live_rows=c.live[2], det=det), ops._s()), "layernorm_bwd")
    elif c.kind == "bwd":
        ops.layernorm_bwd(t["dy"], t["x"], t["w"], t["stats"], t["dx"], M, D, lddy=c.lddy, dymap=mp["dy"], ldx=c.ldx, xmap=mp["x"],
                          lddx=c.lddx, dxmap=mp["dx"], gelu_in=c.gelu, accumulate=c.accumulate, dw=t.get("dw"), db=t.get("db"),
                          dx16=t.get("dx16"), det=det, **lk)
    else:
        ops.inject_resid_bwd(t["dy"], t["x"], t["proj"], t["gamma"], t["dx"], t["dproj"], t["dgamma"], M, D, lddy=c.lddy, dymap=mp["dy"],
                             ldx=c.ldx, xmap=mp["x"], lddx=c.lddx, dxmap=mp["dx"], dx_accumulate=c.accumulate, det=det)


def logical(c, t):
    """{output name: the logical tensor} out of the buffers (row maps and leading dimensions undone)."""
    M, D = c.M, c.D
    out = {}
    if c.kind in ("fwd", "add"):
        out["y"] = t["y"][c.yrow.to(t["y"].device), :D]
        if "stats" in c.init:
            out["mean"], out["rstd"] = t["stats"][:M, 0], t["stats"][:M, 1]
        if c.kind == "add":
            out["h"] = t["h"][:M]
        return out
    out["dx"] = t["dx"][c.dxrow.to(t["dx"].device), :D]
    for k in ("dx16", "dproj"):
        if k in c.init:
            out[k] = t[k][:M]
    for k in ("dw", "db", "dgamma"):
        if k in c.init:
            out[k] = t[k][:D]
    return out


def run_gpu(ops, c, dev="cuda"):
    """One call of the case on the device -> {"ratios": {output: ratio}, "at": {output: where}, "canary": {buffer: changed elements}}
    (+ for a dropout case "dropped", "dropped_exact", "mixed_passes", "dead_rows")."""
    t = device_buffers(c, dev)
    res, mask, spec = {}, None, None
    if c.drop:
        p, pp, rpp = c.drop
        rng = torch.tensor([123, 456, 7, 0], dtype=torch.int32, device=dev)
        ones = torch.ones(c.M, c.D, device=dev)
        alive = [True]
        for path_site in range(41, 73):      # the first DropPath site that drops one pass and keeps another (the mask is read from the device)
            spec = ops.dropout_spec(rng, 40, p, path_site, pp, rpp)
            mk = torch.zeros(c.M, c.D, device=dev)
            ops.dropout_f32(ones, mk, c.M, c.D, spec)
            torch.cuda.synchronize()
            alive = [bool((mk[a:a + rpp] != 0).any()) for a in range(0, c.M, rpp)]
            if pp == 0.0 or (any(alive) and not all(alive)):
                break
        res["mixed_passes"] = pp == 0.0 or (any(alive) and not all(alive))
        mask = mk.to(c.device)
        t["_rng"] = rng
        if pp > 0.0:      # the branch rows of a dropped pass were never written
            for i, a in enumerate(range(0, c.M, rpp)):
                if not alive[i]:
                    t["branch"][a:a + rpp] = NAN
            res["dead_rows"] = sum(min(rpp, c.M - a) for i, a in enumerate(range(0, c.M, rpp)) if not alive[i])
    before = {k: t[k].clone() for k in c.init}
    launch(ops, c, t, spec)
    torch.cuda.synchronize()
    got = {k: v.to(c.device) for k, v in logical(c, t).items()}
    m = measure(c, got, mask=mask)
    res["ratios"] = {k: v[0] for k, v in m.items()}
    res["at"] = {k: where(k, v[1], c) for k, v in m.items()}
    res["canary"] = {k: check_untouched(before[k], t[k], c.written[k])[0] for k in c.init}
    if c.drop:
        dead = mask == 0
        x = c.bufs["x"][:, :c.D]
        res["dropped"] = int(dead.sum())
        res["dropped_exact"] = bool(torch.equal(got["h"][dead].view(torch.int32), x[dead].view(torch.int32)))
    return res


def failure(name, r):
    """None, or what is wrong with the result of one case."""
    bad = []
    for k, v in r["ratios"].items():
        if not v <= 1.0:
            bad.append(f"worst |got - ref| / bound = {v:.3g} > 1 at {r['at'][k]}")
    for k, n in r["canary"].items():
        if n:
            bad.append(f"{n} elements of the {k} buffer outside the written ones changed")
    if "dropped" in r and not (r["dropped"] > 0 and r["dropped_exact"] and r["mixed_passes"]):
        bad.append(f"dropout: {r['dropped']} dropped elements, h equal to x bit for bit there: {r['dropped_exact']}, "
                   f"a dropped and a kept pass: {r['mixed_passes']}")
    return f"{name}: " + "; ".join(bad) if bad else None


def line(name, r):
    return f"{name}: " + ", ".join(f"{k} {v:.3f}" for k, v in r["ratios"].items()) + f", canaries changed {sum(r['canary'].values())}"
