"""CPU tests of tests/norm_edge_ref.py, the helper tests/test_norm_edges_gpu.py measures the LayerNorm kernels with: a plain float32
emulation of every case of the GPU matrix (every D, dtype triple, form and regime) stays inside the derived per-element bounds, every
planted fault leaves them (the test says in which cases and outputs), the closed-form backward with exact statistics is float64
autograd, the A&S erf polynomial is within the 1.5e-7 csrc/common.h states, the canary check sees a single changed bit, and the three
launchers refuse a leading dimension their vector accesses cannot take."""
import os
import subprocess
import sys

import pytest
import torch

import norm_edge_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_CASES = [n for n, kw in R.MATRIX.items() if not R.on_device(kw["M"])]
FAULT_CASES = [n for n in CPU_CASES if R.MATRIX[n]["M"] in (9, 67)]


def test_the_matrix_names_what_the_issue_lists():
    ms = lambda pre: {kw["M"] for n, kw in R.MATRIX.items() if n.startswith(pre)}
    assert ms("rows-") == set(R.SMALL_M) and ms("cap512-") == set(R.PARAM_M) and set(R.GRID_M) <= ms("grid-")
    for form in R.FORMS:
        assert {kw["M"] for n, kw in R.MATRIX.items() if n.startswith(f"rows-{form}-M")} == set(R.SMALL_M), form
    # every grid cap is crossed by the kernel that has it: 512 (PARAM, DET, inject), 4096 x 4 (ln_grid), 8192 x 2 and 16384 (the packed pair)
    big = lambda **sel: [n for n, kw in R.MATRIX.items() if kw["M"] > 16384 and all(kw.get(k) == v for k, v in sel.items())]
    assert big(kind="fwd", D=256) and big(kind="bwd", D=256) and big(kind="add") and big(kind="fwd", D=3072, gelu=True) and big(kind="bwd", D=3072, gelu=True)
    for n in big(D=3072):
        assert R.case_of(dict(R.MATRIX[n], M=9, live=None)).packed, n
    # every (D, dtypes, gelu) the dispatch accepts
    fwd = {(kw["D"], kw.get("xdt", "f32"), kw.get("odt", "f32"), kw.get("gelu", False)) for kw in R.MATRIX.values() if kw["kind"] == "fwd"}
    assert fwd >= {(D, a, b, g) for D in (256, 768, 2304, 3072) for a, b in (("f32", "f32"), ("f32", "f16"), ("f16", "f16")) for g in (False, True)}
    bwd = {(kw["D"], kw.get("dydt", "f32"), kw.get("xdt", "f32"), kw.get("odt", "f32"), kw.get("gelu", False), kw.get("param", False),
            kw.get("det", False), kw.get("live") is not None) for kw in R.MATRIX.values() if kw["kind"] == "bwd"}
    for D in (256, 768, 2304, 3072):
        for tr in (("f32", "f32", "f32"), ("f16", "f32", "f32"), ("f16", "f32", "f16")):
            assert (D, *tr, False, False, False, False) in bwd and (D, *tr, False, False, False, True) in bwd
            if tr[0] == "f32" or D <= 768:
                assert (D, *tr, False, True, False, False) in bwd and (D, *tr, False, True, True, False) in bwd
        assert (D, "f16", "f16", "f16", True, False, False, False) in bwd
    regimes = {kw.get("regime", "plain") for kw in R.MATRIX.values()}
    assert regimes == set(R.REGIMES) | {"tails"}


def test_the_erf_polynomial_is_within_the_constant_common_h_states():
    z = torch.linspace(0.0, 8.0, 2_000_001, dtype=torch.float64)
    err = float((R.as_erf(z) - torch.erf(z)).abs().max())
    print(f"A&S 7.1.26 in float64 against torch.erf on [0, 8]: worst |error| = {err:.3e}")
    assert err <= R.ERF_ERR
    x = torch.linspace(-8.0, 8.0, 400_001, dtype=torch.float64)
    g, dg, gp, dgp = R.gelu_terms(x)
    assert bool(((R.as_gelu(x) - g).abs() <= dg).all()) and bool(((R.as_gelu(x, grad=True) - gp).abs() <= dgp).all())
    # the float32 evaluation the emulation uses is inside the same bounds
    assert bool(((R.as_gelu(x.float()).double() - R.gelu_terms(x.float().double())[0]).abs() <= R.gelu_terms(x.float().double())[1]).all())


@pytest.mark.parametrize("name", CPU_CASES)
def test_emulation_is_inside_the_bound(name):
    c = R.case_of(R.MATRIX[name])
    ref = R.reference(c)
    m = R.measure(c, R.cpu_emulation(c), ref=ref)
    print(f"{name}: " + ", ".join(f"{k} {v[0]:.3f}" for k, v in m.items()))
    for k, (ratio, at) in m.items():
        assert ratio <= 1.0, R.where(k, at, c)
        bd = ref[k][1][c.cmp[0]:c.cmp[1]] if (c.cmp and k in ("y", "mean", "rstd", "dx")) else ref[k][1]
        assert bd.numel() == 0 or float(bd.min()) > 0.0
    if c.regime == "const" and c.kind == "fwd" and not c.add_period:      # y of a constant row is b, within the bound
        y = ref["y"][0]
        assert float((y - c.b.double()).abs().max()) < 1e-11
    if c.M * c.D > 1_000_000:
        R.make_case.cache_clear()      # (the tensors of the large cases are not kept)


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_fault_is_outside_the_bound(fault):
    hits, tried, worst = [], 0, {}
    for name in FAULT_CASES:
        c = R.case_of(R.MATRIX[name])
        if not R.fault_applies(c, fault):
            continue
        tried += 1
        m = R.measure(c, R.cpu_emulation(c, fault))
        out = {k: v[0] for k, v in m.items() if v[0] > 1.0}
        if out:
            hits.append(name)
            k = max(out, key=out.get)
            key = (c.kind, c.regime, k)
            if out[k] > worst.get(key, (0.0, ""))[0]:
                worst[key] = (out[k], name)
    R.make_case.cache_clear()
    print(f"{fault}: outside the bound in {len(hits)} of the {tried} cases it applies to")
    for (kind, regime, k), (ratio, name) in sorted(worst.items()):
        print(f"    {kind:4s} {regime:10s} {k:6s} worst ratio {ratio:9.3g}  ({name})")
    assert hits, f"{fault} is inside the bound in every case it applies to"
    regimes = {r for (_, r, _) in worst}
    if fault == "onepass_var":
        assert {"mean1000", "nearconst"} <= regimes
    if fault == "bessel":
        assert any(k in ("rstd", "y") and r == "plain" for (_, r, k) in worst)
        # with an fp16 y the divisor hides in the output rounding: the per-row statistics are what sees it
        c = R.case_of(R.MATRIX["regime-plain-fwd-f32-f16-D768"])
        m = R.measure(c, R.cpu_emulation(c, fault))
        assert m["rstd"][0] > 1.0
    if fault == "no_eps":
        assert {"nearconst", "const"} <= regimes
        assert max(v[0] for (_, r, _), v in worst.items() if r == "const") == float("inf")


def test_closed_form_backward_with_exact_statistics_is_float64_autograd():
    torch.manual_seed(3)
    for D, gelu in ((256, False), (768, True)):
        M = 7
        x = (torch.randn(M, D, dtype=torch.float64) * 1.5).requires_grad_(True)
        w, dy = 1 + 0.1 * torch.randn(D, dtype=torch.float64), torch.randn(M, D, dtype=torch.float64)
        v = torch.nn.functional.gelu(x) if gelu else x
        torch.nn.functional.layer_norm(v, (D,), w, None, 1e-5).backward(dy)
        vd = v.detach()
        mean = vd.mean(1, keepdim=True)
        rstd = ((vd - mean).pow(2).mean(1, keepdim=True) + 1e-5).rsqrt()
        xh, g = (vd - mean) * rstd, dy * w
        dx = rstd * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
        if gelu:
            gl, _, gp, _ = R.gelu_terms(x.detach())
            assert float((gl - vd).abs().max()) < 1e-14
            dx = dx * gp
        assert float((dx - x.grad).abs().max()) < 1e-10


def test_reference_with_the_given_statistics_is_the_closed_form_of_the_case():
    c = R.case_of(R.MATRIX["dispatch-bwd-h-f-f-param-D768"])
    ref = R.reference(c)
    x = c.bufs["x"][:, :c.D].double().requires_grad_(True)
    w = c.w.double().requires_grad_(True)
    torch.nn.functional.layer_norm(x, (c.D,), w, None, c.eps32).backward(c.bufs["dy"][:, :c.D].double())
    # (the statistics of the case are the exact ones rounded to fp32: autograd agrees to that rounding)
    assert float((ref["dx"][0] - x.grad).abs().max()) < 1e-4
    assert float((ref["dw"][0] - c.init["dw"][:c.D].double() - w.grad).abs().max()) < 1e-4


def test_maps_padding_and_canaries_of_a_case():
    c = R.case_of(R.MATRIX["maps-bwd-all-L5"])
    assert c.dxrow.tolist()[:6] == [1, 2, 3, 4, 5, 7] and c.lddx == c.D + 4 and c.lddy == c.D + 8
    assert bool(torch.isnan(c.bufs["dy"][0]).all()) and bool(torch.isnan(c.bufs["dy"][:, c.D:]).all()) and bool(torch.isnan(c.bufs["x"][6]).all())
    assert not bool(c.written["dx"][0].any()) and not bool(c.written["dx"][:, c.D:].any()) and not bool(c.written["dx"][-2:].any())
    assert int(c.written["dx"].sum()) == c.M * c.D
    assert bool(torch.isfinite(c.init["dx"][c.dxrow, :c.D]).all())            # accumulating: the old values, NaN around them
    c = R.case_of(R.MATRIX["live-fwd-gelu-packed-M9"])
    assert (c.first, c.end) == (3, 9) and c.packed and int(c.written["y"].sum()) == 6 * c.D and int(c.written["stats"].sum()) == 12
    c = R.case_of(R.MATRIX["dispatch-fwd-x-bcast"])
    assert c.xrow.tolist() == [0, 1, 2, 3, 4, 0, 1, 2, 3] and c.bufs["x"].shape[0] == 5
    c = R.case_of(R.MATRIX["live-fwd-gelu-packed-odd-3rows"])      # an odd live range: the last pair of rows has one row
    assert (c.first, c.end) == (3, 6) and c.packed and int(c.written["y"].sum()) == 3 * c.D
    assert not R.case_of(R.MATRIX["dispatch-fwd-gelu-ld+4-D3072"]).packed and R.case_of(R.MATRIX["dispatch-fwd-gelu-dense-D3072"]).packed


def test_metric_counts_a_nan_as_a_miss_and_names_row_chunk_and_lane():
    c = R.case_of(R.MATRIX["regime-plain-fwd-f32-D768"])
    got = R.cpu_emulation(c)
    got["y"][5, 300] = float("nan")
    ratio, at = R.measure(c, got)["y"]
    assert ratio == float("inf") and at == (5, 300)
    assert "row 5" in R.where("y", at) and "256-column chunk 1, lane 11, element 0" in R.where("y", at)
    p = R.case_of(R.MATRIX["rows-fwd-gelu-packed-M9"])      # the packed pair: 8 columns per lane, two waves per row, two rows per workgroup
    assert p.packed and "wave 1 of the row, its 512-column chunk 2, lane 3, element 5" in R.where("y", (5, 1536 + 1024 + 29), p)
    assert "row 1 of its two-row workgroup" in R.where("y", (5, 0), p)
    q = R.case_of(R.MATRIX["rows-bwd-gelu-packed-M9"])      # backward: three waves per row
    assert "wave 2 of the row, its 512-column chunk 1, lane 63, element 7" in R.where("dx", (5, 3071), q)
    assert R.failure("x", dict(ratios=dict(y=ratio), at=dict(y=R.where("y", at)), canary=dict(y=0))) is not None
    assert R.failure("x", dict(ratios=dict(y=0.5), at=dict(y=""), canary=dict(y=0))) is None
    assert R.failure("x", dict(ratios=dict(y=0.5), at=dict(y=""), canary=dict(y=1))) is not None


@pytest.mark.parametrize("name,buf", [("maps-fwd-y-L5", "y"), ("rows-bwd-param-M9", "dw"), ("rows-inj-engine-M9", "dx"), ("rows-add-M9", "stats")])
def test_canary_check_sees_one_changed_bit_outside_the_written_elements(name, buf):
    c = R.case_of(R.MATRIX[name])
    before = c.init[buf]
    after = before.clone()
    after[c.written[buf]] = 1.0
    assert R.check_untouched(before, after, c.written[buf]) == (0, None)      # (NaN canaries compare by their bits)
    first = int((~c.written[buf].reshape(-1)).nonzero()[0])
    it = torch.int16 if after.dtype == torch.float16 else torch.int32
    after.view(-1).view(it)[first] ^= 1
    assert R.check_untouched(before, after, c.written[buf]) == (1, first)


_PROBE = r'''
import ctypes as C
import sys
sys.path.insert(0, %r)
from modaltune_amd import _lib
lib = _lib.load()
mem = (C.c_float * 64)()          # host memory: the checks answer before anything reads through a pointer
p = C.addressof(mem)
for which, (lddy, ldx, lddx) in dict(ok=(772, 772, 772), lddy=(770, 772, 772), ldx=(772, 769, 772), lddx=(772, 772, 774)).items():
    # D = 512 has no kernel: with well-formed leading dimensions the answer is MT_ERR_UNSUPPORTED, and nothing is ever launched
    print("bwd", which, lib.mt_layernorm_bwd(p, lddy, None, 1, p, ldx, None, 1, 0, p, p, p, lddx, None, 1, 0, None, None, None, None, 4, 512, None, None), flush=True)
    if which != "ok":
        print("inj", which, lib.mt_inject_resid_bwd(p, lddy, None, p, ldx, None, p, p, p, lddx, None, 0, p, p, 4, 768, None, None), flush=True)
    if which in ("lddy", "ldx"):
        print("fwd", which, lib.mt_layernorm_fwd(p, ldx, None, 1, 0, p, p, None, 0, p, lddy if which == "lddy" else 772, None, 1, None, 4, 512, None, None), flush=True)
'''


def test_launchers_refuse_leading_dimensions_their_vector_accesses_cannot_take():
    """mt_layernorm_fwd, mt_layernorm_bwd and mt_inject_resid_bwd read and write rows with 8- and 16-byte vector accesses: a leading
    dimension that is no multiple of 4 elements is MT_ERR_BAD_ARG, before any launch.  In a child process that sees no device."""
    import __graft_entry__ as ge
    ge.build()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, "-c", _PROBE % ROOT], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-400:] + p.stderr[-400:]
    rows = [ln.split() for ln in p.stdout.splitlines() if ln.split()[:1] and ln.split()[0] in ("bwd", "inj", "fwd")]
    assert ["bwd", "ok", "-3"] in rows
    bad = [r for r in rows if r[1] != "ok"]
    assert len(bad) == 8 and all(r[2] == "-1" for r in bad), rows
