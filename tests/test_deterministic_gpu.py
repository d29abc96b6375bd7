"""GPU: the deterministic forms (MtLaunchOpts.partials, include/modaltune_hip.h; ops: det=) of the six launchers that sum a parameter gradient over workgroups
with fp32 atomics.  Every case checks

  (a) the reduced outputs against the float64 restatement tests/test_kernels_gpu.py uses for the default form, at the bar that test
      carries (its asserts hold the literals: gemm_tn / colsum 1e-4, LayerNorm dw / db 1e-4, injector dk / dv 1e-3, extractor dq 3e-3;
      the injector's dgamma, which has no kernel test of its own, takes the LayerNorm bar -- the same fp32 sum of M products per column);
  (b) ten launches from identical inputs: torch.equal;
  (c) the partial workspace pre-filled with NaN, and a larger allocation entered at an offset and pre-filled with 1e30: finite results,
      the same bits -- no slot is read that the call did not write;
  (d) destinations pre-filled with random values: the `+=` of the default form;
  (e) every output that is not reduced across workgroups: torch.equal to the default kernel's.

Shapes: the smallest that cross each boundary (one slot, an exactly full block, one row into the next, several; empty M-splits)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from modaltune_amd import ops  # noqa: E402
from modaltune_amd._lib import rowmap  # noqa: E402

from test_kernels_gpu import _mha_ref, rel, rng  # noqa: E402

DEV = "cuda"
TN_TOL = 1e-4         # test_kernels_gpu.py::test_gemm_tn_and_colsum
LN_TOL = 1e-4         # test_kernels_gpu.py::test_layernorm_fwd_bwd_f32 (dw, db)
INJ_DKV_TOL = 1e-3    # test_kernels_gpu.py::test_inject_attention / test_adapter_width_gpu.py::test_inject_attention_at_width (dk, dv)
EXT_DQ_TOL = 3e-3     # test_kernels_gpu.py::test_extract_attention / test_adapter_width_gpu.py::test_extract_attention_at_width (dq)
REPEATS = 10


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _workspaces(need):
    """(c): the exact size full of NaN; a larger allocation full of 1e30 entered 16 bytes in."""
    nan = torch.full((need,), float("nan"), device=DEV)
    big = torch.full((2 * need + 64,), 1.0e30, device=DEV)
    return nan, big[4:]


def _check_repeatable(run, need, reduced, plain, default):
    """run(det) -> {name: tensor}.  (b), (c), (e); returns the first result."""
    nan_ws, off_ws = _workspaces(need)
    first = run(nan_ws)
    torch.cuda.synchronize()
    for n in reduced + plain:
        assert bool(torch.isfinite(first[n].float()).all()), n
    for _ in range(REPEATS - 1):
        nan_ws.fill_(float("nan"))
        again = run(nan_ws)
        for n in reduced + plain:
            assert torch.equal(first[n], again[n]), n
    other = run(off_ws)
    for n in reduced + plain:
        assert torch.equal(first[n], other[n]), (n, "offset workspace")
    for n in plain:
        assert torch.equal(first[n], default[n]), (n, "differs from the default kernel")
    return first


# ---------------------------------------------------------------- gemm_tn / colsum
@pytest.mark.parametrize("with_colsum", [True, False])
@pytest.mark.parametrize("M,N1,N2,mapped", [(1, 64, 64, False), (33, 192, 768, False), (114, 768, 192, False), (4503, 384, 768, True)])
def test_gemm_tn_and_colsum_det(M, N1, N2, mapped, with_colsum):
    _gpu()
    g = rng(M + N1)
    if mapped:        # rows through a segmented view (seg_rows 1500, seg_stride 1501, row0 1) and a strided C (ldc > N2)
        mp, ldc = rowmap(1500, 1501, 1), N2 + 64
        m = torch.arange(M)
        phys = (m // 1500) * 1501 + 1 + m % 1500
        rows = int(phys.max()) + 1
    else:
        mp, ldc, phys, rows = None, N2, torch.arange(M), M
    A = torch.randn(rows, N1, generator=g).half()
    B = torch.randn(rows, N2, generator=g).half()
    C0 = torch.randn(N1, ldc, generator=g)
    b0 = torch.randn(N1, generator=g)
    Ad, Bd = A.to(DEV), B.to(DEV)
    ref = A[phys].double().t() @ B[phys].double()
    refcs = A[phys].double().sum(0)
    if M == 114:      # four 32-row steps: 4 of the 8 launched splits hold rows
        assert ops.det_elems("gemm_tn_f16", M, N1, N2, 0) == 4 * N1 * N2

    def run(det):
        out, bsum, cs = C0.to(DEV).clone(), b0.to(DEV).clone(), b0.to(DEV).clone()
        ops.gemm_tn(Ad, Bd, out, M, N1, N2, amap=mp, bmap=mp, ldc=ldc, colsum=bsum if with_colsum else None, det=det)
        if with_colsum:
            ops.colsum(Ad, cs, M, N1, amap=mp, det=det)
        return dict(out=out, bsum=bsum, cs=cs)

    need = max(ops.det_elems("gemm_tn_f16", M, N1, N2, int(with_colsum)), ops.det_elems("colsum_f16", M, N1))
    got = _check_repeatable(run, need, ["out", "bsum", "cs"], [], {})
    want = C0.double().clone()
    want[:, :N2] += ref
    fig = dict(C=rel(got["out"], want))
    assert torch.equal(got["out"][:, N2:].cpu(), C0[:, N2:])          # the columns between N2 and ldc are nobody's
    if with_colsum:
        fig.update(colsum=rel(got["bsum"], b0.double() + refcs), colsum_kernel=rel(got["cs"], b0.double() + refcs))
    print(f"gemm_tn_det M={M} {N1}x{N2} colsum={with_colsum}", {k: f"{v:.2e}" for k, v in fig.items()})
    assert max(fig.values()) < TN_TOL, fig


def test_det_launchers_refuse_a_short_or_missing_workspace():
    _gpu()
    M, N1, N2 = 114, 128, 64
    A = torch.zeros(M, N1, dtype=torch.float16, device=DEV)
    B = torch.zeros(M, N2, dtype=torch.float16, device=DEV)
    out = torch.zeros(N1, N2, device=DEV)
    need = ops.det_elems("gemm_tn_f16", M, N1, N2, 0)
    with pytest.raises(RuntimeError, match="bad argument"):
        ops.gemm_tn(A, B, out, M, N1, N2, det=torch.zeros(need - 1, device=DEV))
    with pytest.raises(RuntimeError, match="bad argument"):
        ops.colsum(A, torch.zeros(N1, device=DEV), M, N1, det=torch.zeros(N1 - 1, device=DEV))
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0          # nothing was launched


# ---------------------------------------------------------------- LayerNorm backward (PARAM) / injector residual
def _patch_geometry(M):
    """M = B * L patch rows of a [B, L + 1, D] token buffer (row 0 of a pass is its cls row)."""
    B = 3 if M % 3 == 0 else 1
    L = M // B
    return B, L, L + 1, rowmap(L, L + 1, 1)


@pytest.mark.parametrize("side", ["token", "patch"])
@pytest.mark.parametrize("M", [1, 5, 111, 4503])
def test_layernorm_bwd_det(M, side):
    """token side: fp32 dy / x / dx, dense (tape.Tape.layernorm); patch side: fp16 dy, x and dx rows of the [B, N, D] stream through
    the patch row map, accumulating (Engine._injector / _extractor)."""
    _gpu()
    D = 768
    g = rng(M + (7 if side == "patch" else 0))
    w = (1 + 0.1 * torch.randn(D, generator=g)).to(DEV)
    b = (0.1 * torch.randn(D, generator=g)).to(DEV)
    if side == "token":
        rows, mp, phys = M, None, torch.arange(M)
        dy = torch.randn(M, D, generator=g).to(DEV)
    else:
        B, L, N, mp = _patch_geometry(M)
        rows = B * N
        m = torch.arange(M)
        phys = (m // L) * N + 1 + m % L
        dy = torch.randn(M, D, generator=g).half().to(DEV)
    x = (torch.randn(rows, D, generator=g) * 2 + 0.5).to(DEV)
    dx0 = torch.randn(rows, D, generator=g).to(DEV)
    dw0, db0 = torch.randn(D, generator=g).to(DEV), torch.randn(D, generator=g).to(DEV)
    y = torch.empty(M, D, dtype=torch.float16, device=DEV)
    stats = torch.empty(M, 2, device=DEV)
    ops.layernorm_fwd(x, w, b, y, stats, M, D, xmap=mp)
    xs = x.double().cpu()[phys]
    mean, rstd = stats[:, 0:1].double().cpu(), stats[:, 1:2].double().cpu()
    dyd = dy.double().cpu()
    ref_dw, ref_db = (dyd * (xs - mean) * rstd).sum(0), dyd.sum(0)

    def run(det):
        dx, dw, db = dx0.clone(), dw0.clone(), db0.clone()
        d16 = torch.zeros(M, D, dtype=torch.float16, device=DEV)
        ops.layernorm_bwd(dy, x, w, stats, dx, M, D, xmap=mp, dxmap=mp, accumulate=True, dw=dw, db=db,
                          dx16=d16 if side == "patch" else None, det=det)
        return dict(dx=dx, dw=dw, db=db, d16=d16)

    default = run(None)
    got = _check_repeatable(run, ops.det_elems("layernorm_bwd", M, D), ["dw", "db"], ["dx", "d16"], default)
    fig = dict(dw=rel(got["dw"], dw0.double().cpu() + ref_dw), db=rel(got["db"], db0.double().cpu() + ref_db))
    print(f"layernorm_bwd_det {side} M={M}", {k: f"{v:.2e}" for k, v in fig.items()})
    assert max(fig.values()) < LN_TOL, fig


@pytest.mark.parametrize("M", [1, 5, 111, 4503])
def test_inject_resid_bwd_det(M):
    _gpu()
    D = 768
    B, L, N, pm = _patch_geometry(M)
    g = rng(M + 11)
    dy = torch.randn(B * N, D, generator=g).to(DEV)
    x = torch.randn(L, D, generator=g).to(DEV)            # block 0's source: the shared patch embedding, broadcast to the passes
    xm = rowmap(L, 0, 0)
    proj = torch.randn(M, D, generator=g).half().to(DEV)
    gamma = (0.1 * torch.randn(D, generator=g)).to(DEV)
    dg0 = torch.randn(D, generator=g).to(DEV)
    m = torch.arange(M)
    phys = (m // L) * N + 1 + m % L
    ref = (dy.double().cpu()[phys] * (x.double().cpu()[m % L] + proj.double().cpu())).sum(0)

    def run(det):
        dx, dproj, dg = torch.zeros(B * N, D, device=DEV), torch.zeros(M, D, dtype=torch.float16, device=DEV), dg0.clone()
        ops.inject_resid_bwd(dy, x, proj, gamma, dx, dproj, dg, M, D, dymap=pm, xmap=xm, dxmap=pm, det=det)
        return dict(dx=dx, dproj=dproj, dgamma=dg)

    default = run(None)
    got = _check_repeatable(run, ops.det_elems("inject_resid_bwd", M, D), ["dgamma"], ["dx", "dproj"], default)
    fig = rel(got["dgamma"], dg0.double().cpu() + ref)
    print(f"inject_resid_bwd_det M={M} dgamma {fig:.2e}")
    assert fig < LN_TOL, fig


# ---------------------------------------------------------------- adapter attention cores
# the full cross at the shipped 12 x 16 (rows: one block, an exactly full block, one row into a second block, three blocks); the other
# head dims where a second block and a partial token block meet
ATTN_CASES = [(12, 16, L, T) for L in (37, 512, 513, 1500) for T in (7, 65, 128)] + [(6, 32, 513, 65), (9, 64, 513, 65)]


@pytest.mark.parametrize("heads,hd,L,T", ATTN_CASES)
def test_inject_attn_bwd_det(heads, hd, L, T):
    _gpu()
    E, B = heads * hd, 3
    g = rng(L + T)
    q = torch.randn(B, L, E, generator=g).half()
    k, v = torch.randn(B, T, E, generator=g), torch.randn(B, T, E, generator=g)
    da = torch.randn(B, L, E, generator=g).half()
    dk0, dv0 = torch.randn(B, T, E, generator=g), torch.randn(B, T, E, generator=g)
    qd, kd, vd = q.double().requires_grad_(True), k.double().requires_grad_(True), v.double().requires_grad_(True)
    _mha_ref(qd, kd, vd, heads).backward(da.double())
    qg, kg, vg, dag = q.to(DEV).view(B * L, E), k.to(DEV), v.to(DEV), da.to(DEV).view(B * L, E)
    a = torch.zeros(B * L, E, dtype=torch.float16, device=DEV)
    alse = torch.zeros(B * L, heads, device=DEV)
    ops.inject_attn_fwd(qg, kg, vg, a, B * L, L, T, lse=alse, heads=heads, head_dim=hd)

    def run(det):
        dq, dk, dv = torch.zeros(B * L, E, dtype=torch.float16, device=DEV), dk0.to(DEV), dv0.to(DEV)
        ops.inject_attn_bwd(qg, a, alse, dag, kg, vg, dq, dk, dv, B * L, L, T, heads=heads, head_dim=hd, det=det)
        return dict(dq=dq, dk=dk, dv=dv)

    default = run(None)
    need = ops.det_elems("inject_attn_bwd_hd", B * L, L, T, heads, hd)
    assert need == 2 * math.ceil(L / 512) * B * T * E
    got = _check_repeatable(run, need, ["dk", "dv"], ["dq"], default)
    fig = dict(dk=rel(got["dk"], dk0.double() + kd.grad), dv=rel(got["dv"], dv0.double() + vd.grad))
    print(f"inject_attn_bwd_det {heads}x{hd} L={L} T={T}", {n: f"{x:.2e}" for n, x in fig.items()})
    assert max(fig.values()) < INJ_DKV_TOL, fig


@pytest.mark.parametrize("heads,hd,L,T", ATTN_CASES)
def test_extract_attn_bwd_det(heads, hd, L, T):
    _gpu()
    E, B = heads * hd, 3
    g = rng(L + T + 1)
    q = torch.randn(B, T, E, generator=g)
    kv = torch.randn(B, L, 2 * E, generator=g).half()
    dout = torch.randn(B, T, E, generator=g)
    dq0 = torch.randn(B, T, E, generator=g)
    qd, kvd = q.double().requires_grad_(True), kv.double().requires_grad_(True)
    _mha_ref(qd, kvd[..., :E], kvd[..., E:], heads).backward(dout.double())
    qg, kvg, dog = q.to(DEV), kv.to(DEV).view(B * L, 2 * E), dout.to(DEV)
    out, lse = torch.zeros(B, T, E, device=DEV), torch.zeros(B, T, heads, device=DEV)
    kps = -(-(-(-L // max(1, min(64, L // 256)))) // 64) * 64       # (the engine's split rule)
    nsplit = -(-L // kps)
    pa, pml = torch.zeros(B * heads * nsplit * T * hd, device=DEV), torch.zeros(B * heads * nsplit * T * 2, device=DEV)
    ops.extract_attn_fwd(qg, kvg, out, lse, pa, pml, B, T, L, nsplit, heads=heads, head_dim=hd)

    def run(det):
        dq, dkv = dq0.to(DEV), torch.zeros(B * L, 2 * E, dtype=torch.float16, device=DEV)
        ops.extract_attn_bwd(qg, kvg, out, lse, dog, dq, dkv, B, T, L, heads=heads, head_dim=hd, det=det)
        return dict(dq=dq, dkv=dkv)

    default = run(None)
    need = ops.det_elems("extract_attn_bwd_hd", B, T, L, heads, hd)
    assert need == math.ceil(L / 512) * B * T * E
    got = _check_repeatable(run, need, ["dq"], ["dkv"], default)
    fig = rel(got["dq"], dq0.double() + qd.grad)
    print(f"extract_attn_bwd_det {heads}x{hd} L={L} T={T} dq {fig:.2e}")
    assert fig < EXT_DQ_TOL, fig
