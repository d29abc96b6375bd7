"""GPU: mt_layernorm_pool_fwd -- out[b] = LN_post(mean over rows [r0, r1) of LN_pre(x[b, r])) -- against fp64 numpy.

The bar is the one tests/test_kernels_gpu.py holds the LayerNorm forward to against fp64 (test_layernorm_fwd_bwd_f32: max |y - ref| /
max |ref| < 1e-5), on that test's input distribution (x ~ 2 N(0, 1) + 0.5, weight 1 + 0.1 N, bias 0.1 N).  Row counts: 1, 2, the
64-row share of one workgroup and its neighbours 63 / 65 (the one-workgroup form ends at 64), 1 023 and 1 500."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV, D = "cuda", 768
BAR = 1e-5
PRE_EPS, POST_EPS = 1e-5, 1e-6


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from modaltune_amd import ops as _ops
    return _ops


def _ln64(v, w, b, eps):
    m = v.mean(-1, keepdims=True)
    var = ((v - m) ** 2).mean(-1, keepdims=True)
    return (v - m) / np.sqrt(var + eps) * w + b


def _ref(x, r0, r1, pre, post):
    v = x[:, r0:r1, :D].astype(np.float64)
    if pre is not None:
        v = _ln64(v, pre[0].astype(np.float64), pre[1].astype(np.float64), PRE_EPS)
    p = v.mean(axis=1)
    if post is not None:
        p = _ln64(p, post[0].astype(np.float64), post[1].astype(np.float64), POST_EPS)
    return p


def _rel(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / (np.abs(b).max() + 1e-30))


@pytest.fixture(scope="module")
def data():
    """One draw shared by every case: x [3, 1502, ldx = 776], two LayerNorm affines."""
    g = np.random.Generator(np.random.PCG64(20240))
    x = (g.standard_normal((3, 1502, D + 8)) * 2 + 0.5).astype(np.float32)
    aff = [(1 + 0.1 * g.standard_normal(D)).astype(np.float32) if i % 2 == 0 else (0.1 * g.standard_normal(D)).astype(np.float32) for i in range(4)]
    return x, (aff[0], aff[1]), (aff[2], aff[3])


def _run(ops, x, B, rows, ldx, r0, r1, pre, post, poison=True):
    """x: numpy [>= B, >= r1, >= ldx].  Rows outside [r0, r1) and the stride padding are NaN on the device, the workspace holds garbage."""
    xs = np.ascontiguousarray(x[:B, :rows, :ldx]).copy()
    if poison:
        xs[:, :r0] = np.nan
        xs[:, r1:] = np.nan
        xs[:, :, D:] = np.nan
    xd = torch.from_numpy(xs).to(DEV)
    t = lambda p: None if p is None else (torch.from_numpy(p[0]).to(DEV), torch.from_numpy(p[1]).to(DEV))
    ne = ops.layernorm_pool_partials_elems(B, r1 - r0, D)
    part = torch.full((ne,), float("nan"), dtype=torch.float64, device=DEV) if ne else None
    out = torch.full((B, D), float("nan"), device=DEV)
    ops.layernorm_pool_fwd(xd, B, rows, r0, r1, out, pre=t(pre), post=t(post), pre_eps=PRE_EPS, post_eps=POST_EPS, partials=part, ldx=ldx)
    out2 = torch.full((B, D), float("nan"), device=DEV)
    if part is not None:
        part.fill_(-1e300)
    ops.layernorm_pool_fwd(xd, B, rows, r0, r1, out2, pre=t(pre), post=t(post), pre_eps=PRE_EPS, post_eps=POST_EPS, partials=part, ldx=ldx)
    torch.cuda.synchronize()
    assert torch.equal(out, out2)                 # same input, same bits -- whatever the workspace held
    return out.cpu().numpy()


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1023, 1500])
@pytest.mark.parametrize("B", [1, 3])
def test_pooled_readout_against_fp64(ops, data, n, B):
    """Every (pre, post) combination, r0 in {0, 1}, dense and padded strides; poisoned surroundings must not leak."""
    x, pre, post = data
    report = {}
    for r0 in (0, 1):
        for ldx in (D, D + 8):
            for use_pre in (False, True):
                for use_post in (False, True):
                    p, q = (pre if use_pre else None), (post if use_post else None)
                    out = _run(ops, x, B, r0 + n + 1, ldx, r0, r0 + n, p, q)
                    assert np.isfinite(out).all(), (r0, ldx, use_pre, use_post)
                    report[(r0, ldx, use_pre, use_post)] = _rel(out, _ref(x[:B], r0, r0 + n, p, q))
    worst = max(report, key=report.get)
    print(f"rows {n} B {B}: worst {report[worst]:.2e} at (r0, ldx, pre, post) = {worst}")
    assert report[worst] < BAR, report


def test_the_four_reference_readouts(ops, data):
    """cls = rows [0, 1), pool = rows [1, N); with encoder.layer_norm in front (single output) and without (hidden states)."""
    x, pre, post = data
    N = 1501
    for r0, r1 in ((0, 1), (1, N)):
        for p in (pre, None):
            out = _run(ops, x, 2, N, D, r0, r1, p, post, poison=False)
            assert _rel(out, _ref(x[:2], r0, r1, p, post)) < BAR
    # the two LayerNorms do not commute with the mean: the pre-LN form is not the post-only form
    a = _run(ops, x, 1, N, D, 1, N, pre, post, poison=False)
    b = _run(ops, x, 1, N, D, 1, N, None, post, poison=False)
    assert _rel(a, b.astype(np.float64)) > 1e-2


def test_bad_arguments_return_the_documented_status(ops, data):
    from modaltune_amd import _lib
    lib = _lib.load()
    x = torch.zeros(2, 200, D, device=DEV)
    w = torch.ones(D, device=DEV)
    out = torch.zeros(2, D, device=DEV)
    part = torch.zeros(ops.layernorm_pool_partials_elems(2, 199, D), dtype=torch.float64, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    f = lib.mt_layernorm_pool_fwd

    def call(r0=1, r1=200, ldx=D, pw=None, pb=None, parts=part, ne=None, Dd=D, pre_eps=0.0, post_eps=1e-6, xp=None):
        return f(x.data_ptr() if xp is None else xp, ldx, 2, 200, r0, r1, pw, pb, pre_eps, w.data_ptr(), w.data_ptr(), post_eps, out.data_ptr(),
                 None if parts is None else parts.data_ptr(), (0 if parts is None else parts.numel()) if ne is None else ne, Dd, s)
    assert call() == 0
    assert call(r0=5, r1=5) == -1 and call(r1=201) == -1 and call(r0=-1) == -1
    assert call(ldx=D - 4) == -1 and call(ldx=D + 2) == -1
    assert call(pw=w.data_ptr()) == -1                                     # LN_pre's weight without its bias
    assert call(parts=None) == -1 and call(ne=part.numel() - 1) == -1      # a missing / short workspace: before any launch
    assert call(r1=65, parts=None) == 0                                    # 64 rows: one workgroup per pass, no workspace needed
    assert call(xp=x.data_ptr() + 4) == -1                                 # 16-byte loads
    assert call(Dd=1024, ldx=1024) == -3
    assert call(pre_eps=-1e-5) == -1 and call(post_eps=float("nan")) == -1
    assert call(pre_eps=1e-6, pw=w.data_ptr(), pb=w.data_ptr()) == 0
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="layernorm_pool"):
        ops.layernorm_pool_fwd(x, 2, 200, 1, 200, out, partials=None)


def test_torch_op_matches_the_launcher(ops, data):
    import modaltune_amd.torch_ops  # noqa: F401
    x, pre, post = data
    xd = torch.from_numpy(np.ascontiguousarray(x[:2, :300, :D])).to(DEV)
    tw = [torch.from_numpy(a).to(DEV) for a in (*pre, *post)]
    y = torch.ops.modaltune_hip.layernorm_pool_fwd(xd, 1, 300, tw[0], tw[1], PRE_EPS, tw[2], tw[3], POST_EPS)
    assert _rel(y.cpu().numpy(), _ref(x[:2, :300], 1, 300, pre, post)) < BAR
    y0 = torch.ops.modaltune_hip.layernorm_pool_fwd(xd, 0, 1, None, None, PRE_EPS, None, None, POST_EPS)
    assert torch.equal(y0, xd[:, 0])                                       # one row, no LayerNorm: the row itself
