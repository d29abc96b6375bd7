"""GPU: the kernels behind global-norm clipping -- mt_grad_sumsq (sum of squares in double, two launches, no atomics on floats),
mt_grad_clip_coef (torch's clip_grad_norm_ coefficient on the device) and mt_adamw_step driven through `scale / coef`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SKIP_PATTERN = [0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0]      # test_kernels_gpu.py's: back-off, growth at the interval, two skips in a row


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from modaltune_amd import ops as _ops
    return _ops


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def rng(seed):
    return torch.Generator().manual_seed(seed)


SUMSQ_GRID_CAP = 2048 * 256 * 4 * 4            # mt_grad_sumsq stage 1: 2048 workgroups x 256 threads x 4 float4 loads before the grid stride
SIZES = [1, 3, 4, 5, 63, 64, 65, 1023, 10007, SUMSQ_GRID_CAP + 77]
FMAX = float(np.finfo(np.float32).max)


@pytest.fixture(scope="module")
def base():
    """One random vector for every case (host copy + device copy; cases are slices of it at every alignment)."""
    x = torch.randn(SIZES[-1] + 3, generator=rng(2024))
    return x.numpy(), x.to(DEV)


def _sumsq(ops, g, found=None, fill=float("nan")):
    n = g.numel()
    ws = torch.full((ops.grad_sumsq_partials_elems(n),), fill, dtype=torch.float64, device=DEV)      # (the workspace needs no initialisation)
    out = torch.full((1,), fill, dtype=torch.float64, device=DEV)
    ops.grad_sumsq(g, n, ws, out, found)
    return out


@pytest.mark.parametrize("n", SIZES)
def test_grad_sumsq_against_float64_at_every_alignment(ops, base, n):
    """sumsq against numpy float64 for g at 0 .. 3 floats behind a 16-byte boundary (scalar head and tail, float4 body, the grid
    stride at the largest n): relative <= 1e-12 -- double accumulation of <= 2^24 terms errs by <= 2^24 * 2^-53 = 2e-9 in the worst
    case and by about sqrt(n) * 2^-53 (3e-13 at the largest n) in practice.  Two calls give the same bits; the partials workspace and
    the output start as NaN; a clean vector leaves the flag alone."""
    host, dev = base
    assert dev.data_ptr() % 16 == 0
    assert ops.grad_sumsq_partials_elems(n) == min(2048, -(-n // 4096))
    found = torch.zeros(1, dtype=torch.int32, device=DEV)
    for off in range(4):
        g = dev[off:off + n]
        want = float(np.square(host[off:off + n].astype(np.float64)).sum())
        a, b = _sumsq(ops, g, found), _sumsq(ops, g, found, fill=-1.0)
        err = abs(float(a) - want) / want
        print(f"grad_sumsq n={n} offset={off}: relative error {err:.3e}")
        assert err <= 1e-12, (n, off, float(a), want)
        assert torch.equal(a, b), (n, off, "two calls, two results")
    assert int(found) == 0


@pytest.mark.parametrize("n", [1, 63, 64, 65, 10007, SUMSQ_GRID_CAP + 77])
def test_grad_sumsq_flag_follows_check_finite(ops, base, n):
    """inf / -inf / NaN at the positions test_check_finite_positions_values_and_sticky_flag uses (first, last, first element of the last
    partial wave; behind the grid capacity at the largest n): the flag is set, ORed and never cleared, also without a flag pointer
    nothing faults; +-FLT_MAX and subnormals are finite.  mt_grad_clip_coef behind a set flag: coef == 1, out[2] == scale."""
    host, dev = base
    xd = torch.empty(n + 1, device=DEV)[1:]          # (4 bytes behind a 16-byte boundary)
    xd.copy_(dev[:n])
    for j, sv in enumerate([FMAX, -FMAX, 1e-40, -1e-40, 2.0 ** -149, float(np.finfo(np.float32).tiny)]):
        xd[(j * 7919 + n - 1) % n] = sv
    found = torch.zeros(1, dtype=torch.int32, device=DEV)
    s = _sumsq(ops, xd, found)
    assert int(found) == 0 and np.isfinite(float(s))
    _sumsq(ops, xd, None)
    positions = {0, n - 1, (n - 1) // 64 * 64}
    if n > SUMSQ_GRID_CAP:
        positions |= {SUMSQ_GRID_CAP, SUMSQ_GRID_CAP + 64, n - 70}
    scale = torch.tensor([2.0 ** 15], device=DEV)
    out = torch.zeros(3, device=DEV)
    for pos in sorted(positions):
        for bad in (float("inf"), float("-inf"), float("nan")):
            keep = xd[pos].clone()
            xd[pos] = bad
            found.zero_()
            s = _sumsq(ops, xd, found)
            assert int(found) == 1 and not np.isfinite(float(s)), (pos, bad)
            ops.grad_clip_coef(s, 1, 0.5, scale, 1e-3, found, out)
            o = out.cpu()
            assert float(o[1]) == 1.0 and float(o[2]) == 2.0 ** 15 and not np.isfinite(float(o[0])), (pos, bad, o)
            xd[pos] = keep
            _sumsq(ops, xd, found)                # a clean vector behind a dirty one: the flag stays
            assert int(found) == 1, (pos, bad, "sticky")
    found.zero_()
    _sumsq(ops, xd, found)
    assert int(found) == 0


def _ulp32(a):
    return float(np.spacing(np.abs(np.float32(a))))


@pytest.mark.parametrize("nsums", [1, 3])
@pytest.mark.parametrize("scale", [None, 2.0 ** 15, 3.0])
def test_grad_clip_coef_against_the_float64_formula(ops, nsums, scale):
    """out = {norm, coef, scale / coef} against sqrt(S) * grad_mult / scale, min(1, max_norm / (norm + 1e-6)) and scale / coef in
    float64: 1 fp32 ulp each (computed in double, rounded once).  norm <= max_norm and max_norm = +inf: coef == 1 and out[2] is the
    scale bit for bit."""
    sums = torch.tensor([1234.5678, 0.25, 98765.4321][:nsums], dtype=torch.float64)
    S = 0.0
    for v in sums.tolist():
        S += v
    sc = 1.0 if scale is None else scale
    scale_dev = None if scale is None else torch.tensor([scale], device=DEV)
    gm = 1.0 / 6.0
    norm = np.sqrt(S) * gm / sc
    out = torch.zeros(3, device=DEV)
    for max_norm in (norm * 0.37, norm * 0.999, 1e-3, norm * 1.5, 1e9, float("inf")):
        ops.grad_clip_coef(sums.to(DEV), nsums, gm, scale_dev, max_norm, None, out)
        o = out.cpu().double().numpy()
        coef = min(1.0, max_norm / (norm + 1e-6))
        assert abs(o[0] - norm) <= _ulp32(norm), (max_norm, o[0], norm)
        assert abs(o[1] - coef) <= _ulp32(coef), (max_norm, o[1], coef)
        if coef == 1.0:
            assert o[1] == 1.0 and np.float32(o[2]) == np.float32(sc), (max_norm, o)
        else:
            assert o[1] < 1.0 and abs(o[2] - sc / coef) <= _ulp32(sc / coef), (max_norm, o[2], sc / coef)


def test_grad_clip_coef_norm_that_overflows_fp32(ops):
    """A vector of +-FLT_MAX is finite (flag clear) and its sum of squares is finite in double; its norm is +inf in fp32, coef = 0 as with
    torch, and AdamW driven by out[2] sees a zero gradient: no NaN reaches a parameter or a moment."""
    n = 1000
    g = torch.full((n,), FMAX, device=DEV)
    g[::2] = -FMAX
    found = torch.zeros(1, dtype=torch.int32, device=DEV)
    s = _sumsq(ops, g, found)
    assert int(found) == 0 and np.isfinite(float(s)) and abs(float(s) / (n * FMAX ** 2) - 1.0) < 1e-12
    out = torch.zeros(3, device=DEV)
    ops.grad_clip_coef(s, 1, 1.0, None, 1.0, found, out)
    o = out.cpu()
    assert float(o[0]) == float("inf") and float(o[1]) == 0.0
    p, m, v = torch.ones(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    ops.adamw_step(p, g, m, v, n, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, scale=out[2:3], found_inf=found)
    assert all(bool(torch.isfinite(t).all()) for t in (p, m, v))
    assert float(m.abs().max()) == 0.0 and float(v.abs().max()) == 0.0


def test_clipped_adamw_over_a_sequence_with_skips(ops):
    """test_adamw_step_device_state_over_a_sequence_with_skips with the clip in front: mt_grad_sumsq (the flag), mt_grad_clip_coef,
    mt_adamw_step with out + 2 as its scale, mt_scaler_update; max_norm is the median float64 norm of the clean steps' averaged
    gradients, so half of them clip.  Oracle: adamw_update fed coef * grad_mult * g with coef from float64; that test's bar,
    rel < 1e-6 on p, m and v; skipped steps leave all three bit-identical."""
    from oracle import modaltune_oracle as O
    n, lr, gm = 10007, 1e-3, 0.5
    g = rng(31)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) for _ in SKIP_PATTERN]
    norms = [float(gr.double().norm()) * gm for gr, f in zip(grads, SKIP_PATTERN) if not f]
    max_norm = float(np.median(norms))
    assert 2 <= sum(nm > max_norm for nm in norms) <= len(norms) - 2
    p, m, v = p0.to(DEV).clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    scale = torch.tensor([8.0], device=DEV)
    tracker = torch.zeros(1, dtype=torch.int32, device=DEV)
    found = torch.zeros(1, dtype=torch.int32, device=DEV)
    step_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    lr_dev = torch.full((1,), lr, device=DEV)
    lr_ref = float(lr_dev.cpu())
    out = torch.zeros(3, device=DEV)
    pr, mr, vr = p0.double(), torch.zeros(n).double(), torch.zeros(n).double()
    bad_values, bad_at = [float("inf"), float("nan"), float("-inf")], [n - 1, n // 2, 0]
    clean = skipped = clipped = 0
    for i, (f, gr) in enumerate(zip(SKIP_PATTERN, grads)):
        s = float(scale)
        gd = (gr * s).to(DEV)                     # (s is a power of two: the scaled gradient is exact)
        if f:
            gd[bad_at[skipped % 3]] = bad_values[skipped % 3]
            skipped += 1
        before = (p.clone(), m.clone(), v.clone())
        ss = _sumsq(ops, gd, found)
        ops.grad_clip_coef(ss, 1, gm, scale, max_norm, found, out)
        ops.adamw_step(p, gd, m, v, n, 123.0, 0.9, 0.999, 1e-8, 0.01, 0, out[2:3], found, grad_mult=gm, step_dev=step_dev, lr_dev=lr_dev)
        torch.cuda.synchronize()
        assert int(found) == f, i
        o = out.cpu().double().numpy()
        if f:
            assert torch.equal(p, before[0]) and torch.equal(m, before[1]) and torch.equal(v, before[2]), i
            assert o[1] == 1.0 and o[2] == s, (i, o)
        else:
            clean += 1
            norm = float(gr.double().norm()) * gm
            coef = min(1.0, max_norm / (norm + 1e-6))
            clipped += coef < 1.0
            assert abs(o[0] - norm) <= 1e-6 * norm and abs(o[1] - coef) <= 1e-6, (i, o, norm, coef)
            pr, mr, vr = O.adamw_update(pr, coef * gm * gr.double(), mr, vr, clean, lr_ref)
        ops.scaler_update(scale, tracker, found, step_dev, 2.0, 0.5, 3)
        assert int(step_dev) == clean and int(found) == 0, i
    assert clean == SKIP_PATTERN.count(0) and 2 <= clipped <= clean - 2 and float(scale) != 8.0
    print("clipped adamw:", rel(p, pr), rel(m, mr), rel(v, vr), "clipped", clipped, "of", clean)
    assert rel(p, pr) < 1e-6 and rel(m, mr) < 1e-6 and rel(v, vr) < 1e-6, (rel(p, pr), rel(m, mr), rel(v, vr))
    assert rel(p, p0) > 1e-4
