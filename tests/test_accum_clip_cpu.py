"""CPU: the host side of gradient accumulation and global-norm clipping -- the three C entry points answer without a device, and
modaltune_amd.optim.clip_grad_norm_ falls back to torch's own call wherever its fast path does not apply."""
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_PROBE = r'''
import ctypes as C
import sys
sys.path.insert(0, %r)
from modaltune_amd import _lib
lib = _lib.load()
elems = lib.mt_grad_sumsq_partials_elems
ns = sorted(set([1, 2, 3, 4, 5, 4095, 4096, 4097, 2048 * 4096 - 1, 2048 * 4096, 2048 * 4096 + 1, 1 << 24]
                + [1 << k for k in range(25)] + [(1 << k) + 1 for k in range(24)] + list(range(1, 1 << 24, 65537))))
vals = [elems(n) for n in ns]
print("elems_positive", int(all(v >= 1 for v in vals)))
print("elems_monotone", int(all(a <= b for a, b in zip(vals, vals[1:]))))
print("elems_first_last", vals[0], vals[-1])
print("elems_zero", elems(0), elems(-5))
keep = (C.c_double * 4)(), (C.c_float * 4)()          # host memory: only the pointers matter, nothing reads through them
d, f = C.addressof(keep[0]), C.addressof(keep[1])
# mt_grad_sumsq(g, n, partials, partials_elems, sumsq, found_inf, stream)
print("sumsq", lib.mt_grad_sumsq(None, 8, d, 4, d, None, None), lib.mt_grad_sumsq(f, 0, d, 4, d, None, None),
      lib.mt_grad_sumsq(f, 8, None, 4, d, None, None), lib.mt_grad_sumsq(f, 8, d, 4, None, None, None),
      lib.mt_grad_sumsq(f, 8, d, 0, d, None, None), lib.mt_grad_sumsq(f + 2, 8, d, 4, d, None, None))
# mt_grad_clip_coef(sumsq, nsums, grad_mult, scale, max_norm, found_inf, out, stream)
print("coef", lib.mt_grad_clip_coef(None, 1, 1.0, None, 1.0, None, f, None), lib.mt_grad_clip_coef(d, 0, 1.0, None, 1.0, None, f, None),
      lib.mt_grad_clip_coef(d, 1, 1.0, None, 1.0, None, None, None), lib.mt_grad_clip_coef(d, 1, 1.0, None, -1.0, None, f, None),
      lib.mt_grad_clip_coef(d, 1, 1.0, None, float("nan"), None, f, None), lib.mt_grad_clip_coef(d, 1, 0.0, None, 1.0, None, f, None))
'''


def test_clip_entry_points_answer_on_the_host():
    """mt_grad_sumsq_partials_elems: positive and non-decreasing over n = 1 .. 2^24, negative at n <= 0; mt_grad_sumsq and
    mt_grad_clip_coef return a negative MtStatus for null pointers, zero sizes, a workspace that is too small, a misaligned pointer and
    a negative / NaN max_norm -- before any HIP call (a child process, as in test_abi.py: there is no GPU here)."""
    import __graft_entry__ as ge
    ge.build()
    p = subprocess.run([sys.executable, "-c", _PROBE % ROOT], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-400:] + p.stderr[-400:]
    rows = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in p.stdout.splitlines()}
    assert rows["elems_positive"] == [1] and rows["elems_monotone"] == [1]
    assert rows["elems_first_last"] == [1, 2048]                      # (capped like the other streaming kernels)
    assert all(v < 0 for v in rows["elems_zero"])
    assert len(rows["sumsq"]) == 6 and all(v < 0 for v in rows["sumsq"]), rows["sumsq"]
    assert len(rows["coef"]) == 6 and all(v < 0 for v in rows["coef"]), rows["coef"]


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(s, generator=g, requires_grad=True) for s in [(7, 5), (11,), (3, 2, 4)]]
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g) * 3.0
    return ps


def test_clip_grad_norm_falls_back_to_torch_on_cpu_tensors_and_other_norms():
    """CPU tensors (norm_type 2) and norm_type 1 / inf: the same returned norm and the same clipped gradients as
    torch.nn.utils.clip_grad_norm_, bit for bit -- it IS that call."""
    from modaltune_amd.optim import clip_grad_norm_
    for norm_type, max_norm in [(2.0, 0.5), (2.0, 1e9), (1.0, 0.5), (float("inf"), 0.1)]:
        a, b = _params(3), _params(3)
        na = clip_grad_norm_(a, max_norm, norm_type=norm_type)
        nb = torch.nn.utils.clip_grad_norm_(b, max_norm, norm_type=norm_type)
        assert torch.equal(na, nb), (norm_type, na, nb)
        assert all(torch.equal(p.grad, q.grad) for p, q in zip(a, b))
    one = _params(5)[0]
    ref = _params(5)[0]
    assert torch.equal(clip_grad_norm_(one, 0.1), torch.nn.utils.clip_grad_norm_(ref, 0.1)) and torch.equal(one.grad, ref.grad)


def test_trainstep_rejects_bad_window_arguments():
    """The constructor's checks need no device: they run before anything is allocated."""
    import pytest
    from modaltune_amd.trainer import TrainStep

    class _Eng:
        device = "cpu"
    for kw in (dict(accumulate=0), dict(accumulate=-2), dict(max_grad_norm=-1.0), dict(max_grad_norm=float("nan"))):
        with pytest.raises(ValueError):
            TrainStep(_Eng(), **kw)
