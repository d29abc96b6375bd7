"""GPU: mt_adamw_step_groups_ema and mt_swap_f32 (csrc/optim.hip).  Every comparison is BIT FOR BIT on the int32 view of the buffers,
NaN guards included: the parameter side is compared GPU against GPU (mt_adamw_step_groups on a copy), the average against the numpy
restatement of its three separately rounded fp32 operations (tests/ema_ref.py) applied to that copy's new parameters.

Sizes: 1, 3, 4, 5 (nothing but head / tail scalars, one vector), 1023, 2055 (more than one workgroup: a workgroup covers 2 * 256
vectors = 2048 elements) and 3073 = 256 * 4 * 3 + 1 (an odd number of workgroup rows and one tail scalar).  Every buffer view starts
0 .. 3 elements behind a 16-byte boundary, so the scalar head in front of the first vector is 0 .. 3 long."""
import numpy as np
import pytest
import torch

from ema_ref import ema_ref

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 1023, 2055, 3073]
OFFSETS = [0, 1, 2, 3]
GUARD = 8                                     # NaN elements in front of and behind every view (32 bytes: the alignment is the offset's)
LR, B1, B2, EPS, DECAY = 1e-3, 0.9, 0.999, 1e-8, 0.9
SCALE, GRAD_MULT = 1024.0, 0.5
GROUPS3 = [(1.0, 0.01), (0.0, 0.0), (0.5, 0.0)]          # group 1 is held still: lr_mult = 0, weight_decay = 0
NAMES = ("p", "g", "m", "v", "ema")


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _bits(t):
    return t.view(torch.int32)


def _table(kind, off, n):
    """(seg_end, seg_group, groups) over the ABSOLUTE indices [off, off + n): ends are ascending multiples of 4, the last at or behind
    off + n.  "four": four segments over three groups, the second and fourth in the still group."""
    total = (off + n + 3) // 4 * 4
    if kind == "one":
        return [total], [0], [(1.0, 0.01)]
    q = max(4, total // 4 // 4 * 4)
    return [q, 2 * q, 3 * q, max(total, 4 * q)], [0, 1, 2, 1], GROUPS3


def _still_mask(kind, off, n):
    """Which elements of the view lie in a segment of the still group."""
    end, grp, _ = _table(kind, off, n)
    a = np.arange(off, off + n)
    seg = np.minimum(np.searchsorted(np.asarray(end), a, side="right"), len(end) - 1)
    return torch.from_numpy(np.asarray(grp)[seg] == 1)


_STATE = {}


def _state(kind, off, n):
    """Five buffers of GUARD + off + n + GUARD elements, NaN outside the view (never modified: every run works on clones).  Values in
    the normal fp32 range: weights ~1e-2, gradients ~1e-3 x SCALE, first moment ~1e-3, second ~1e-6; the average starts a little off
    the parameters -- and ON them, bit for bit, in the still group."""
    key = (kind, off, n)
    if key not in _STATE:
        g = torch.Generator().manual_seed(1000 * n + 10 * off + (kind == "four"))
        body = {"p": 1e-2 * torch.randn(n, generator=g), "g": 1e-3 * SCALE * torch.randn(n, generator=g),
                "m": 1e-3 * torch.randn(n, generator=g), "v": 1e-6 * (0.5 + torch.rand(n, generator=g))}
        body["ema"] = torch.where(_still_mask(kind, off, n), body["p"], body["p"] + 1e-3 * torch.randn(n, generator=g))
        bufs = {}
        for k, b in body.items():
            full = torch.full((GUARD + off + n + GUARD,), float("nan"))
            full[GUARD + off:GUARD + off + n] = b
            bufs[k] = full.cuda()
        _STATE[key] = bufs
    return _STATE[key]


def _clones(bufs, off, n):
    c = {k: t.clone() for k, t in bufs.items()}
    return c, {k: t[GUARD + off:GUARD + off + n] for k, t in c.items()}


def _launch(kind, off, n, *, ema=True, pieces=None, found_inf=0, step_dev=4, step_count=0, decay=DECAY, warmup=False, plain=False):
    """One update of fresh clones: `plain` -- mt_adamw_step_groups (the average is not handed over); else mt_adamw_step_groups_ema with
    the average (or None).  step_dev None: the host's step_count.  Returns the full buffers, guards included."""
    from modaltune_amd import ops
    end, grp, hp = _table(kind, off, n)
    end_d, grp_d = torch.tensor(end, dtype=torch.int32).cuda(), torch.tensor(grp, dtype=torch.uint8).cuda()
    full, view = _clones(_state(kind, off, n), off, n)
    kw = dict(scale=torch.full((1,), SCALE, device="cuda"), grad_mult=GRAD_MULT, lr_dev=torch.full((1,), LR, device="cuda"),
              found_inf=torch.full((1,), found_inf, dtype=torch.int32, device="cuda"),
              step_dev=None if step_dev is None else torch.full((1,), step_dev, dtype=torch.int32, device="cuda"))
    for o, k in (pieces or [(0, n)]):
        args = (view["p"][o:o + k], view["g"][o:o + k], view["m"][o:o + k], view["v"][o:o + k], k, off + o, end_d, grp_d, hp, 123.0, B1, B2, EPS,
                step_count)
        if plain:
            ops.adamw_step_groups(*args, **kw)
        else:
            ops.adamw_step_groups_ema(*args, view["ema"][o:o + k] if ema else None, decay, warmup, **kw)
    torch.cuda.synchronize()
    return full


def _reference(kind, off, n, t, decay=DECAY, warmup=False, **kw):
    """mt_adamw_step_groups on a copy, then ema_ref on the host from the copy's new parameters; t: the 1-based optimiser step."""
    want = _launch(kind, off, n, plain=True, **kw)
    lo, hi = GUARD + off, GUARD + off + n
    e = ema_ref(want["ema"][lo:hi].cpu().numpy(), want["p"][lo:hi].cpu().numpy(), decay, warmup, t)
    want["ema"][lo:hi] = torch.from_numpy(e).cuda()
    return want


def _diff(got, want, what):
    for k in NAMES:
        d = int((_bits(got[k]) != _bits(want[k])).sum())
        assert d == 0, f"{what}: {d} words of {k} differ"


@pytest.mark.parametrize("kind", ["one", "four"])
def test_the_ema_launch_is_the_grouped_launch_plus_the_host_recurrence(kind):
    _gpu()
    for n in SIZES:
        for off in OFFSETS:
            what = f"{kind} n={n} off={off}"
            init = _state(kind, off, n)
            got, want = _launch(kind, off, n), _reference(kind, off, n, t=5)
            _diff(got, want, what)
            lo, hi = GUARD + off, GUARD + off + n
            # the guards are still NaN, the gradient was only read, the average moved wherever it was off the parameters
            for k in NAMES:
                assert bool(torch.isnan(got[k][:lo]).all()) and bool(torch.isnan(got[k][hi:]).all()), (what, k)
            assert torch.equal(_bits(got["g"]), _bits(init["g"]))
            still = _still_mask(kind, off, n).cuda() if kind == "four" else torch.zeros(n, dtype=torch.bool, device="cuda")
            moved = _bits(got["ema"][lo:hi]) != _bits(init["ema"][lo:hi])
            assert bool(moved[~still].all()), what
            # the still group (lr_mult = 0, weight_decay = 0, ema == p on entry): p and the average keep every bit, its moments run
            assert torch.equal(_bits(got["p"][lo:hi])[still], _bits(init["p"][lo:hi])[still]), what
            assert torch.equal(_bits(got["ema"][lo:hi])[still], _bits(init["ema"][lo:hi])[still]), what
            if int(still.sum()):
                assert bool((_bits(got["m"][lo:hi])[still] != _bits(init["m"][lo:hi])[still]).any()), what
            if kind == "four" and n >= 1023:
                assert 0 < int(still.sum()) < n


@pytest.mark.parametrize("off", [0, 3])
def test_one_launch_equals_two_launches_composed_by_index_base(off):
    _gpu()
    n = 2055
    whole = _launch("four", off, n)
    for k in (1025, 1026, 1027, 5, 2050):          # k = 1, 2, 3, 1, 2 mod 4: the second piece's head, the first piece's tail
        got = _launch("four", off, n, pieces=[(0, k), (k, n - k)])
        _diff(got, whole, f"off={off} cut at {k}")
    # ... and a piece alone leaves everything outside it alone
    init = _state("four", off, n)
    got = _launch("four", off, n, pieces=[(1026, 7)])
    inside = torch.zeros_like(init["p"], dtype=torch.bool)
    inside[GUARD + off + 1026:GUARD + off + 1033] = True
    for k in ("p", "m", "v", "ema"):
        assert torch.equal(_bits(got[k]), torch.where(inside, _bits(whole[k]), _bits(init[k]))), k


def test_a_set_found_inf_changes_no_byte():
    _gpu()
    for n, off in ((5, 1), (2055, 2), (3073, 0)):
        got, init = _launch("four", off, n, found_inf=1), _state("four", off, n)
        _diff(got, init, f"found_inf n={n} off={off}")


def test_without_an_average_it_is_the_grouped_launch():
    _gpu()
    for kind in ("one", "four"):
        for n, off in ((3, 3), (1023, 1), (3073, 0)):
            # (decay and warm-up are not read then: out-of-range values pass)
            got, want = _launch(kind, off, n, ema=False, decay=7.0, warmup=True), _launch(kind, off, n, plain=True)
            _diff(got, want, f"ema NULL {kind} n={n} off={off}")
            assert torch.equal(_bits(got["ema"]), _bits(_state(kind, off, n)["ema"]))


# warm-up on: step_dev 0 and 5 take (1 + t) / (10 + t) (t = step_dev + 1: 2 / 11, 7 / 16), 89, 90 and 200 take the decay; 78, 79 and 80
# (t = 79, 80, 81) sit around the step where the ratio reaches 0.9 = 81 / 90
@pytest.mark.parametrize("warmup,step_dev", [(True, s) for s in (0, 5, 89, 90, 200, 78, 79, 80)] + [(False, 0), (False, 200)])
def test_warmup_weight_from_the_device_count_and_from_the_host_count(warmup, step_dev):
    _gpu()
    n, off = 2055, 1
    got = _launch("four", off, n, step_dev=step_dev, warmup=warmup)
    want = _reference("four", off, n, t=step_dev + 1, warmup=warmup, step_dev=step_dev)
    _diff(got, want, f"warmup={warmup} step_dev={step_dev}")
    host = _launch("four", off, n, step_dev=None, step_count=step_dev + 1, warmup=warmup)
    _diff(host, got, f"host step_count {step_dev + 1} against the device count")


def test_warmup_changes_the_average_only_while_it_is_below_the_decay():
    _gpu()
    n, off = 1023, 0
    lo, hi = GUARD + off, GUARD + off + n
    early_on, early_off = _launch("one", off, n, step_dev=0, warmup=True), _launch("one", off, n, step_dev=0, warmup=False)
    assert not torch.equal(_bits(early_on["ema"][lo:hi]), _bits(early_off["ema"][lo:hi]))
    assert all(torch.equal(_bits(early_on[k]), _bits(early_off[k])) for k in ("p", "m", "v"))
    late_on, late_off = _launch("one", off, n, step_dev=200, warmup=True), _launch("one", off, n, step_dev=200, warmup=False)
    _diff(late_on, late_off, "past the warm-up")


# ------------------------------------------------------------------------------------------------ mt_swap_f32
SPECIALS = [0x7FC00001, 0x7F800001, 0xFFC12345, 0x7FFFFFFF, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF]
# (quiet and signalling NaNs with payloads, +-inf, -0.0, the smallest and the largest subnormal)


def _words(n, seed):
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    k = min(n, len(SPECIALS))
    w[rng.permutation(n)[:k]] = np.asarray(SPECIALS[:k], dtype=np.uint32)
    return torch.from_numpy(w.view(np.int32).copy())


@pytest.mark.parametrize("n", SIZES)
def test_swap_moves_bit_patterns_at_every_alignment(n):
    """Every pair of offsets 0 .. 3: equal offsets take the 16-byte form, unequal ones the 4-byte form."""
    _gpu()
    from modaltune_amd import ops
    for oa in OFFSETS:
        for ob in OFFSETS:
            wa, wb = _words(n, 7 * n + oa), _words(n, 11 * n + ob + 100)
            guard_a, guard_b = 0x7FC0AAAA, 0x7FC0BBBB
            fa = torch.full((GUARD + oa + n + GUARD,), guard_a, dtype=torch.int32)
            fb = torch.full((GUARD + ob + n + GUARD,), guard_b, dtype=torch.int32)
            fa[GUARD + oa:GUARD + oa + n], fb[GUARD + ob:GUARD + ob + n] = wa, wb
            a0, b0 = fa.cuda(), fb.cuda()
            a, b = a0.clone(), b0.clone()
            va, vb = a.view(torch.float32)[GUARD + oa:GUARD + oa + n], b.view(torch.float32)[GUARD + ob:GUARD + ob + n]
            ops.swap_f32(va, vb, n)
            torch.cuda.synchronize()
            want_a, want_b = a0.clone(), b0.clone()
            want_a[GUARD + oa:GUARD + oa + n], want_b[GUARD + ob:GUARD + ob + n] = wb.cuda(), wa.cuda()
            assert torch.equal(a, want_a) and torch.equal(b, want_b), (n, oa, ob)
            ops.swap_f32(va, vb)          # (n defaults to the view's length) two swaps: the identity
            torch.cuda.synchronize()
            assert torch.equal(a, a0) and torch.equal(b, b0), (n, oa, ob)


def test_swap_refuses_overlap_and_bad_sizes():
    _gpu()
    from modaltune_amd import ops
    a = torch.zeros(64, device="cuda")
    for x, y, n in ((a[:32], a[16:48], 32), (a[:8], a[:8], 8), (a[:8], a[32:40], 0)):
        with pytest.raises(RuntimeError, match=r"bad argument"):
            ops.swap_f32(x, y, n)
