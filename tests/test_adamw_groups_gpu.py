"""GPU: mt_adamw_step_groups against the kernel it extends.  One grouped launch must equal, BIT FOR BIT in p, m and v, mt_adamw_step
launched on every segment alone with that group's learning rate and weight decay -- no tolerance anywhere: every comparison is on
the int32 view of the buffers, NaN guards included."""
import numpy as np
import pytest
import torch

from modaltune_amd import optim

pytestmark = pytest.mark.gpu

NUMELS = [1, 3, 4, 5, 64, 255, 256, 1027, 4099, 70001]
GUARD = 8                                     # NaN elements in front of and behind every buffer (32 bytes: the payload stays 16-byte aligned)
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
MULTS, DECAYS = (1.0, 0.5, 0.1, 0.0), (0.01, 0.0, 0.3)

PATTERNS = {      # name -> (group id of every tensor, [(lr_mult, weight_decay)] of every group)
    "one": ([0] * 10, [(1.0, 0.01)]),
    "alternating": ([i % 2 for i in range(10)], [(1.0, 0.01), (0.5, 0.0)]),
    "merge": ([0, 1, 1, 0, 1, 0, 0, 1, 0, 1], [(1.0, 0.01), (0.1, 0.3)]),
    "last_alone": ([0] * 9 + [1], [(0.5, 0.3), (0.0, 0.0)]),
    "three": ([i % 3 for i in range(10)], [(1.0, 0.01), (0.5, 0.0), (0.1, 0.3)]),
    "sixteen": ([15, 3, 7, 0, 12, 9, 5, 14, 1, 10], [(MULTS[i % 4], DECAYS[i % 3]) for i in range(16)]),
}
MODES = {      # host values only / everything the step hands over on the device
    "host": dict(lr_dev=False, step_dev=False, scale=None, grad_mult=1.0, step_count=3),
    "device": dict(lr_dev=True, step_dev=True, scale=1024.0, grad_mult=0.5, step_count=0),
}


def _layout():
    offs, o = [], 0
    for n in NUMELS:
        offs.append(o)
        o += (n + 3) // 4 * 4
    return offs, o


@pytest.fixture(scope="module")
def state():
    """Four flat buffers in 16-byte slots between NaN guards (never modified: every run works on clones)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    offs, n = _layout()
    g = torch.Generator().manual_seed(11)
    used = torch.zeros(n, dtype=torch.bool)
    for o, k in zip(offs, NUMELS):
        used[o:o + k] = True
    bufs = {}
    for name, draw in (("p", lambda: torch.randn(n, generator=g)), ("g", lambda: 0.1 * torch.randn(n, generator=g)),
                       ("m", lambda: 0.05 * torch.randn(n, generator=g)), ("v", lambda: 0.01 * torch.rand(n, generator=g))):
        body = torch.where(used, draw(), torch.zeros(n))
        full = torch.full((n + 2 * GUARD,), float("nan"))
        full[GUARD:GUARD + n] = body
        bufs[name] = full.cuda()
    return {"offs": offs, "n": n, "used": used.cuda(), "bufs": bufs}


def _table(st, pattern):
    ids, hp = PATTERNS[pattern]
    end, grp = optim.segment_table([(o, k, i) for o, k, i in zip(st["offs"], NUMELS, ids)])
    return end, grp, hp


def _clones(st):
    c = {k: t.clone() for k, t in st["bufs"].items()}
    return c, {k: t[GUARD:GUARD + st["n"]] for k, t in c.items()}


def _shared(mode):
    mo = MODES[mode]
    dev = "cuda"
    return dict(scale=None if mo["scale"] is None else torch.full((1,), mo["scale"], device=dev), grad_mult=mo["grad_mult"],
                step_dev=torch.full((1,), 4, dtype=torch.int32, device=dev) if mo["step_dev"] else None,
                found_inf=torch.zeros(1, dtype=torch.int32, device=dev)), mo


def _grouped(st, pattern, mode, pieces=None, found_inf=0, hp=None):
    """The grouped launch over `pieces` (default: the whole buffer) on fresh clones; returns the full buffers, guards included."""
    from modaltune_amd import ops
    end, grp, hp0 = _table(st, pattern)
    hp = hp0 if hp is None else hp
    full, view = _clones(st)
    kw, mo = _shared(mode)
    kw["found_inf"].fill_(found_inf)
    lr_dev = torch.full((1,), LR, device="cuda") if mo["lr_dev"] else None
    end_d, grp_d = end.cuda(), grp.cuda()
    for o, k in (pieces or [(0, st["n"])]):
        ops.adamw_step_groups(view["p"][o:o + k], view["g"][o:o + k], view["m"][o:o + k], view["v"][o:o + k], k, o, end_d, grp_d, hp,
                              123.0 if mo["lr_dev"] else LR, B1, B2, EPS, mo["step_count"], lr_dev=lr_dev, **kw)
    torch.cuda.synchronize()
    return full


_REF = {}


def _reference(st, pattern, mode):
    """mt_adamw_step on every segment alone, lr = the group's lr_g (as the fp32 value the grouped kernel forms), its weight decay.
    Computed once per (pattern, mode) and shared."""
    if (pattern, mode) in _REF:
        return _REF[(pattern, mode)]
    from modaltune_amd import ops
    end, grp, hp = _table(st, pattern)
    full, view = _clones(st)
    kw, mo = _shared(mode)
    a = 0
    for b, gid in zip(end.tolist(), grp.tolist()):
        lm, wd = hp[gid]
        lr_g = float(np.float32(np.float64(np.float32(LR)) * np.float64(lm)))
        lr_dev = torch.full((1,), lr_g, device="cuda") if mo["lr_dev"] else None
        ops.adamw_step(view["p"][a:b], view["g"][a:b], view["m"][a:b], view["v"][a:b], b - a, 123.0 if mo["lr_dev"] else lr_g, B1, B2, EPS, wd,
                       mo["step_count"], lr_dev=lr_dev, **kw)
        a = b
    assert a == st["n"]
    torch.cuda.synchronize()
    _REF[(pattern, mode)] = full
    return full


def _bits(t):
    return t.view(torch.int32)


def _same(a, b):
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in ("p", "g", "m", "v"))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_one_grouped_launch_is_the_existing_kernel_on_every_segment(state, pattern, mode):
    got, want = _grouped(state, pattern, mode), _reference(state, pattern, mode)
    for k in ("p", "m", "v", "g"):
        diff = int((_bits(got[k]) != _bits(want[k])).sum())
        assert diff == 0, f"{k}: {diff} words differ from the per-segment launches of mt_adamw_step"
    # the update happened (p, m and v all moved somewhere), the guards are still NaN, the gradient was only read
    n, init = state["n"], state["bufs"]
    assert all(not torch.equal(_bits(got[k]), _bits(init[k])) for k in ("m", "v")) and torch.equal(_bits(got["g"]), _bits(init["g"]))
    assert all(bool(torch.isnan(got[k][:GUARD]).all()) and bool(torch.isnan(got[k][GUARD + n:]).all()) for k in ("p", "m", "v"))
    # the slot padding is +0 afterwards: all bits zero
    pad = ~state["used"]
    assert int(pad.sum()) > 0 and all(int((_bits(got[k][GUARD:GUARD + n])[pad] != 0).sum()) == 0 for k in ("p", "m", "v"))


def test_one_group_is_the_existing_kernel_over_the_whole_buffer(state):
    """(_reference's segment list is the whole buffer for one group: spelled out once, with the call the trainer makes.)"""
    from modaltune_amd import ops
    full, view = _clones(state)
    n = state["n"]
    ops.adamw_step(view["p"], view["g"], view["m"], view["v"], n, LR, B1, B2, EPS, 0.01, 3)
    torch.cuda.synchronize()
    assert _same(full, _grouped(state, "one", "host"))


@pytest.mark.parametrize("pattern", ["alternating", "sixteen"])
def test_pieces_compose_and_leave_everything_else_alone(state, pattern):
    n, init = state["n"], state["bufs"]
    whole = _reference(state, pattern, "device")
    singles = [0, 3, 6, state["offs"][7] + 1026, state["offs"][9] - 1, n - 1]          # k = 1: vector heads, tails, a tensor's last element
    for pieces in ([(0, n)], [(5, 1030)], [(n - 7, 7)], [(o, 1) for o in singles], [(0, 5), (5, 1030), (1035, n - 1035)]):
        got = _grouped(state, pattern, "device", pieces=pieces)
        inside = torch.zeros(n + 2 * GUARD, dtype=torch.bool, device="cuda")
        for o, k in pieces:
            inside[GUARD + o:GUARD + o + k] = True
        for k in ("p", "m", "v"):
            want = torch.where(inside, _bits(whole[k]), _bits(init[k]))
            diff = int((_bits(got[k]) != want).sum())
            assert diff == 0, f"pieces {pieces[:3]}: {diff} words of {k} differ (inside: the whole launch's bits; outside: untouched)"


def test_a_set_found_inf_changes_no_byte(state):
    for mode in MODES:
        got = _grouped(state, "three", mode, found_inf=1)
        assert _same(got, state["bufs"])


def test_a_group_with_lr_mult_0_and_no_decay_keeps_its_parameter_bits_while_its_moments_move(state):
    n, init = state["n"], state["bufs"]
    got = _grouped(state, "last_alone", "device")
    o, k = GUARD + state["offs"][9], NUMELS[9]
    assert torch.equal(_bits(got["p"][o:o + k]), _bits(init["p"][o:o + k]))                      # frozen: every bit
    assert int((_bits(got["m"][o:o + k]) != _bits(init["m"][o:o + k])).sum()) > k // 2 and \
        int((_bits(got["v"][o:o + k]) != _bits(init["v"][o:o + k])).sum()) > k // 2               # the moments keep updating
    assert int((_bits(got["p"][GUARD:o]) != _bits(init["p"][GUARD:o])).sum()) > (o - GUARD) // 2  # ... and the neighbours trained


def test_seventeen_groups_are_unsupported(state):
    with pytest.raises(RuntimeError, match=r"unsupported configuration \(-3\)"):
        _grouped(state, "one", "host", hp=[(1.0, 0.01)] * 17)
    with pytest.raises(RuntimeError, match=r"unsupported configuration \(-3\)"):
        _grouped(state, "one", "host", hp=[])
