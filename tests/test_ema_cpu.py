"""CPU: the host side of the EMA of the trainable weights -- the two C entry points answer bad arguments without a device, TrainStep
validates its EMA arguments and guards the ema_weights() context before anything touches the GPU, and the checkpoint packs, unpacks
and seals the optional `ema` entry on plain CPU tensors.  Every comparison is an integer, a string or torch.equal."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from modaltune_amd import checkpoint as ck

from ema_ref import ema_decay_t, ema_ref, ema_w
from test_checkpoint_cpu import _checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_PROBE = r'''
import ctypes as C
import sys
sys.path.insert(0, %r)
from modaltune_amd import _lib
lib = _lib.load()
print("version", lib.mt_version())
keep = [(C.c_float * 64)() for _ in range(5)]          # host memory, 16-byte aligned below: only the pointers matter, nothing reads through them
p, g, m, v, e = [(C.addressof(k) + 15) // 16 * 16 for k in keep]
end, grp = (C.c_int * 1)(32), (C.c_ubyte * 1)(0)
end, grp = C.addressof(end), C.addressof(grp)
tab = (_lib.MtAdamGroup * 1)((1.0, 0.01))


def ema_step(p=p, g=g, m=m, v=v, n=32, base=0, ema=e, decay=0.9, warmup=0, step=1):
    return lib.mt_adamw_step_groups_ema(p, g, m, v, n, base, end, grp, 1, tab, 1, 1e-3, 0.9, 0.999, 1e-8, step, None, 1.0, None, None, None,
                                        ema, decay, warmup, None)


print("decay", ema_step(decay=1.0), ema_step(decay=-0.1), ema_step(decay=float("nan")), ema_step(decay=1.5))
print("overlap", ema_step(ema=p), ema_step(ema=p + 16), ema_step(ema=m), ema_step(ema=g + 16))
print("args", ema_step(n=0), ema_step(n=-3), ema_step(p=None), ema_step(g=None), ema_step(m=None), ema_step(v=None), ema_step(step=0),
      ema_step(ema=e + 4), ema_step(ema=e + 2))          # (the last two: the average does not lie in its buffer as index_base says)
print("swap", lib.mt_swap_f32(None, e, 8, None), lib.mt_swap_f32(p, None, 8, None), lib.mt_swap_f32(p, e, 0, None), lib.mt_swap_f32(p, e, -1, None),
      lib.mt_swap_f32(p + 2, e, 8, None), lib.mt_swap_f32(p, p + 16, 8, None))
'''


def test_the_two_entry_points_refuse_bad_arguments_without_a_device():
    """mt_adamw_step_groups_ema: MT_ERR_BAD_ARG (-1) for a decay of 1.0, -0.1, NaN or 1.5, for an average that overlaps p (ema == p, ema
    inside p) or another buffer, for n <= 0, null pointers, no step count, and an average misplaced against index_base; mt_swap_f32: for
    null pointers, n <= 0, a misaligned pointer and overlapping ranges -- all before any HIP call (a child process, as in test_abi.py:
    there is no GPU here)."""
    import __graft_entry__ as ge
    ge.build()
    p = subprocess.run([sys.executable, "-c", _PROBE % ROOT], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-400:] + p.stderr[-400:]
    rows = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in p.stdout.splitlines()}
    assert rows["version"][0] >= 350
    assert rows["decay"] == [-1] * 4, rows["decay"]
    assert rows["overlap"] == [-1] * 4, rows["overlap"]
    assert rows["args"] == [-1] * 9, rows["args"]
    assert rows["swap"] == [-1] * 6, rows["swap"]


def test_entry_points_are_declared_bound_and_wrapped():
    import re
    from modaltune_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "modaltune_hip.h")).read()
    assert re.search(r"\bint\s+mt_adamw_step_groups_ema\s*\(", header) and re.search(r"\bint\s+mt_swap_f32\s*\(", header)
    sig, base = _lib.SIGNATURES["mt_adamw_step_groups_ema"], _lib.SIGNATURES["mt_adamw_step_groups"]
    assert sig == base[:-1] + [_lib.P, _lib.D, _lib.I, _lib.P]          # float* ema, double ema_decay, int ema_warmup in front of the stream
    assert _lib.SIGNATURES["mt_swap_f32"] == [_lib.P, _lib.P, _lib.L, _lib.P]
    assert callable(ops.adamw_step_groups_ema) and callable(ops.swap_f32)


# ---------------------------------------------------------------------------------------------- the reference form itself
def test_reference_weight_and_update():
    """decay_t and w in double: (1 + t) / (10 + t) reaches 0.9 at t = 80 (below it the warm-up side of the min, from there on the
    decay); the update in float32 keeps e == p bit for bit at any w, which decay * e + (1 - decay) * p does not."""
    assert ema_decay_t(0.9, False, 1) == 0.9 and ema_decay_t(0.9, True, 1) == 2.0 / 11.0 and ema_decay_t(0.9, True, 6) == 7.0 / 16.0
    assert ema_decay_t(0.9, True, 79) == 80.0 / 89.0 < 0.9 and ema_decay_t(0.9, True, 80) == 0.9 == 81.0 / 90.0
    assert ema_decay_t(0.9, True, 81) == 0.9 < 82.0 / 91.0 and ema_decay_t(0.9, True, 90) == 0.9 and ema_decay_t(0.9, True, 201) == 0.9
    assert ema_w(0.9, False, 7) == np.float32(1.0 - 0.9) and ema_w(0.9, True, 1) == np.float32(1.0 - 2.0 / 11.0)
    rng = np.random.default_rng(3)
    p = (1e-2 * rng.standard_normal(4096)).astype(np.float32)
    assert np.array_equal(ema_ref(p, p, 0.9, False, 1).view(np.int32), p.view(np.int32))
    blend = (np.float32(0.9) * p + np.float32(1.0 - 0.9) * p).astype(np.float32)
    assert not np.array_equal(blend.view(np.int32), p.view(np.int32))          # (why the kernel uses the difference form)
    e = (1e-2 * rng.standard_normal(4096)).astype(np.float32)
    out = ema_ref(e, p, 0.9, False, 1)
    assert out.dtype == np.float32 and np.allclose(out, 0.9 * e.astype(np.float64) + 0.1 * p.astype(np.float64), rtol=0, atol=1e-8)


# ---------------------------------------------------------------------------------------------- TrainStep, on a bare object
def _bare(cls, **attrs):
    """An object of class `cls` that was never constructed (no device, no library): only what the entry point under test reads."""
    obj = object.__new__(cls)
    obj.__dict__.update(attrs)
    return obj


def test_trainstep_validates_its_ema_arguments_before_anything_is_allocated():
    from modaltune_amd.trainer import TrainStep, _valid_ema_decay

    class _Eng:
        device = "cpu"
    for bad in (1.0, -0.1, 1.5, float("nan"), float("inf"), "0.9", True):
        with pytest.raises(ValueError, match="ema_decay"):
            TrainStep(_Eng(), ema_decay=bad)
        with pytest.raises(ValueError, match="ema_decay"):
            _valid_ema_decay(bad)
    assert _valid_ema_decay(None) is None and _valid_ema_decay(0) == 0.0 and _valid_ema_decay(0.999) == 0.999


def test_set_ema_decay_validates_and_drops_the_captures_only_on_a_change():
    from modaltune_amd.trainer import TrainStep
    dropped = []
    ts = _bare(TrainStep, ema=object(), ema_decay=0.9, ema_warmup=False, _ema_swapped=False)
    ts._drop_captures = lambda: dropped.append(1)
    for bad in (1.0, -0.1, float("nan"), None):
        with pytest.raises(ValueError):
            ts.set_ema_decay(bad)
    assert (ts.ema_decay, ts.ema_warmup, dropped) == (0.9, False, [])
    ts.set_ema_decay(0.9)
    ts.set_ema_decay(0.9, warmup=False)
    assert dropped == []                                   # nothing changed: the captures stay
    ts.set_ema_decay(0.99)
    assert (ts.ema_decay, ts.ema_warmup, dropped) == (0.99, False, [1])
    ts.set_ema_decay(0.99, warmup=True)
    assert (ts.ema_decay, ts.ema_warmup, dropped) == (0.99, True, [1, 1])


def test_without_an_average_every_ema_call_says_so():
    from modaltune_amd.trainer import TrainStep
    ts = _bare(TrainStep, ema=None, ema_decay=None, ema_warmup=False, _ema_swapped=False)
    for call in (lambda: ts.set_ema_decay(0.9), ts.ema_reset, ts.ema_state, lambda: ts.ema_weights().__enter__()):
        with pytest.raises(RuntimeError, match="keeps no average"):
            call()


def test_inside_ema_weights_training_saving_and_nesting_raise():
    """The guards run first, before any argument is looked at or any device call is made: a bare object is enough."""
    from modaltune_amd.trainer import TrainStep
    ts = _bare(TrainStep, ema=object(), ema_decay=0.9, ema_warmup=False, _ema_swapped=True, window_pos=0, accumulate=1)
    calls = {"step()": lambda: ts.step(None, None, None, None), "step_graphed()": lambda: ts.step_graphed(None, None, None, None),
             "finish_window()": ts.finish_window, "state_dict()": ts.state_dict, "load_state_dict()": lambda: ts.load_state_dict({}),
             "ema_weights()": lambda: ts.ema_weights().__enter__(), "ema_reset()": ts.ema_reset}
    for what, call in calls.items():
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value).startswith(what + " inside ema_weights()"), (what, str(e.value))
    # ... and entering inside an open accumulation window
    ts = _bare(TrainStep, ema=object(), ema_decay=0.9, ema_warmup=False, _ema_swapped=False, window_pos=1, accumulate=2)
    with pytest.raises(RuntimeError, match="open accumulation window"):
        ts.ema_weights().__enter__()


# ---------------------------------------------------------------------------------------------- the checkpoint's optional entry
def _with_ema(seed=0):
    sd, slots, n_flat, bufs = _checkpoint(seed)
    g = torch.Generator().manual_seed(seed + 100)
    ema = torch.zeros(n_flat)
    for o, n, _ in slots.values():
        ema[o:o + n] = torch.randn(n, generator=g)
    sd["ema"] = ck.pack_ema(ema, slots, 0.99, True)
    sd["checksums"]["ema"] = ck.checksum64_reference(ema)
    return sd, slots, n_flat, ema


def test_checkpoint_packs_and_unpacks_the_average():
    sd, slots, n_flat, ema = _with_ema()
    assert sorted(sd) == sorted(ck.REQUIRED_KEYS + ("ema",)) and ck.check_format(sd) is True
    assert sorted(sd["ema"]) == ["decay", "model", "warmup"] and list(sd["ema"]["model"]) == list(slots)          # specs order
    assert all(tuple(sd["ema"]["model"][k].shape) == tuple(slots[k][2]) for k in slots)
    assert sum(t.numel() for t in sd["ema"]["model"].values()) == sum(n for _, n, _ in slots.values()) <= n_flat          # no padding stored
    back, decay, warmup = ck.unpack_ema(sd["ema"], slots, n_flat)
    assert torch.equal(back, ema) and (decay, warmup) == (0.99, True)
    names = list(slots)
    with pytest.raises(KeyError, match="decay"):
        ck.unpack_ema({k: v for k, v in sd["ema"].items() if k != "decay"}, slots, n_flat)
    with pytest.raises(ValueError, match="outside"):
        ck.unpack_ema(dict(sd["ema"], decay=1.0), slots, n_flat)
    with pytest.raises(KeyError, match="ema: tensor " + names[5].replace(".", r"\.")):
        ck.unpack_ema(dict(sd["ema"], model={k: v for k, v in sd["ema"]["model"].items() if k != names[5]}), slots, n_flat)
    with pytest.raises(ValueError, match="ema: " + names[9].replace(".", r"\.")):
        ck.unpack_ema(dict(sd["ema"], model=dict(sd["ema"]["model"], **{names[9]: torch.zeros(2, 5)})), slots, n_flat)
    with pytest.raises(KeyError, match="no_such_tensor"):
        ck.unpack_ema(dict(sd["ema"], model=dict(sd["ema"]["model"], no_such_tensor=torch.zeros(1))), slots, n_flat)


def test_verify_file_accepts_the_average_and_names_it_after_one_flipped_bit(tmp_path):
    sd, slots, n_flat, ema = _with_ema()
    path = str(tmp_path / "ema.pt")
    torch.save(sd, path)
    back = ck.verify_file(path)          # torch.load(weights_only=True) inside
    assert sorted(back) == sorted(ck.REQUIRED_KEYS + ("ema",)) and back["ema"]["decay"] == 0.99 and back["ema"]["warmup"] is True
    assert torch.equal(ck.unpack_ema(back["ema"], slots, n_flat)[0], ema) and back["checksums"]["ema"] == sd["checksums"]["ema"]
    raw = sd["ema"]["model"][list(slots)[11]].view(torch.uint8).reshape(-1)
    raw[2] ^= 0x10          # one bit of one byte of the average
    torch.save(sd, path)
    with pytest.raises(RuntimeError, match="`ema`"):
        ck.verify_file(path)
    raw[2] ^= 0x10
    del sd["checksums"]["ema"]          # an average without its seal is no checkpoint
    torch.save(sd, path)
    with pytest.raises(KeyError, match="ema"):
        ck.verify_file(path)


def test_without_the_average_the_key_set_is_what_it_was(tmp_path):
    sd, slots, n_flat, _ = _checkpoint()
    assert sorted(sd) == sorted(ck.REQUIRED_KEYS) and "ema" not in ck.REQUIRED_KEYS and ck.FORMAT == 1
    path = str(tmp_path / "plain.pt")
    torch.save(sd, path)
    back = ck.verify_file(path)
    assert sorted(back) == sorted(ck.REQUIRED_KEYS) and sorted(back["checksums"]) == ["flat", "m", "v"]
