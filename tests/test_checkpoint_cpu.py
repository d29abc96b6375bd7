"""CPU: the checkpoint format of the fused train step (modaltune_amd/checkpoint.py) on plain tensors -- the reference form of the
64-bit checksum, the optimiser / scaler dicts against torch's own classes, the refusals, and a file's round trip through torch.save,
torch.load(weights_only=True) and verify_file.  Every comparison is an integer or torch.equal: nothing here has a tolerance."""
import numpy as np
import pytest
import torch

from modaltune_amd import checkpoint as ck
from modaltune_amd import synth
from modaltune_amd.config import ModelConfig

M64 = (1 << 64) - 1


def _toy():
    """The L = 150 toy configuration of tests/accum_clip_dp_worker.py (its shapes only: nothing runs)."""
    cfg = ModelConfig(depth=3, interaction_indexes=((0, 0), (1, 1), (2, 2)), slide_ngrids=32, dropout=0.0, drop_path_rate=0.0)
    sizes = synth.toy_group_sizes()
    slots, n_flat = ck.slots_of(synth.param_specs(cfg, sizes))
    return cfg, sizes, slots, n_flat


def _mix_py(j):
    z = (j + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return (z ^ (z >> 31)) | 1


# ---------------------------------------------------------------------------------------------- checksum64_reference
def test_reference_checksum_of_a_fixed_vector():
    """The two constants were computed once from the issue's formula with Python ints (_mix_py above, sum of mix(base + i) * (w + 1))."""
    v = np.array([0, 1, 0xFFFFFFFF, 0x3F800000, 12345, 0xDEADBEEF, 7], dtype=np.uint32)
    assert ck.checksum64_reference(v) == 0xC46D4CF3897A4874
    assert ck.checksum64_reference(v, index_base=1 << 33) == 0x38F788D061576656
    assert ck.checksum64_reference(v) == sum(_mix_py(i) * (int(w) + 1) for i, w in enumerate(v)) & M64
    assert ck.checksum64_reference(torch.from_numpy(v.view(np.float32).copy())) == 0xC46D4CF3897A4874      # (the words, whatever the dtype)


def test_reference_checksum_composes_and_sees_every_change():
    r = np.random.default_rng(3)
    a = r.integers(0, 1 << 32, size=1000, dtype=np.uint64).astype(np.uint32)
    whole = ck.checksum64_reference(a)
    for k in (1, 257, 999):
        assert (ck.checksum64_reference(a[:k]) + ck.checksum64_reference(a[k:], index_base=k)) & M64 == whole
    b = r.integers(0, 1 << 32, size=64, dtype=np.uint64).astype(np.uint32)
    base = ck.checksum64_reference(b)
    seen = {base}
    for i in range(64):
        for bit in range(32):
            c = b.copy()
            c[i] ^= np.uint32(1 << bit)
            seen.add(ck.checksum64_reference(c))
    assert len(seen) == 1 + 64 * 32          # every single-bit flip gives a value of its own
    c = b.copy()
    assert c[5] != c[40]
    c[5], c[40] = b[40], b[5]
    assert ck.checksum64_reference(c) != base
    for n in (1, 4, 255):
        assert ck.checksum64_reference(np.zeros(n, np.uint32)) != ck.checksum64_reference(np.zeros(n + 1, np.uint32))


# ---------------------------------------------------------------------------------------------- optimiser
def _hyper():
    return {"lr": 1e-3, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.01}


def test_packed_optimizer_loads_into_torch_adamw_and_comes_back():
    cfg, sizes, slots, n_flat = _toy()
    names = list(slots)
    g = torch.Generator().manual_seed(0)
    m, v = torch.randn(n_flat, generator=g), torch.rand(n_flat, generator=g)
    sd = ck.pack_optimizer(m, v, 7, slots, names, _hyper())
    assert sorted(sd) == ["param_groups", "state"] and len(sd["param_groups"]) == 1 and len(sd["state"]) == len(names)
    params = [torch.nn.Parameter(torch.zeros(slots[k][2])) for k in names]
    opt = torch.optim.AdamW(params, lr=5.0)
    opt.load_state_dict(sd)
    grp = opt.param_groups[0]
    assert (grp["lr"], tuple(grp["betas"]), grp["eps"], grp["weight_decay"]) == (1e-3, (0.9, 0.999), 1e-8, 0.01)
    for k, p in zip(names, params):
        o, n, shape = slots[k]
        s = opt.state[p]
        assert tuple(s["exp_avg"].shape) == tuple(shape) and float(s["step"]) == 7.0
        assert torch.equal(s["exp_avg"].reshape(-1), m[o:o + n]) and torch.equal(s["exp_avg_sq"].reshape(-1), v[o:o + n])
    # one real CPU step of that optimiser, then its OWN state_dict back into flat buffers
    for p in params:
        p.grad = torch.full_like(p, 0.25)
    opt.step()
    m2, v2, step, hyper = ck.unpack_optimizer(opt.state_dict(), slots, names, n_flat)
    assert step == 8 and hyper == _hyper()
    used = torch.zeros(n_flat, dtype=torch.bool)
    for k, p in zip(names, params):
        o, n, _ = slots[k]
        used[o:o + n] = True
        assert torch.equal(m2[o:o + n], opt.state[p]["exp_avg"].reshape(-1)) and torch.equal(v2[o:o + n], opt.state[p]["exp_avg_sq"].reshape(-1))
        assert not torch.equal(m2[o:o + n], m[o:o + n])
    assert int((~used).sum()) > 0 and not m2[~used].any() and not v2[~used].any()          # the slot padding is zero
    # the padding is not stored either: garbage in it does not survive a pack / unpack
    m3 = m.clone()
    m3[~used] = 9.0
    back = ck.unpack_optimizer(ck.pack_optimizer(m3, v, 7, slots, names, _hyper()), slots, names, n_flat)[0]
    assert not back[~used].any() and torch.equal(back[used], m[used])


def test_disagreeing_steps_and_wrong_shapes_name_the_tensor():
    cfg, sizes, slots, n_flat = _toy()
    names = list(slots)
    sd = ck.pack_optimizer(torch.zeros(n_flat), torch.zeros(n_flat), 3, slots, names, _hyper())
    sd["state"][4]["step"] = torch.tensor(5.0)
    with pytest.raises(ValueError, match=names[4].replace(".", r"\.")):
        ck.unpack_optimizer(sd, slots, names, n_flat)
    sd = ck.pack_optimizer(torch.zeros(n_flat), torch.zeros(n_flat), 3, slots, names, _hyper())
    sd["state"][2]["exp_avg"] = torch.zeros(3, 3)
    with pytest.raises(ValueError, match=names[2].replace(".", r"\.")):
        ck.unpack_optimizer(sd, slots, names, n_flat)
    empty = {"state": {}, "param_groups": sd["param_groups"]}          # an optimiser that never stepped
    m, v, step, _ = ck.unpack_optimizer(empty, slots, names, n_flat)
    assert step == 0 and not m.any() and not v.any()


# ---------------------------------------------------------------------------------------------- a whole checkpoint
def _checkpoint(seed=0):
    cfg, sizes, slots, n_flat = _toy()
    names = list(slots)
    g = torch.Generator().manual_seed(seed)
    flat, m, v = (torch.zeros(n_flat) for _ in range(3))
    model = {}
    for k in names:
        o, n, shape = slots[k]
        for buf in (flat, m, v):
            buf[o:o + n] = torch.randn(n, generator=g)
        model[k] = flat[o:o + n].clone().view(shape)
    sd = {"format": ck.FORMAT, "model": model, "optimizer": ck.pack_optimizer(m, v, 3, slots, names, _hyper()),
          "scaler": ck.pack_scaler(2.0 ** 15, 1, 4), "rng": torch.tensor([1, 2, 3, 0], dtype=torch.int32), "stochastic": True, "lr": 1e-3,
          "window": None, "schedule": {"split_decisions": {4096: True}},
          "checksums": {n: ck.checksum64_reference(b) for n, b in (("flat", flat), ("m", m), ("v", v))},
          "build_id": "0" * 64, "world": 1, "config": ck.config_dict(cfg, sizes)}
    return sd, slots, n_flat, (flat, m, v)


def test_wrong_format_missing_key_and_wrong_shape_are_refused_by_name():
    sd, slots, n_flat, _ = _checkpoint()
    names = list(slots)
    shapes = {k: s[2] for k, s in slots.items()}
    assert ck.check_format(sd) is True
    assert ck.check_format({k: sd[k] for k in ("model", "optimizer", "scaler")}) is False          # the module path's dict
    with pytest.raises(ValueError, match="format 2"):
        ck.check_format(dict(sd, format=2))
    with pytest.raises(KeyError, match="scaler"):
        ck.check_format({k: v for k, v in sd.items() if k != "scaler"})
    with pytest.raises(KeyError, match="optimizer"):
        ck.check_format({"model": {}, "scaler": {}})
    ck.check_model_shapes(sd["model"], shapes, names)
    gone = {k: v for k, v in sd["model"].items() if k != names[7]}
    with pytest.raises(KeyError, match=names[7].replace(".", r"\.")):
        ck.check_model_shapes(gone, shapes, names)
    bad = dict(sd["model"])
    bad[names[9]] = torch.zeros(2, 5)
    with pytest.raises(ValueError, match=names[9].replace(".", r"\.")):
        ck.check_model_shapes(bad, shapes, names)
    with pytest.raises(KeyError, match="no_such_tensor"):
        ck.check_model_shapes(dict(sd["model"], no_such_tensor=torch.zeros(1)), shapes, names)
    # another pathway grouping: the gene encoder's shapes differ
    other, _ = ck.slots_of(synth.param_specs(ck.config_from_dict(sd["config"])[0], synth.toy_group_sizes(5)))
    with pytest.raises((ValueError, KeyError), match="gene_encoder"):
        ck.check_model_shapes(sd["model"], {k: s[2] for k, s in other.items()}, list(other))


def test_scaler_dict_round_trips_through_torch_gradscaler():
    sd = ck.pack_scaler(2.0 ** 13, 3, 4)
    assert sorted(sd) == ["_growth_tracker", "backoff_factor", "growth_factor", "growth_interval", "scale"]
    scaler = torch.amp.GradScaler("cpu", enabled=True, init_scale=1.0)
    scaler.load_state_dict(sd)
    back = scaler.state_dict()
    assert back == sd and sorted(back) == sorted(sd)
    assert ck.unpack_scaler(back) == (2.0 ** 13, 3, 4)
    with pytest.raises(ValueError, match="growth / backoff"):
        ck.unpack_scaler(dict(sd, growth_factor=3.0))
    with pytest.raises(KeyError, match="_growth_tracker"):
        ck.unpack_scaler({k: v for k, v in sd.items() if k != "_growth_tracker"})


def test_file_round_trip_verifies_and_one_flipped_byte_does_not(tmp_path):
    sd, slots, n_flat, (flat, m, v) = _checkpoint()
    path = str(tmp_path / "ck.pt")
    torch.save(sd, path)
    back = ck.verify_file(path)          # torch.load(weights_only=True) inside
    assert sorted(back) == sorted(ck.REQUIRED_KEYS) and back["schedule"]["split_decisions"] == {4096: True}
    f2, m2, v2, step, hyper = ck.flat_buffers(back, slots, n_flat)
    assert torch.equal(f2, flat) and torch.equal(m2, m) and torch.equal(v2, v) and step == 3 and hyper == _hyper()
    assert torch.equal(back["rng"], sd["rng"]) and back["checksums"] == sd["checksums"]
    cfg, sizes = ck.config_from_dict(back["config"])
    assert ck.slots_of(synth.param_specs(cfg, sizes))[0] == slots
    raw = sd["optimizer"]["state"][11]["exp_avg"].view(torch.uint8).reshape(-1)
    raw[2] ^= 0x10          # one bit of one byte of m
    torch.save(sd, path)
    with pytest.raises(RuntimeError, match="`m`"):
        ck.verify_file(path)
