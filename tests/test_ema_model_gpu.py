"""GPU: the EMA of the trainable weights through TrainStep, on the model_L37_d3 golden's model (L = 37, depth 3, the 6-pathway toy
grouping; test_checkpoint_gpu._fresh), deterministic engine.  Every comparison is bit for bit: the average against the numpy
recurrence of tests/ema_ref.py fed the step's own parameter buffer, everything else GPU against GPU (torch.equal, checksums)."""
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

from modaltune_amd import checkpoint, synth  # noqa: E402

from ema_ref import ema_ref  # noqa: E402
from test_checkpoint_gpu import _fresh  # noqa: E402

LR, DECAY = 1e-3, 0.9
README_GROUPS = [{"kinds": ("b", "lnw", "lnb", "gamma", "tok"), "weight_decay": 0.0}, {"match": r"^gene_encoder\.", "lr_mult": 0.1}]


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _bits(t):
    return t.view(torch.int32)


def _cs(ts, t) -> int:
    """mt_checksum64 of a flat buffer, read back."""
    out = torch.empty(1, dtype=torch.int64, device="cuda")
    ts._checksum_into(t, out)
    return checkpoint.as_unsigned(int(out))


def _host_step(prev, flat, decay, warmup, t):
    return torch.from_numpy(ema_ref(prev.cpu().numpy(), flat.cpu().numpy(), decay, warmup, t)).cuda()


@pytest.mark.parametrize("warmup", [False, True])
def test_four_eager_steps_follow_the_host_recurrence(golden_dir, monkeypatch, warmup):
    _gpu()
    eng, ts, slide, _ = _fresh(monkeypatch, golden_dir, lr=LR, ema_decay=DECAY, ema_warmup=warmup)
    st = eng.store
    assert ts.ema.shape == st.flat.shape and ts.ema.data_ptr() != st.flat.data_ptr() and torch.equal(_bits(ts.ema), _bits(st.flat))
    for i in range(4):
        prev = ts.ema.clone()
        ts.step(*slide)
        torch.cuda.synchronize()
        assert int(ts.step_dev) == i + 1
        want = _host_step(prev, st.flat, DECAY, warmup, i + 1)
        bad = int((_bits(ts.ema) != _bits(want)).sum())
        assert bad == 0, f"step {i + 1}: {bad} of {st.n_flat} words of the average differ from the host recurrence"
        assert not torch.equal(ts.ema, prev) and not torch.equal(ts.ema, st.flat)
    # ema_state(): views into the average under the model's names; the slot padding stayed +0
    views = ts.ema_state()
    assert list(views) == list(st.slots) and all(v.shape == st.tensors[k].shape and v.data_ptr() == ts.ema.data_ptr() + 4 * st.slots[k][0]
                                                 for k, v in views.items())
    used = torch.zeros(st.n_flat, dtype=torch.bool, device="cuda")
    for o, n, _ in st.slots.values():
        used[o:o + n] = True
    assert int((_bits(ts.ema)[~used] != 0).sum()) == 0
    # ema_reset(): a copy of the current parameters again
    ts.ema_reset()
    assert torch.equal(_bits(ts.ema), _bits(st.flat))


@pytest.mark.parametrize("groups", [None, README_GROUPS], ids=["one_segment", "readme_groups"])
def test_a_twin_without_the_average_ends_with_the_same_bits(golden_dir, monkeypatch, groups):
    """Without parameter groups the EMA step goes through the grouped kernel with a one-segment table, its twin through mt_adamw_step;
    with the README's two rules both take the grouped kernel."""
    _gpu()
    kw = {} if groups is None else {"param_groups": groups}
    eng_a, ts_a, slide, _ = _fresh(monkeypatch, golden_dir, lr=LR, ema_decay=DECAY, **kw)
    eng_b, ts_b, _, _ = _fresh(monkeypatch, golden_dir, lr=LR, **kw)
    assert ts_b.ema is None and ts_a._grouped() == ts_b._grouped() == (groups is not None)
    for i in range(3):
        ts_a.step(*slide)
        ts_b.step(*slide)
        torch.cuda.synchronize()
        assert torch.equal(_bits(ts_a.loss), _bits(ts_b.loss)), i
    for name, a, b in (("flat", eng_a.store.flat, eng_b.store.flat), ("m", ts_a.m, ts_b.m), ("v", ts_a.v, ts_b.v)):
        assert torch.equal(_bits(a), _bits(b)), name
    assert int(ts_a.step_dev) == int(ts_b.step_dev) == 3 and not torch.equal(ts_a.ema, eng_a.store.flat)


def test_a_skipped_step_leaves_the_average_and_the_next_clean_step_moves_it(golden_dir, monkeypatch):
    _gpu()
    eng, ts, slide, _ = _fresh(monkeypatch, golden_dir, lr=LR, ema_decay=DECAY)
    ts.step(*slide)
    before, cs0, scale0 = ts.ema.clone(), _cs(ts, ts.ema), float(ts.scale)
    ts.scale.fill_(2.0 ** 40)          # (test_overflow_gpu.OVERFLOW_SCALE: the fp16 activation-gradient stream saturates)
    ts.step(*slide)
    torch.cuda.synchronize()
    assert int(ts.step_dev) == 1 and float(ts.scale) == 2.0 ** 39, "the step was skipped"
    assert _cs(ts, ts.ema) == cs0 and torch.equal(_bits(ts.ema), _bits(before))
    ts.scale.fill_(scale0)
    ts.step(*slide)
    torch.cuda.synchronize()
    assert int(ts.step_dev) == 2 and _cs(ts, ts.ema) != cs0
    # the skipped step did not count: the step behind it is step 2 of the recurrence (warm-up off: any t; the bits say it moved once)
    assert torch.equal(_bits(ts.ema), _bits(_host_step(before, eng.store.flat, DECAY, False, 2)))


def test_with_accumulation_the_average_moves_at_boundaries_only(golden_dir, monkeypatch):
    _gpu()
    eng, ts, slide, _ = _fresh(monkeypatch, golden_dir, lr=LR, ema_decay=DECAY, accumulate=2)
    sums = [_cs(ts, ts.ema)]
    for _ in range(4):
        ts.step(*slide)
        sums.append(_cs(ts, ts.ema))
    assert sums[1] == sums[0] and sums[2] != sums[1] and sums[3] == sums[2] and sums[4] != sums[3], sums
    assert int(ts.step_dev) == 2


def test_replayed_steps_give_the_eager_runs_average(golden_dir, monkeypatch):
    _gpu()
    eng_g, ts_g, slide, _ = _fresh(monkeypatch, golden_dir, lr=LR, ema_decay=DECAY, ema_warmup=True, capture_after=1)
    eng_e, ts_e, _, _ = _fresh(monkeypatch, golden_dir, lr=LR, ema_decay=DECAY, ema_warmup=True)

    def both(n):
        for _ in range(n):
            ts_g.step_graphed(*slide)
            ts_e.step(*slide)
        torch.cuda.synchronize()
    both(4)                                    # an eager visit, the capture and its replay, two replays
    assert ts_g._graphs is not None and ts_g.graph_replays == 3
    assert torch.equal(_bits(ts_g.ema), _bits(ts_e.ema)) and torch.equal(_bits(eng_g.store.flat), _bits(eng_e.store.flat))
    assert not torch.equal(ts_g.ema, eng_g.store.flat)
    # decay and warm-up are launch arguments: set_ema_decay drops the captures, the geometry is captured again with the new values
    for t in (ts_g, ts_e):
        t.set_ema_decay(0.5, warmup=False)
    assert ts_g._graphs is None and (ts_g.ema_decay, ts_g.ema_warmup) == (0.5, False)
    both(3)
    assert ts_g._graphs is not None and ts_g.graph_replays == 6          # (the visit counts stayed: the first call captures again)
    assert torch.equal(_bits(ts_g.ema), _bits(ts_e.ema)) and torch.equal(_bits(eng_g.store.flat), _bits(eng_e.store.flat))
    graphs = ts_g._graphs
    ts_g.set_ema_decay(0.5)                    # nothing changes: the captures stay
    assert ts_g._graphs == graphs


def test_ema_weights_shows_the_average_to_the_extractor_and_puts_everything_back(golden_dir, monkeypatch):
    _gpu()
    from modaltune_amd.evaluate import EmbeddingExtractor
    eng, ts, slide, _ = _fresh(monkeypatch, golden_dir, lr=LR, ema_decay=DECAY)
    x, coords, genes, _ = slide
    for _ in range(3):
        ts.step(*slide)
    ex = EmbeddingExtractor(eng, capture_after=1)
    ex(x, coords, genes)
    before = ex(x, coords, genes)              # (captured and replayed: the graph holds the addresses of the fp16 operand caches)
    assert ex.graph_replays == 1
    cs_flat, cs_ema, gen = _cs(ts, eng.store.flat), _cs(ts, ts.ema), eng.generation
    # a fresh engine that holds the averaged weights
    eng2, _, _, _ = _fresh(monkeypatch, golden_dir)
    eng2.load_state_dict({k: v.clone() for k, v in ts.ema_state().items()}, strict=False)
    want = EmbeddingExtractor(eng2, graphed=False)(x, coords, genes)
    with ts.ema_weights() as inside:
        assert inside is ts and eng.generation == gen
        assert _cs(ts, eng.store.flat) == cs_ema and _cs(ts, ts.ema) == cs_flat
        got = ex(x, coords, genes)
        assert ex.graph_replays == 2, "the captured graph stayed valid"
        with pytest.raises(RuntimeError, match=r"step\(\) inside ema_weights\(\)"):
            ts.step(*slide)
        with pytest.raises(RuntimeError, match=r"ema_weights\(\) inside ema_weights\(\)"):
            with ts.ema_weights():
                pass
        with pytest.raises(RuntimeError, match=r"state_dict\(\) inside ema_weights\(\)"):
            ts.state_dict()
        assert _cs(ts, eng.store.flat) == cs_ema      # (the refusals moved nothing)
    torch.cuda.synchronize()
    assert torch.equal(_bits(got), _bits(want)), float((got - want).abs().max())
    assert not torch.equal(got, before)
    assert _cs(ts, eng.store.flat) == cs_flat and _cs(ts, ts.ema) == cs_ema and eng.generation == gen
    after = ex(x, coords, genes)
    assert torch.equal(_bits(after), _bits(before)) and ex.graph_replays == 3
    # an exception inside the context still puts the weights back
    with pytest.raises(KeyError):
        with ts.ema_weights():
            raise KeyError("evaluation failed")
    assert _cs(ts, eng.store.flat) == cs_flat and _cs(ts, ts.ema) == cs_ema
    ts.step(*slide)                            # ... and training goes on
    torch.cuda.synchronize()
    assert int(ts.step_dev) == 4 and _cs(ts, ts.ema) != cs_ema


def test_checkpoint_resumes_the_average_and_seals_it(golden_dir, monkeypatch, tmp_path):
    _gpu()
    kw = dict(lr=LR, ema_decay=DECAY, ema_warmup=True)
    eng_a, ts_a, slide, _ = _fresh(monkeypatch, golden_dir, **kw)
    for _ in range(4):
        ts_a.step(*slide)
    eng_b, ts_b, _, _ = _fresh(monkeypatch, golden_dir, **kw)
    for _ in range(2):
        ts_b.step(*slide)
    path = str(tmp_path / "ema.pt")
    torch.save(ts_b.state_dict(), path)
    sd = checkpoint.verify_file(path)          # (the device's checksum of the average holds on the CPU)
    assert sorted(sd) == sorted(checkpoint.REQUIRED_KEYS + ("ema",)) and sorted(sd["checksums"]) == ["ema", "flat", "m", "v"]
    assert sd["ema"]["decay"] == DECAY and sd["ema"]["warmup"] is True and list(sd["ema"]["model"]) == list(eng_b.store.slots)
    assert sd["checksums"]["ema"] == _cs(ts_b, ts_b.ema)
    # a fresh step on other weights, built with another decay and without warm-up: the checkpoint's values win
    eng_c, ts_c, _, _ = _fresh(monkeypatch, golden_dir, weights_seed=99, lr=LR, ema_decay=0.5, ema_warmup=False)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ts_c.load_state_dict(sd)
    assert (ts_c.ema_decay, ts_c.ema_warmup) == (DECAY, True) and torch.equal(_bits(ts_c.ema), _bits(ts_b.ema))
    for _ in range(2):
        ts_c.step(*slide)
    torch.cuda.synchronize()
    assert torch.equal(_bits(ts_c.ema), _bits(ts_a.ema)) and torch.equal(_bits(eng_c.store.flat), _bits(eng_a.store.flat))
    # one flipped bit in the stored average: the load raises and names it
    name = list(eng_b.store.slots)[7]
    bad = dict(sd, ema=dict(sd["ema"], model=dict(sd["ema"]["model"])))
    bad["ema"]["model"][name] = sd["ema"]["model"][name].clone()
    bad["ema"]["model"][name].view(torch.int32).reshape(-1)[0] ^= 1 << 9
    with pytest.raises(RuntimeError, match="checksum of `ema`"):
        ts_c.load_state_dict(bad)
    # a checkpoint without an average (a step that keeps none wrote it): a warning, and the average starts at the loaded parameters
    eng_d, ts_d, _, _ = _fresh(monkeypatch, golden_dir, lr=LR)
    ts_d.step(*slide)
    plain = ts_d.state_dict()
    assert sorted(plain) == sorted(checkpoint.REQUIRED_KEYS) and sorted(plain["checksums"]) == ["flat", "m", "v"]
    with pytest.warns(UserWarning, match="no `ema` entry"):
        ts_c.load_state_dict(plain)
    assert torch.equal(_bits(ts_c.ema), _bits(eng_c.store.flat)) and torch.equal(_bits(eng_c.store.flat), _bits(eng_d.store.flat))
    # ... and a checkpoint with one, loaded into a step that keeps none: ignored with a warning
    with pytest.warns(UserWarning, match="`ema` entry is ignored"):
        ts_d.load_state_dict(sd)
    assert ts_d.ema is None and torch.equal(_bits(eng_d.store.flat), _bits(ts_b.engine.store.flat))
