"""The host-side rules of the pass-group schedule (modaltune_amd/pass_groups.py): group bounds, workspace slots, the MT_SPLIT_PASSES
reader and the eligibility predicate.  No GPU."""
from types import SimpleNamespace

import pytest

from modaltune_amd import pass_groups


def test_group_bounds_follow_the_trainers_rule():
    want = {1: [(0, 1)], 2: [(0, 1), (1, 2)], 3: [(0, 2), (2, 3)], 4: [(0, 3), (3, 4)], 5: [(0, 4), (4, 5)], 6: [(0, 4), (4, 6)]}
    for B in range(1, 7):
        assert pass_groups.group_bounds(B) == want[B], B
        assert pass_groups.group_bounds(B, singles=True) == [(i, i + 1) for i in range(B)], B
        for groups in (pass_groups.group_bounds(B), pass_groups.group_bounds(B, singles=True)):      # a partition of the passes, in order
            assert groups[0][0] == 0 and groups[-1][1] == B and all(a < b for a, b in groups)
            assert all(groups[i][1] == groups[i + 1][0] for i in range(len(groups) - 1))


@pytest.mark.parametrize("groups, want", [([(0, 2), (2, 3)], [0, 0]), ([(0, 1), (1, 2)], [0, 1]), (pass_groups.group_bounds(3, singles=True), [0, 1, 2])])
def test_groups_of_equal_size_get_workspace_slots_of_their_own(groups, want):
    assert pass_groups.group_slots(groups) == want
    assert pass_groups.group_slots(groups, base=8) == [8 + s for s in want]


@pytest.mark.parametrize("value, want", [(None, "auto"), ("0", "off"), ("off", "off"), ("1", "on"), ("force", "force"), ("auto", "auto")])
def test_split_mode_reads_the_environment(monkeypatch, value, want):
    if value is None:
        monkeypatch.delenv("MT_SPLIT_PASSES", raising=False)
    else:
        monkeypatch.setenv("MT_SPLIT_PASSES", value)
    assert pass_groups.split_mode() == want
    assert pass_groups.SPLIT_MIN_PATCHES == 7500


def test_eligibility_at_its_floors():
    eng = SimpleNamespace(cfg=SimpleNamespace(is_multi=True), collect_taps=False)
    T = pass_groups.SPLIT_MIN_PATCHES
    ok = lambda B, L, **k: pass_groups.eligible(eng, B, L, T, True, **k)
    assert ok(3, T) and not ok(2, T)                              # the three non-trainer users' floor
    assert ok(2, T, min_passes=2) and not ok(1, T, min_passes=2)      # the trainer's
    assert ok(3, T) and not ok(3, T - 1)
    assert ok(3, None) and not pass_groups.eligible(eng, 3, T, T, False)
    assert not pass_groups.eligible(SimpleNamespace(cfg=SimpleNamespace(is_multi=False), collect_taps=False), 3, T, T, True)
    assert not pass_groups.eligible(SimpleNamespace(cfg=SimpleNamespace(is_multi=True), collect_taps=True), 3, T, T, True)
