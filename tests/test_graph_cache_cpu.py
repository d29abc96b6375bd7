"""The host-side bookkeeping of the captured-graph cache (modaltune_amd/graph_cache.py): admission, the LRU, retirement by generation and
the pool-handle rule, on stand-in entries.  No GPU, no torch.cuda call."""
from types import SimpleNamespace

import torch

from modaltune_amd import graph_cache
from modaltune_amd.engine import flatten_genes
from modaltune_amd.graph_cache import GraphCache


def entry(generation):
    return SimpleNamespace(generation=generation)


def test_a_key_is_admitted_after_capture_after_eager_visits_and_not_counted_further():
    c = GraphCache(size=8, capture_after=2)
    assert [c.admit("a") for _ in range(4)] == [False, False, True, True]
    assert c.visits == {"a": 2}
    c.capture_after = 3                     # (owners change it while running: read when used)
    assert [c.admit("a") for _ in range(2)] == [False, True] and c.visits == {"a": 3}


def test_lru_evicts_the_least_recently_used_capture_and_keeps_its_visit_count():
    c = GraphCache(size=2, capture_after=2)
    c.sync(0)
    ents = {k: entry(0) for k in "abc"}
    for k in "abc":
        assert not c.admit(k) and not c.admit(k) and c.admit(k)
    c.put("a", ents["a"])
    c.put("b", ents["b"])
    assert c.get("a") is ents["a"]
    c.put("c", ents["c"])
    assert list(c.entries) == ["a", "c"] and c.get("b") is None
    assert c.visits["b"] == 2 and c.admit("b")          # no new eager visits for the evicted geometry


def test_size_is_read_at_eviction_time():
    c = GraphCache(size=2, capture_after=0)
    c.sync(0)
    c.put(0, entry(0))
    c.put(1, entry(0))
    c.size = 4
    c.put(2, entry(0))
    c.put(3, entry(0))
    assert list(c.entries) == [0, 1, 2, 3]
    c.size = 1
    c.put(4, entry(0))
    assert list(c.entries) == [4]
    c.size = 0                              # (never fewer than one: the capture that was just made is about to be replayed)
    c.put(5, entry(0))
    assert list(c.entries) == [5]


def test_one_off_keys_neither_evict_a_capture_nor_grow_the_visit_counts_without_bound():
    c = GraphCache(size=2, capture_after=2)
    c.sync(0)
    hot = entry(0)
    assert not c.admit("hot") and not c.admit("hot") and c.admit("hot")
    c.put("hot", hot)
    wiped = False
    for i in range(5000):
        assert not c.admit(("one-off", i))
        assert len(c.visits) <= graph_cache.MAX_VISIT_KEYS + 1 == 4097
        wiped = wiped or "hot" not in c.visits
    assert wiped and c.get("hot") is hot and list(c.entries) == ["hot"]
    # the counts were wiped: a hot geometry WITHOUT a capture (evicted, retired) is counted afresh -- a decision, not an accident
    assert [c.admit("hot") for _ in range(3)] == [False, False, True]


def test_entries_are_retired_by_the_generation_they_were_captured_under():
    c = GraphCache(size=8, capture_after=1)
    assert not c.admit("a") and not c.admit("b")
    c.put("a", entry(3))
    c.put("b", entry(3))
    assert c.sync(3) is False and list(c.entries) == ["a", "b"] and c.get("a") is not None
    assert c.sync(4) is True and not c.entries and c.visits == {"a": 1, "b": 1}
    assert c.sync(4) is False
    # an entry held outside the cache across a generation bump and put back (TrainStep's schedule trial holds the first schedule's
    # capture while it captures the second): it keeps the generation of its capture, so it is never live again
    held = entry(4)
    c.put("a", held)
    assert c.pop("a") is held and c.pop("a") is None
    c.sync(5)
    c.put("a", held)
    assert c.get("a") is None
    assert c.sync(5) is True and "a" not in c.entries and c.get("a") is None


def test_clear_empties_the_entries_and_the_cache_stays_usable():
    c = GraphCache(size=2, capture_after=1)
    c.sync(0)
    assert not c.admit("a")
    c.put("a", entry(0))
    c.clear()
    assert not c.entries and c.get("a") is None and c.visits == {"a": 1}
    assert c.admit("a")
    c.put("a", entry(0))
    assert c.get("a") is not None


def test_a_fresh_pool_handle_is_taken_only_when_no_graph_of_the_current_pool_is_alive(monkeypatch):
    handles = iter(range(100))
    monkeypatch.setattr(torch.cuda, "graph_pool_handle", lambda: next(handles))

    class Graph:        # (weak-referenceable, as torch.cuda.CUDAGraph is)
        pass

    c = GraphCache(size=2, capture_after=1)
    g1, g2 = Graph(), Graph()
    assert c.pool_for(g1) == 0 and c.pool_for(g2) == 0
    del g1
    g3 = Graph()
    assert c.pool_for(g3) == 0              # g2 lives in the pool
    del g2, g3                              # held outside the entries or inside makes no difference: the last graph died, and the pool with it
    g4 = Graph()
    assert c.pool_for(g4) == 1 and c.pool_for(Graph()) == 1
    assert torch.cuda.CUDAGraph.__weakrefoffset__ > 0


def test_flatten_genes_is_a_view_of_one_tensor_and_a_concatenation_of_several():
    t = torch.arange(6.0).reshape(2, 3)
    assert flatten_genes(t).data_ptr() == t.data_ptr() and flatten_genes([t]).data_ptr() == t.data_ptr()
    parts = [torch.arange(3.0).reshape(1, 3), torch.arange(3.0, 6.0)]
    assert torch.equal(flatten_genes(parts), t.reshape(-1)) and torch.equal(flatten_genes(iter(parts)), t.reshape(-1))
    assert flatten_genes([t.half(), t.half()]).dtype == torch.float16       # dtype and device stay the caller's business
