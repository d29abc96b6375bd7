"""CPU: the host side of the deterministic mode -- the `_det_elems` size queries of include/modaltune_hip.h, the switches that turn the
mode on, the TITAN refusal, and what TrainStep does with a deterministic engine.  (The kernels: tests/test_deterministic_gpu.py; the
train step: tests/test_deterministic_model_gpu.py.)"""
import inspect
import json
import math
import os
import re

import pytest
import torch

from modaltune_amd import engine as engine_mod
from modaltune_amd import ops
from modaltune_amd.aggregators import Aggregator

GROUPS = {f"g{i}": [f"x{j}" for j in range(5 + i)] for i in range(4)}


def cdiv(a, b):
    return -(-a // b)


def _tn_slots(M, N1, N2):
    """(splits of the deterministic mt_gemm_tn_f16 that hold rows, splits launched).  csrc/gemm.hip: 64 x 64 tiles, ~1024 workgroups (512 for fewer
    than 16 tiles), at least 256 rows per split, a multiple of the 8 XCDs -- the default form's launch; the 32-row steps are dealt out
    evenly over the first min(steps, launched) splits."""
    tiles = (N1 // 64) * (N2 // 64)
    split = cdiv(max(1, min(cdiv(M, 256), cdiv(1024 if tiles >= 16 else 512, tiles))), 8) * 8
    return min(cdiv(M, 32), split), split


def test_elems_queries_cover_exactly_the_slots_that_get_written():
    for M, N1, N2 in [(1, 64, 64), (33, 192, 768), (114, 768, 192), (4503, 384, 768), (30000, 768, 192)]:
        slots, split = _tn_slots(M, N1, N2)
        assert slots <= split
        assert ops.det_elems("gemm_tn_f16", M, N1, N2, 0) == slots * N1 * N2
        assert ops.det_elems("gemm_tn_f16", M, N1, N2, 1) == slots * N1 * (N2 + 1)
        assert ops.det_elems("colsum_f16", M, N1) == cdiv(M, 256) * N1
    assert _tn_slots(114, 768, 192) == (4, 8)            # the empty M-splits own no slot
    for M in (1, 5, 111, 4503, 100000):
        slots = min(cdiv(M, 4), 512)
        assert ops.det_elems("layernorm_bwd", M, 768) == slots * 2 * 768
        assert ops.det_elems("inject_resid_bwd", M, 768) == slots * 768
    for heads, hd in [(12, 16), (6, 32), (9, 64)]:
        for L in (37, 512, 513, 1500):
            for T in (7, 65, 128):
                E = heads * hd
                assert ops.det_elems("inject_attn_bwd_hd", 3 * L, L, T, heads, hd) == 2 * cdiv(L, 512) * 3 * T * E      # rows t >= T: no storage
                assert ops.det_elems("extract_attn_bwd_hd", 3, T, L, heads, hd) == cdiv(L, 512) * 3 * T * E


def test_elems_queries_are_monotone_in_the_row_count():
    rows = [1, 2, 31, 32, 33, 255, 256, 257, 511, 512, 513, 1024, 2047, 2048, 2049, 4503, 8191, 8192, 8193, 30000, 100000]
    for name, shape in [("gemm_tn_f16", lambda m: (m, 768, 192, 1)), ("gemm_tn_f16", lambda m: (m, 384, 768, 0)),
                        ("gemm_tn_f16", lambda m: (m, 64, 64, 1)), ("colsum_f16", lambda m: (m, 768)),
                        ("layernorm_bwd", lambda m: (m, 768)), ("inject_resid_bwd", lambda m: (m, 768)),
                        ("inject_attn_bwd_hd", lambda m: (3 * m, m, 65, 12, 16)), ("extract_attn_bwd_hd", lambda m: (3, 65, m, 12, 16))]:
        got = [ops.det_elems(name, *shape(m)) for m in rows]
        assert got == sorted(got) and got[0] > 0, (name, got)


@pytest.mark.parametrize("name,shape", [
    ("gemm_tn_f16", (0, 64, 64, 0)), ("gemm_tn_f16", (10, 65, 64, 0)), ("gemm_tn_f16", (10, 64, 0, 1)), ("gemm_tn_f16", (-1, 64, 64, 1)),
    ("colsum_f16", (0, 64)), ("colsum_f16", (5, 12)), ("layernorm_bwd", (0, 768)), ("layernorm_bwd", (5, 100)),
    ("inject_resid_bwd", (5, 256)), ("inject_resid_bwd", (0, 768)), ("inject_attn_bwd_hd", (10, 3, 7, 12, 16)),
    ("inject_attn_bwd_hd", (9, 3, 129, 12, 16)), ("inject_attn_bwd_hd", (9, 3, 7, 4, 48)), ("extract_attn_bwd_hd", (0, 7, 5, 12, 16)),
    ("extract_attn_bwd_hd", (1, 0, 5, 12, 16)), ("extract_attn_bwd_hd", (1, 7, 0, 12, 16)), ("extract_attn_bwd_hd", (1, 7, 5, 12, 24))])
def test_elems_queries_reject_bad_shapes_with_a_negative_status(name, shape):
    from modaltune_amd import _lib
    assert getattr(_lib.load(), f"mt_{name}_det_elems")(*shape) < 0
    with pytest.raises(RuntimeError, match="det_elems"):
        ops.det_elems(name, *shape)


def _kwargs(name):
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ctor_defaults.json")
    kw = dict(json.load(open(golden))[name]["kwargs"])
    kw["pretrained"] = False
    return kw


@pytest.mark.parametrize("name", ["titan_gene_adapter", "titan_gene_clinical_adapter"])
def test_titan_refuses_the_mode_and_names_the_kernel(name, monkeypatch):
    with pytest.raises(NotImplementedError, match="scatter_rows_kernel"):
        Aggregator.create(name, gene_group_defination=GROUPS, multi_task=3, device="cpu", deterministic=True)
    monkeypatch.setenv("MT_DETERMINISTIC", "1")           # the default switch is refused as loudly
    with pytest.raises(NotImplementedError, match="scatter_rows_kernel"):
        Aggregator.create(name, gene_group_defination=GROUPS, multi_task=3, device="cpu")


def test_environment_and_torch_flag_set_the_default(monkeypatch):
    name = "longnetvit_gene_adapter"
    make = lambda **k: Aggregator.create(name, gene_group_defination=GROUPS, multi_task=3, device="cpu", **k, **_kwargs(name)).engine
    monkeypatch.delenv("MT_DETERMINISTIC", raising=False)
    assert not torch.are_deterministic_algorithms_enabled()
    assert engine_mod.deterministic_default() is False and make().deterministic is False
    assert make(deterministic=True).deterministic is True
    monkeypatch.setenv("MT_DETERMINISTIC", "1")
    assert engine_mod.deterministic_default() is True and make().deterministic is True
    assert make(deterministic=False).deterministic is False          # an explicit argument wins
    monkeypatch.setenv("MT_DETERMINISTIC", "0")
    assert make().deterministic is False
    torch.use_deterministic_algorithms(True)
    try:
        assert engine_mod.deterministic_default() is True and make().deterministic is True
    finally:
        torch.use_deterministic_algorithms(False)


def test_deterministic_train_step_runs_no_schedule_trial(monkeypatch):
    from modaltune_amd.trainer import TrainStep
    monkeypatch.delenv("MT_DETERMINISTIC", raising=False)
    monkeypatch.delenv("MT_SPLIT_PASSES", raising=False)
    name = "longnetvit_gene_clinical_adapter"
    eng = lambda det: Aggregator.create(name, gene_group_defination=GROUPS, multi_task=3, device="cpu", deterministic=det, **_kwargs(name)).engine
    ts = TrainStep(eng(True))                 # split_passes="auto"
    assert ts.deterministic is True and ts.auto_split is False and ts.split_decisions == {}
    assert ts.split_passes is True            # the threshold rule stays
    off = TrainStep(eng(False))
    assert off.deterministic is False and off.auto_split is True


def test_leaf_stream_and_the_mode_exclude_each_other(monkeypatch):
    name = "longnetvit_gene_adapter"
    monkeypatch.setenv("MT_LEAF_STREAM", "1")
    with pytest.raises(ValueError, match="MT_LEAF_STREAM"):
        Aggregator.create(name, gene_group_defination=GROUPS, multi_task=3, device="cpu", deterministic=True, **_kwargs(name))
    monkeypatch.delenv("MT_LEAF_STREAM")
    e = Aggregator.create(name, gene_group_defination=GROUPS, multi_task=3, device="cpu", deterministic=True, **_kwargs(name)).engine
    e.leaf_stream = True                      # (switched on after construction)
    with pytest.raises(ValueError, match="MT_LEAF_STREAM"):
        e._leaf(lambda: None)


def test_workspace_spec_holds_the_partial_buffer_only_in_the_mode():
    name = "longnetvit_gene_adapter"
    make = lambda det: Aggregator.create(name, gene_group_defination=GROUPS, multi_task=3, device="cpu", deterministic=det, **_kwargs(name)).engine
    on, off = make(True), make(False)
    assert "det" not in off._ws_spec(3, 1500)
    small, large = on._ws_spec(2, 37)["det"], on._ws_spec(2, 10000)["det"]
    assert small[0] == torch.float32 and 0 < small[1][0] <= large[1][0]
    cfg = on.cfg
    assert large[1][0] >= ops.det_elems("gemm_tn_f16", 2 * 10000, 2 * cfg.adapter_dim, cfg.embed_dim, 1)      # the k | v weight gradient


def test_torch_ops_forward_to_no_atomic_launcher():
    """modaltune_amd/torch_ops.py registers no op on top of a launcher that reduces over workgroups with atomics, so the registered
    ops are bit-reproducible under torch.use_deterministic_algorithms(True) as they stand; one that is added later on such a launcher
    has to pass det= (or raise under the flag) -- this test then fails until it does."""
    from modaltune_amd import torch_ops
    src = inspect.getsource(torch_ops)
    for fn in ("gemm_tn", "colsum", "inject_resid_bwd", "inject_attn_bwd", "extract_attn_bwd"):
        assert not re.search(rf"ops\.{fn}\(", src), fn
    for call in re.findall(r"ops\.layernorm_bwd\(([^\n]*)", src):
        assert "dw=" not in call or "det=" in call, call


def test_abi_lists_a_twin_and_a_query_for_each_of_the_six():
    """The deterministic form of each of the six is an option of the base entry (MtLaunchOpts.partials), not an entry of its own: the
    options pointer stands directly in front of the stream, and the size query is there."""
    from modaltune_amd import _lib
    assert [f for f, _ in _lib.MtLaunchOpts._fields_][3:5] == ["partials", "partials_elems"]
    assert dict(_lib.MtLaunchOpts._fields_)["partials_elems"] is _lib.L
    for n in ("mt_gemm_tn_f16", "mt_colsum_f16", "mt_layernorm_bwd", "mt_inject_resid_bwd", "mt_inject_attn_bwd_hd", "mt_extract_attn_bwd_hd"):
        assert n + "_det" not in _lib.SIGNATURES
        assert _lib.SIGNATURES[n][-2:] == [_lib.C.POINTER(_lib.MtLaunchOpts), _lib.P]         # ... options, stream
        assert _lib.SIGNATURES[n + "_det_elems"] and all(t is _lib.I for t in _lib.SIGNATURES[n + "_det_elems"])
        assert _lib._RESTYPE[n + "_det_elems"] is _lib.C.c_long
