"""The slide protocol on the host: Engine and TitanEngine answer the same three calls (stage_slide, slide_prologue, forward_slide)
and say themselves what they can do (replayable, the refusals), so no caller asks which engine it holds.  The refusal messages are
the ones the callers' own `hasattr` checks raised before the protocol existed, copied here as literals."""
import inspect
import types

import pytest
import torch

from modaltune_amd.engine import Engine, GenePoints, PatchPoints
from modaltune_amd.titan import TitanEngine

ATTENTION_MAPS = ("attention maps of the TITAN configuration are not supported: its adapters attend over gridded "
                  "cells, and drawing them on the slide needs the cell-to-coordinate map")
POINTS = "input gradients of the TITAN configuration are not supported"
INTEGRATED_GRADIENTS = "Integrated Gradients over the gene inputs of the TITAN configuration are not supported"
STAGE_SLIDE = "hipGraph replay of the TITAN configuration needs the native backbone with its native embedding"


def _bare(cls, **attrs):
    """An engine of class `cls` that was never constructed (no device, no library): only what the entry point under test reads."""
    eng = object.__new__(cls)
    eng.__dict__.update(attrs)
    return eng


def _backbone(kind, embed_w):
    return types.SimpleNamespace(kind=kind, embed_w=embed_w)


@pytest.mark.parametrize("name", ["stage_slide", "slide_prologue", "forward_slide"])
def test_both_engines_define_the_call_and_the_override_accepts_every_base_parameter(name):
    assert name in vars(Engine) and name in vars(TitanEngine)
    base, over = inspect.signature(vars(Engine)[name]), inspect.signature(vars(TitanEngine)[name])
    catch_all = any(p.kind is p.VAR_KEYWORD for p in over.parameters.values())
    for pname, p in base.parameters.items():
        if p.kind is p.VAR_KEYWORD:
            assert catch_all, f"{name}: the base passes **{pname} on, the override does not"
            continue
        assert pname in over.parameters, f"{name}: the override does not accept {pname}"
        q = over.parameters[pname]
        assert q.kind is p.kind, f"{name}({pname}): {q.kind.description} in the override, {p.kind.description} in the base"
        if p.kind is p.POSITIONAL_OR_KEYWORD:      # callers may pass it by position: same place in both
            assert list(over.parameters).index(pname) == list(base.parameters).index(pname), (name, pname)
        assert (p.default is p.empty) == (q.default is q.empty), f"{name}({pname}): required in one engine, optional in the other"


def test_replayable_is_a_property_of_both_and_false_in_each_of_its_three_ways():
    assert isinstance(vars(Engine)["replayable"], property) and isinstance(vars(TitanEngine)["replayable"], property)
    assert _bare(Engine).replayable is True
    assert _bare(TitanEngine, backbone=_backbone("native", object())).replayable is True
    assert _bare(TitanEngine, backbone=None).replayable is False                              # no backbone attached
    assert _bare(TitanEngine, backbone=_backbone("torch", object())).replayable is False      # the module's own torch blocks
    assert _bare(TitanEngine, backbone=_backbone("native", None)).replayable is False         # native blocks, the module's own embedding


@pytest.mark.parametrize("backbone", [None, _backbone("torch", object()), _backbone("native", None)])
def test_stage_slide_refuses_what_is_not_replayable(backbone):
    with pytest.raises(NotImplementedError) as e:
        _bare(TitanEngine, backbone=backbone).stage_slide(torch.zeros(3, 8), torch.zeros(3, 2))
    assert str(e.value) == STAGE_SLIDE


def test_each_refusal_raises_the_recorded_type_and_message_at_its_entry_point():
    from modaltune_amd.aggregators import LongNetGeneAdapter
    from modaltune_amd.attribution import IntegratedGradients
    from modaltune_amd.evaluate import EmbeddingExtractor
    eng = _bare(TitanEngine, device=torch.device("cpu"))
    z = torch.zeros(1)
    entry_points = [
        (ATTENTION_MAPS, lambda: eng.attention_map_shapes(1, 1)),
        (ATTENTION_MAPS, lambda: eng.new_attention_maps(["x"], 1, 1)),
        (ATTENTION_MAPS, lambda: EmbeddingExtractor(eng, attention=True)),
        (POINTS, lambda: eng._check_points(GenePoints(z, z, z, z), 1)),
        (POINTS, lambda: eng._check_patch_points(PatchPoints(z, z, z, z), 1, 1, True)),
        (INTEGRATED_GRADIENTS, lambda: IntegratedGradients(eng)),
        (INTEGRATED_GRADIENTS, lambda: IntegratedGradients(eng, inputs="patches")),
        (INTEGRATED_GRADIENTS, lambda: LongNetGeneAdapter.integrated_gradients(types.SimpleNamespace(engine=eng), None, None, None, None)),
    ]
    for message, call in entry_points:
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == message
    assert Engine.REFUSALS == {} and Engine.DETERMINISTIC_REFUSAL is None and "fp32 atomics" in TitanEngine.DETERMINISTIC_REFUSAL
    for feature in TitanEngine.REFUSALS:
        _bare(Engine).refuse(feature)          # the base refuses nothing


def test_the_capabilities_are_class_attributes_that_the_titan_engine_turns():
    assert (Engine.ROWS_FROM_STAGING, Engine.PASS_GROUPS, Engine.MODULE_REPLAY) == (False, True, True)
    assert (TitanEngine.ROWS_FROM_STAGING, TitanEngine.PASS_GROUPS, TitanEngine.MODULE_REPLAY) == (True, False, False)
