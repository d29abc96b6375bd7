"""CPU: the full-width adapters, E = 768 -- `with_cffn=False` (no q_proj / output_proj, no Extractor FFN; `cffn_ratio >= 1` with the
wrap stays refused: tests/test_adapter_width_cpu.py pins that) -- where nn.MultiheadAttention packs q / k / v into one in_proj_weight
[2304, 768]: what ModelConfig.validate() accepts, the parameter layout against the reference's own state_dict (tests/golden/full_width_layout.json), the packed matrix's init family, the float64
restatements of tests/full_width_ref.py against reference goldens (tests/golden/make_golden_full_width.py) -- the yardstick the GPU
tests of tests/test_full_width_gpu.py are held against -- and the row slices of the packed gradient in the flat gradient buffer."""
import json
import math
import os

import numpy as np
import pytest
import torch

from modaltune_amd import init, synth
from modaltune_amd.config import GIGAPATH_JSON, ModelConfig, flops_per_slide_step, segment_lengths
from modaltune_amd.titan import titan_model_config

import full_width_ref as R
import unit_inputs
from test_oracle_golden import F64, _maxrel as _maxrel_np

SETTINGS = {"nocffn": dict(with_cffn=False), "nocffn_h24": dict(with_cffn=False, num_heads=24)}
INTER = [[0, 0], [1, 1], [2, 2]]
SIZES = synth.toy_group_sizes(6)


@pytest.fixture(scope="module")
def layout(golden_dir):
    return json.load(open(os.path.join(golden_dir, "full_width_layout.json")))


def _cfg(extra):
    return ModelConfig.from_json(dict(GIGAPATH_JSON, depth=3, interaction_indexes=INTER, slide_ngrids=128, pretrained=False, **extra),
                                 multi_task=3)


# ---------------------------------------------------------------- (a) validate
@pytest.mark.parametrize("heads", [12, 24, 48])
@pytest.mark.parametrize("kw", [dict(with_cffn=False), dict(with_cffn=False, cffn_ratio=1.0), dict(with_cffn=False, cffn_ratio=0.25)])
def test_validate_accepts_the_full_width(kw, heads):
    cfg = ModelConfig(num_heads=heads, **kw)
    cfg.validate()
    assert (cfg.adapter_dim, cfg.adapter_head_dim) == (768, 768 // heads)
    assert cfg.packed_in_proj and cfg.extractor_ffn == kw.get("with_cffn", True)


def test_the_shipped_configuration_is_not_packed():
    cfg = ModelConfig()
    assert (cfg.adapter_dim, cfg.packed_in_proj, cfg.extractor_ffn) == (192, False, True)
    assert not ModelConfig(cffn_ratio=0.75, num_heads=9).packed_in_proj


@pytest.mark.parametrize("kw,match", [
    (dict(cffn_ratio=1.5, num_heads=18), "E = 1152 >= embed_dim.*E > 768"),
    (dict(cffn_ratio=1.0), "E = 768 >= embed_dim.*with_cffn=False runs the full width"),
    (dict(with_cffn=False, num_heads=6), "with_cffn=False.*num_heads=6"),
    (dict(with_cffn=False, num_heads=8), "with_cffn=False.*num_heads=8"),
])
def test_validate_still_refuses_the_rest(kw, match):
    with pytest.raises(NotImplementedError, match=match):
        ModelConfig(**kw).validate()


@pytest.mark.parametrize("extra", list(SETTINGS.values()))
def test_titan_refuses_the_full_width_with_its_own_message(extra):
    from test_titan_cpu import TITAN_JSON
    with pytest.raises(NotImplementedError, match="full-width adapters are built for the LongNet configurations"):
        titan_model_config(dict(TITAN_JSON, **extra), 3, False, depth=6)
    titan_model_config(TITAN_JSON, 3, False, depth=6).validate()


def test_flop_count_takes_the_missing_projections():
    a = flops_per_slide_step(10000, 65)
    assert a == flops_per_slide_step(10000, 65, E=192, cffn=True)          # the defaults (what bench.py prints) have not moved
    full, bare = flops_per_slide_step(10000, 65, E=768), flops_per_slide_step(10000, 65, E=768, cffn=False)
    L, T, D = 10000, 65, 768
    assert full["adapter"] - bare["adapter"] == 2.0 * 2 * D * D * (3 * L + 5 * T)      # q_proj + output_proj of 3 Injectors, 5 Extractors
    assert bare["adapter"] > a["adapter"] and bare["gemm_layer"] == a["gemm_layer"]


# ---------------------------------------------------------------- (b) the parameter layout is the reference's
@pytest.mark.parametrize("tag", list(SETTINGS))
def test_param_specs_reproduce_the_reference_state_dict(layout, tag):
    ref = layout[tag]
    assert ref["config"] == SETTINGS[tag]
    specs = synth.param_specs(_cfg(SETTINGS[tag]), SIZES)
    assert [k for k, _, _, _ in specs] == list(ref["shapes"].keys())          # names, in state_dict order
    assert {k: list(sh) for k, sh, _, _ in specs} == ref["shapes"]
    assert [k for k, _, _, t in specs if t] == ref["trainable"]
    keys = {k for k in ref["shapes"] if not k.startswith("encoder.")}
    assert ref["shapes"]["interactions.2.injector.attn.multihead_attn.in_proj_weight"] == [2304, 768]
    assert ref["shapes"]["prompt_selfattention.1.self_attn.in_proj_weight"] == [2304, 768]
    assert not any(k.endswith(("q_proj_weight", "k_proj_weight", "v_proj_weight")) for k in keys)
    cffn = SETTINGS[tag].get("with_cffn", True)
    assert any(".ffn." in k and k.startswith("interactions.") for k in keys) == cffn
    assert any(k.endswith("attn.q_proj.weight") for k in keys) == cffn
    assert any(k.endswith("attn.output_proj.weight") for k in keys) == cffn


# ---------------------------------------------------------------- (c) init family of the packed matrix
@pytest.mark.parametrize("tag", ["nocffn", "nocffn_h24"])
def test_packed_matrix_init_matches_the_reference_statistics(layout, tag):
    """tests/test_init_cpu.py's bars on every in_proj_weight: xavier-uniform over the PACKED [2304, 768] shape, bound
    sqrt(6 / 3072) -- not the sqrt(6 / 1536) three separate [768, 768] matrices would get."""
    sd = init.init_state_dict(_cfg(SETTINGS[tag]), SIZES, seed=123, trainable_only=True)
    ref = layout[tag]["stats"]
    assert len(ref) == 10 and set(ref) == {k for k in sd if k.endswith("in_proj_weight")}
    bound = math.sqrt(6.0 / (2304 + 768))
    for k, (mean, std, lo, hi, n) in ref.items():
        v = sd[k].double()
        assert v.numel() == n == 2304 * 768, k
        s = float(v.std())
        assert abs(s / std - 1.0) < max(0.03, 8.0 / math.sqrt(2 * n)), (k, s, std)
        assert abs(float(v.mean()) - mean) < 6.0 * std / math.sqrt(n) * math.sqrt(2), (k, float(v.mean()), mean)
        tail, tail_ref = float(v.abs().max()) / s, max(abs(lo), abs(hi)) / std
        assert abs(tail / tail_ref - 1.0) < 0.25, (k, tail, tail_ref)
        assert float(v.abs().max()) <= bound and max(abs(lo), abs(hi)) <= bound * (1 + 1e-6)
        assert float(v.abs().max()) > 0.99 * bound


# ---------------------------------------------------------------- (d) the float64 restatements against the reference
def _t(a):
    return torch.from_numpy(np.asarray(a)).to(F64)


def _maxrel(a, b):
    return _maxrel_np(a.detach() if torch.is_tensor(a) else a, b)


@pytest.fixture(scope="module")
def unit(golden_dir):
    return np.load(os.path.join(golden_dir, "unit_full_width.npz"))


def _unit_case(unit):
    seed, T, L, heads = int(unit["seed"]), int(unit["T"]), int(unit["L"]), int(unit["heads"])
    cfg = _cfg(dict(with_cffn=False))
    sd = {k: _t(v) for k, v in synth.synth_state_dict(cfg, synth.toy_group_sizes(), seed).items()}
    x, c, pe = (_t(a) for a in unit_inputs.adapter_inputs(seed, T, L))
    r = np.random.Generator(np.random.PCG64([seed, T, 1]))
    dy_x, dy_c = _t(r.standard_normal((1, L, 768))), _t(r.standard_normal((1, T, 768)))
    return sd, x, c, pe, dy_x, dy_c, heads, int(unit["row_stride"])


def _check_param_grads(unit, tag, sd, prefix):
    n = 0
    for k in unit.files:
        if k.startswith(f"{tag}/gnorm/"):
            name = k[len(f"{tag}/gnorm/"):]
            g = sd[prefix + "." + name].grad
            assert abs(float(g.norm()) - float(unit[k])) <= 1e-9 * float(unit[k]), k
            if f"{tag}/grad/{name}" in unit.files:
                assert _maxrel(g, unit[f"{tag}/grad/{name}"]) < 1e-9, k
            else:
                rows = unit[f"{tag}/grad_rows/{name}"]
                nr = rows.shape[0] // 3 if name.endswith("in_proj_weight") else rows.shape[0]
                E = g.shape[1]
                ours = torch.cat([g[i * E:i * E + nr] for i in range(3)]) if name.endswith("in_proj_weight") else g[:nr]
                assert _maxrel(ours, rows) < 1e-9, k
            n += 1
    return n


def _leaf_sd(sd, prefix):
    return {k: (v.clone().requires_grad_(True) if k.startswith(prefix + ".") else v) for k, v in sd.items()}


def test_injector_restatement_matches_the_reference(unit):
    sd, x, c, pe, dy_x, _, heads, rs = _unit_case(unit)
    sd = _leaf_sd(sd, "interactions.0.injector")
    xv, cv = x.clone().requires_grad_(True), c.clone().requires_grad_(True)
    y = R.injector_nocffn(xv, cv, pe, sd, "interactions.0.injector", heads)
    y.backward(dy_x)
    assert _maxrel(y[:, ::rs], unit["injector/y_rows"]) < 1e-9
    assert _maxrel(xv.grad[:, ::rs], unit["injector/dx_rows"]) < 1e-9
    assert _maxrel(cv.grad, unit["injector/dc"]) < 1e-9
    assert _check_param_grads(unit, "injector", sd, "interactions.0.injector") == 9      # gamma, packed w / b, out_proj w / b, 2 norms
    assert float(sd["interactions.0.injector.gamma"].detach().abs().max()) > 0                  # (the synthetic gamma exercises the branch)


def test_extractor_restatement_matches_the_reference(unit):
    sd, x, c, pe, _, dy_c, heads, rs = _unit_case(unit)
    sd = _leaf_sd(sd, "interactions.0.extractor")
    xv, cv = x.clone().requires_grad_(True), c.clone().requires_grad_(True)
    y = R.extractor_nocffn(cv, xv, pe, sd, "interactions.0.extractor", heads)
    y.backward(dy_c)
    assert _maxrel(y, unit["extractor/y"]) < 1e-9
    assert _maxrel(xv.grad[:, ::rs], unit["extractor/dx_rows"]) < 1e-9
    assert _maxrel(cv.grad, unit["extractor/dc"]) < 1e-9
    assert _check_param_grads(unit, "extractor", sd, "interactions.0.extractor") == 8


def test_prompt_layer_restatement_matches_the_reference(unit):
    sd, _, c, pe, _, dy_c, heads, _ = _unit_case(unit)
    sd = _leaf_sd(sd, "prompt_selfattention.1")
    cv = c.clone().requires_grad_(True)
    y = R.prompt_self_attention_nocffn_masked(cv, pe, sd, "prompt_selfattention.1", heads)
    y.backward(dy_c)
    assert _maxrel(y, unit["selfattn/y"]) < 1e-9
    assert _maxrel(cv.grad, unit["selfattn/dc"]) < 1e-9
    assert _check_param_grads(unit, "selfattn", sd, "prompt_selfattention.1") == 6


def test_prompt_layer_restatement_under_the_reference_masks(unit):
    """p = 0.25, the masks the reference drew: mask 1 on the softmax probabilities, mask 2 on out_proj's result (with_cffn=False has
    no output_proj, adapter_modules.py:92)."""
    heads, p = int(unit["pd/meta"][0]), float(unit["pd/meta"][1])
    assert p == 0.25
    sd = {"l." + k[len("pd/sd/"):]: _t(unit[k]).requires_grad_(True) for k in unit.files if k.startswith("pd/sd/")}
    assert sorted(k[2:] for k in sd) == ["norm.bias", "norm.weight", "self_attn.in_proj_bias", "self_attn.in_proj_weight",
                                         "self_attn.out_proj.bias", "self_attn.out_proj.weight"]
    x = _t(unit["pd/x"]).requires_grad_(True)
    B, T, D = x.shape
    keep1, keep2 = torch.from_numpy(unit["pd/mask1"]).view(B, heads, T, T), torch.from_numpy(unit["pd/mask2"])
    assert 0 < int(keep1.sum()) < keep1.numel() and 0 < int(keep2.sum()) < keep2.numel()
    y = R.prompt_self_attention_nocffn_masked(x, _t(unit["pd/query_pos"]), sd, "l", heads, keep1, keep2, p)
    y.backward(_t(unit["pd/dy"]))
    assert _maxrel(y, unit["pd/y"]) < 1e-9
    assert _maxrel(x.grad, unit["pd/dx"]) < 1e-9
    for k in sd:
        assert _maxrel(sd[k].grad, unit["pd/grad/" + k[2:]]) < 1e-9, k
    # without the masks the result differs: the fixture does pin them
    y0 = R.prompt_self_attention_nocffn_masked(x, _t(unit["pd/query_pos"]), sd, "l", heads)
    assert _maxrel(y0, unit["pd/y"]) > 1e-3


def test_oracle_route_equals_the_restatements(unit):
    """The unchanged oracle fed `oracle_state` (packed rows as q / k / v views, identity q_proj / output_proj, a zero FFN) computes
    what the explicit with_cffn=False restatements compute, bit for bit: the constants are exact no-ops."""
    from oracle import modaltune_oracle as O
    sd, x, c, pe, _, _, heads, _ = _unit_case(unit)
    osd = R.oracle_state(sd, _cfg(dict(with_cffn=False)))
    assert torch.equal(O.injector(x, c, pe, osd, "interactions.0.injector", heads),
                       R.injector_nocffn(x, c, pe, sd, "interactions.0.injector", heads))
    assert torch.equal(O.extractor(c, x, pe, osd, "interactions.0.extractor", heads),
                       R.extractor_nocffn(c, x, pe, sd, "interactions.0.extractor", heads))
    assert torch.equal(O.prompt_self_attention(c, pe, osd, "prompt_selfattention.1", heads),
                       R.prompt_self_attention_nocffn_masked(c, pe, sd, "prompt_selfattention.1", heads))


def run_model_case(path, dtype=F64):
    """tests/test_oracle_golden.py::_run_model_case over a full-width fixture (the oracle through full_width_ref.oracle_state)."""
    g = np.load(path)
    L, depth, seed, ngrids = int(g["L"]), int(g["depth"]), int(g["seed"]), int(g["ngrids"])
    sizes = [int(s) for s in g["sizes"]]
    cfg = ModelConfig(depth=depth, interaction_indexes=tuple(tuple(int(i) for i in p) for p in g["inter"]), slide_ngrids=ngrids,
                      clinical=bool(int(g["clinical"])), token_agg=str(g["token_agg"]), multi_task=int(g["multi_task"]),
                      **json.loads(str(g["extra_cfg"])))
    cfg.validate()
    sd = {k: torch.from_numpy(v).to(dtype) for k, v in synth.synth_state_dict(cfg, sizes, seed).items()}
    inp = synth.synth_inputs(L, sizes, seed, grid=ngrids)
    psd = {k: torch.from_numpy(v).to(dtype) for k, v in synth.projector_state(seed).items()}
    x, coords = torch.from_numpy(inp["x"]).to(dtype), torch.from_numpy(inp["coords"]).to(dtype)
    genes = [torch.from_numpy(a).to(dtype) for a in inp["genes"]]
    logits, loss, grads = R.train_step_loss_and_grads(sd, cfg, synth.trainable_keys(cfg, sizes), x, coords, genes,
                                                      torch.from_numpy(inp["text"]).to(dtype), psd, segment_lengths())
    return g, cfg, logits, loss, grads


@pytest.mark.parametrize("tag", list(SETTINGS))
def test_oracle_route_reproduces_the_reference_model(golden_dir, tag):
    """tests/test_oracle_golden.py::test_full_train_step_f64's bars."""
    g, cfg, logits, loss, grads = run_model_case(os.path.join(golden_dir, f"model_L37_d3_{tag}.npz"))
    assert json.loads(str(g["extra_cfg"])) == SETTINGS[tag] and cfg.packed_in_proj
    assert _maxrel(logits, g["f64_logits"]) < 1e-9
    assert abs(float(loss) - float(g["f64_loss"])) < 1e-9 * abs(float(g["f64_loss"]))
    names = [str(n) for n in g["f64_grad_names"]]
    assert sorted(names) == sorted(grads.keys())
    ours = np.array([float(grads[n].norm()) for n in names])
    ref = g["f64_grad_norms"]
    assert np.abs(ours - ref).max() <= 1e-8 * ref.max()
    n = 0
    for k in g.files:
        if k.startswith("f64_grad/"):
            assert _maxrel(grads[k[len("f64_grad/"):]], g[k]) < 1e-8
            n += 1
    assert n >= (7 if cfg.extractor_ffn else 5)


# ---------------------------------------------------------------- (e) the parameter store: slices of ONE tensor, round trips
@pytest.fixture(scope="module")
def cpu_engines():
    from modaltune_amd.engine import Engine
    return {tag: Engine(_cfg(extra), SIZES, "cpu") for tag, extra in SETTINGS.items()}


@pytest.mark.parametrize("tag", ["nocffn", "nocffn_h24"])
def test_q_and_kv_rows_are_views_of_the_flat_buffers(cpu_engines, tag):
    eng = cpu_engines[tag]
    st, E, D = eng.store, 768, 768
    esz = st.flat.element_size()
    for pref in eng._cross_attn_prefixes():
        mp = pref + "multihead_attn."
        off, n, shape = st.slots[mp + "in_proj_weight"]
        assert (n, tuple(shape)) == (3 * E * D, (3 * E, D))
        Wq, Wk, Wv, bq, bk, bv = eng._mha_in(mp)
        for i, prm in enumerate((Wq, Wk, Wv)):
            assert tuple(prm.data.shape) == tuple(prm.grad.shape) == (E, D) and prm.data.is_contiguous() and prm.grad.is_contiguous()
            assert prm.data.data_ptr() == st.flat.data_ptr() + (off + i * E * D) * esz            # no second copy of the parameter
            assert prm.grad.data_ptr() == st.flat_grad.data_ptr() + (off + i * E * D) * esz       # ... nor of its gradient
        gkv = eng._mha_kv_grad(mp, st.grads)
        assert tuple(gkv.shape) == (2 * E, D) and gkv.is_contiguous() and gkv.stride(0) == D
        assert gkv.data_ptr() == Wk.grad.data_ptr() and gkv.data_ptr() + E * D * esz == Wv.grad.data_ptr()
        boff = st.slots[mp + "in_proj_bias"][0]
        for i, prm in enumerate((bq, bk, bv)):
            assert prm.grad.data_ptr() == st.flat_grad.data_ptr() + (boff + i * E) * esz
    # a second gradient set (pass groups): the slices follow it
    old = st.use_grad_set(*st.new_grad_set())
    try:
        mp = "interactions.0.extractor.attn.multihead_attn."
        assert eng._mha_kv_grad(mp, st.grads).data_ptr() == st.flat_grad.data_ptr() + (st.slots[mp + "in_proj_weight"][0] + E * D) * esz
        assert eng._mha_in(mp)[0].grad.data_ptr() == st.flat_grad.data_ptr() + st.slots[mp + "in_proj_weight"][0] * esz
    finally:
        st.use_grad_set(*old)
    assert st.n_flat == sum((int(np.prod(sh)) + 3) // 4 * 4 for _, sh, _, t in st.specs if t)      # one buffer, nothing beside it


def test_shipped_layout_keeps_its_adjacent_k_v_destination():
    from modaltune_amd.engine import Engine
    eng = Engine(_cfg({}), SIZES, "cpu")
    st = eng.store
    mp = "interactions.1.extractor.attn.multihead_attn."
    gkv = eng._mha_kv_grad(mp, st.grads)
    assert gkv.data_ptr() == st.grads[mp + "k_proj_weight"].data_ptr()
    assert st.slots[mp + "v_proj_weight"][0] == st.slots[mp + "k_proj_weight"][0] + 192 * 768
    assert eng._mha_in(mp)[0].grad.data_ptr() == st.grads[mp + "q_proj_weight"].data_ptr()


@pytest.mark.parametrize("tag", ["nocffn", "nocffn_h24"])
def test_module_round_trips_a_reference_shaped_state_dict(layout, tag):
    from modaltune_amd.aggregators import Aggregator
    groups = {i: ["g"] * n for i, n in enumerate(SIZES)}
    kw = dict(GIGAPATH_JSON, depth=3, interaction_indexes=INTER, slide_ngrids=128, pretrained=False)
    model = Aggregator.create("longnetvit_gene_adapter", gene_group_defination=groups, multi_task=3, device="cpu", **dict(kw, **SETTINGS[tag]))
    ref = layout[tag]["shapes"]
    sd = model.state_dict()
    assert list(sd.keys()) == list(ref.keys()) and {k: list(v.shape) for k, v in sd.items()} == ref
    assert [k for k, p in model.named_parameters() if p.requires_grad] == layout[tag]["trainable"]
    new = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(model.cfg, SIZES, 5).items()}
    res = model.load_state_dict(new, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    back = model.state_dict()
    assert all(torch.equal(back[k], new[k]) for k in new)
    # a checkpoint of the other layout: the real missing / unexpected keys
    shipped = Aggregator.create("longnetvit_gene_adapter", gene_group_defination=groups, multi_task=3, device="cpu", **kw)
    with pytest.raises(RuntimeError) as e:
        shipped.load_state_dict(new, strict=True)
    assert "q_proj_weight" in str(e.value) and "in_proj_weight" in str(e.value)
    with pytest.raises(RuntimeError) as e:
        model.load_state_dict(shipped.state_dict(), strict=True)
    assert "in_proj_weight" in str(e.value) and "k_proj_weight" in str(e.value)
