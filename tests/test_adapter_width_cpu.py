"""CPU: adapter widths other than the shipped 12 heads x 16 (`cffn_ratio`, `num_heads`): what ModelConfig.validate() accepts and
refuses, and the unchanged oracle against reference goldens generated at four new widths
(tests/golden/make_golden_adapter_width.py) -- the yardstick the GPU tests of tests/test_adapter_width_gpu.py are held against."""
import os

import numpy as np
import pytest
import torch

from modaltune_amd.config import ModelConfig, flops_per_slide_step, flops_per_titan_step
from modaltune_amd.titan import titan_model_config
from oracle import modaltune_oracle as O

from test_oracle_golden import F64, _maxrel, _run_model_case

# (cffn_ratio, num_heads) -> (E, head dim): every supported family member the reference's state-dict layout was compared at
SUPPORTED = {(0.25, 12): (192, 16), (0.25, 6): (192, 32), (0.25, 3): (192, 64), (1 / 3, 8): (256, 32), (0.5, 24): (384, 16),
             (0.5, 12): (384, 32), (0.5, 6): (384, 64), (0.75, 9): (576, 64), (0.75, 36): (576, 16)}
WIDTH_TAGS = ["h6x64", "h6x32", "h24x16", "h9x64"]


@pytest.mark.parametrize("ratio,heads", sorted(SUPPORTED))
def test_validate_accepts_the_supported_widths(ratio, heads):
    cfg = ModelConfig(cffn_ratio=ratio, num_heads=heads)
    cfg.validate()
    assert (cfg.adapter_dim, cfg.adapter_head_dim) == SUPPORTED[(ratio, heads)]
    assert cfg.adapter_dim == heads * cfg.adapter_head_dim


@pytest.mark.parametrize("kw,exc,match", [
    (dict(num_heads=5), ValueError, "num_heads=5 does not divide the adapter width E = 192"),
    (dict(num_heads=48), NotImplementedError, "head dim of 4.*16, 32 and 64"),
    (dict(num_heads=2), NotImplementedError, "head dim of 96"),
    (dict(cffn_ratio=1.0), NotImplementedError, "E = 768 >= embed_dim.*in_proj_weight"),
    (dict(cffn_ratio=2.0, num_heads=24), NotImplementedError, "in_proj_weight"),
    (dict(cffn_ratio=0.3), ValueError, "E = int\\(768 \\* cffn_ratio\\) = 230.*multiple of 64"),
    (dict(cffn_ratio=0.01), ValueError, "multiple of 64"),
    (dict(num_heads=0), ValueError, "num_heads=0"),
])
def test_validate_refuses_everything_else_and_names_the_rule(kw, exc, match):
    with pytest.raises(exc, match=match):
        ModelConfig(**kw).validate()


def test_earlier_refusals_come_first():
    """A configuration that an older check refuses still raises THAT error, whatever its width."""
    with pytest.raises(ValueError, match="Prov-GigaPath geometry"):
        ModelConfig(embed_dim=256, num_heads=5).validate()
    with pytest.raises(NotImplementedError, match="with_cffn=False"):
        ModelConfig(with_cffn=False, num_heads=5).validate()
    with pytest.raises(NotImplementedError, match="freeze_vit=False"):
        ModelConfig(freeze_vit=False, cffn_ratio=0.3).validate()
    with pytest.raises(ValueError, match="add_prompt_feature=False"):
        ModelConfig(add_prompt_feature=False, cffn_ratio=1.0).validate()


def test_titan_config_carries_the_width():
    from test_titan_cpu import TITAN_JSON
    cfg = titan_model_config(dict(TITAN_JSON, num_heads=6), 3, False, depth=6)
    cfg.validate()
    assert (cfg.adapter_dim, cfg.num_heads, cfg.adapter_head_dim) == (192, 6, 32)
    with pytest.raises(ValueError, match="num_heads=5"):
        titan_model_config(dict(TITAN_JSON, num_heads=5), 3, False, depth=6).validate()


def test_flop_counts_take_the_adapter_width():
    a, b = flops_per_slide_step(10000, 65), flops_per_slide_step(10000, 65, E=192)
    assert a == b                                         # the default is the shipped width
    wide = flops_per_slide_step(10000, 65, E=384)
    assert wide["adapter"] > 2 * a["adapter"] * 0.99 and wide["gemm_layer"] == a["gemm_layer"]
    assert flops_per_titan_step(3000, 65) == flops_per_titan_step(3000, 65, E=192)
    assert flops_per_titan_step(3000, 65, E=576)["adapter"] > flops_per_titan_step(3000, 65)["adapter"]


@pytest.mark.parametrize("tag", WIDTH_TAGS)
def test_oracle_reproduces_the_reference_at_the_new_widths(golden_dir, tag):
    """tests/test_oracle_golden.py::test_full_train_step_f64's bars: the oracle is a valid yardstick at these widths."""
    g, cfg, logits, loss, grads = _run_model_case(os.path.join(golden_dir, f"model_L37_d3_{tag}.npz"), F64)
    assert f"h{cfg.num_heads}x{cfg.adapter_head_dim}" == tag
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
    assert n >= 6


def test_oracle_titan_flow_at_6x32(golden_dir):
    """tests/test_titan_cpu.py's oracle check on the 6 x 32 TITAN fixture."""
    import json
    import titan_standin
    from modaltune_amd import synth
    from test_titan_cpu import TITAN_JSON
    g = np.load(os.path.join(golden_dir, "model_titan_L300_h6x32.npz"))
    extra = json.loads(str(g["extra_cfg"]))
    assert extra == {"num_heads": 6}
    L, seed, grid = int(g["L"]), int(g["seed"]), int(g["grid"])
    sizes = [int(s) for s in g["sizes"]]
    cfg = titan_model_config(dict(TITAN_JSON, **extra), 3, False, depth=6)
    inp = synth.synth_inputs_titan(L, sizes, seed, grid=grid)
    vit = titan_standin.VisionTransformer()
    titan_standin.init_standin(vit, seed)
    vit = vit.double()
    trainable = set(synth.trainable_keys(cfg, sizes))
    sd = {k: torch.from_numpy(v).to(F64) for k, v in synth.synth_state_dict(cfg, sizes, seed).items()}
    sd = {k: (v.clone().requires_grad_(True) if k in trainable else v) for k, v in sd.items()}
    x, coords = torch.from_numpy(inp["x"]).to(F64), torch.from_numpy(inp["coords"])
    genes = [torch.from_numpy(a).to(F64) for a in inp["genes"]]
    logits = torch.cat([O.titan_model_forward(sd, cfg, vit, x, coords, genes, torch.eye(3, dtype=F64)[t], clinical=None) for t in range(3)])
    psd = {k: torch.from_numpy(v).to(F64) for k, v in synth.projector_state(seed).items()}
    loss = O.distill_loss(logits, O.projector_forward(torch.from_numpy(inp["text"]).to(F64), psd))
    loss.backward()
    assert float((logits.detach() - torch.from_numpy(g["f64_logits"])).abs().max()) < 1e-9 * float(np.abs(g["f64_logits"]).max())
    assert abs(float(loss.detach()) - float(g["f64_loss"])) < 1e-9 * abs(float(g["f64_loss"]))
    names = [str(n) for n in g["f64_grad_names"]]
    ours = np.array([float(sd[n].grad.norm()) for n in names])
    assert np.abs(ours - g["f64_grad_norms"]).max() <= 1e-8 * g["f64_grad_norms"].max()
