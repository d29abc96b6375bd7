"""Golden attention maps of the Modal-Adapter: runs the REFERENCE (imported read-only from /root/reference, as make_golden.py does) on
seeded synthetic weights / inputs and records the head-averaged attention weights that forward hooks on its nn.MultiheadAttention
modules read as output[1] -- the maps of the reference's README Figure 3.

Run in the build container only:   python tests/golden/make_golden_attn_maps.py
Writes attn_maps_<case>.npz (float32 maps per site, the three task passes of multitask_forward stacked as rows; the config and seed
that regenerate weights and inputs through modaltune_amd/synth.py) and attn_sites.json (per config: the reference's site names in
named_modules() order and the token legend, each token identified by matching the injector's token input against the reference's
own task / gene_cls / clinical / gene-encoder outputs).  Nothing from the reference is copied; weights and inputs are not stored.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import ref_shims  # noqa: E402

ref_shims.install()

from models.aggregators import Aggregator  # noqa: E402  (reference)

from modaltune_amd.config import ModelConfig  # noqa: E402
from modaltune_amd import synth  # noqa: E402

REF_CFG = json.load(open("/root/reference/model_configs/modaltune_gigapath_config.json"))
INTER = [[0, 0], [1, 1], [2, 2]]
# L = 1500: a few sites, one task pass each where the map is [T, L] or [L, T] (a committed file stays well below 1 MiB)
SUBSET_1500 = {"interactions.0.extractor.attn.multihead_attn": (1,), "interactions.2.injector.attn.multihead_attn": (2,),
               "prompt_selfattention.2.self_attn": (0, 1, 2)}


def tt(a, dtype):
    return torch.from_numpy(np.asarray(a)).to(dtype)


def run_case(L, seed, clinical=False, token_agg=None, extra=None, dt=torch.float64):
    cfg_kw = dict(REF_CFG)
    cfg_kw.update(depth=3, interaction_indexes=INTER, slide_ngrids=128, pretrained=False)
    if token_agg:
        cfg_kw["token_agg"] = token_agg
    cfg_kw.update(extra or {})
    cfg = ModelConfig.from_json(cfg_kw, multi_task=3, clinical=clinical)
    sizes = synth.toy_group_sizes(6)
    groups = {i: ["g"] * n for i, n in enumerate(sizes)}
    sd = synth.synth_state_dict(cfg, sizes, seed)
    inp = synth.synth_inputs(L, sizes, seed, grid=128)
    model = Aggregator.create("longnetvit_gene_clinical_adapter" if clinical else "longnetvit_gene_adapter",
                              gene_group_defination=groups, **cfg_kw, multi_task=3)
    model.load_state_dict({k: tt(v, torch.float32) for k, v in sd.items()}, strict=True)
    model = model.to(dt)
    ref_shims.zero_dropout(model)
    model.eval()
    sites = [n for n, m in model.named_modules() if isinstance(m, torch.nn.MultiheadAttention)]
    maps, feats = {s: [] for s in sites}, []

    def hook(name):
        def f(mod, args, out):
            maps[name].append(out[1].detach().numpy().astype(np.float32))
        return f
    hs = [m.register_forward_hook(hook(n)) for n, m in model.named_modules() if n in maps]
    hs.append(model.interactions[0].injector.register_forward_pre_hook(
        lambda mod, args, kwargs: feats.append(kwargs["feat"].detach().clone()), with_kwargs=True))
    x, coords = tt(inp["x"], dt), tt(inp["coords"], dt)
    genes = {i: tt(g, dt) for i, g in enumerate(inp["genes"])}
    clin = tt(inp["clinical"], dt) if clinical else []
    with torch.no_grad():
        logits = torch.cat([model(x=x, coords=coords, genes=genes, clinical=clin, task_token=torch.eye(3, dtype=dt)[t])
                            for t in (0, 1, 2)], dim=0)
        # token legend: which reference component each row of the injector's token input is
        cands = {"task": model.task_weight(torch.eye(3, dtype=dt)[0].unsqueeze(0)).reshape(1, -1)}
        if hasattr(model, "gene_cls") and model.prompt_agg == "cls":
            cands["gene_cls"] = model.gene_cls.reshape(1, -1)
        if clinical:
            cands["clinical"] = model.clinical_mlp(clin).reshape(1, -1)
        gemb = model.gene_encoder(genes).reshape(-1, cands["task"].shape[-1])
        legend = []
        for row in feats[0].reshape(-1, gemb.shape[-1]):
            hit = [k for k, c in cands.items() if torch.allclose(row, c[0], rtol=0, atol=1e-12)]
            hit += [f"gene:{g}" for g in range(gemb.shape[0]) if torch.allclose(row, gemb[g], rtol=0, atol=1e-12)]
            assert len(hit) == 1, hit
            legend.append(hit[0])
    for h in hs:
        h.remove()
    meta = {"L": L, "depth": 3, "inter": np.array(INTER), "seed": seed, "ngrids": 128, "sizes": np.array(sizes), "clinical": int(clinical),
            "token_agg": cfg.token_agg, "multi_task": 3, "extra_cfg": json.dumps(extra or {}), "f64_logits": logits.numpy()}
    return sites, legend, {s: np.concatenate(v, axis=0) for s, v in maps.items()}, meta


def record(name, L, seed, subset=None, **kw):
    sites, legend, maps, meta = run_case(L, seed, **kw)
    out = dict(meta)
    for s in sites:
        if subset is None:
            out["map/" + s] = maps[s]
        elif s in subset:
            for t in subset[s]:
                out[f"map/{s}/task{t}"] = maps[s][t]
    path = os.path.join(HERE, f"attn_maps_{name}.npz")
    np.savez_compressed(path, **out)
    print(name, len(sites), "sites", os.path.getsize(path), "bytes", flush=True)
    return sites, legend


if __name__ == "__main__":
    torch.manual_seed(0)
    table = {}
    for name, L, seed, kw, subset in (("L37_d3", 37, 41, {}, None),
                                      ("L37_d3_cls_cat", 37, 42, dict(token_agg="cat", extra=dict(prompt_agg="cls")), None),
                                      ("L37_d3_clin", 37, 43, dict(clinical=True), None),
                                      ("L1500_d3", 1500, 44, {}, SUBSET_1500)):
        sites, legend = record(name, L, seed, subset, **kw)
        table[name] = {"config": {"clinical": bool(kw.get("clinical", False)), "token_agg": kw.get("token_agg", "sum"),
                                  **kw.get("extra", {})}, "sites": sites, "tokens": legend}
    for name, extra in (("no_prompt_sa", dict(use_prompt_sa=False)), ("no_extra_extractor", dict(use_extra_extractor=False))):
        sites, legend, _, _ = run_case(5, 45, extra=extra)
        table[name] = {"config": {"clinical": False, "token_agg": "sum", **extra}, "sites": sites, "tokens": legend}
    with open(os.path.join(HERE, "attn_sites.json"), "w") as f:
        json.dump(table, f, indent=1)
        f.write("\n")
