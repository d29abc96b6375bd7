"""Golden vectors at adapter widths other than the shipped 12 heads x 16: runs the REFERENCE (imported read-only, as make_golden.py
does) with `cffn_ratio` / `num_heads` overridden -- adapter width E = int(768 * cffn_ratio), nn.MultiheadAttention(E, num_heads)
(adapter_modules.py:153-164) -- on seeded synthetic weights / inputs.

Run in the build container only:   python tests/golden/make_golden_adapter_width.py
Writes, per width, model_L37_d3_<tag>.npz (make_golden.model_case: three task passes, loss, backward, fp64) and
attn_maps_L37_d3_<tag>.npz (make_golden_attn_maps.run_case: the head-averaged attention of every site), and one TITAN case on the
stand-in backbone at 6 heads x 32, model_titan_L300_h6x32.npz (make_golden.titan_case's recipe with num_heads overridden: that
function reads the shipped TITAN JSON and takes no override).  Nothing from the reference is copied; weights and inputs are not
stored.  A committed fixture stays below 1 MiB: of the interaction-block taps that model_case records, the [T, 768] token taps are
kept for the first and last block of task pass 0 only (tests report the taps, they do not assert on them).
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (installs the reference shims, imports the reference)
import make_golden_attn_maps as MA  # noqa: E402

INTER = [[0, 0], [1, 1], [2, 2]]
# tag -> (seed, overrides): heads x head dim = 6 x 64, 6 x 32, 24 x 16 and 9 x 64 (E = 384, 192, 384, 576: the widest)
WIDTHS = {"h6x64": (51, dict(cffn_ratio=0.5, num_heads=6)),
          "h6x32": (52, dict(num_heads=6)),
          "h24x16": (53, dict(cffn_ratio=0.5, num_heads=24)),
          "h9x64": (54, dict(cffn_ratio=0.75, num_heads=9))}
TITAN_HEADS = 6


def slim(path):
    """Of the nine [1, T, 768] token taps (0.2 MB each, 1.8 of the 2.2 MB model_case writes) keep task pass 0's first and last."""
    g = np.load(path)
    kept_taps = ("f64_tap/task0/c0", f"f64_tap/task0/c{len(INTER) - 1}")

    def dropped(k):
        last = k.split("/")[-1]
        return k.startswith("f64_tap/") and last.startswith("c") and not last.startswith("cls") and k not in kept_taps
    keep = {k: g[k] for k in g.files if not dropped(k)}
    np.savez_compressed(path, **keep)
    print(os.path.basename(path), os.path.getsize(path), "bytes", flush=True)


def titan_width_case(name, L, seed, num_heads, grid=24):
    """make_golden.titan_case (same stand-in backbone, same recorded keys) with `num_heads` overridden; the override is recorded
    as `extra_cfg`."""
    import titan_standin
    from modaltune_amd import synth
    from modaltune_amd.titan import titan_model_config
    cfg_kw = json.load(open("/root/reference/model_configs/modaltune_titan_config.json"))
    cfg_kw.update(pretrained=False, drop_path_rate=0.0, num_heads=num_heads)
    sizes = synth.toy_group_sizes(6)
    groups = {i: ["g"] * n for i, n in enumerate(sizes)}
    dt = torch.float64
    model = MG.Aggregator.create("titan_gene_adapter", gene_group_defination=groups, **cfg_kw, multi_task=3)
    titan_standin.init_standin(model, seed)
    cfg = titan_model_config(cfg_kw, 3, False, depth=6)
    adapter_sd = {k: MG.tt(v, torch.float32) for (k, _, _, train), v in
                  zip(synth.param_specs(cfg, sizes), synth.synth_state_dict(cfg, sizes, seed).values()) if train}
    res = model.load_state_dict(adapter_sd, strict=False)
    backbone_keys = set(titan_standin.VisionTransformer().state_dict().keys())
    assert not res.unexpected_keys and set(res.missing_keys) <= backbone_keys
    assert sorted(k for k, p in model.named_parameters() if p.requires_grad) == sorted(adapter_sd.keys())
    model = model.to(dt)
    MG.ref_shims.zero_dropout(model)
    model.train()
    inp = synth.synth_inputs_titan(L, sizes, seed, grid=grid)
    proj = MG.TM.Projection_layer(512, 256)
    proj.load_state_dict({k: MG.tt(v, torch.float32) for k, v in synth.projector_state(seed).items()}, strict=True)
    proj = proj.to(dt)
    for prm in proj.parameters():
        prm.requires_grad = False
    x, coords = MG.tt(inp["x"], dt), torch.from_numpy(inp["coords"])
    genes = {i: MG.tt(g, dt) for i, g in enumerate(inp["genes"])}
    text = proj(MG.tt(inp["text"], dt)); text = text / text.norm(dim=-1, keepdim=True)
    torch.set_default_dtype(dt)      # (preprocess_features builds its grid with torch.zeros(...): default dtype)
    fg, cg, bgm = model.preprocess_features(x, coords, 1024)
    logits = torch.cat([model(x=x, coords=coords, genes=genes, task_token=torch.eye(3, dtype=dt)[t]) for t in (0, 1, 2)], dim=0)
    logit = logits / logits.norm(dim=-1, keepdim=True)
    loss = torch.nn.KLDivLoss(reduction="sum")(torch.nn.functional.log_softmax(logit, dim=1),
                                              torch.nn.functional.softmax(text[[0, 1, 3], :], dim=1)) * 10
    loss.backward()
    torch.set_default_dtype(torch.float32)
    names, norms = [], []
    for k, p in model.named_parameters():
        if p.requires_grad:
            names.append(k); norms.append(float(p.grad.double().norm()))
    out = {"L": L, "seed": seed, "grid": grid, "sizes": np.array(sizes), "clinical": 0, "extra_cfg": json.dumps({"num_heads": num_heads}),
           "grid_hw": np.array(fg.shape[-2:]), "n_foreground": int(bgm.sum()), "bg_mask": bgm.numpy(),
           "grid_feature_sum": fg.sum(dim=1).numpy().astype(np.float32), "coords_grid": cg.numpy(),
           "f64_logits": logits.detach().numpy(), "f64_loss": loss.detach().numpy(), "f64_grad_names": np.array(names),
           "f64_grad_norms": np.array(norms)}
    params = dict(model.named_parameters())
    for k in MG.GRAD_KEYS_FULL:
        if k in params:
            out["f64_grad/" + k] = params[k].grad.numpy().copy()
    path = os.path.join(HERE, f"model_{name}.npz")
    np.savez_compressed(path, **out)
    print(name, "loss", float(loss), "foreground", int(bgm.sum()), os.path.getsize(path), "bytes", flush=True)


if __name__ == "__main__":
    torch.manual_seed(0)
    which = sys.argv[1:] or list(WIDTHS) + ["titan"]
    for tag, (seed, extra) in WIDTHS.items():
        if tag not in which:
            continue
        MG.model_case(f"L37_d3_{tag}", 37, 3, INTER, seed, dtypes=(torch.float64,), extra=extra)
        slim(os.path.join(HERE, f"model_L37_d3_{tag}.npz"))
        sites, legend, maps, meta = MA.run_case(37, seed, extra=extra)
        out = dict(meta)
        out.update({"map/" + s: maps[s] for s in sites})
        path = os.path.join(HERE, f"attn_maps_L37_d3_{tag}.npz")
        np.savez_compressed(path, **out)
        print(os.path.basename(path), len(sites), "sites", os.path.getsize(path), "bytes", flush=True)
    if "titan" in which:
        titan_width_case(f"titan_L300_h{TITAN_HEADS}x32", 300, 61, TITAN_HEADS)
