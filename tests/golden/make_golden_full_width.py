"""Golden vectors of the full-width adapters (E = 768): runs the REFERENCE (imported read-only, as make_golden.py does) with
`with_cffn=False` -- no q_proj / output_proj, no Extractor FFN, nn.MultiheadAttention(768, heads, kdim=vdim=768) with ONE packed
in_proj_weight [2304, 768] (adapter_modules.py:24-94,139-234,296-335) -- on seeded synthetic weights / inputs.

Run in the build container only:   python tests/golden/make_golden_full_width.py
Writes model_L37_d3_{nocffn,nocffn_h24}.npz (make_golden.model_case: three task passes, loss, backward, fp64; slimmed as
make_golden_adapter_width.py does), attn_maps_L37_d3_nocffn.npz (make_golden_attn_maps.run_case), unit_full_width.npz (the
reference's Injector / Extractor / SelfAttentionLayer with with_cffn=False in float64 at T = 7, L = 37: outputs, input gradients
(of the [L, 768] patch-side tensors every third row: the file stays below 1 MiB), the small parameter gradients in full and every
parameter gradient's norm and the leading rows of each q / k / v third; plus a narrow
prompt layer at p = 0.25 under masks the reference drew, the recipe of make_golden_prompt_dropout.py) and full_width_layout.json (per
setting: the reference's state_dict key -> shape, its trainable names, and mean / std / min / max / numel of the freshly
initialised packed matrices).  Nothing from the reference is copied; the model weights and inputs are regenerated from (config, seed)
through modaltune_amd/synth.py and are not stored.
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (installs the reference shims, imports the reference)
import make_golden_attn_maps as MA  # noqa: E402
import unit_inputs  # noqa: E402
from make_golden_adapter_width import INTER, slim  # noqa: E402

from modaltune_amd import synth  # noqa: E402
from modaltune_amd.config import ModelConfig  # noqa: E402

# tag -> (seed, overrides)
SETTINGS = {"nocffn": (81, dict(with_cffn=False)),
            "nocffn_h24": (82, dict(with_cffn=False, num_heads=24))}
UNIT_SEED, UNIT_T, UNIT_L, UNIT_HEADS = 84, 7, 37, 12
ROW_STRIDE = 3         # patch rows kept of the [L, 768] outputs / input gradients
LEAD_ROWS = 2          # rows kept of each q / k / v third of a [2304, 768] gradient
PD_CASE = (85, 64, 4, 0.25, 3, 5)      # seed, d_model (= E: 4 heads x 16), heads, p, B, T


def _grads(mod, out, prefix):
    """Parameter gradients of `mod`: norms of all, small ones in full, the leading rows of each third of a packed matrix."""
    for k, q in mod.named_parameters():
        g = q.grad.numpy()
        out[f"{prefix}/gnorm/{k}"] = np.float64(np.linalg.norm(g))
        if g.ndim == 1:
            out[f"{prefix}/grad/{k}"] = g.copy()
        elif k.endswith("in_proj_weight"):
            E = g.shape[1]
            out[f"{prefix}/grad_rows/{k}"] = np.concatenate([g[i * E:i * E + LEAD_ROWS] for i in range(3)])
        else:
            out[f"{prefix}/grad_rows/{k}"] = g[:LEAD_ROWS].copy()


def unit_full_width():
    cfg = ModelConfig.from_json(MG.REF_CFG, depth=3, interaction_indexes=INTER, with_cffn=False)
    sd = synth.synth_state_dict(cfg, synth.toy_group_sizes(), UNIT_SEED)
    dt = torch.float64
    T, L = UNIT_T, UNIT_L
    x, c, pe = unit_inputs.adapter_inputs(UNIT_SEED, T, L)
    r = np.random.Generator(np.random.PCG64([UNIT_SEED, T, 1]))
    dy_x, dy_c = r.standard_normal((1, L, 768)), r.standard_normal((1, T, 768))
    out = {"seed": UNIT_SEED, "T": T, "L": L, "heads": UNIT_HEADS, "row_stride": ROW_STRIDE}

    def leaves():
        return MG.tt(x, dt).requires_grad_(True), MG.tt(c, dt).requires_grad_(True)

    inj = MG.Injector(dim=768, num_heads=UNIT_HEADS, init_values=0.0, with_cffn=False).double()
    inj.load_state_dict(MG.sub_state(sd, "interactions.0.injector.", dt), strict=True)
    xv, cv = leaves()
    y = inj(query=xv, feat=cv, pos=MG.tt(pe, dt))
    y.backward(MG.tt(dy_x, dt))
    out["injector/y_rows"], out["injector/dx_rows"], out["injector/dc"] = y.detach().numpy()[:, ::ROW_STRIDE].copy(), xv.grad.numpy()[:, ::ROW_STRIDE].copy(), cv.grad.numpy()
    _grads(inj, out, "injector")

    ext = MG.Extractor(dim=768, num_heads=UNIT_HEADS, with_cffn=False, drop=0.0, drop_path=0.0).double()
    ext.load_state_dict(MG.sub_state(sd, "interactions.0.extractor.", dt), strict=True)
    assert not hasattr(ext, "ffn") and not hasattr(ext, "drop_path")
    xv, cv = leaves()
    y = ext(query=cv, feat=xv, pos=MG.tt(pe, dt))
    y.backward(MG.tt(dy_c, dt))
    out["extractor/y"], out["extractor/dx_rows"], out["extractor/dc"] = y.detach().numpy(), xv.grad.numpy()[:, ::ROW_STRIDE].copy(), cv.grad.numpy()
    _grads(ext, out, "extractor")

    sa = MG.SelfAttentionLayer(d_model=768, nheads=UNIT_HEADS, dropout=0.0, normalize_before=True, with_cffn=False).double()
    sa.load_state_dict(MG.sub_state(sd, "prompt_selfattention.1.", dt), strict=True)
    _, cv = leaves()
    y = sa(cv, MG.tt(pe, dt))
    y.backward(MG.tt(dy_c, dt))
    out["selfattn/y"], out["selfattn/dc"] = y.detach().numpy(), cv.grad.numpy()
    _grads(sa, out, "selfattn")

    for k, v in prompt_dropout_case(*PD_CASE).items():
        out["pd/" + k] = v
    path = os.path.join(HERE, "unit_full_width.npz")
    np.savez_compressed(path, **out)
    print(os.path.basename(path), os.path.getsize(path), "bytes", flush=True)


def prompt_dropout_case(seed, d_model, heads, p, B, T):
    """make_golden_prompt_dropout.run_case with with_cffn=False: the second mask sits on out_proj's result (adapter_modules.py:92)."""
    torch.manual_seed(seed)
    layer = MG.SelfAttentionLayer(d_model=d_model, nheads=heads, dropout=p, normalize_before=True, with_cffn=False)
    assert not hasattr(layer, "q_proj") and layer.self_attn.in_proj_weight is not None
    with torch.no_grad():      # biases and the LayerNorm away from their 0 / 1 initial values; everything exactly float32
        for q in layer.parameters():
            if q.dim() == 1:
                q.add_(0.1 * torch.randn_like(q))
            q.copy_(q.float())
    layer = layer.double()
    x = torch.randn(B, T, d_model).double().requires_grad_(True)
    pos = torch.randn(T, d_model).double()
    dy = torch.randn(B, T, d_model).double()
    calls = []
    gen = torch.Generator().manual_seed(seed + 1000)
    real = F.dropout

    def recording_dropout(t, p=0.5, training=True, inplace=False):
        if not training or p == 0.0:
            return t
        keep = (torch.rand(t.shape, generator=gen) >= p)
        calls.append((tuple(t.shape), float(p), keep))
        return t * keep.to(t.dtype) / (1.0 - p)
    F.dropout = torch.nn.functional.dropout = recording_dropout
    try:
        layer.eval()
        layer(x, pos)
        assert not calls, "eval() must draw no mask"
        layer.train()
        y = layer(x, pos)
    finally:
        F.dropout = torch.nn.functional.dropout = real
    assert [c[0] for c in calls] == [(B * heads, T, T), (B, T, d_model)], [c[0] for c in calls]      # exactly two, in this order
    assert all(c[1] == p for c in calls)
    y.backward(dy)
    out = {"meta": np.array([heads, p], dtype=np.float64), "x": x.detach().numpy(), "query_pos": pos.numpy(), "dy": dy.numpy(),
           "mask1": calls[0][2].numpy().astype(np.uint8), "mask2": calls[1][2].numpy().astype(np.uint8),
           "y": y.detach().numpy(), "dx": x.grad.numpy()}
    for k, v in layer.state_dict().items():
        out["sd/" + k] = v.numpy().astype(np.float32)
        assert np.array_equal(out["sd/" + k].astype(np.float64), v.numpy())
    for k, q in layer.named_parameters():
        out["grad/" + k] = q.grad.numpy()
    return out


def layout():
    """state_dict key -> shape, trainable names and the init statistics of the packed matrices, per setting."""
    sizes = synth.toy_group_sizes(6)
    groups = {i: ["g"] * n for i, n in enumerate(sizes)}
    table = {}
    for tag, (_, extra) in SETTINGS.items():
        cfg_kw = dict(MG.REF_CFG)
        cfg_kw.update(depth=3, interaction_indexes=INTER, slide_ngrids=128, pretrained=False)
        cfg_kw.update(extra)
        torch.manual_seed(0)
        model = MG.Aggregator.create("longnetvit_gene_adapter", gene_group_defination=groups, **cfg_kw, multi_task=3)
        stats = {}
        for k, v in model.state_dict().items():
            if k.endswith("in_proj_weight"):
                v = v.double()
                stats[k] = [float(v.mean()), float(v.std()), float(v.min()), float(v.max()), int(v.numel())]
        table[tag] = {"config": extra, "shapes": {k: list(v.shape) for k, v in model.state_dict().items()},
                      "trainable": [k for k, p in model.named_parameters() if p.requires_grad], "stats": stats}
    with open(os.path.join(HERE, "full_width_layout.json"), "w") as f:
        json.dump(table, f, indent=1)
        f.write("\n")
    print("wrote full_width_layout.json:", {k: len(v["shapes"]) for k, v in table.items()}, flush=True)


if __name__ == "__main__":
    torch.manual_seed(0)
    which = sys.argv[1:] or ["layout", "unit"] + list(SETTINGS) + ["maps"]
    if "layout" in which:
        layout()
    if "unit" in which:
        unit_full_width()
    for tag, (seed, extra) in SETTINGS.items():
        if tag in which:
            MG.model_case(f"L37_d3_{tag}", 37, 3, INTER, seed, dtypes=(torch.float64,), extra=extra)
            slim(os.path.join(HERE, f"model_L37_d3_{tag}.npz"))
    if "maps" in which:
        seed, extra = SETTINGS["nocffn"]
        sites, legend, maps, meta = MA.run_case(37, seed, extra=extra)
        out = dict(meta)
        out.update({"map/" + s: maps[s] for s in sites})
        path = os.path.join(HERE, "attn_maps_L37_d3_nocffn.npz")
        np.savez_compressed(path, **out)
        print(os.path.basename(path), len(sites), "sites", os.path.getsize(path), "bytes", flush=True)
