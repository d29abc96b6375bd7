"""Golden outcomes of the plain Prov-GigaPath slide encoder: runs the REFERENCE's LongNetViT.forward (imported read-only from
/root/reference through ref_shims, as make_golden.py does) on seeded synthetic weights / inputs, in fp64 and in fp32.

Run in the build container only:   python tests/golden/make_golden_slide_encoder.py
Writes slide_encoder_L<L>.npz -- per (global_pool, all_layer_embed) the outcomes [K, N, 768] (K = 1, or depth + 1 with all_layer_embed) in
fp64 and fp32, the first rows of the `return_feats` state per all_layer_embed, and the config / seeds that regenerate weights and inputs
through modaltune_amd/synth.py -- and slide_encoder_state_keys.json, the reference module's state-dict keys and shapes.  Nothing from
the reference is copied; weights and inputs are not stored.  The LayerNorm affines are synth's random ones: with default-initialised
LayerNorms a missing encoder.layer_norm moves the cls outcome by ~1e-6 only.
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

from models.prov_gigapath.gigapath.slide_encoder import LongNetViT  # noqa: E402  (reference)

from modaltune_amd import synth  # noqa: E402
from modaltune_amd.config import ModelConfig  # noqa: E402

DEPTH, NGRIDS, IN_CHANS, FEAT_ROWS = 3, 128, 1536, 8
# (L, weight seed, input seed of every bag of the batch)
CASES = ((37, 61, (71, 72)), (513, 62, (73,)), (1500, 63, (74,)))


def tt(a, dtype):
    return torch.from_numpy(np.asarray(a)).to(dtype)


def backbone_state(seed):
    cfg = ModelConfig(depth=DEPTH, interaction_indexes=tuple((i, i) for i in range(DEPTH)), slide_ngrids=NGRIDS, in_chans=IN_CHANS)
    return {k: synth.synth_tensor(k, sh, kind, seed) for k, sh, kind, train in synth.param_specs(cfg, synth.toy_group_sizes(6)) if not train}


def build(seed, dt):
    m = LongNetViT(in_chans=IN_CHANS, embed_dim=768, depth=DEPTH, slide_ngrids=NGRIDS, mlp_ratio=4, dropout=0.25, drop_path_rate=0.1,
                   norm_layer=lambda d: torch.nn.LayerNorm(d, eps=1e-6), return_feats=True)      # (gigapath_slide_enc12l768d's norm, at depth 3)
    m.load_state_dict({k: tt(v, torch.float32) for k, v in backbone_state(seed).items()}, strict=True)
    m = m.to(dt)
    ref_shims.zero_dropout(m)
    return m.eval()


def run_case(L, wseed, iseeds):
    out = {"L": L, "depth": DEPTH, "ngrids": NGRIDS, "in_chans": IN_CHANS, "wseed": wseed, "iseeds": np.array(iseeds)}
    bags = [synth.synth_inputs(L, [], s, grid=NGRIDS, in_chans=IN_CHANS) for s in iseeds]
    x = np.concatenate([b["x"] for b in bags], 0)
    coords = np.concatenate([b["coords"] for b in bags], 0)
    for dt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        m = build(wseed, dt)
        for gp in (0, 1):
            m.global_pool = bool(gp)
            for al in (0, 1):
                with torch.no_grad():
                    outs, feats = m(tt(x, dt), tt(coords, dt), all_layer_embed=bool(al))
                assert len(outs) == (DEPTH + 1 if al else 1)
                out[f"{tag}/gp{gp}_al{al}"] = torch.stack(outs, 0).numpy()
                if gp == 0:
                    out[f"{tag}/feats_al{al}"] = feats[:, :FEAT_ROWS].numpy()
    return out, m


if __name__ == "__main__":
    torch.manual_seed(0)
    keys = None
    for L, wseed, iseeds in CASES:
        out, m = run_case(L, wseed, iseeds)
        path = os.path.join(HERE, f"slide_encoder_L{L}.npz")
        np.savez_compressed(path, **out)
        print(L, os.path.getsize(path), "bytes", flush=True)
        keys = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    with open(os.path.join(HERE, "slide_encoder_state_keys.json"), "w") as f:
        json.dump({"depth": DEPTH, "in_chans": IN_CHANS, "keys": keys}, f, indent=1)
        f.write("\n")
