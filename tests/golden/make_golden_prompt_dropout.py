"""Golden vectors of the prompt self-attention layer in train() with prompt_dropout > 0: runs the REFERENCE's
SelfAttentionLayer(normalize_before=True, with_cffn=True) (imported read-only through ref_shims) in float64 with
torch.nn.functional.dropout replaced by a function that draws a seeded Bernoulli keep mask, RECORDS it and returns x * mask / (1 - p).
What the fixture pins is where the two masks enter the layer and how they are scaled (nn.MultiheadAttention's dropout on the softmax
probabilities [B * heads, T, T]; nn.Dropout on output_proj's result [B, T, d_model]) -- neither depends on the width, so the layers are
narrow (d_model 32) and the file stays small.

Run in the build container only:   python tests/golden/make_golden_prompt_dropout.py
Writes unit_prompt_sa_dropout.npz: per case <c>/sd/<key> (float32 values, used as float64), <c>/x, <c>/query_pos, <c>/dy, <c>/mask1
[B * heads, T, T] and <c>/mask2 [B, T, d_model] (uint8), <c>/y, <c>/dx, <c>/grad/<key> (float64), <c>/meta = (heads, p).
Nothing from the reference is copied."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_shims  # noqa: E402

ref_shims.install()
from models.vitadapter.adapter_modules import SelfAttentionLayer  # noqa: E402

# name -> (seed, d_model, cffn_ratio, heads, p, B, T): 4 heads x 16 and 2 heads x 64
CASES = {"h4x16": (71, 32, 2.0, 4, 0.1, 3, 5),
         "h2x64": (72, 32, 4.0, 2, 0.5, 2, 7)}


def run_case(seed, d_model, ratio, heads, p, B, T):
    torch.manual_seed(seed)
    layer = SelfAttentionLayer(d_model=d_model, nheads=heads, dropout=p, normalize_before=True, with_cffn=True, cffn_ratio=ratio)
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
    E = int(d_model * ratio)
    assert E // heads in (16, 64)
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


if __name__ == "__main__":
    blob = {}
    for name, spec in CASES.items():
        for k, v in run_case(*spec).items():
            blob[f"{name}/{k}"] = v
    path = os.path.join(HERE, "unit_prompt_sa_dropout.npz")
    np.savez_compressed(path, **blob)
    print(os.path.basename(path), os.path.getsize(path), "bytes")
