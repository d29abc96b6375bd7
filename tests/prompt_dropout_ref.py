"""Helper (not a test module): a float64 torch restatement of the reference's prompt self-attention layer in train() with the two
dropout keep masks as ARGUMENTS -- SelfAttentionLayer.forward_pre (adapter_modules.py:81-94) with normalize_before=True,
with_cffn=True:

    t = LN(c);  k_in = t + pe;  q = in_q(q_proj(k_in));  k = in_k(k_in);  v = in_v(t)
    P = softmax(q k^T / sqrt(hd)) per head;  P~ = P * keep1 / (1 - p)              nn.MultiheadAttention(dropout=p), [B, heads, T, T]
    y = c + keep2 / (1 - p) * output_proj(out_proj(P~ v))                          nn.Dropout(p), [B, T, d_model]

`sd` maps the layer's state_dict keys behind `prefix` ("<prefix>.norm.weight", "<prefix>.self_attn.q_proj_weight", ...), as
oracle.modaltune_oracle.prompt_self_attention reads them; keep1 / keep2 None = all ones.  Plain autograd gives the backward."""
import math

import torch
import torch.nn.functional as F

LN_EPS = 1e-5


def attention_core(q, k, v, heads, keep1=None, p=0.0):
    """q, k, v [B, T, E] -> (out [B, T, E], P [B, heads, T, T] pre-dropout); keep1 [B, heads, T, T] (0 / 1) or None."""
    B, T, E = q.shape
    hd = E // heads
    sp = lambda t: t.view(B, T, heads, hd).transpose(1, 2)
    P = torch.softmax(sp(q) @ sp(k).transpose(-1, -2) / math.sqrt(hd), dim=-1)
    Pd = P if keep1 is None else P * keep1.to(P.dtype).view(B, heads, T, T) / (1.0 - p)
    return (Pd @ sp(v)).transpose(1, 2).reshape(B, T, E), P


def prompt_self_attention_masked(c, pe, sd, prefix, heads, keep1=None, keep2=None, p=0.0):
    """c [B, T, D], pe [T, D] -> y [B, T, D]."""
    D = c.shape[-1]
    t = F.layer_norm(c, (D,), sd[prefix + ".norm.weight"], sd[prefix + ".norm.bias"], LN_EPS)
    k_in = t + pe
    E = sd[prefix + ".self_attn.q_proj_weight"].shape[0]
    b = sd[prefix + ".self_attn.in_proj_bias"]
    q = F.linear(F.linear(k_in, sd[prefix + ".q_proj.weight"], sd[prefix + ".q_proj.bias"]), sd[prefix + ".self_attn.q_proj_weight"], b[:E])
    k = F.linear(k_in, sd[prefix + ".self_attn.k_proj_weight"], b[E:2 * E])
    v = F.linear(t, sd[prefix + ".self_attn.v_proj_weight"], b[2 * E:])
    a, _ = attention_core(q, k, v, heads, keep1, p)
    o = F.linear(F.linear(a, sd[prefix + ".self_attn.out_proj.weight"], sd[prefix + ".self_attn.out_proj.bias"]),
                 sd[prefix + ".output_proj.weight"], sd[prefix + ".output_proj.bias"])
    if keep2 is not None:
        o = o * keep2.to(o.dtype).view(o.shape) / (1.0 - p)
    return c + o


def mask_linear_index(B, heads, T):
    """int64 [B, heads, T, T]: the linear index ((b heads + h) T + i) T + j of the softmax-dropout mask element (b, h, i, j) -- the element
    index the kernels feed the counter-based generator, and the position in the flat row the GPU tests export the mask through."""
    import numpy as np
    b, h, i, j = np.meshgrid(np.arange(B), np.arange(heads), np.arange(T), np.arange(T), indexing="ij")
    return ((b.astype(np.int64) * heads + h) * T + i) * T + j


def flat_row_len(n):
    """Length of the flat row of ones the device's mask is exported with (mt_dropout_f32 wants a multiple of 4)."""
    return (int(n) + 3) // 4 * 4
