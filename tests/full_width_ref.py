"""Helper (not a test module): float64 torch restatements of the reference's adapter layers at the full width E = 768, where
nn.MultiheadAttention(768, heads, kdim=768, vdim=768) keeps ONE packed in_proj_weight [3E, E] (rows [0, E) q, [E, 2E) k, [2E, 3E) v).

with_cffn=False (adapter_modules.py:24-94,139-234,296-335) -- no q_proj / output_proj, no Extractor FFN / DropPath:

    Injector      y = x + gamma * (x + MHA(q = LN(x), k = v = LN_kq(c) + pe))
    Extractor     y = c + (c + MHA(q = LN(c) + pe, k = v = LN_kq(x)))                          = 2 c + out_proj(attn)
    prompt layer  t = LN(c);  y = c + keep2 / (1 - p) * MHA(q = k = t + pe, v = t; P~ = P * keep1 / (1 - p))

`sd` maps the layer's state_dict keys behind `prefix`; the two dropout keep masks of the prompt layer are ARGUMENTS (None = all ones),
as in tests/prompt_dropout_ref.py.  Plain autograd gives the backward.

Whole models: `oracle_state` turns a reference-shaped state dict with the packed matrix into the key names the unchanged oracle
(oracle/modaltune_oracle.py) reads -- the packed matrix split into q / k / v_proj_weight views and, with_cffn=False, the modules that
form lacks filled with constants that make them exact no-ops in floating point (q_proj = output_proj = identity with bias 0: x * 1 +
0 * ... is x; the Extractor FFN's linear2 = 0: c1 + 0 is c1).  Gradients flow to the packed leaves through the views."""
import math

import torch
import torch.nn.functional as F

from prompt_dropout_ref import attention_core

LN_EPS = 1e-5


def _ln(x, sd, p):
    return F.layer_norm(x, (x.shape[-1],), sd[p + ".weight"], sd[p + ".bias"], LN_EPS)


def packed_mha(q_in, k_in, v_in, sd, prefix, heads, keep1=None, p=0.0):
    """nn.MultiheadAttention with the packed in_proj_weight: -> (out_proj(attn) [B, Lq, E], P [B, heads, Lq, Lk] pre-dropout)."""
    W, b = sd[prefix + ".in_proj_weight"], sd[prefix + ".in_proj_bias"]
    E = W.shape[1]
    assert tuple(W.shape) == (3 * E, E)
    q = F.linear(q_in, W[:E], b[:E])
    k = F.linear(k_in, W[E:2 * E], b[E:2 * E])
    v = F.linear(v_in, W[2 * E:], b[2 * E:])
    B, Lq, Lk, hd = q.shape[0], q.shape[1], k.shape[1], E // heads
    if Lq == Lk:
        a, P = attention_core(q, k, v, heads, keep1, p)
    else:
        assert keep1 is None
        sp = lambda t, n: t.view(B, n, heads, hd).transpose(1, 2)
        P = torch.softmax(sp(q, Lq) @ sp(k, Lk).transpose(-1, -2) / math.sqrt(hd), dim=-1)
        a = (P @ sp(v, Lk)).transpose(1, 2).reshape(B, Lq, E)
    return F.linear(a, sd[prefix + ".out_proj.weight"], sd[prefix + ".out_proj.bias"]), P


def injector_nocffn(x, c, pe, sd, prefix, heads):
    """x [B, L, D] patch rows, c [B, T, D] tokens, pe [T, D] -> y [B, L, D]."""
    mem = _ln(c, sd, prefix + ".attn.norm_kq") + pe
    a, _ = packed_mha(_ln(x, sd, prefix + ".attn.norm"), mem, mem, sd, prefix + ".attn.multihead_attn", heads)
    return x + sd[prefix + ".gamma"] * (x + a)


def extractor_nocffn(c, x, pe, sd, prefix, heads):
    """c [B, T, D], x [B, L, D], pe [T, D] -> y [B, T, D]."""
    mem = _ln(x, sd, prefix + ".attn.norm_kq")
    a, _ = packed_mha(_ln(c, sd, prefix + ".attn.norm") + pe, mem, mem, sd, prefix + ".attn.multihead_attn", heads)
    return c + (c + a)


def prompt_self_attention_nocffn_masked(c, pe, sd, prefix, heads, keep1=None, keep2=None, p=0.0):
    """c [B, T, D], pe [T, D] -> y [B, T, D]; keep1 [B, heads, T, T] / keep2 [B, T, D] (0 / 1) or None."""
    t = _ln(c, sd, prefix + ".norm")
    k_in = t + pe
    o, _ = packed_mha(k_in, k_in, t, sd, prefix + ".self_attn", heads, keep1, p)
    if keep2 is not None:
        o = o * keep2.to(o.dtype).view(o.shape) / (1.0 - p)
    return c + o


def _attention_prefixes(cfg):
    n = len(cfg.interaction_indexes)
    cross = []
    for i in range(n):
        cross += [f"interactions.{i}.injector.attn", f"interactions.{i}.extractor.attn"]
        if i == n - 1 and cfg.use_extra_extractor:
            cross += [f"interactions.{i}.extra_extractors.{j}.attn" for j in range(2)]
    prompt = [f"prompt_selfattention.{i}" for i in range(1, n if cfg.use_prompt_sa else 1)]
    return cross, prompt


def oracle_state(sd, cfg):
    """A reference-shaped state dict of a full-width configuration under the key names oracle.modaltune_oracle reads (see the module
    docstring).  Values are views of `sd`'s tensors (autograd reaches the packed leaves) or constants."""
    assert cfg.packed_in_proj
    E, D = cfg.adapter_dim, cfg.embed_dim
    out = dict(sd)
    cross, prompt = _attention_prefixes(cfg)
    some = next(iter(sd.values()))
    eye, zD = torch.eye(D, dtype=some.dtype), torch.zeros(D, dtype=some.dtype)
    for lay, mha in [(p, p + ".multihead_attn") for p in cross] + [(p, p + ".self_attn") for p in prompt]:
        W = out[mha + ".in_proj_weight"]          # (stays: the packed restatements above read it)
        out[mha + ".q_proj_weight"], out[mha + ".k_proj_weight"], out[mha + ".v_proj_weight"] = W[:E], W[E:2 * E], W[2 * E:]
        if not cfg.extractor_ffn:
            out[lay + ".q_proj.weight"], out[lay + ".q_proj.bias"] = eye, zD
            out[lay + ".output_proj.weight"], out[lay + ".output_proj.bias"] = eye, zD
    if not cfg.extractor_ffn:
        for p in cross:
            if ".injector." in p:
                continue
            f = p[:-len(".attn")] + ".ffn"
            out[f + ".norm.weight"], out[f + ".norm.bias"] = torch.ones(D, dtype=some.dtype), zD
            out[f + ".linear1.weight"], out[f + ".linear1.bias"] = eye, zD
            out[f + ".linear2.weight"], out[f + ".linear2.bias"] = torch.zeros(D, D, dtype=some.dtype), zD
    return out


def train_step_loss_and_grads(sd, cfg, trainable, x, coords, genes, text, psd, seg_lengths, clinical=None):
    """oracle.train_step_loss_and_grads over a reference-shaped full-width state dict: the leaves are `sd`'s own keys."""
    from oracle import modaltune_oracle as O
    tr = set(trainable)
    leaves = {k: (v.clone().requires_grad_(True) if k in tr else v) for k, v in sd.items()}
    logits = O.multitask_logits(oracle_state(leaves, cfg), cfg, x, coords, genes, seg_lengths, clinical=clinical)
    loss = O.distill_loss(logits, O.projector_forward(text, psd))
    loss.backward()
    return logits.detach(), loss.detach(), {k: leaves[k].grad for k in trainable}
