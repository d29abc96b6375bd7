"""CPU: prompt_dropout in the prompt self-attention (train mode) -- the arithmetic, the mask index and the ABI surface.

* tests/prompt_dropout_ref.py (float64, masks as arguments) reproduces the REFERENCE's SelfAttentionLayer in train() under the masks the
  reference itself drew (tests/golden/unit_prompt_sa_dropout.npz, written by make_golden_prompt_dropout.py): y, dx and every parameter
  gradient to 1e-12, test_oracle_golden's bar; with all-ones masks and p = 0 it IS oracle.prompt_self_attention.
* ModelConfig.validate refuses a prompt_dropout outside [0, 1).
* mt_token_mha_fwd_drop / mt_token_mha_bwd_drop exist in the header, the library and _lib.SIGNATURES and refuse null arguments.
* The mask index: element (b, h, i, j) <-> linear index ((b heads + h) T + i) T + j is the [B * heads, T, T] layout torch's dropout call
  sees, and the flat row the GPU tests export the device's mask through covers it, padding included."""
import os
import re

import numpy as np
import pytest
import torch

import prompt_dropout_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _case(golden_dir, name):
    g = np.load(os.path.join(golden_dir, "unit_prompt_sa_dropout.npz"))
    pre = name + "/"
    d = {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}
    heads, p = int(d["meta"][0]), float(d["meta"][1])
    sd = {"l." + k[3:]: torch.from_numpy(v.astype(np.float64)) for k, v in d.items() if k.startswith("sd/")}
    return d, sd, heads, p


def _maxrel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


@pytest.mark.parametrize("name", ["h4x16", "h2x64"])
def test_restatement_matches_the_reference_under_its_own_masks(golden_dir, name):
    d, sd, heads, p = _case(golden_dir, name)
    B, T, D = d["x"].shape
    assert d["mask1"].shape == (B * heads, T, T) and d["mask2"].shape == (B, T, D)
    assert 0 < d["mask1"].mean() < 1 and 0 < d["mask2"].mean() < 1          # both masks drop something and keep something
    sd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    x = torch.from_numpy(d["x"]).requires_grad_(True)
    y = R.prompt_self_attention_masked(x, torch.from_numpy(d["query_pos"]), sd, "l", heads,
                                       torch.from_numpy(d["mask1"]).view(B, heads, T, T), torch.from_numpy(d["mask2"]), p)
    y.backward(torch.from_numpy(d["dy"]))
    assert _maxrel(y.detach().numpy(), d["y"]) < 1e-12
    assert _maxrel(x.grad.numpy(), d["dx"]) < 1e-12
    grads = [k for k in d if k.startswith("grad/")]
    assert len(grads) == 12          # norm, q_proj, output_proj (w, b each); q / k / v weights, in_proj_bias, out_proj (w, b)
    for k in grads:
        assert _maxrel(sd["l." + k[5:]].grad.numpy(), d[k]) < 1e-12, k


@pytest.mark.parametrize("name", ["h4x16", "h2x64"])
def test_restatement_without_masks_is_the_oracles_layer(golden_dir, name):
    from oracle import modaltune_oracle as O
    d, sd, heads, _ = _case(golden_dir, name)
    B, T, D = d["x"].shape
    x, pe = torch.from_numpy(d["x"]), torch.from_numpy(d["query_pos"])
    want = O.prompt_self_attention(x, pe, sd, "l", heads)
    ones1, ones2 = torch.ones(B, heads, T, T, dtype=torch.uint8), torch.ones(B, T, D, dtype=torch.uint8)
    assert _maxrel(R.prompt_self_attention_masked(x, pe, sd, "l", heads, ones1, ones2, 0.0).numpy(), want.numpy()) < 1e-12
    assert _maxrel(R.prompt_self_attention_masked(x, pe, sd, "l", heads).numpy(), want.numpy()) < 1e-12
    # ... and the masks matter: the reference's own differ from it
    y = R.prompt_self_attention_masked(x, pe, sd, "l", heads, torch.from_numpy(d["mask1"]).view(B, heads, T, T), torch.from_numpy(d["mask2"]),
                                       float(d["meta"][1]))
    assert _maxrel(y.numpy(), want.numpy()) > 1e-3


def test_config_refuses_a_prompt_dropout_outside_the_unit_interval():
    from modaltune_amd.config import ModelConfig
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="prompt_dropout"):
            ModelConfig(prompt_dropout=bad).validate()
    for ok in (0.0, 0.5):
        ModelConfig(prompt_dropout=ok).validate()
    ModelConfig(prompt_dropout=0.5, use_prompt_sa=False).validate()          # accepted, no effect: as in the reference


def test_header_declares_the_drop_entries():
    text = open(os.path.join(ROOT, "include", "modaltune_hip.h")).read()
    fwd = re.search(r"int mt_token_mha_fwd_drop\(([^;]*)\);", text)
    bwd = re.search(r"int mt_token_mha_bwd_drop\(([^;]*)\);", text)
    assert fwd and bwd
    for m, plain in ((fwd, "mt_token_mha_fwd"), (bwd, "mt_token_mha_bwd")):
        args = " ".join(m.group(1).split())
        base = " ".join(re.search(r"int %s\(([^;]*)\);" % plain, text).group(1).split())
        # the plain entry's argument list with `const MtDropout* drop` in front of the stream
        assert args == base.replace(", mt_stream_t stream", ", const MtDropout* drop, mt_stream_t stream"), (args, base)


def test_library_exports_the_drop_entries_and_they_refuse_null_arguments():
    import __graft_entry__ as ge
    ge.build()
    from modaltune_amd import _lib
    lib = _lib.load()
    assert lib.mt_version() >= 310
    for name, plain in (("mt_token_mha_fwd_drop", "mt_token_mha_fwd"), ("mt_token_mha_bwd_drop", "mt_token_mha_bwd")):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        sig = _lib.SIGNATURES[name]
        assert sig == _lib.SIGNATURES[plain][:-1] + [_lib.DR, _lib.P]
        args = [0 if t is _lib.I else None for t in sig]
        assert getattr(lib, name)(*args) == -1          # MT_ERR_BAD_ARG, before any HIP call (no device here)


@pytest.mark.parametrize("B,heads,T", [(3, 12, 65), (3, 6, 7), (1, 1, 5)])
def test_mask_linear_index_is_torchs_dropout_layout_and_the_flat_row_covers_it(B, heads, T):
    idx = R.mask_linear_index(B, heads, T)
    n = B * heads * T * T
    # torch's call sees attn_output_weights as [B * heads, T, T] (batch-major heads): its C-order element number is the linear index
    seen = np.arange(n, dtype=np.int64).reshape(B * heads, T, T)
    assert np.array_equal(idx.reshape(B * heads, T, T), seen)
    b, h, i, j = B - 1, heads - 1, T - 1, T // 2
    assert idx[b, h, i, j] == ((b * heads + h) * T + i) * T + j
    # the export: one row of flat_row_len(n) ones through the element dropout (index m * D + d = d for the single row); gathering it at
    # `idx` returns every element of the mask exactly once, the padding (n = 882 and 25 are no multiples of 4) is never addressed
    D = R.flat_row_len(n)
    assert D % 4 == 0 and 0 <= D - n < 4 and (T == 65 or (n % 4 != 0 and D > n))
    row = np.arange(D)
    assert np.array_equal(np.sort(row[idx].ravel()), np.arange(n)) and idx.max() == n - 1 < D
