"""TEST INFRASTRUCTURE: the plain Prov-GigaPath slide-encoder forward (LongNetViT.forward, gigapath/slide_encoder.py:213-290) restated
from the oracle's pinned pieces -- pos_embed_rows, encoder_layer, _ln -- plus the weights / inputs of the slide_encoder_L*.npz fixtures
(tests/golden/make_golden_slide_encoder.py).  tests/test_slide_encoder_cpu.py holds it to those fixtures at 1e-9; the GPU tests use it
for bags the fixtures do not cover (L = 1, 2)."""
import numpy as np
import torch

from modaltune_amd import synth
from modaltune_amd.config import DILATED_RATIOS, ModelConfig, segment_lengths
from oracle import modaltune_oracle as O

NORM_EPS = 1e-6      # gigapath_slide_enc12l768d builds `norm` with eps 1e-6 (SE:368-377); encoder.layer_norm keeps the encoder's 1e-5


def backbone_cfg(depth=3, ngrids=128, in_chans=1536, **kw) -> ModelConfig:
    return ModelConfig(depth=depth, interaction_indexes=tuple((i, i) for i in range(depth)), slide_ngrids=ngrids, in_chans=in_chans, **kw)


def backbone_state(seed, depth=3, ngrids=128, in_chans=1536):
    """The frozen (= LongNetViT) tensors of synth's state dict: name -> fp32 numpy."""
    cfg = backbone_cfg(depth, ngrids, in_chans)
    return {k: synth.synth_tensor(k, sh, kind, seed) for k, sh, kind, train in synth.param_specs(cfg, synth.toy_group_sizes(6)) if not train}


def bags(L, iseeds, ngrids=128, in_chans=1536):
    """(x [N, L, C], coords [N, L, 2]) fp32 numpy: one synth bag per input seed."""
    b = [synth.synth_inputs(L, [], int(s), grid=ngrids, in_chans=in_chans) for s in iseeds]
    return np.concatenate([q["x"] for q in b], 0), np.concatenate([q["coords"] for q in b], 0)


def forward(sd, x, coords, depth, global_pool=False, all_layer_embed=False, ngrids=128, seg_lengths=None):
    """sd: name -> tensor (any float dtype); x [N, L, C], coords [N, L, 2] -> (outcomes: list of [N, 768], last state [N, L + 1, 768])."""
    seg = seg_lengths or segment_lengths()
    h = torch.nn.functional.linear(x, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"])                  # SE:227
    h = h + O.pos_embed_rows(coords, h.shape[-1], ngrids, h.dtype)                                                # SE:230-232
    h = torch.cat((sd["cls_token"].expand(h.shape[0], -1, -1), h), dim=1)                                         # SE:235-240 (pos_embed[0] = 0)
    states = [h] if all_layer_embed else []                                                                       # ENC:400-403
    for l in range(depth):
        h = O.encoder_layer(h, sd, f"encoder.layers.{l}", seg, DILATED_RATIOS)
        if all_layer_embed:
            states.append(h)                                                                                      # ENC:420-422
    if not all_layer_embed:
        states = [O._ln(h, sd, "encoder.layer_norm")]                                                             # ENC:425-426
    outs = []
    for s in states:                                                                                              # SE:277-285
        outs.append(O._ln(s[:, 1:].mean(dim=1), sd, "norm", NORM_EPS) if global_pool else O._ln(s, sd, "norm", NORM_EPS)[:, 0])
    return outs, states[-1]
