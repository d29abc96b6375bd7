"""CPU: the attention-map surface that needs no GPU -- site names and token legend computed from ModelConfig alone (against the
reference's own lists, tests/golden/attn_sites.json) and evaluate.attention_to_grid on hand-built patch layouts."""
import json
import os

import numpy as np
import pytest

from modaltune_amd.config import ModelConfig, attention_sites, token_legend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SITES = json.load(open(os.path.join(ROOT, "tests", "golden", "attn_sites.json")))


@pytest.mark.parametrize("name", sorted(SITES))
def test_sites_and_token_legend_match_the_reference(name):
    ent = SITES[name]
    kw = dict(ent["config"])
    cfg = ModelConfig(depth=3, interaction_indexes=((0, 0), (1, 1), (2, 2)), multi_task=3, **kw)
    assert attention_sites(cfg) == ent["sites"]
    assert token_legend(cfg) == ent["tokens"]
    assert len(token_legend(cfg)) == cfg.num_tokens


def test_legend_of_the_single_task_model_has_no_task_token():
    cfg = ModelConfig(depth=3, interaction_indexes=((0, 0), (1, 1), (2, 2)), multi_task=1)
    assert token_legend(cfg) == [f"gene:{g}" for g in range(64)] and cfg.num_tokens == 64


def test_attention_to_grid_gaps_and_duplicates():
    from modaltune_amd.evaluate import attention_to_grid
    # 256-px patches at cells (0,0), (0,2), (1,1), (2,0); the last two patches share cell (1,1)
    coords = np.array([[0, 0], [0, 512], [256, 256], [512, 0], [300, 400]], dtype=np.float32)
    w = np.array([0.1, 0.2, 0.3, 0.15, 0.25])
    g = attention_to_grid(w, coords)
    assert g.shape == (3, 3)
    want = np.full((3, 3), np.nan)
    want[0, 0], want[0, 2], want[1, 1], want[2, 0] = 0.1, 0.2, (0.3 + 0.25) / 2, 0.15
    np.testing.assert_array_equal(np.isnan(g), np.isnan(want))
    np.testing.assert_allclose(g[~np.isnan(g)], want[~np.isnan(want)], rtol=0, atol=1e-15)
    # another tile size: the same coordinates on a 512-px grid
    g2 = attention_to_grid(w, coords, tile=512)
    assert g2.shape == (2, 2) and np.isnan(g2[1, 1]) and g2[0, 0] == pytest.approx((0.1 + 0.3 + 0.25) / 3)


def test_attention_to_grid_of_a_concatenated_case():
    """A case of two slides (the reference's dataset puts the second slide at max(coords[:, 1]) + 1500 px, data_utils/datasets.py:
    237-238): both appear on one grid with the empty band between them."""
    import torch
    from modaltune_amd.evaluate import attention_to_grid
    a = np.array([[r * 256, c * 256] for r in range(2) for c in range(3)], dtype=np.float32)      # 2 x 3 patches
    off = a[:, 1].max() + 1500
    b = a[:4] + np.array([0, off], dtype=np.float32)                                               # 4 patches of slide 2
    coords = np.concatenate([a, b])
    w = torch.arange(10, dtype=torch.float32) / 45.0
    g = attention_to_grid(w, torch.from_numpy(coords))
    c0 = int(np.floor(off / 256))
    assert g.shape == (2, c0 + 3)
    np.testing.assert_allclose(g[:, :3].reshape(-1), np.arange(6) / 45.0, rtol=1e-6)
    assert np.isnan(g[:, 3:c0]).all()
    np.testing.assert_allclose([g[0, c0], g[0, c0 + 1], g[0, c0 + 2], g[1, c0]], np.arange(6, 10) / 45.0, rtol=1e-6)
    assert np.isnan(g[1, c0 + 1:]).all()


def test_attention_to_grid_rejects_mismatched_lengths():
    from modaltune_amd.evaluate import attention_to_grid
    with pytest.raises(ValueError, match="weights"):
        attention_to_grid(np.ones(3), np.zeros((4, 2)))
