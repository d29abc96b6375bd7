"""CPU: the yardstick of the Integrated-Gradients tests -- the midpoint rule through the float64 oracle with torch.autograd -- and the
host-side pieces of modaltune_amd.attribution.

`_oracle_ig` is what tests/test_ig_gpu.py compares the HIP path with (same quadrature, same target, same baseline).  The rule's own
error is pinned here: on fixture model_L37_d3 (six pathways of 5..10 genes), target ones(256) / 16, zero baseline, the completeness gap
|sum attr - dF| / |dF| at m = 32 is 6.8e-3 / 4.8e-3 / 1.1e-3 for tasks 0 / 1 / 2.  The rule does not converge monotonically on this
model (m = 64: 1.2e-2 / 1.9e-2 / 2.0e-3; m = 128: 3.7e-3 / 6.9e-3 / 2.5e-4), so the m is part of the condition."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from modaltune_amd import synth
from modaltune_amd.config import ModelConfig, segment_lengths
from oracle import modaltune_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
F64 = torch.float64


@functools.lru_cache(maxsize=4)
def _case(name):
    """(cfg, sizes, state dict, x, coords, genes, clinical) of fixture model_<name>.npz in float64."""
    g = np.load(os.path.join(GOLDEN, f"model_{name}.npz"))
    L, seed, ngrids = int(g["L"]), int(g["seed"]), int(g["ngrids"])
    sizes = [int(s) for s in g["sizes"]]
    cfg = ModelConfig(depth=int(g["depth"]), interaction_indexes=tuple(tuple(int(i) for i in p) for p in g["inter"]), slide_ngrids=ngrids,
                      clinical=bool(int(g["clinical"])) if "clinical" in g.files else False,
                      token_agg=str(g["token_agg"]) if "token_agg" in g.files else "sum",
                      multi_task=int(g["multi_task"]) if "multi_task" in g.files else 3,
                      **(json.loads(str(g["extra_cfg"])) if "extra_cfg" in g.files else {}))
    cfg.validate()
    sd = {k: torch.from_numpy(np.asarray(v)).to(F64) for k, v in synth.synth_state_dict(cfg, sizes, seed).items()}
    inp = synth.synth_inputs(L, sizes, seed, grid=ngrids)
    x, coords = torch.from_numpy(inp["x"]).to(F64), torch.from_numpy(inp["coords"]).to(F64)
    genes = [torch.from_numpy(a).to(F64) for a in inp["genes"]]
    clin = torch.from_numpy(inp["clinical"]).to(F64) if cfg.clinical else None
    return cfg, sizes, sd, x, coords, genes, clin, inp


def _oracle_f_and_grad(name, task, target, point, need_grad=True):
    """F = <target, logits_task> of the oracle at the gene tensors `point` (list of [1, n_i] float64) and dF/dgenes (flat)."""
    cfg, sizes, sd, x, coords, genes, clin, _ = _case(name)
    gs = [p.clone().requires_grad_(need_grad) for p in point]
    tok = torch.eye(cfg.multi_task, dtype=F64)[task]
    logits = O.model_forward(sd, cfg, x, coords, gs, tok, segment_lengths(), clinical=clin)
    f = (logits.reshape(-1) * torch.as_tensor(target, dtype=F64)).sum()
    if not need_grad:
        return float(f), None
    grads = torch.autograd.grad(f, gs)
    return float(f.detach()), torch.cat([d.reshape(-1) for d in grads]).numpy()


@functools.lru_cache(maxsize=16)
def _oracle_ig_cached(name, task, target_bytes, m):
    target = np.frombuffer(target_bytes, dtype=np.float64).copy()
    cfg, sizes, sd, x, coords, genes, clin, _ = _case(name)
    base = [torch.zeros_like(g) for g in genes]
    acc = np.zeros(sum(sizes))
    for k in range(m):
        a = (k + 0.5) / m
        _, d = _oracle_f_and_grad(name, task, target, [b + a * (g - b) for g, b in zip(genes, base)])
        acc += d / m
    diff = torch.cat([(g - b).reshape(-1) for g, b in zip(genes, base)]).numpy()
    attr = diff * acc
    offs = np.concatenate([[0], np.cumsum(sizes)])
    f_in, _ = _oracle_f_and_grad(name, task, target, genes, need_grad=False)
    f_base, _ = _oracle_f_and_grad(name, task, target, base, need_grad=False)
    delta = f_in - f_base
    return {"attributions": attr, "pathway": np.array([attr[offs[i]:offs[i + 1]].sum() for i in range(len(sizes))]),
            "f_input": f_in, "f_baseline": f_base, "delta": delta, "gap": abs(attr.sum() - delta) / abs(delta)}


def _oracle_ig(name, task, target, m):
    """Integrated Gradients of F_task = <target, logits_task> over the gene inputs of fixture `name` from a zero baseline: midpoint rule
    with m points, torch.autograd through the float64 oracle.  Results are cached per (name, task, target, m): read-only."""
    return _oracle_ig_cached(name, int(task), np.asarray(target, dtype=np.float64).tobytes(), int(m))


TARGET = np.ones(256) / 16


@pytest.mark.parametrize("task", [0, 1, 2])
def test_oracle_midpoint_rule_is_complete_to_one_percent_at_m32(task):
    r = _oracle_ig("L37_d3", task, TARGET, 32)
    print(f"task {task}: completeness gap at m = 32: {r['gap']:.2e} (delta {r['delta']:.4e})")
    assert r["gap"] < 1e-2, r["gap"]
    assert r["attributions"].shape == (sum(_case("L37_d3")[1]),) and np.isfinite(r["attributions"]).all()


def test_top_pathways_sorts_by_magnitude():
    from modaltune_amd.attribution import top_pathways
    res = {"pathway": torch.tensor([[0.5, -2.0, 0.0, 1.5], [1.0, 0.0, 0.0, 0.0]])}
    names = ["a", "b", "c", "d"]
    assert top_pathways(res, names, task=0, k=3) == [("b", -2.0), ("d", 1.5), ("a", 0.5)]
    assert top_pathways(res, names, task=1, k=10)[0] == ("a", 1.0) and len(top_pathways(res, names, task=1)) == 4
    with pytest.raises(ValueError):
        top_pathways(res, names[:3], task=0)


def test_new_entry_points_are_declared_and_bound():
    from modaltune_amd import _lib, ops
    for n in ("mt_gene_snn_fwd_points", "mt_gene_snn_bwd_input", "mt_ig_finalize"):
        assert n in _lib.SIGNATURES
    assert all(hasattr(ops, n) for n in ("gene_snn_fwd_points", "gene_snn_bwd_input", "ig_finalize"))
