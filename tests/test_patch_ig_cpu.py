"""CPU: the yardstick of the patch Integrated-Gradients tests -- the midpoint rule through the float64 oracle with torch.autograd over
the patch FEATURES x [L, in_chans] -- the identity that lets the HIP path work in the embedding space, and the host-side pieces.

`_oracle_patch_ig` is what tests/test_patch_ig_gpu.py compares the HIP path with (same quadrature, same target, zero baselines).  The
rule's own error is pinned here: on fixture model_L37_d3, target ones(256) / 16, zero baseline bag, the completeness gap
|sum attr - dF| / |dF| for tasks 0 / 1 / 2 is 1.4e-3 / 3.6e-3 / 4.0e-3 at m = 16 and 2.5e-3 / 1.3e-3 / 1.5e-3 at m = 32; |attr| per patch
lies between 7e-4 and 1e-1, so no patch sits at zero and a relative L2 over the patches weighs all of them.

The identity: the patch embedding is affine, x0_l = W x_l + b + pos_l, and F depends on x only through x0, so
sum_c (x - base)_{l,c} dF/dx_{l,c} = <W (x - base)_l, dF/dx0_l> = <e_x,l - e_base,l, dF/dx0_l> at every point of the path.

F is piecewise smooth (the Extractors' FFN has a ReLU): `_f_and_grads(relu_sides=...)` is the oracle's derivative with the side of a
kink that float64 alone can tell from zero taken from the forward under test (KINK_TAU), for the one-point check on the GPU."""
import functools
import types

import numpy as np
import pytest
import torch

from modaltune_amd.config import segment_lengths
from oracle import modaltune_oracle as O
from test_ig_cpu import TARGET, _case

F64 = torch.float64


KINK_TAU = 2.0 ** -11      # half an ulp of fp16, relative: what a pre-activation fed by fp16 patch-row operands can be off by


def _extractor_with_sides(sides, found):
    """oracle.extractor with the side of the FFN's ReLU kink chosen by `sides` where the oracle cannot tell it.  F is piecewise smooth:
    the Extractor's FFN is linear2(relu(linear1(.))), and a unit whose pre-activation is zero within the accuracy of ANY forward that
    rounds the patch-row operands to fp16 (|pre| <= KINK_TAU * mean |pre| of its row) has two one-sided derivatives, both valid; which
    one a forward takes is decided by its rounding.  sides: {prefix: bool [T, E], True = the unit is on} -- taken from the forward whose
    gradient is being checked; used ONLY for those units, every other unit keeps the oracle's own sign.  found: list that receives
    (prefix, row, unit, pre, side) of every such unit."""
    def extractor(c, x, pe, sd, prefix, heads):
        attn = O.cross_attention_pre(c, x, sd, prefix + ".attn", heads, pos=None, query_pos=pe, patch_kv=True)
        c1 = c + attn
        h = O._linear(O._ln(c1, sd, prefix + ".ffn.norm"), sd, prefix + ".ffn.linear1")
        hd = h.detach()
        on = hd > 0
        near = hd.abs() <= KINK_TAU * hd.abs().mean(-1, keepdim=True)
        if bool(near.any()):
            side = torch.as_tensor(np.asarray(sides[prefix])).reshape(on.shape)
            for idx in near.nonzero().tolist():
                found.append((prefix, idx[-2], idx[-1], float(hd[tuple(idx)]), bool(side[tuple(idx)])))
            on = torch.where(near, side, on)
        return c1 + O._linear(h * on.to(h.dtype), sd, prefix + ".ffn.linear2")
    return extractor


def _f_and_grads(name, task, target, x, genes, need_grad=True, sd=None, relu_sides=None, found=None):
    """F = <target, logits_task> of the oracle at the patch features x [L, C] and the gene tensors `genes`; dF/dx [L, C] and dF/dgenes
    (flat) as numpy.  relu_sides / found: see _extractor_with_sides (None: the oracle as it is)."""
    if relu_sides is not None:
        keep, O.extractor = O.extractor, _extractor_with_sides(relu_sides, found if found is not None else [])
        try:
            return _f_and_grads(name, task, target, x, genes, need_grad=need_grad, sd=sd)
        finally:
            O.extractor = keep
    cfg, sizes, sd0, _, coords, _, clin, _ = _case(name)
    xs = x.clone().requires_grad_(need_grad)
    gs = [g.clone().requires_grad_(need_grad) for g in genes]
    tok = torch.eye(cfg.multi_task, dtype=F64)[task]
    logits = O.model_forward(sd0 if sd is None else sd, cfg, xs, coords, gs, tok, segment_lengths(), clinical=clin)
    f = (logits.reshape(-1) * torch.as_tensor(target, dtype=F64)).sum()
    if not need_grad:
        return float(f), None, None
    grads = torch.autograd.grad(f, [xs] + gs)
    return float(f.detach()), grads[0].reshape(-1, x.shape[-1]).numpy(), torch.cat([d.reshape(-1) for d in grads[1:]]).numpy()


@functools.lru_cache(maxsize=16)
def _cached(name, task, target_bytes, m, joint):
    target = np.frombuffer(target_bytes, dtype=np.float64).copy()
    cfg, sizes, sd, x, coords, genes, clin, _ = _case(name)
    xb = torch.zeros_like(x)
    gb = [torch.zeros_like(g) for g in genes] if joint else genes          # (not joint: the genes stay at their values)
    accx, accg = np.zeros(tuple(x.reshape(-1, x.shape[-1]).shape)), np.zeros(sum(sizes))
    for k in range(m):
        a = (k + 0.5) / m
        _, dx, dg = _f_and_grads(name, task, target, xb + a * (x - xb), [b + a * (g - b) for g, b in zip(genes, gb)])
        accx += dx / m
        accg += dg / m
    patches = ((x - xb).reshape(accx.shape).numpy() * accx).sum(1)
    gattr = torch.cat([(g - b).reshape(-1) for g, b in zip(genes, gb)]).numpy() * accg
    f_in = _f_and_grads(name, task, target, x, genes, need_grad=False)[0]
    f_base = _f_and_grads(name, task, target, xb, gb, need_grad=False)[0]
    delta = f_in - f_base
    return {"patches": patches, "patches_total": patches.sum(), "attributions": gattr, "f_input": f_in, "f_baseline": f_base,
            "delta": delta, "gap": abs(patches.sum() + gattr.sum() - delta) / abs(delta)}


def _oracle_patch_ig(name, task, target, m):
    """Integrated Gradients of F_task = <target, logits_task> over the patch features of fixture `name` from a zero baseline bag, the
    genes at their values: midpoint rule with m points, torch.autograd through the float64 oracle; `patches` [L] is the attribution
    summed over the input channels.  Results are cached per (name, task, target, m): read-only."""
    return _cached(name, int(task), np.asarray(target, dtype=np.float64).tobytes(), int(m), False)


def _oracle_joint_ig(name, task, target, m):
    """The same along ONE straight path through both modalities (zero bag and zero genes -> the slide): `patches` [L] and the gene
    `attributions`; `gap` is the completeness gap of their joint sum."""
    return _cached(name, int(task), np.asarray(target, dtype=np.float64).tobytes(), int(m), True)


@pytest.mark.parametrize("m", [16, 32])
@pytest.mark.parametrize("task", [0, 1, 2])
def test_oracle_patch_midpoint_rule_is_complete_to_one_percent(task, m):
    r = _oracle_patch_ig("L37_d3", task, TARGET, m)
    mag = np.abs(r["patches"])
    print(f"task {task}, m = {m}: completeness gap {r['gap']:.2e} (delta {r['delta']:.4e}); |attr| per patch {mag.min():.1e} .. {mag.max():.1e}")
    assert r["gap"] < 1e-2, r["gap"]
    assert r["patches"].shape == (37,) and np.isfinite(r["patches"]).all()
    assert not np.any(r["attributions"])                       # the genes did not move
    assert mag.min() > 1e-4 and mag.max() < 1.0                # no patch sits at zero


@pytest.mark.parametrize("task", [0, 1, 2])
def test_embedding_space_identity(task):
    """sum_c (x - base)_c dF/dx_c per patch, against <e_x - e_base, dF/dx0> with dF/dx0 taken from a model whose patch embedding is the
    identity on the first 768 channels and whose input carries W x + b there -- the same function of x0, so its input gradient IS
    dF/dx0 -- at the midpoint of the path."""
    cfg, sizes, sd, x, coords, genes, clin, _ = _case("L37_d3")
    D, C = cfg.embed_dim, x.shape[-1]
    W, b = sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"]
    x2, xb = x.reshape(-1, C), torch.zeros_like(x.reshape(-1, C))
    xa = xb + 0.5 * (x2 - xb)
    _, dx, _ = _f_and_grads("L37_d3", task, TARGET, xa.reshape(x.shape), genes)
    direct = ((x2 - xb).numpy() * dx).sum(1)
    sd_id = dict(sd)
    sd_id["patch_embed.proj.weight"] = torch.cat([torch.eye(D, dtype=F64), torch.zeros(D, C - D, dtype=F64)], dim=1)
    sd_id["patch_embed.proj.bias"] = torch.zeros(D, dtype=F64)
    embed = lambda t: t @ W.T + b
    ea = torch.cat([embed(xa), torch.zeros(xa.shape[0], C - D, dtype=F64)], dim=1)
    f_id, dx0, _ = _f_and_grads("L37_d3", task, TARGET, ea.reshape(x.shape), genes, sd=sd_id)
    f, _, _ = _f_and_grads("L37_d3", task, TARGET, xa.reshape(x.shape), genes, need_grad=False)
    assert abs(f_id - f) <= 1e-12 * abs(f)                       # the same function
    via_embedding = ((embed(x2) - embed(xb)).numpy() * dx0[:, :D]).sum(1)
    err = np.abs(via_embedding - direct).max() / np.abs(direct).max()
    print(f"task {task}: embedding-space identity, largest difference / largest attribution: {err:.1e}")
    assert err <= 1e-12, err


def test_the_slides_own_point_sits_on_a_relu_kink_for_task_0():
    """Why the one-point check on the GPU resolves kinks: at the fixture's own features, task 0, unit 40 of the first Extractor's FFN has a
    pre-activation of -1.3e-6 in the task-token row (1.2e-6 of the row's mean |pre|) -- zero for every forward that is not float64 --
    and the two one-sided derivatives of the per-patch quantity differ by 2 %: twice the bar a gradient is held to.  (The task-token
    row carries 20 times the gradient of a gene-token row.)  With every unit on its own side the modified Extractor IS the oracle's."""
    cfg, sizes, sd, x, coords, genes, clin, _ = _case("L37_d3")
    C = x.shape[-1]
    T, E = 1 + 64, cfg.adapter_dim
    per_patch = lambda dx: (x.reshape(-1, C).numpy() * dx).sum(1)
    _, dx, _ = _f_and_grads("L37_d3", 0, TARGET, x, genes)
    prefixes = [f"interactions.{i}.extractor" for i in range(3)] + [f"interactions.2.extra_extractors.{j}" for j in range(2)]
    own, found = {p: np.zeros((T, E), dtype=bool) for p in prefixes}, []
    _f_and_grads("L37_d3", 0, TARGET, x, genes, need_grad=False, relu_sides=own, found=found)
    print(f"{len(found)} of {len(prefixes) * T * E} units within KINK_TAU of zero; the closest:", min(found, key=lambda f: abs(f[3])))
    for p, r, j, pre, _ in found:
        own[p][r, j] = pre > 0
    kink = ("interactions.0.extractor", 0, 40)
    assert kink in [f[:3] for f in found] and min(found, key=lambda f: abs(f[3]))[:3] == kink
    assert abs([f for f in found if f[:3] == kink][0][3]) < 1e-5
    _, dx_own, _ = _f_and_grads("L37_d3", 0, TARGET, x, genes, relu_sides=own)
    assert np.array_equal(dx_own, dx)
    other = {p: a.copy() for p, a in own.items()}
    other[kink[0]][kink[1], kink[2]] ^= True
    _, dx_other, _ = _f_and_grads("L37_d3", 0, TARGET, x, genes, relu_sides=other)
    gap = np.linalg.norm(per_patch(dx_other) - per_patch(dx)) / np.linalg.norm(per_patch(dx))
    print(f"the two one-sided derivatives at that unit, per patch, differ by {gap:.2e}")
    assert gap > 1e-2


def test_new_entry_points_are_declared_and_bound():
    from modaltune_amd import _lib, ops
    for n in ("mt_patch_points_fwd", "mt_patch_ig_accumulate"):
        assert n in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["mt_patch_points_fwd"]) == 8 and len(_lib.SIGNATURES["mt_patch_ig_accumulate"]) == 11
    assert all(hasattr(ops, n) for n in ("patch_points_fwd", "patch_ig_accumulate"))
    from modaltune_amd import engine
    assert engine.PatchPoints.__slots__ == ("x0_base", "alphas", "weights", "dpatch", "unscale")


def test_argument_errors_raise_before_the_library_is_loaded(monkeypatch):
    from modaltune_amd import _lib
    from modaltune_amd.attribution import IntegratedGradients
    from modaltune_amd.engine import Engine, PatchPoints
    from modaltune_amd.titan import TitanEngine

    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    cfg = _case("L37_d3")[0]

    def bare(cls, **attrs):      # an engine of class `cls` that was never constructed: the checks below read nothing but these attributes
        eng = object.__new__(cls)
        eng.__dict__.update(attrs)
        return eng
    fake = bare(Engine, cfg=cfg, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="inputs"):
        IntegratedGradients(fake, (0,), steps=4, inputs="pixels")
    late = bare(Engine, cfg=types.SimpleNamespace(first_interaction_layer=2), device=torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="first_interaction_layer"):
        IntegratedGradients(late, (0,), steps=4, inputs="patches")
    with pytest.raises(NotImplementedError, match="TITAN"):
        IntegratedGradients(bare(TitanEngine), inputs="patches")
    # the engine's own checks: shape, dtype, device and the modes it cannot serve
    B, L, D = 3, 5, cfg.embed_dim
    ok = lambda: PatchPoints(torch.zeros(L, D), torch.zeros(B), torch.zeros(B), torch.zeros(L), torch.ones(1))
    Engine._check_patch_points(fake, ok(), B, L, True)
    for field, bad in (("x0_base", torch.zeros(L + 1, D)), ("x0_base", torch.zeros(L, D, dtype=torch.float64)), ("alphas", torch.zeros(B + 1)),
                       ("weights", None), ("dpatch", torch.zeros(L, 1)), ("unscale", torch.ones(2)), ("x0_base", torch.zeros(D, L).t())):
        pp = ok()
        setattr(pp, field, bad)
        with pytest.raises(ValueError, match=f"patch_points.{field}"):
            Engine._check_patch_points(fake, pp, B, L, True)
    with pytest.raises(ValueError, match="need_grad"):
        Engine._check_patch_points(fake, ok(), B, L, False)
    with pytest.raises(ValueError, match="at most"):
        Engine._check_patch_points(fake, ok(), 5, L, True)
    with pytest.raises(NotImplementedError, match="first_interaction_layer"):
        Engine._check_patch_points(late, ok(), B, L, True)
    with pytest.raises(NotImplementedError, match="TITAN"):
        Engine._check_patch_points(bare(TitanEngine), ok(), B, L, True)
