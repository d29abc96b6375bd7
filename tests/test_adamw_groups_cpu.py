"""CPU: parameter groups of the fused AdamW on the host -- the segment table, the rule resolution of TrainStep(param_groups=...), the
optimiser dict with groups against torch's own class, the group helpers, and the C ABI of mt_adamw_step_groups (declared, exported,
bound, its argument errors).  Every comparison is exact."""
import ctypes as C
import os
import re

import pytest
import torch

from modaltune_amd import checkpoint as ck
from modaltune_amd import optim, synth
from modaltune_amd.config import ModelConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _toy():
    cfg = ModelConfig(depth=3, interaction_indexes=((0, 0), (1, 1), (2, 2)), slide_ngrids=32, dropout=0.0, drop_path_rate=0.0)
    sizes = synth.toy_group_sizes()
    specs = synth.param_specs(cfg, sizes)
    slots, n_flat = ck.slots_of(specs)
    kinds = {k: kind for k, _, kind, train in specs if train}
    return cfg, sizes, slots, n_flat, kinds


# ---------------------------------------------------------------------------------------------- the table
def test_segment_table_merges_equal_neighbours_and_keeps_padding_inside_a_segment():
    #          offset numel group
    entries = [(0, 1, 0), (4, 3, 0), (8, 4, 1), (12, 5, 1), (20, 64, 0), (84, 255, 2), (340, 256, 2), (596, 1027, 0)]
    end, grp = optim.segment_table(entries)
    assert end.dtype == torch.int32 and grp.dtype == torch.uint8
    assert end.tolist() == [8, 20, 84, 596, 1624] and grp.tolist() == [0, 1, 0, 2, 0]      # (1623 rounds up to the slot's end)
    assert all(e % 4 == 0 for e in end.tolist())
    # one group: one segment; alternating: one segment per tensor
    assert optim.segment_table([(o, n, 0) for o, n, _ in entries])[0].tolist() == [1624]
    end, grp = optim.segment_table([(o, n, i % 2) for i, (o, n, _) in enumerate(entries)])
    assert end.tolist() == [4, 8, 12, 20, 84, 340, 596, 1624] and grp.tolist() == [0, 1] * 4


def test_segment_table_asserts_the_slot_rule_and_the_group_limit():
    with pytest.raises(ValueError, match="16-byte slot"):
        optim.segment_table([(0, 3, 0), (3, 5, 1)])              # the second tensor starts inside the first one's slot
    with pytest.raises(ValueError, match="16-byte slot"):
        optim.segment_table([(0, 8, 0), (4, 4, 1)])              # overlap
    with pytest.raises(ValueError, match="16-byte slot"):
        optim.segment_table([(8, 4, 0), (0, 4, 1)])              # not in address order
    sixteen = [(4 * i, 4, i) for i in range(16)]
    end, grp = optim.segment_table(sixteen)
    assert grp.tolist() == list(range(16))
    with pytest.raises(ValueError, match="at most 16"):
        optim.segment_table(sixteen + [(64, 4, 16)])
    with pytest.raises(ValueError, match="group ids"):
        optim.segment_table([(0, 4, 0), (4, 4, 16)])             # two groups, but an id the kernel's table has no row for
    with pytest.raises(ValueError):
        optim.segment_table([])


# ---------------------------------------------------------------------------------------------- rule resolution
def test_rules_first_match_wins_unmatched_go_to_the_default_group_and_a_dead_rule_raises():
    _, _, slots, _, kinds = _toy()
    named = [(k, kinds[k]) for k in slots]
    rules = [{"match": r"^gene_encoder\.", "lr_mult": 0.1},
             {"kinds": ("b", "lnw", "lnb", "gamma", "tok"), "weight_decay": 0.0},
             {"match": r"^interactions\.0\.", "kinds": "w", "lr_mult": 0.0, "weight_decay": 0.0}]
    groups, group_of = optim.resolve_param_groups(named, rules, 0.01)
    assert [(g["lr_mult"], g["weight_decay"]) for g in groups] == [(1.0, 0.01), (0.1, 0.01), (1.0, 0.0), (0.0, 0.0)]
    assert sorted(k for g in groups for k in g["names"]) == sorted(slots) and all(g["names"] for g in groups)
    for k, kind in named:
        if k.startswith("gene_encoder."):
            want = 1                                              # first match wins: the encoder's biases too
        elif kind != "w":
            want = 2
        elif k.startswith("interactions.0."):
            want = 3
        else:
            want = 0                                              # unmatched: the default group, with the constructor's weight decay
        assert group_of[k] == want, k
        assert k in groups[want]["names"]
    # names keep the buffer's order inside a group
    order = {k: i for i, k in enumerate(slots)}
    assert all([order[k] for k in g["names"]] == sorted(order[k] for k in g["names"]) for g in groups)
    # no rules / everything matched: no default group
    assert [len(g["names"]) for g in optim.resolve_param_groups(named, None, 0.02)[0]] == [len(slots)]
    assert len(optim.resolve_param_groups(named, [{"match": "."}], 0.02)[0]) == 1
    with pytest.raises(ValueError, match="matches no trainable tensor"):
        optim.resolve_param_groups(named, rules + [{"match": r"^no_such_module\."}], 0.01)
    with pytest.raises(ValueError, match="matches no trainable tensor"):      # shadowed by an earlier rule: dead as well
        optim.resolve_param_groups(named, [{"match": "."}, {"match": r"^gene_encoder\."}], 0.01)
    with pytest.raises(ValueError, match="unknown keys"):
        optim.resolve_param_groups(named, [{"match": ".", "lr": 1e-3}], 0.01)
    with pytest.raises(ValueError, match="at most 16"):
        optim.resolve_param_groups(named, [{"match": "^" + re.escape(k) + "$", "lr_mult": 0.5} for k in list(slots)[:17]], 0.01)


# ---------------------------------------------------------------------------------------------- the optimiser dict
def _hyper():
    return {"lr": 1e-3, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.01}


def _groups(slots, kinds):
    named = [(k, kinds[k]) for k in slots]
    return optim.resolve_param_groups(named, [{"match": r"^gene_encoder\.", "lr_mult": 0.1},
                                              {"kinds": optim.NO_DECAY_KINDS, "weight_decay": 0.0}], 0.01)[0]


def test_uniform_optimizer_dict_is_unchanged():
    _, _, slots, n_flat, kinds = _toy()
    names = list(slots)
    g = torch.Generator().manual_seed(0)
    m, v = torch.randn(n_flat, generator=g), torch.rand(n_flat, generator=g)
    a, b = ck.pack_optimizer(m, v, 7, slots, names, _hyper()), ck.pack_optimizer(m, v, 7, slots, names, _hyper(), groups=None)
    assert len(a["param_groups"]) == 1 and a["param_groups"] == b["param_groups"]
    assert sorted(a["param_groups"][0]) == sorted(["lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "foreach", "capturable",
                                                   "differentiable", "fused", "decoupled_weight_decay", "params"])
    out = ck.unpack_optimizer(a, slots, names, n_flat)
    assert len(out) == 4 and out[2] == 7 and out[3] == _hyper()                   # the exact hyper of a uniform dict: no "groups"
    # several groups with EQUAL hyper-parameters are uniform too
    two = {"state": a["state"], "param_groups": [dict(a["param_groups"][0], params=list(range(5))),
                                                 dict(a["param_groups"][0], params=list(range(5, len(names))))]}
    assert ck.unpack_optimizer(two, slots, names, n_flat)[3] == _hyper()


def test_grouped_optimizer_dict_round_trips_through_torch_adamw_with_the_same_groups():
    _, _, slots, n_flat, kinds = _toy()
    names = list(slots)
    groups = _groups(slots, kinds)
    assert len(groups) == 3
    g = torch.Generator().manual_seed(1)
    m, v = torch.randn(n_flat, generator=g), torch.rand(n_flat, generator=g)
    sd = ck.pack_optimizer(m, v, 7, slots, names, _hyper(), groups=groups)
    assert [(pg["lr"], pg["weight_decay"], pg["lr_mult"]) for pg in sd["param_groups"]] == [(1e-3, 0.01, 1.0), (1e-3 * 0.1, 0.01, 0.1),
                                                                                           (1e-3, 0.0, 1.0)]
    assert all(isinstance(pg["lr"], float) for pg in sd["param_groups"])
    assert [[names[i] for i in pg["params"]] for pg in sd["param_groups"]] == [gr["names"] for gr in groups]
    # a real torch.optim.AdamW built with the same groups takes it ...
    params = {k: torch.nn.Parameter(torch.zeros(slots[k][2])) for k in names}
    opt = torch.optim.AdamW([{"params": [params[k] for k in gr["names"]]} for gr in groups], lr=5.0)
    opt.load_state_dict(sd)
    assert [(pg["lr"], pg["weight_decay"]) for pg in opt.param_groups] == [(1e-3, 0.01), (1e-3 * 0.1, 0.01), (1e-3, 0.0)]
    for k in names:
        o, n, shape = slots[k]
        s = opt.state[params[k]]
        assert float(s["step"]) == 7.0 and torch.equal(s["exp_avg"].reshape(-1), m[o:o + n]) and torch.equal(s["exp_avg_sq"].reshape(-1), v[o:o + n])
    # ... steps, and its OWN state_dict (torch has renumbered `params`; lr_mult and names came along) comes back
    for p in params.values():
        p.grad = torch.full_like(p, 0.25)
    opt.step()
    back = opt.state_dict()
    assert [i for pg in back["param_groups"] for i in pg["params"]] == list(range(len(names)))
    m2, v2, step, hyper = ck.unpack_optimizer(back, slots, names, n_flat, base_lr=1e-3)
    assert step == 8 and hyper["lr"] == 1e-3 and hyper["betas"] == (0.9, 0.999) and hyper["eps"] == 1e-8
    assert hyper["groups"] == [{"names": gr["names"], "lr_mult": gr["lr_mult"], "weight_decay": gr["weight_decay"]} for gr in groups]
    for k in names:
        o, n, _ = slots[k]
        assert torch.equal(m2[o:o + n], opt.state[params[k]]["exp_avg"].reshape(-1)), k
        assert torch.equal(v2[o:o + n], opt.state[params[k]]["exp_avg_sq"].reshape(-1)), k
    # without base_lr (a module-path dict): the first group's lr / lr_mult
    assert ck.unpack_optimizer(back, slots, names, n_flat)[3]["lr"] == 1e-3
    # a group list that leaves a tensor out or lists one twice is refused when it is written
    with pytest.raises(ValueError, match="exactly one group"):
        ck.pack_optimizer(m, v, 7, slots, names, _hyper(), groups=groups[:2])


def test_a_torch_dict_without_lr_mult_loads_a_zero_base_raises_and_differing_betas_raise():
    _, _, slots, n_flat, kinds = _toy()
    names = list(slots)
    # a plain torch optimiser over the tensors in order, split into three groups: no lr_mult, no names
    params = [torch.nn.Parameter(torch.zeros(slots[k][2])) for k in names]
    cut = (0, 10, 40, len(names))
    opt = torch.optim.AdamW([{"params": params[cut[0]:cut[1]], "lr": 2e-3}, {"params": params[cut[1]:cut[2]], "lr": 5e-4, "weight_decay": 0.0},
                             {"params": params[cut[2]:cut[3]], "lr": 0.0}], lr=1e-3, weight_decay=0.01)
    for p in params:
        p.grad = torch.full_like(p, 0.5)
    opt.step()
    sd = opt.state_dict()
    assert not any("lr_mult" in pg or "names" in pg for pg in sd["param_groups"])
    m, v, step, hyper = ck.unpack_optimizer(sd, slots, names, n_flat)
    assert step == 1 and hyper["lr"] == 2e-3                                         # the first group's lr is the base
    assert [(g["lr_mult"], g["weight_decay"]) for g in hyper["groups"]] == [(1.0, 0.01), (5e-4 / 2e-3, 0.0), (0.0, 0.01)]
    assert [g["names"] for g in hyper["groups"]] == [names[a:b] for a, b in zip(cut, cut[1:])]
    for k, p in zip(names, params):
        o, n, _ = slots[k]
        assert torch.equal(m[o:o + n], opt.state[p]["exp_avg"].reshape(-1))
    assert [g["lr_mult"] for g in ck.unpack_optimizer(sd, slots, names, n_flat, base_lr=1e-3)[3]["groups"]] == [2.0, 0.5, 0.0]
    # a zero base: the multipliers are undefined
    with pytest.raises(ValueError, match="base learning rate is 0"):
        ck.unpack_optimizer(sd, slots, names, n_flat, base_lr=0.0)
    opt.param_groups[0]["lr"] = 0.0
    with pytest.raises(ValueError, match="base learning rate is 0"):
        ck.unpack_optimizer(opt.state_dict(), slots, names, n_flat)
    # ... unless the dict says them itself
    packed = ck.pack_optimizer(m, v, 1, slots, names, dict(_hyper(), lr=0.0), groups=_groups(slots, kinds))
    assert [g["lr_mult"] for g in ck.unpack_optimizer(packed, slots, names, n_flat, base_lr=0.0)[3]["groups"]] == [1.0, 0.1, 1.0]
    # betas / eps are shared by the fused step's groups
    for key, val in (("betas", (0.8, 0.999)), ("eps", 1e-6)):
        bad = opt.state_dict()
        bad["param_groups"][1][key] = val
        with pytest.raises(ValueError, match="betas / eps"):
            ck.unpack_optimizer(bad, slots, names, n_flat)


def _pack_unpack(groups, base, slots, n_flat, through_torch=False):
    names = list(slots)
    sd = ck.pack_optimizer(torch.zeros(n_flat), torch.zeros(n_flat), 2, slots, names, dict(_hyper(), lr=base), groups=groups)
    if through_torch:      # (torch renumbers `params` and carries the extra keys)
        params = {k: torch.nn.Parameter(torch.zeros(slots[k][2])) for k in names}
        opt = torch.optim.AdamW([{"params": [params[k] for k in g["names"]]} for g in groups], lr=5.0)
        opt.load_state_dict(sd)
        sd = opt.state_dict()
    return ck.unpack_optimizer(sd, slots, names, n_flat, base_lr=base)[3]


@pytest.mark.parametrize("through_torch", [False, True])
def test_groups_whose_written_products_coincide_still_come_back_as_groups(through_torch):
    """Whether a dict is grouped is said by its keys, not by lr = base x lr_mult: the products of a grouped step are equal (a) at base
    0 -- what a warm-up scheduler sets at epoch 0 --, (b) with one multiplier and one decay everywhere, (c) for ONE group that holds
    everything still; and (d) a partition with uniform values keeps its names.  Read as uniform, a resumed step would train every
    tensor at the base rate."""
    _, _, slots, n_flat, kinds = _toy()
    names = list(slots)
    named = [(k, kinds[k]) for k in slots]
    enc = [{"match": r"^gene_encoder\."}]
    # (a) lr_mult (1, 0.1), equal decay, base 0
    a = optim.resolve_param_groups(named, [dict(enc[0], lr_mult=0.1)], 0.01)[0]
    h = _pack_unpack(a, 0.0, slots, n_flat, through_torch)
    assert h["lr"] == 0.0 and h["groups"] == a and [g["lr_mult"] for g in h["groups"]] == [1.0, 0.1]
    # (b) every group lr_mult 0.5, one decay: the written lr is 0.0005 everywhere, the base stays 1e-3
    b = optim.resolve_param_groups(named, [dict(enc[0], lr_mult=0.5), {"match": ".", "lr_mult": 0.5}], 0.01)[0]
    h = _pack_unpack(b, 1e-3, slots, n_flat, through_torch)
    assert h["lr"] == 1e-3 and h["groups"] == b and len(b) == 2
    # (c) the documented freeze over everything: one group, lr_mult 0, weight_decay 0
    c = optim.resolve_param_groups(named, [{"match": ".", "lr_mult": 0.0, "weight_decay": 0.0}], 0.01)[0]
    h = _pack_unpack(c, 1e-3, slots, n_flat, through_torch)
    assert h["lr"] == 1e-3 and h["groups"] == c and len(c) == 1 and c[0]["names"] == names
    # (d) two groups with the default values: the partition and its names survive
    d = optim.resolve_param_groups(named, enc, 0.01)[0]
    h = _pack_unpack(d, 1e-3, slots, n_flat, through_torch)
    assert h["groups"] == d and [(g["lr_mult"], g["weight_decay"]) for g in d] == [(1.0, 0.01)] * 2
    # one group with lr_mult 1 IS the uniform dict: the exact hyper, no "groups"
    e = optim.resolve_param_groups(named, None, 0.01)[0]
    assert _pack_unpack(e, 1e-3, slots, n_flat, through_torch) == _hyper()


# ---------------------------------------------------------------------------------------------- helpers
def test_no_decay_groups_puts_exactly_the_small_kinds_in_the_zero_decay_group():
    _, _, slots, _, kinds = _toy()
    named = [(k, torch.nn.Parameter(torch.zeros(slots[k][2]))) for k in slots]
    named.append(("frozen.weight", torch.nn.Parameter(torch.zeros(3), requires_grad=False)))      # frozen tensors are left out
    groups = optim.no_decay_groups(named, 0.01)
    assert [g["weight_decay"] for g in groups] == [0.01, 0.0]
    assert set(groups[1]["names"]) == {k for k in slots if kinds[k] in ("b", "lnw", "lnb", "gamma", "tok")}
    assert set(groups[0]["names"]) == {k for k in slots if kinds[k] == "w"}
    assert {kinds[k] for k in groups[1]["names"]} == {"b", "lnw", "lnb", "gamma", "tok"}
    by_name = dict(named)
    assert all(p is by_name[k] for g in groups for k, p in zip(g["names"], g["params"]))
    # torch takes the lists as they are and carries the names through its state_dict
    opt = torch.optim.AdamW(groups, lr=1e-3)
    assert [pg["names"] for pg in opt.state_dict()["param_groups"]] == [g["names"] for g in groups]
    # with a rule: the rule's group is split the same way
    four = optim.no_decay_groups(named, 0.01, rules=[{"match": r"^gene_encoder\.", "lr": 1e-4}])
    assert [(g.get("lr"), g["weight_decay"]) for g in four] == [(None, 0.01), (None, 0.0), (1e-4, 0.01), (1e-4, 0.0)]
    assert sorted(k for g in four for k in g["names"]) == sorted(slots)
    assert all(k.startswith("gene_encoder.") == (g.get("lr") == 1e-4) for g in four for k in g["names"])


def test_module_path_refuses_the_grouped_launch_on_a_span_that_is_not_16_byte_aligned():
    """Parameters that are views into a buffer of the user's own may start between two 16-byte lines: the grouped kernel's vectors need
    them, so the table is refused (None) before anything is built and step() takes torch's own step, as for every unmet precondition."""
    ps = [torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(4))]
    opt = optim.AdamW([{"params": ps[:1], "lr": 1e-3}, {"params": ps[1:], "lr": 1e-4}])
    assert opt._grouped()
    fl = {"lo": 4096 + 4, "p": None}
    assert opt._segment_table(fl) is None and fl["seg"] is None
    assert opt._segment_table(fl) is None          # (cached under the groups' key)


def test_groups_by_name_first_match_wins_and_a_dead_rule_raises():
    _, _, slots, _, _ = _toy()
    named = [(k, torch.nn.Parameter(torch.zeros(slots[k][2]))) for k in slots]
    groups = optim.groups_by_name(named, [{"match": r"^gene_encoder\.", "lr": 1e-4}, {"match": r"\.weight$", "lr": 3e-4, "weight_decay": 0.0}])
    assert "lr" not in groups[0] and groups[1]["lr"] == 1e-4 and (groups[2]["lr"], groups[2]["weight_decay"]) == (3e-4, 0.0)
    assert all(k.startswith("gene_encoder.") for k in groups[1]["names"]) and any(k.endswith(".weight") for k in groups[1]["names"])
    assert all(k.endswith(".weight") and not k.startswith("gene_encoder.") for k in groups[2]["names"])
    assert groups[0]["names"] and not any(k.endswith(".weight") or k.startswith("gene_encoder.") for k in groups[0]["names"])
    assert sorted(k for g in groups for k in g["names"]) == sorted(slots)
    with pytest.raises(ValueError, match="matches no trainable parameter"):
        optim.groups_by_name(named, [{"match": r"^nothing\."}])


# ---------------------------------------------------------------------------------------------- the C ABI
def test_grouped_entry_point_is_declared_exported_bound_and_checks_its_arguments():
    import __graft_entry__ as ge
    ge.build()
    from modaltune_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "modaltune_hip.h")).read()
    assert re.search(r"\bint\s+mt_adamw_step_groups\s*\(", header) and "#define MT_ADAM_MAX_GROUPS 16" in header
    assert re.search(r"typedef\s+struct\s*\{\s*double\s+lr_mult;\s*double\s+weight_decay;\s*\}\s*MtAdamGroup;", header)
    lib = _lib.load()
    assert hasattr(lib, "mt_adamw_step_groups") and "mt_adamw_step_groups" in _lib.SIGNATURES and callable(ops.adamw_step_groups)
    assert lib.mt_version() >= 340 and _lib.MT_ADAM_MAX_GROUPS == optim.MAX_GROUPS == 16
    assert C.sizeof(_lib.MtAdamGroup) == 16
    OK_, BAD, UNSUP = 0, -1, -3
    tab = (_lib.MtAdamGroup * 17)(*[(1.0, 0.01)] * 17)
    A = 0x10000          # never dereferenced: every call below is answered before anything touches the device

    def call(p=A, g=A, m=A, v=A, n=8, base=0, end=A, grp=A, nseg=1, groups=tab, ngroups=2, step=1):
        return lib.mt_adamw_step_groups(p, g, m, v, n, base, end, grp, nseg, groups, ngroups, 1e-3, 0.9, 0.999, 1e-8, step, None, 1.0, None,
                                        None, None, None)
    assert call(ngroups=0) == UNSUP and call(ngroups=17) == UNSUP and call(ngroups=-1) == UNSUP
    for kw in ({"p": None}, {"g": None}, {"m": None}, {"v": None}, {"end": None}, {"grp": None}, {"groups": None}, {"nseg": 0}, {"n": 0},
               {"base": -1}, {"step": 0}):
        assert call(**kw) == BAD, kw
    # a piece must lie in its buffers as index_base says: (address / 4) mod 4 == index_base mod 4, in all four
    assert call(base=1) == BAD and call(p=A + 4, base=1) == BAD and call(g=A + 8) == BAD and call(p=A + 2) == BAD
    assert OK_ == 0
