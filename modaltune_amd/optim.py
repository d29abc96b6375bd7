"""`torch.optim.AdamW`-shaped optimiser for the drop-in modules: the second import a trainer may swap.

The reference builds `torch.optim.AdamW(filter(requires_grad, model.parameters()), lr, weight_decay, betas)` and steps it through
`GradScaler.step` (train_modaltune.py:139-149, 235-238): 244 tensors (1 544 with the real pathways) walked per step by torch's
multi-tensor AdamW after GradScaler's unscale pass and a host read-back of `found_inf`.  The drop-in models keep every trainable
tensor as a view of ONE flat fp32 buffer (engine.ParamStore) and hand autograd gradients that are views of ONE flat buffer in the
same layout, so the whole update is one `mt_adamw_step` launch (csrc/optim.hip) -- unscale, inf check and skip included:

    from modaltune_amd.optim import AdamW          # instead of torch.optim.AdamW; same constructor, same state_dict
    opt = AdamW(params, lr=..., weight_decay=..., betas=...)
    scaler.step(opt)                                # GradScaler hands over `grad_scale` / `found_inf`: no unscale (division) pass and
                                                    # no read-back; its inf check over the gradients (_check_inf_per_device) still runs

It IS a `torch.optim.AdamW` (schedulers, `state_dict()`, `zero_grad()`, param groups behave as before).  Gradients that are not
views of one flat buffer (autograd cloned them, a DDP reducer owns them) are gathered by one multi-tensor copy first; whenever the
fused precondition does not hold at all -- parameters of some other module, a parameter without a gradient, amsgrad / maximize,
param groups that differ in betas or eps, more than 16 groups -- the step is torch's own, on the same state.

Param groups may differ in `lr` and `weight_decay` (no decay on biases and LayerNorm affines, a smaller rate for the gene encoder, a
sub-module held still): the step is then ONE `mt_adamw_step_groups` launch, which reads each tensor's two values from a segment table
(segment_table below) -- `no_decay_groups` and `groups_by_name` build such group lists for any optimiser.
"""
from __future__ import annotations

import re
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import ops


MAX_GROUPS = 16                # include/modaltune_hip.h: MT_ADAM_MAX_GROUPS
NO_DECAY_KINDS = ("b", "lnb", "lnw", "gamma", "tok")      # synth.param_specs kinds that conventionally take no weight decay
_TOKEN_PARAMS = ("gene_pe", "gene_cls")


# ------------------------------------------------------------------------------------------------ parameter groups (host only)
def segment_table(entries: Sequence[Tuple[int, int, int]], max_groups: int = MAX_GROUPS) -> Tuple[torch.Tensor, torch.Tensor]:
    """The table mt_adamw_step_groups reads, as CPU tensors (seg_end int32, seg_group uint8), from [(offset, numel, group)] of the
    tensors of one flat buffer in address order (offsets in elements from the buffer's 16-byte aligned start).  A segment is a run of
    neighbouring tensors of one group; it ends where the next segment's first tensor starts (the slot padding behind a tensor belongs
    to it), the last one at the end of the last slot.  Raises when a tensor does not start on a 16-byte slot or overlaps the one before
    it, when a group id lies outside 0 .. max_groups - 1, and for more than max_groups distinct groups."""
    if not entries:
        raise ValueError("segment_table: no tensors")
    ids = sorted({int(g) for _, _, g in entries})
    if len(ids) > max_groups:
        raise ValueError(f"segment_table: {len(ids)} parameter groups, the fused step carries at most {max_groups}")
    if ids[0] < 0 or ids[-1] >= max_groups:
        raise ValueError(f"segment_table: group ids must lie in 0 .. {max_groups - 1} (got {ids[0]} .. {ids[-1]})")
    ends, groups, cur = [], [], 0
    for i, (o, n, g) in enumerate(entries):
        o, n, g = int(o), int(n), int(g)
        if o % 4 or n < 1 or o < cur:
            raise ValueError(f"segment_table: tensor {i} (offset {o}, {n} elements) does not start on a 16-byte slot behind the tensor "
                             f"before it (which ends at {cur})")
        if groups and groups[-1] == g:
            ends.pop(); groups.pop()          # the same group as its neighbour: one segment
        elif ends:
            ends[-1] = o                      # the segment before ends where this tensor starts
        cur = o + n
        ends.append((cur + 3) // 4 * 4)
        groups.append(g)
    if ends[-1] >= 2 ** 31:
        raise ValueError(f"segment_table: the buffer ends at element {ends[-1]}, the table holds 32-bit indices")
    return torch.tensor(ends, dtype=torch.int32), torch.tensor(groups, dtype=torch.uint8)


def resolve_param_groups(named_kinds: Sequence[Tuple[str, str]], rules: Optional[Sequence[dict]], weight_decay: float):
    """TrainStep(param_groups=rules): rules are {"match": regex on the state_dict name and / or "kinds": (...), "lr_mult": 1.0,
    "weight_decay": <the default>}; the first rule that matches a tensor takes it (`match` is re.search; with both keys both must hold),
    unmatched tensors form the default group (lr_mult 1, `weight_decay`).  named_kinds: [(name, kind)] of the trainable tensors in
    buffer order.  Returns (groups, group_of): groups = [{"names", "lr_mult", "weight_decay"}] -- the default group first when it
    has tensors, then the rules in order -- and {name: index into groups}.  A rule that matches nothing, an unknown rule key and more
    than MAX_GROUPS groups raise."""
    rules = list(rules or [])
    compiled = []
    for i, r in enumerate(rules):
        unknown = set(r) - {"match", "kinds", "lr_mult", "weight_decay"}
        if unknown or not ("match" in r or "kinds" in r):
            raise ValueError(f"param_groups[{i}]: needs `match` and / or `kinds`; unknown keys {sorted(unknown)}")
        kinds = r.get("kinds")
        kinds = None if kinds is None else ((kinds,) if isinstance(kinds, str) else tuple(kinds))
        lm, wd = float(r.get("lr_mult", 1.0)), float(r.get("weight_decay", weight_decay))
        if not (lm >= 0.0 and wd >= 0.0):
            raise ValueError(f"param_groups[{i}]: lr_mult and weight_decay must be >= 0 (got {lm}, {wd})")
        compiled.append((re.compile(r["match"]) if "match" in r else None, kinds, lm, wd))
    default, taken = [], [[] for _ in rules]
    for name, kind in named_kinds:
        for i, (rx, kinds, _, _) in enumerate(compiled):
            if (rx is None or rx.search(name)) and (kinds is None or kind in kinds):
                taken[i].append(name)
                break
        else:
            default.append(name)
    for i, names in enumerate(taken):
        if not names:
            raise ValueError(f"param_groups[{i}] ({ {k: rules[i][k] for k in ('match', 'kinds') if k in rules[i]} }) matches no trainable tensor")
    groups = ([{"names": default, "lr_mult": 1.0, "weight_decay": float(weight_decay)}] if default else []) + \
             [{"names": names, "lr_mult": lm, "weight_decay": wd} for names, (_, _, lm, wd) in zip(taken, compiled)]
    if len(groups) > MAX_GROUPS:
        raise ValueError(f"param_groups resolve to {len(groups)} groups, the fused step carries at most {MAX_GROUPS}")
    return groups, {n: i for i, g in enumerate(groups) for n in g["names"]}


def _named_trainable(model) -> List[Tuple[str, torch.Tensor]]:
    pairs = model.named_parameters() if hasattr(model, "named_parameters") else model
    return [(k, p) for k, p in pairs if getattr(p, "requires_grad", True)]


def takes_no_decay(name: str, param) -> bool:
    """Biases, LayerNorm affines, the Injector gamma (everything with ndim <= 1) and the token parameters gene_pe / gene_cls: the
    kinds b, lnw, lnb, gamma and tok of synth.param_specs."""
    return param.ndim <= 1 or name.rsplit(".", 1)[-1] in _TOKEN_PARAMS


def groups_by_name(model, rules: Sequence[dict]) -> List[dict]:
    """torch-style param groups for any optimiser from rules {"match": regex on the parameter name, <hyper-parameters: lr,
    weight_decay, ...>}: the first rule that matches (re.search) takes the tensor, unmatched tensors form a leading group with the
    optimiser's defaults.  `model`: an nn.Module or (name, parameter) pairs; frozen parameters are left out.  Every group carries its
    tensor names under "names" (torch keeps unknown group keys through state_dict() / load_state_dict(); checkpoint.unpack_optimizer
    maps the state by them).  A rule that matches nothing raises."""
    rules = list(rules)
    rx = [re.compile(r["match"]) for r in rules]
    default, taken = [], [[] for _ in rules]
    for k, p in _named_trainable(model):
        for i, r in enumerate(rx):
            if r.search(k):
                taken[i].append((k, p))
                break
        else:
            default.append((k, p))
    for i, t in enumerate(taken):
        if not t:
            raise ValueError(f"groups_by_name: rule {i} ({rules[i]['match']!r}) matches no trainable parameter")
    out = [{"params": [p for _, p in default], "names": [k for k, _ in default]}] if default else []
    for r, t in zip(rules, taken):
        out.append({**{k: v for k, v in r.items() if k != "match"}, "params": [p for _, p in t], "names": [k for k, _ in t]})
    return out


def no_decay_groups(model, weight_decay: float, rules: Optional[Sequence[dict]] = None) -> List[dict]:
    """The usual fine-tuning recipe as torch-style param groups: weight_decay on the matrices, 0 on biases, LayerNorm affines, the
    Injector gamma and the token parameters (takes_no_decay).  With `rules` (groups_by_name's) every rule's group -- a smaller `lr` for
    the gene encoder, say -- is split the same way; a rule's own weight_decay replaces `weight_decay` for its matrices."""
    base = groups_by_name(model, rules) if rules else [{"params": [p for _, p in _named_trainable(model)],
                                                        "names": [k for k, _ in _named_trainable(model)]}]
    out = []
    for g in base:
        pairs = list(zip(g["names"], g["params"]))
        hyper = {k: v for k, v in g.items() if k not in ("params", "names", "weight_decay")}
        for wd, part in ((float(g.get("weight_decay", weight_decay)), [q for q in pairs if not takes_no_decay(*q)]),
                         (0.0, [q for q in pairs if takes_no_decay(*q)])):
            if part:
                out.append({**hyper, "weight_decay": wd, "params": [p for _, p in part], "names": [k for k, _ in part]})
    return out


def _param_span(ps):
    """(lowest address, fp32 elements up to the highest end) when `ps` are contiguous fp32 CUDA tensors of ONE storage that fill their
    span (gaps allowed: ParamStore pads slots to 16 bytes), else None."""
    if not ps or any(p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous() for p in ps):
        return None
    base = ps[0].untyped_storage().data_ptr()
    if any(p.untyped_storage().data_ptr() != base for p in ps):
        return None
    lo = min(p.data_ptr() for p in ps)
    n = (max(p.data_ptr() + p.numel() * 4 for p in ps) - lo) // 4
    # everything inside the span that is not a parameter must be padding an update may touch: true for ParamStore.flat (its gaps
    # are zero-filled slot padding); refuse anything that is mostly holes (a few tensors of a much larger storage)
    if (lo - base) % 16 or n <= 0 or sum(p.numel() for p in ps) < 0.95 * n:
        return None
    return lo, n


def _flat_grad_view(ps, lo: int, n: int) -> Optional[torch.Tensor]:
    """The gradients of `ps` as ONE flat tensor laid out like the parameters' span (lo, n) -- what the module bridge hands autograd --
    else None.  The one test of "the gradients are one flat buffer": AdamW.step and clip_grad_norm_ share it."""
    g0 = ps[0].grad
    if g0 is None or g0.dtype != torch.float32 or not g0.is_cuda:
        return None
    gst = g0.untyped_storage()
    gbase = gst.data_ptr()
    delta = g0.data_ptr() - ps[0].data_ptr()
    for p in ps:
        g = p.grad
        if g is None or g.dtype != torch.float32 or not g.is_contiguous() or g.data_ptr() - p.data_ptr() != delta \
                or g.untyped_storage().data_ptr() != gbase:
            return None
    glo = lo + delta
    if glo < gbase or glo + n * 4 > gbase + gst.nbytes() or (glo - gbase) % 4:
        return None
    return torch.empty(0, dtype=torch.float32, device=g0.device).set_(gst, (glo - gbase) // 4, (n,), (1,))


def _fills_span(ps, lo: int, n: int) -> bool:
    """`ps` ARE the span: sorted by address, every tensor starts less than 16 bytes behind the end of the one before it (ParamStore's
    slot padding) and the last one ends the span.  A list that leaves out a tensor of the buffer -- whose gradient would then be counted
    in the norm and scaled with the rest -- fails this (a slot is at least 16 bytes)."""
    cur = lo
    for p in sorted(ps, key=lambda t: t.data_ptr()):
        if not 0 <= p.data_ptr() - cur < 16:
            return False
        cur = p.data_ptr() + p.numel() * 4
    return cur == lo + n * 4


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None) -> torch.Tensor:
    """`torch.nn.utils.clip_grad_norm_` for the reference-style loop (scaler.unscale_(opt); clip; scaler.step(opt)).

    When the gradients are one flat buffer laid out like the parameters (the drop-in modules; the test AdamW.step makes), `parameters`
    are ALL the tensors of that buffer (a subset is torch's call: its norm is over the listed tensors only) and norm_type is 2, three launches replace torch's walk over 244 to 1 544 tensors: mt_grad_sumsq (sum of squares in double),
    mt_grad_clip_coef (min(1, max_norm / (norm + 1e-6))) and one in-place mt_axpy_dev g *= coef.  The norm comes back as a 0-d device
    tensor and nothing synchronises with the host unless error_if_nonfinite is set.  Anything else -- another norm_type, CPU tensors,
    gradients in separate allocations -- is torch's own call, unchanged.

    One difference from torch on the fast path: non-finite gradients are left as they are (coefficient 1) where torch multiplies them
    by NaN; GradScaler skips the step either way."""
    if torch.is_tensor(parameters):
        parameters = [parameters]
    ps = list(parameters)
    g = None
    if float(norm_type) == 2.0 and ps and all(p.grad is not None for p in ps):
        span = _param_span(ps)
        g = _flat_grad_view(ps, *span) if span is not None and _fills_span(ps, *span) else None
    if g is None:
        return torch.nn.utils.clip_grad_norm_(ps, max_norm, norm_type=norm_type, error_if_nonfinite=error_if_nonfinite, foreach=foreach)
    n = g.numel()
    sumsq = torch.empty(1, dtype=torch.float64, device=g.device)
    ws = torch.empty(ops.grad_sumsq_partials_elems(n), dtype=torch.float64, device=g.device)
    out = torch.empty(3, dtype=torch.float32, device=g.device)
    with torch.cuda.device(g.device):
        ops.grad_sumsq(g, n, ws, sumsq)
        ops.grad_clip_coef(sumsq, 1, 1.0, None, float(max_norm), None, out)
        if error_if_nonfinite and not bool(torch.isfinite(out[0])):
            raise RuntimeError(f"The total norm of order {float(norm_type)} for gradients from `parameters` is non-finite, so it cannot be "
                               "clipped. To disable this error and scale the gradients by the non-finite norm anyway, set "
                               "`error_if_nonfinite=False`")
        ops.axpy_dev(None, g, out[1:2], g, n)
    return out[0]


class AdamW(torch.optim.AdamW):
    _step_supports_amp_scaling = True          # GradScaler.step: leave unscaling and the skip decision to step() (grad_scale / found_inf)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False, **kw):
        # torch's own implementation must stay usable on this object's state: no foreach / fused / capturable flavours of it
        kw.pop("foreach", None); kw.pop("fused", None); kw.pop("capturable", None)
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=False, **kw)
        self._step_supports_amp_scaling = True
        self._flat = None             # (base pointer, numel, exp_avg, exp_avg_sq, step_dev) once the parameters proved to be one flat buffer
        self._flat_failed = False
        self._host_steps = 0          # fused steps taken so far (the per-parameter `step` entries are brought up to date lazily)
        self._steps_dirty = False
        self.last_step_fused: Optional[bool] = None

    def add_param_group(self, param_group):
        """A new group changes the parameter set the flat views (moments, gathered-gradient views) were built for: rebind at the next step
        (moments already accumulated are carried over through the per-parameter state, see _bind_flat)."""
        if getattr(self, "_flat", None) is not None:
            self._sync_steps()                # (the step counts of the parameters bound so far, before the set changes)
        super().add_param_group(param_group)
        self._flat, self._flat_failed = None, False

    # ------------------------------------------------------------------ the flat view of the parameters
    def _all_params(self) -> List[torch.Tensor]:
        return [p for g in self.param_groups for p in g["params"]]

    def _uniform_groups(self) -> bool:
        g0 = self.param_groups[0]
        keys = ("lr", "betas", "eps", "weight_decay", "amsgrad", "maximize")
        return all(all(g[k] == g0[k] for k in keys) for g in self.param_groups) and not g0["amsgrad"] and not g0["maximize"] \
            and not torch.is_tensor(g0["lr"])

    def _grouped(self) -> bool:
        """The groups differ, but in `lr` / `weight_decay` only, and there are at most MAX_GROUPS of them: mt_adamw_step_groups' case."""
        gs = self.param_groups
        g0 = gs[0]
        return 1 < len(gs) <= MAX_GROUPS and all(all(g[k] == g0[k] for k in ("betas", "eps", "amsgrad", "maximize")) for g in gs) \
            and not g0["amsgrad"] and not g0["maximize"] and not any(torch.is_tensor(g["lr"]) or torch.is_tensor(g["weight_decay"]) for g in gs)

    def _segment_table(self, fl):
        """The device table of the bound parameters (rebuilt when the groups' membership changed), or None when they do not sit in
        16-byte slots of a 16-byte aligned span: the step is then torch's own, as for every other unmet precondition."""
        key = tuple(len(g["params"]) for g in self.param_groups)
        if fl.get("seg_key") != key:
            if fl["lo"] % 16:      # (views into a buffer of the user's that starts between two 16-byte lines: the kernel's vectors need them)
                fl["seg"], fl["seg_key"] = None, key
                return None
            ents = sorted(((p.data_ptr() - fl["lo"]) // 4, p.numel(), gi) for gi, g in enumerate(self.param_groups) for p in g["params"])
            try:
                end, grp = segment_table(ents)
                fl["seg"] = (end.to(fl["p"].device), grp.to(fl["p"].device))
            except ValueError:
                fl["seg"] = None
            fl["seg_key"] = key
        return fl["seg"]

    def _bind_flat(self):
        """Do all parameters live in one contiguous fp32 buffer (gaps allowed: ParamStore pads slots to 16 bytes with zeros that
        AdamW leaves at zero)?  If so, build the flat moment buffers and make every parameter's optimiser state a VIEW of them, so
        `state_dict()` / `load_state_dict()` / a later torch step see ordinary per-parameter AdamW state."""
        ps = self._all_params()
        span = _param_span(ps)
        if span is None:
            return None
        lo, n = span
        st = ps[0].untyped_storage()
        base = st.data_ptr()
        dev = ps[0].device
        m = torch.zeros(n, dtype=torch.float32, device=dev)
        v = torch.zeros(n, dtype=torch.float32, device=dev)
        for p in ps:
            o = (p.data_ptr() - lo) // 4
            s = self.state[p]
            if "exp_avg" in s:          # state loaded / produced by torch steps before the first fused one: carry it over
                m[o:o + p.numel()].copy_(s["exp_avg"].reshape(-1))
                v[o:o + p.numel()].copy_(s["exp_avg_sq"].reshape(-1))
                self._host_steps = max(self._host_steps, int(float(s["step"])))
            s["exp_avg"] = m[o:o + p.numel()].view(p.shape)
            s["exp_avg_sq"] = v[o:o + p.numel()].view(p.shape)
            s.setdefault("step", torch.tensor(0.0, dtype=torch.float32))
        flat_p = torch.empty(0, dtype=torch.float32, device=dev).set_(st, (lo - base) // 4, (n,), (1,))
        step_dev = torch.full((1,), self._host_steps, dtype=torch.int32, device=dev)
        return {"lo": lo, "n": n, "p": flat_p, "m": m, "v": v, "step_dev": step_dev, "gbuf": None, "gviews": None,
                "ids": tuple(id(p) for p in ps)}

    def _gathered_grad(self, fl) -> Optional[torch.Tensor]:
        """Gradients that exist for every parameter but live in their own allocations (autograd clones them when several nodes feed
        one parameter -- the per-task calls of a slide run one by one --, a DDP reducer owns them, ...): ONE multi-tensor copy into a
        flat buffer laid out like the parameters, then the fused step as usual.  None when some parameter has no gradient (torch's
        AdamW leaves such a parameter alone; the flat kernel would still decay it)."""
        ps = self._all_params()
        grads = [p.grad for p in ps]
        if any(g is None or g.dtype != torch.float32 or not g.is_cuda or g.shape != p.shape for g, p in zip(grads, ps)):
            return None
        if fl["gbuf"] is None:
            fl["gbuf"] = torch.zeros(fl["n"], dtype=torch.float32, device=ps[0].device)      # (the padding between slots stays zero)
            fl["gviews"] = [fl["gbuf"][(p.data_ptr() - fl["lo"]) // 4:(p.data_ptr() - fl["lo"]) // 4 + p.numel()].view(p.shape) for p in ps]
        torch._foreach_copy_(fl["gviews"], grads)
        return fl["gbuf"]

    def _flat_grad(self, fl) -> Optional[torch.Tensor]:
        """The gradients as ONE flat tensor laid out like the parameters (what the module bridge hands autograd), else None."""
        return _flat_grad_view(self._all_params(), fl["lo"], fl["n"])

    def _sync_steps(self):
        if self._steps_dirty and self._flat is not None:
            # (skipped steps -- GradScaler found an inf -- do not count: the device counter is the truth)
            k = float(int(self._flat["step_dev"].item()))
            self._host_steps = int(k)
            for p in self._all_params():
                self.state[p]["step"] = torch.tensor(k, dtype=torch.float32)
            self._steps_dirty = False

    def state_dict(self):
        self._sync_steps()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._flat, self._flat_failed, self._steps_dirty = None, False, False      # rebind (the loaded tensors are fresh allocations)
        self._host_steps = 0

    # ------------------------------------------------------------------ step
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        grad_scale, found_inf = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)
        fl = None
        uniform = self._uniform_groups()
        if not self._flat_failed and (uniform or self._grouped()):
            if self._flat is not None and self._flat["ids"] != tuple(id(p) for p in self._all_params()):
                self._sync_steps()            # param_groups were edited in place: the cached views describe another parameter set
                self._flat = None
            if self._flat is None:
                self._flat = self._bind_flat()
                self._flat_failed = self._flat is None
            fl = self._flat
        g = self._flat_grad(fl) if fl is not None else None
        seg = None
        if fl is not None and not uniform:
            seg = self._segment_table(fl)
            if seg is None:
                fl = g = None
            elif g is not None and g.data_ptr() % 16:      # (the grouped kernel's vectors sit on 16-byte addresses in all four buffers)
                g = None
        if g is None and fl is not None:
            g = self._gathered_grad(fl)
        if g is not None:
            grp = self.param_groups[0]
            b1, b2 = grp["betas"]
            # found_inf: GradScaler's 0.0 / 1.0 float, read by the kernel as a word that is zero or not; grad_scale: its fp32 scale
            if uniform:
                ops.adamw_step(fl["p"], g, fl["m"], fl["v"], fl["n"], float(grp["lr"]), float(b1), float(b2), float(grp["eps"]),
                               float(grp["weight_decay"]), 0, scale=grad_scale, found_inf=found_inf, step_dev=fl["step_dev"])
            else:
                # base lr 1.0 and lr_mult = the group's lr: (float)(1.0f * lr) is what mt_adamw_step forms from the same value; the
                # values are kernel arguments read at every step, so a scheduler that edits group["lr"] costs nothing
                ops.adamw_step_groups(fl["p"], g, fl["m"], fl["v"], fl["n"], 0, seg[0], seg[1],
                                      [(float(q["lr"]), float(q["weight_decay"])) for q in self.param_groups], 1.0, float(b1), float(b2),
                                      float(grp["eps"]), 0, scale=grad_scale, found_inf=found_inf, step_dev=fl["step_dev"])
            if found_inf is not None:
                fl["step_dev"].add_((found_inf == 0).to(torch.int32).reshape(1))
            else:
                fl["step_dev"].add_(1)
            self._steps_dirty = True
            self.last_step_fused = True
            self._bump_versions()             # (derived fp16 weight caches key on the parameters' version counters)
            return loss
        # torch's own step on the same state (per-tensor): unscale first when GradScaler left that to us
        self.last_step_fused = False
        self._sync_steps()
        if grad_scale is not None or found_inf is not None:
            grads = [p.grad for p in self._all_params() if p.grad is not None]
            if found_inf is not None and bool(found_inf.item()):
                return loss
            if grad_scale is not None and grads:
                torch._foreach_div_(grads, grad_scale.to(grads[0].device))
            try:                              # (the base class must not see the scaler's attributes a second time)
                gs, fi = self.__dict__.pop("grad_scale", None), self.__dict__.pop("found_inf", None)
                super().step()
            finally:
                if gs is not None:
                    self.grad_scale = gs
                if fi is not None:
                    self.found_inf = fi
        else:
            super().step()
        if self._flat is not None:            # (a later fused step continues from the same count)
            self._flat["step_dev"].add_(1)
            self._host_steps += 1
        return loss

    def _bump_versions(self):
        """The update went through a raw pointer: tell autograd / the modules' weight caches that the parameters changed."""
        ps = self._all_params()
        torch._C._autograd._unsafe_set_version_counter(ps, [p._version + 1 for p in ps])
