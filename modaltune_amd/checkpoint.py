"""The checkpoint of the fused train step (trainer.TrainStep.state_dict / load_state_dict): its format, on plain CPU tensors.

Nothing here touches the device: torch and numpy only, so the format, its checks and its checksums are testable -- and a file is
verifiable -- without a GPU.  A checkpoint is a flat dict of CPU tensors, ints, floats, strings, lists and dicts (`torch.save`-able,
read back with `torch.load(..., weights_only=True)`):

    format      1
    model       {key: tensor}: the trainable tensors under the reference's state_dict names (include_frozen: every tensor)
    optimizer   torch.optim.AdamW.state_dict() format: state[i] = {"step", "exp_avg", "exp_avg_sq"} of the i-th TRAINABLE tensor in
                ParamStore.specs order (= the order filter(requires_grad, model.parameters()) gives the reference trainer), one param group
                -- or, with TrainStep(param_groups=...), one torch param group per resolved group: `lr` = base lr x lr_mult,
                its `weight_decay`, `params` = the indices of its tensors, and two extra keys torch carries along: `lr_mult`
                and `names` (the tensors' names; torch renumbers `params` on its way through an optimiser, the names stay)
    scaler      torch.amp.GradScaler.state_dict() format
    rng         int32[4]: the Philox seed / step counter of the dropout masks;  stochastic: whether the masks were on
    lr          the learning rate on the device (the scheduler's last set_lr)
    window      None (empty accumulation window) or {"pos", "accumulate", "grad_scale", "grad"}: the micro-steps held and their summed
                flat gradient
    schedule    {"split_decisions": {patches: bool}}: which recurring geometries run as pass groups (the bits depend on it)
    checksums   {"flat", "m", "v"}: mt_checksum64 of the three flat buffers (slot padding included, which is zero) as Python ints
    build_id    of the library that wrote it;  world: the data-parallel world size it was written at
    config      the ModelConfig fields and the pathway group sizes: the shape check, and what verify_file lays the flat buffers out by
    ema         OPTIONAL, only from a TrainStep(ema_decay=...): {"decay", "warmup", "model": {key: tensor}} -- the exponential moving
                average of the trainable tensors under the names of `model`; `checksums` then carries "ema" as well.  REQUIRED_KEYS and
                `format` are what they were: a step without an average writes and reads today's key set exactly

The slot padding of the flat buffers (slots are 16-byte aligned) is not stored; a load zeroes it.
"""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .config import GeneConfig, ModelConfig
from .synth import param_specs

FORMAT = 1
REQUIRED_KEYS = ("format", "model", "optimizer", "scaler", "rng", "stochastic", "lr", "window", "schedule", "checksums", "build_id", "world",
                 "config")
MODULE_KEYS = ("model", "optimizer", "scaler")      # what a dict assembled from the module path (model, AdamW, GradScaler) carries
GROWTH_FACTOR, BACKOFF_FACTOR = 2.0, 0.5            # the fused step's scaler constants (trainer.TrainStep._adam_and_refresh)
_M64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------ the checksum
def _mix(j: np.ndarray) -> np.ndarray:
    """splitmix64(j) | 1 on a uint64 array (array arithmetic wraps mod 2^64)."""
    z = j + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return (z ^ (z >> np.uint64(31))) | np.uint64(1)


def _words(array) -> np.ndarray:
    if torch.is_tensor(array):
        t = array.detach().cpu().contiguous()
        if t.element_size() % 4:
            raise ValueError(f"checksum64: elements of {t.element_size()} bytes are not whole 32-bit words")
        array = t.view(torch.int32).numpy() if t.dtype != torch.int32 else t.numpy()
    a = np.ascontiguousarray(array)
    if a.dtype.itemsize % 4:
        raise ValueError(f"checksum64: elements of {a.dtype.itemsize} bytes are not whole 32-bit words")
    return a.reshape(-1).view(np.uint32)


def checksum64_reference(array, index_base: int = 0) -> int:
    """mt_checksum64 (include/modaltune_hip.h) in numpy uint64:  sum_i mix(index_base + i) * (word_i + 1)  mod 2^64  over the 32-bit
    words of `array` (a numpy array or CPU tensor of 4- or 8-byte elements)."""
    w = _words(array)
    total, chunk = 0, 1 << 22
    with np.errstate(over="ignore"):
        for a in range(0, w.size, chunk):
            part = w[a:a + chunk].astype(np.uint64)
            j = np.arange(a, a + part.size, dtype=np.uint64) + np.uint64((index_base + 0) & _M64)
            total = (total + int((_mix(j) * (part + np.uint64(1))).sum(dtype=np.uint64))) & _M64
    return total


def as_unsigned(value) -> int:
    """The device writes the checksum into an int64 tensor: its value as the unsigned 64-bit integer the formula defines."""
    return int(value) & _M64


# ------------------------------------------------------------------------------------------------ layout
def slots_of(specs) -> Tuple[Dict[str, tuple], int]:
    """engine.ParamStore's layout rule: ({key: (offset, numel, shape)} of the trainable tensors, 16-byte aligned slots in specs order;
    elements of the flat buffers)."""
    off, slots = 0, {}
    for k, shape, _, train in specs:
        if train:
            n = int(np.prod(shape))
            slots[k] = (off, n, tuple(shape))
            off += (n + 3) // 4 * 4
    return slots, off


def config_dict(cfg: ModelConfig, group_sizes: Sequence[int]) -> dict:
    d = dataclasses.asdict(cfg)
    d["interaction_indexes"] = [[int(i) for i in p] for p in cfg.interaction_indexes]
    return {"model": d, "group_sizes": [int(s) for s in group_sizes]}


def config_from_dict(d: dict) -> Tuple[ModelConfig, List[int]]:
    m = dict(d["model"])
    m["gene"] = GeneConfig(**m["gene"])
    m["interaction_indexes"] = tuple(tuple(int(i) for i in p) for p in m["interaction_indexes"])
    return ModelConfig(**m), [int(s) for s in d["group_sizes"]]


def _flat_from(tensors: Dict[str, torch.Tensor], slots: Dict[str, tuple], n_flat: int, what: str) -> torch.Tensor:
    """One zero-padded flat fp32 CPU buffer from per-tensor entries (every slot's tensor must be there, in its shape)."""
    flat = torch.zeros(n_flat, dtype=torch.float32)
    for k, (o, n, shape) in slots.items():
        if k not in tensors:
            raise KeyError(f"{what}: tensor {k} is missing")
        t = tensors[k]
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{what}: {k} has shape {tuple(t.shape)}, this engine holds {tuple(shape)}")
        flat[o:o + n].copy_(t.detach().reshape(-1).to("cpu", torch.float32))
    return flat


# ------------------------------------------------------------------------------------------------ optimiser
def pack_optimizer(m_flat: torch.Tensor, v_flat: torch.Tensor, step: int, slots: Dict[str, tuple], trainable_names: Sequence[str],
                   hyper: dict, groups: Optional[Sequence[dict]] = None) -> dict:
    """The flat AdamW moments as a torch.optim.AdamW.state_dict(): state[i] belongs to trainable_names[i], exp_avg / exp_avg_sq keep the
    parameter's shape, `step` is torch's fp32 scalar; hyper: lr, betas, eps, weight_decay.  Slot padding is not stored.
    groups (TrainStep.param_groups: [{"names", "lr_mult", "weight_decay"}]): one torch param group each -- lr = hyper lr x lr_mult, the
    group's weight_decay, params = the indices of its tensors, plus the keys `lr_mult` and `names`.  None: the one group as ever."""
    m_flat, v_flat = m_flat.detach().to("cpu"), v_flat.detach().to("cpu")
    state = {}
    for i, k in enumerate(trainable_names):
        o, n, shape = slots[k]
        state[i] = {"step": torch.tensor(float(step), dtype=torch.float32), "exp_avg": m_flat[o:o + n].clone().view(shape),
                    "exp_avg_sq": v_flat[o:o + n].clone().view(shape)}
    b1, b2 = hyper["betas"]
    group = {"lr": float(hyper["lr"]), "betas": (float(b1), float(b2)), "eps": float(hyper["eps"]),
             "weight_decay": float(hyper["weight_decay"]), "amsgrad": False, "maximize": False, "foreach": None, "capturable": False,
             "differentiable": False, "fused": None, "decoupled_weight_decay": True, "params": list(range(len(trainable_names)))}
    if groups is None:
        return {"state": state, "param_groups": [group]}
    index = {k: i for i, k in enumerate(trainable_names)}
    listed = [k for g in groups for k in g["names"]]
    if sorted(listed) != sorted(trainable_names):
        raise ValueError(f"optimizer: the groups list {len(listed)} tensors, this engine trains {len(trainable_names)} (every trainable "
                         "tensor belongs to exactly one group)")
    out = []
    for g in groups:
        out.append({**group, "lr": float(hyper["lr"]) * float(g["lr_mult"]), "weight_decay": float(g["weight_decay"]),
                    "params": [index[k] for k in g["names"]], "lr_mult": float(g["lr_mult"]), "names": list(g["names"])})
    return {"state": state, "param_groups": out}


def unpack_optimizer(opt_sd: dict, slots: Dict[str, tuple], trainable_names: Sequence[str], n_flat: int, base_lr: Optional[float] = None):
    """pack_optimizer's inverse, for any torch.optim.AdamW.state_dict() over the trainable tensors in order: (m_flat, v_flat, step,
    hyper) with zero slot padding.  An optimiser that never stepped (empty state) gives zero moments and step 0.  The per-parameter
    `step` entries map to ONE device counter: they must agree.
    A GROUPED dict comes back with hyper["groups"] = [{"names", "lr_mult", "weight_decay"}] and hyper["lr"] the BASE rate.  Grouped is
    said by the dict's KEYS before its values: a group with an `lr_mult` other than 1, or more than one group of which any carries
    `lr_mult` or `names` (what pack_optimizer and the optim helpers write), or -- a plain torch dict -- groups whose lr / weight_decay
    differ.  The written lr = base x lr_mult alone cannot say it: at base 0 (a warm-up's first epoch), with one multiplier everywhere
    or with a single frozen group the products of a grouped step are equal.  The base: `base_lr` (a checkpoint's `lr`), else the first
    group's lr / lr_mult (exact for lr_mult 1, the default group; for another multiplier the quotient may be one ulp off the double
    that was multiplied -- a full checkpoint carries `lr` and does not depend on it), else the first group's lr; a group without an
    `lr_mult` key (the dict came from a torch optimiser) takes lr / base.  Which tensor an entry of `params` is: the group's
    `names` (pack_optimizer, optim.no_decay_groups and optim.groups_by_name write them, torch carries them through) -- without names
    the entries of all groups in order are the trainable tensors in order, as for one group.  A uniform dict: the 4-tuple as ever."""
    if "state" not in opt_sd or "param_groups" not in opt_sd:
        raise KeyError("optimizer: `state` / `param_groups` missing (not a torch.optim.AdamW.state_dict())")
    pgs = opt_sd["param_groups"]
    ids = [i for g in pgs for i in g["params"]]
    if len(ids) != len(trainable_names):
        raise ValueError(f"optimizer: {len(ids)} parameters in its groups, this engine trains {len(trainable_names)} tensors")
    if all("names" in g for g in pgs):
        order = [k for g in pgs for k in g["names"]]
        if len(order) != len(ids) or any(len(g["names"]) != len(g["params"]) for g in pgs) or sorted(order) != sorted(trainable_names):
            raise ValueError("optimizer: the `names` of its param groups are not this engine's trainable tensors, one entry of `params` each")
    else:
        order = list(trainable_names)
    state = opt_sd["state"]
    m, v = torch.zeros(n_flat, dtype=torch.float32), torch.zeros(n_flat, dtype=torch.float32)
    steps = {}
    for k, i in zip(order, ids):
        s = state.get(i, state.get(str(i)))
        if s is None or "exp_avg" not in s:
            continue
        o, n, shape = slots[k]
        for name, flat in (("exp_avg", m), ("exp_avg_sq", v)):
            t = s[name]
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"optimizer: {name} of {k} has shape {tuple(t.shape)}, this engine holds {tuple(shape)}")
            flat[o:o + n].copy_(t.detach().reshape(-1).to("cpu", torch.float32))
        steps[k] = int(float(s["step"]))
    if steps and len(steps) != len(trainable_names):
        missing = [k for k in trainable_names if k not in steps]
        raise KeyError(f"optimizer: no state for {missing[0]} (and {len(missing) - 1} more) while other tensors have one")
    if len(set(steps.values())) > 1:
        lo = min(steps, key=steps.get)
        hi = max(steps, key=steps.get)
        raise ValueError(f"optimizer: the per-parameter `step` entries disagree ({lo}: {steps[lo]}, {hi}: {steps[hi]}); the fused step "
                         "keeps one count for all tensors")
    g0 = pgs[0]
    for g in pgs[1:]:
        if any(tuple(g[key]) != tuple(g0[key]) if key == "betas" else g[key] != g0[key] for key in ("betas", "eps")):
            raise ValueError("optimizer: param groups with different betas / eps; the fused step shares them among its groups (only lr "
                             "and weight_decay are per group)")
    hyper = {"lr": float(g0["lr"]), "betas": (float(g0["betas"][0]), float(g0["betas"][1])), "eps": float(g0["eps"]),
             "weight_decay": float(g0["weight_decay"])}
    keyed = any(float(g.get("lr_mult", 1.0)) != 1.0 for g in pgs) or (len(pgs) > 1 and any("lr_mult" in g or "names" in g for g in pgs))
    if keyed or any(g[key] != g0[key] for g in pgs[1:] for key in ("lr", "weight_decay")):
        if len(pgs) > 16:
            raise ValueError(f"optimizer: {len(pgs)} param groups of their own, the fused step carries at most 16")
        if base_lr is None:
            lm0 = float(g0.get("lr_mult", 1.0))
            base_lr = float(g0["lr"]) / lm0 if lm0 != 0.0 else float(g0["lr"])
        base_lr = float(base_lr)
        groups, pos = [], 0
        for g in pgs:
            if "lr_mult" in g:
                lm = float(g["lr_mult"])
            elif base_lr != 0.0:
                lm = float(g["lr"]) / base_lr
            else:
                raise ValueError("optimizer: param groups with different lr and no `lr_mult` keys, and the base learning rate is 0: the "
                                 "groups' multipliers lr / base are undefined (give the first group a non-zero lr, or save `lr_mult`)")
            groups.append({"names": order[pos:pos + len(g["params"])], "lr_mult": lm, "weight_decay": float(g["weight_decay"])})
            pos += len(g["params"])
        hyper["lr"], hyper["groups"] = base_lr, groups
    return m, v, (next(iter(steps.values())) if steps else 0), hyper


# ------------------------------------------------------------------------------------------------ EMA of the weights
def pack_ema(ema_flat: torch.Tensor, slots: Dict[str, tuple], decay: float, warmup: bool) -> dict:
    """The optional `ema` entry: {"decay", "warmup", "model": {name: tensor}} -- the flat average per tensor, in slot (= specs) order,
    under the names of `model`; slot padding is not stored."""
    ema_flat = ema_flat.detach().to("cpu")
    return {"decay": float(decay), "warmup": bool(warmup),
            "model": {k: ema_flat[o:o + n].clone().view(shape) for k, (o, n, shape) in slots.items()}}


def unpack_ema(ema_sd: dict, slots: Dict[str, tuple], n_flat: int) -> Tuple[torch.Tensor, float, bool]:
    """pack_ema's inverse: (zero-padded flat CPU buffer, decay, warm-up flag); KeyError / ValueError naming what is wrong."""
    for k in ("decay", "warmup", "model"):
        if not isinstance(ema_sd, dict) or k not in ema_sd:
            raise KeyError(f"ema: `{k}` is missing")
    decay = float(ema_sd["decay"])
    if not 0.0 <= decay < 1.0:
        raise ValueError(f"ema: decay {decay} is outside [0, 1)")
    for k in ema_sd["model"]:
        if k not in slots:
            raise KeyError(f"ema: unexpected tensor {k}")
    return _flat_from(ema_sd["model"], slots, n_flat, "ema"), decay, bool(ema_sd["warmup"])


# ------------------------------------------------------------------------------------------------ scaler
def pack_scaler(scale: float, growth_tracker: int, growth_interval: int, growth_factor: float = GROWTH_FACTOR,
                backoff_factor: float = BACKOFF_FACTOR) -> dict:
    """torch.amp.GradScaler.state_dict() format."""
    return {"scale": float(scale), "growth_factor": float(growth_factor), "backoff_factor": float(backoff_factor),
            "growth_interval": int(growth_interval), "_growth_tracker": int(growth_tracker)}


def unpack_scaler(sd: dict) -> Tuple[float, int, int]:
    """(scale, growth tracker, growth interval); the fused step's factors are fixed (2, 0.5): others are refused."""
    for k in ("scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker"):
        if k not in sd:
            raise KeyError(f"scaler: `{k}` is missing (not a GradScaler.state_dict() of an enabled scaler)")
    if float(sd["growth_factor"]) != GROWTH_FACTOR or float(sd["backoff_factor"]) != BACKOFF_FACTOR:
        raise ValueError(f"scaler: growth / backoff factors {sd['growth_factor']} / {sd['backoff_factor']}; the fused step uses "
                         f"{GROWTH_FACTOR} / {BACKOFF_FACTOR}")
    return float(sd["scale"]), int(sd["_growth_tracker"]), int(sd["growth_interval"])


# ------------------------------------------------------------------------------------------------ whole-file checks
def check_format(sd: dict) -> bool:
    """Raises on a wrong `format` or an incomplete key set; returns whether `sd` is a full checkpoint (True) or a dict assembled from
    the module path -- model, optimizer, scaler and nothing that needs this file's format (False)."""
    if not isinstance(sd, dict):
        raise ValueError(f"checkpoint: a dict is expected, got {type(sd).__name__}")
    if "format" not in sd:
        for k in MODULE_KEYS:
            if k not in sd:
                raise KeyError(f"checkpoint: `{k}` is missing")
        return False
    if sd["format"] != FORMAT:
        raise ValueError(f"checkpoint: format {sd['format']!r}, this version reads format {FORMAT}")
    for k in REQUIRED_KEYS:
        if k not in sd:
            raise KeyError(f"checkpoint: `{k}` is missing")
    return True


def check_model_shapes(model: Dict[str, torch.Tensor], shapes: Dict[str, tuple], trainable_names: Sequence[str]):
    """Every trainable tensor present, no unknown key, every shape this engine's: KeyError / ValueError naming the tensor."""
    for k in trainable_names:
        if k not in model:
            raise KeyError(f"model: tensor {k} is missing")
    for k, t in model.items():
        if k not in shapes:
            raise KeyError(f"model: unexpected tensor {k}")
        if tuple(t.shape) != tuple(shapes[k]):
            raise ValueError(f"model: {k} has shape {tuple(t.shape)}, this engine holds {tuple(shapes[k])}")


def flat_buffers(sd: dict, slots: Dict[str, tuple], n_flat: int):
    """(flat, m, v, step, hyper) of a checkpoint dict as zero-padded CPU buffers in the engine's layout."""
    names = list(slots)
    flat = _flat_from(sd["model"], slots, n_flat, "model")
    m, v, step, hyper = unpack_optimizer(sd["optimizer"], slots, names, n_flat, base_lr=sd["lr"] if "format" in sd else None)
    return flat, m, v, step, hyper


def verify_file(path: str) -> dict:
    """Read a checkpoint file (weights_only) and recompute its three checksums (four with an `ema` entry) on the CPU from what it
    stores; RuntimeError naming the buffer on a mismatch.  Returns the checkpoint."""
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not check_format(sd):
        raise ValueError(f"{path}: not a TrainStep checkpoint (no `format`)")
    cfg, sizes = config_from_dict(sd["config"])
    slots, n_flat = slots_of(param_specs(cfg, sizes))
    flat, m, v, _, _ = flat_buffers(sd, slots, n_flat)
    bufs = [("flat", flat), ("m", m), ("v", v)]
    if "ema" in sd:      # (optional: a step that keeps an average)
        if "ema" not in sd["checksums"]:
            raise KeyError(f"{path}: `ema` is stored without its checksum")
        bufs.append(("ema", unpack_ema(sd["ema"], slots, n_flat)[0]))
    for name, buf in bufs:
        have, want = checksum64_reference(buf), as_unsigned(sd["checksums"][name])
        if have != want:
            raise RuntimeError(f"{path}: checksum of `{name}` is {have:#018x}, the file records {want:#018x}")
    return sd
