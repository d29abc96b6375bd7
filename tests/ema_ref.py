"""The EMA of mt_adamw_step_groups_ema (include/modaltune_hip.h) restated in numpy: the weight of a launch in double, the update as
three separately rounded float32 operations.  numpy's float32 arithmetic rounds every operation once and fuses nothing, so the kernel's
bits are reproduced exactly as long as no intermediate is subnormal (the tests draw weights ~1e-2 and gradients ~1e-3)."""
import numpy as np


def ema_decay_t(decay: float, warmup: bool, t: int) -> float:
    """The decay at optimiser step t (1-based: t = completed steps + 1), in double."""
    d = np.float64(decay)
    if warmup:
        d = min(d, (np.float64(1.0) + np.float64(t)) / (np.float64(10.0) + np.float64(t)))
    return float(d)


def ema_w(decay: float, warmup: bool, t: int) -> np.float32:
    """w = (float)(1 - decay_t): one rounding, from double."""
    return np.float32(np.float64(1.0) - np.float64(ema_decay_t(decay, warmup, t)))


def ema_ref(ema: np.ndarray, p_new: np.ndarray, decay: float, warmup: bool, t: int) -> np.ndarray:
    """d = p_new - e;  t = w * d;  e = e + t  -- float32 throughout, each operation rounded once."""
    e, p = np.asarray(ema, dtype=np.float32), np.asarray(p_new, dtype=np.float32)
    w = ema_w(decay, warmup, t)
    d = (p - e).astype(np.float32)
    s = (w * d).astype(np.float32)
    return (e + s).astype(np.float32)
