"""The f64 restatement of ``csrc/average.hip`` (DESIGN.md section 7 "8f-11") and the bounds its tests hold the kernels to.

The update.  The kernel computes ``s' = fmaf(fl(p - s), w, s)`` in correctly rounded f32: two roundings.  With ``u = 2^-24``,
``fl(p - s) = (p - s)(1 + e1)`` and ``s' = (fl(p - s) w + s)(1 + e2)``, ``|e1|, |e2| <= u``, so against
``ref = s + (p - s) w`` evaluated in f64 from the same f32 inputs

    |s' - ref| <= u w |p - s| + u |ref| + u^2 w |p - s|  <=  1.01 u (w |p - s| + |ref|).

Nothing is fitted: the 1.01 covers the second-order term and the f64 evaluation of ``ref``.  The copy (``n == 0``) and the
swap move bit patterns and are exact.  A chain of updates propagates the error of the stored average through ``(1 - w)``:
``E' = |1 - w| E + bound``, because the update is affine in ``s`` with slope ``1 - w``.

The scalars.  ``w`` is evaluated in f64 and rounded once to f32.  ``1 - decay`` is one IEEE subtraction: the device and this
file get the same f64 and therefore the same f32 -- exact.  The warm-up ``(1 + n) / (10 + n)`` and the SWA ``1 / (n + 1)`` hold
an f64 division; a device division that is off by one f64 ulp can straddle an f32 rounding boundary, so these are held to one
f32 ulp (and are expected to be exact).  ``n_after = n + 1`` is exact while ``n < 2^24``.

The schedule is evaluated in f64 and rounded once; the device's ``cos`` is good to a few f64 ulp, so the f32 result is within
one f32 ulp of this file's value rounded to f32 wherever the cancellation in ``1 + cos`` has not eaten the margin: an error of
2^-52 in ``cos`` against ``1 + cos = (pi (T - tc) / T)^2 / 2`` stays below 2^-25 relative while ``(T - tc) / T > 4e-5``, that is for
every integer ``tc < T`` while ``total_steps < 25 000`` (the tests use far less; beyond, the last steps of a decay to
``lr_min = 0`` may be two ulp off, of a rate that is itself below ``1e-9 base``).
"""

import math

import numpy as np
import torch

U = 2.0 ** -24
EMA, SWA = "ema", "swa"


def f32(x: float) -> float:
    return float(np.float32(x))


def ulp32(x: float) -> float:
    """The spacing of f32 at |x| (the smallest subnormal at 0)."""
    return float(np.spacing(np.float32(abs(x))))


def weight(kind: str, n: float, decay: float = 0.999, warmup: bool = False) -> float:
    """The f64 weight of the update that finds ``n`` earlier updates (``n == 0``: the copy, weight 1)."""
    if n == 0:
        return 1.0
    if kind == SWA:
        return 1.0 / (n + 1.0)
    d = min(decay, (1.0 + n) / (10.0 + n)) if warmup else decay
    return 1.0 - d


def weight_is_exact(kind: str, n: float, warmup: bool) -> bool:
    """Whether the f32 weight must equal ``f32(weight(...))`` bit for bit (no f64 division on its path)."""
    return n == 0 or (kind == EMA and not warmup)


def constants(n: float, kind: str = EMA, decay: float = 0.999, warmup: bool = False, start_step: int = 0, every: int = 1,
              t=None, skip: bool = False) -> dict:
    """The block of ``anemoi_average_constants``: w (f64, unrounded), active, copy, n_after."""
    active = not skip and (t is None or (t >= start_step and (int(t) - start_step) % every == 0))
    if not active:
        return dict(w=0.0, active=False, copy=False, n_after=float(n))
    return dict(w=weight(kind, n, decay, warmup), active=True, copy=n == 0, n_after=float(n) + 1.0)


def update(p: torch.Tensor, s: torch.Tensor, w: float, copy: bool = False):
    """(ref, bound) of one update per element in f64; ``w`` as the device rounded it (or exact, for an f64 chain)."""
    p, s = p.detach().double().cpu(), s.detach().double().cpu()
    if copy:
        return p.clone(), torch.zeros_like(p)
    ref = s + (p - s) * w
    return ref, 1.01 * U * (abs(w) * (p - s).abs() + ref.abs())


def chain(ps, kind: str = EMA, decay: float = 0.999, warmup: bool = False, rounded: bool = True):
    """The average after the updates ``ps[0], ps[1], ...`` (a list of tensors) from ``n = 0`` in f64, with the chained bound
    of the f32 kernel: ``E' = |1 - w| E + bound``.  ``rounded``: the weights as f32 (what the kernel uses)."""
    s, err = None, None
    for n, p in enumerate(ps):
        w = weight(kind, float(n), decay, warmup)
        w = f32(w) if rounded else w
        if n == 0:
            s, err = update(p, p, w, copy=True)
        else:
            prev = err
            s, err = update(p, s, w)
            err = abs(1.0 - w) * prev + err
    return s, err


def lr(t: int, base: float, warmup_steps: int, total_steps: int, lr_min: float = 0.0, warmup_start: float = 0.0,
       warmup_prefix: bool = False) -> float:
    """The closed form of ``anemoi_lr_schedule`` at ``t`` completed steps, in f64."""
    if t < warmup_steps:
        return warmup_start + t * (base - warmup_start) / warmup_steps
    tc = t - warmup_steps if warmup_prefix else t
    if tc < total_steps:
        return lr_min + 0.5 * (base - lr_min) * (1.0 + math.cos(math.pi * tc / total_steps))
    return lr_min
