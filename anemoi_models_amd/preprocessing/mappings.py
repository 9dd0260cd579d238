"""The converters of the remappers, mirroring reference preprocessing/mappings.py:13-75 (same function names): each maps a
column of a tensor, or for ``atan2_converter`` a ``[..., 2]`` pair of columns, and is the exact inverse of its partner.

The Box-Cox pair exists for ``lambd = 0.5`` only, where the power is a square root and a square: ``(sqrt(x) - 1) / 0.5`` and
``(0.5 x + 1) ** 2`` (the reference evaluates ``torch.pow`` with these two exponents).  Other values raise ``ValueError``."""

from __future__ import annotations

import math

import torch
from torch import Tensor


def noop(x):
    return x


def cos_converter(x: Tensor) -> Tensor:
    """Angle in degrees -> its cosine."""
    return torch.cos(x / 180 * math.pi)


def sin_converter(x: Tensor) -> Tensor:
    """Angle in degrees -> its sine."""
    return torch.sin(x / 180 * math.pi)


def atan2_converter(x: Tensor) -> Tensor:
    """``x[..., 0]`` = cosine, ``x[..., 1]`` = sine -> the angle in degrees, in ``[0, 360)``."""
    return torch.remainder(torch.atan2(x[..., 1], x[..., 0]) * 180 / math.pi, 360)


def log1p_converter(x: Tensor) -> Tensor:
    return torch.log1p(x)


def expm1_converter(x: Tensor) -> Tensor:
    return torch.expm1(x)


def sqrt_converter(x: Tensor) -> Tensor:
    return torch.sqrt(x)


def square_converter(x: Tensor) -> Tensor:
    return x**2


def _half_only(lambd: float) -> None:
    if lambd != 0.5:
        raise ValueError(f"the Box-Cox converters are defined for lambd = 0.5 only, got {lambd}")


def boxcox_converter(x: Tensor, lambd: float = 0.5) -> Tensor:
    _half_only(lambd)
    return (torch.sqrt(x) - 1) / lambd


def inverse_boxcox_converter(x: Tensor, lambd: float = 0.5) -> Tensor:
    _half_only(lambd)
    return (x * lambd + 1) ** 2
