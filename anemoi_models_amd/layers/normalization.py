"""Normalisation layers of the ensemble model: a LayerNorm whose scale and shift are linear in a per-row condition.

A restatement, not a port: the reference checkout this package mirrors predates anemoi-models' ensemble model, so the layer is
written from the published description of AIFS-CRPS (a LayerNorm without affine parameters, then ``scale`` and ``bias`` Linears
of the noise embedding) with the parameter names anemoi-models is known to use.
"""

from __future__ import annotations

import torch
from torch import Tensor
from torch import nn

from .. import ops
from .. import runtime


class ConditionalLayerNorm(nn.Module):
    """``xhat(x) * (1 + scale(cond)) + bias(cond)`` over the last dimension: ``scale`` and ``bias`` are ``nn.Linear(condition_shape,
    normalized_shape)`` (state dict ``scale.weight``, ``scale.bias``, ``bias.weight``, ``bias.bias``), zero-initialised by
    default, so that a fresh layer is a LayerNorm without affine parameters.  ``x`` is ``[rows, normalized_shape]`` in the compute
    dtype, ``cond`` ``[rows, condition_shape]``; one fused HIP row kernel each way (``anemoi_cond_layer_norm``) for a condition of
    at most 32 columns, composed from a Linear and a LayerNorm beyond."""

    def __init__(self, normalized_shape: int, condition_shape: int, zero_init: bool = True, eps: float = 1e-5) -> None:
        super().__init__()
        self.normalized_shape, self.condition_shape, self.eps = int(normalized_shape), int(condition_shape), float(eps)
        self.scale = nn.Linear(self.condition_shape, self.normalized_shape)
        self.bias = nn.Linear(self.condition_shape, self.normalized_shape)
        if zero_init:
            for lin in (self.scale, self.bias):
                nn.init.zeros_(lin.weight)
                nn.init.zeros_(lin.bias)

    def _args(self):
        return self.scale.weight, self.scale.bias, self.bias.weight, self.bias.bias

    def native(self, x: Tensor, cond: Tensor) -> Tensor:
        """Without an autograd graph, on the forward kernel alone."""
        from .. import autograd

        if not autograd.cond_layer_norm_fused(self.condition_shape):
            with torch.no_grad():
                return autograd.cond_layer_norm_composed(x, cond, *self._args(), self.eps)
        return ops.cond_layer_norm(x, cond, *(runtime.f32c(t) for t in self._args()), self.eps)

    def forward(self, x: Tensor, cond: Tensor) -> Tensor:
        if x.dim() != 2 or cond.dim() != 2 or cond.shape[0] != x.shape[0] or cond.shape[1] != self.condition_shape:
            raise ValueError(f"ConditionalLayerNorm: x {tuple(x.shape)} / cond {tuple(cond.shape)}: expected [rows, "
                             f"{self.normalized_shape}] and [rows, {self.condition_shape}]")
        if torch.is_grad_enabled() and (x.requires_grad or cond.requires_grad or any(p.requires_grad for p in self.parameters())):
            from .. import autograd

            return autograd.cond_layer_norm(x, cond, *self._args(), self.eps)
        return self.native(x, cond)
