"""Training losses on the HIP kernels.

``WeightedMSELoss`` is anemoi-training's node-weighted, variable-scaled MSE with the imputers' loss mask: one deterministic
reduction kernel forward (``anemoi_weighted_mse``), one element-wise kernel backward -- no atomics, the same bits on every run,
like the rest of the training path."""

from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor
from torch import nn

from . import autograd


class WeightedMSELoss(nn.Module):
    """``loss = 1 / (n_lead * V) * sum w^_g * s_v * keep * (pred - target)^2`` over ``pred`` ``[..., G, V]``: ``w^ = w /
    sum(w)`` the normalised node (area) weights, ``s`` the per-variable scaling (``None``: ones), ``n_lead`` the product of
    the leading dimensions (batch, ensemble, and a leading rollout axis where there is one) -- the node-weighted,
    variable-scaled squared error summed over the grid and averaged over the variables and every leading axis.

    ``mask`` ``[G, V]`` is an imputer's ``loss_mask_training`` as it is (1 = observed, 0 = imputed): masked values contribute
    exactly 0 to the loss and receive exactly 0 gradient, even where the target is NaN there."""

    def __init__(self, node_weights: Tensor, variable_weights: Optional[Tensor] = None) -> None:
        super().__init__()
        w = torch.as_tensor(node_weights).detach().double().reshape(-1)
        if w.numel() == 0 or not bool((w >= 0).all()) or float(w.sum()) <= 0:
            raise ValueError("WeightedMSELoss: node_weights must be non-negative with a positive sum")
        self.register_buffer("node_weights", (w / w.sum()).float(), persistent=False)
        s = None if variable_weights is None else torch.as_tensor(variable_weights).detach().float().reshape(-1).clone()
        self.register_buffer("variable_weights", s, persistent=False)

    def forward(self, pred: Tensor, target: Tensor, mask: Optional[Tensor] = None) -> Tensor:
        g, v = self.node_weights.numel(), pred.shape[-1]
        if pred.dim() < 2 or pred.shape[-2] != g:
            raise ValueError(f"WeightedMSELoss: pred {tuple(pred.shape)} does not end in [G = {g}, V]")
        s = self.variable_weights
        if s is None:
            s = torch.ones(v, dtype=torch.float32, device=pred.device)
        elif s.numel() != v:
            raise ValueError(f"WeightedMSELoss: {s.numel()} variable weights for {v} variables")
        if mask is not None and tuple(mask.shape) != (g, v):
            raise ValueError(f"WeightedMSELoss: mask must be [G = {g}, V = {v}], got {tuple(mask.shape)}")
        n_lead = pred.numel() // max(g * v, 1)
        return autograd.weighted_mse(pred, target, self.node_weights.to(pred.device), s.to(pred.device), mask,
                                     1.0 / (max(n_lead, 1) * v))
