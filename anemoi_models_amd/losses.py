"""Training losses and validation metrics on the HIP kernels.

``WeightedMSELoss`` is anemoi-training's node-weighted, variable-scaled MSE with the imputers' loss mask: one deterministic
reduction kernel forward (``anemoi_weighted_mse``), one element-wise kernel backward -- no atomics, the same bits on every run,
like the rest of the training path.

``WeightedMAELoss``, ``WeightedHuberLoss``, ``WeightedLogCoshLoss`` and ``WeightedRMSELoss`` -- and every loss with
``squash=False`` or ``lead_dims > 0`` -- run on the per-variable reduction ``anemoi_weighted_error`` (``[rows, V] -> [groups,
V]``, as deterministic); ``ValidationMetrics`` reports the same reductions in physical units per variable, variable group and
rollout step, one launch pair per kind.

``AlmostFairKernelCRPS`` / ``KernelCRPS`` are the ensemble objectives (``pred`` carries an ensemble axis, ``target`` none) on
``anemoi_ensemble_score``; ``EnsembleMetrics`` reports CRPS, ensemble-mean RMSE, spread and the spread/skill ratio from three
launches of the same kernel."""

from __future__ import annotations

import math
from typing import Mapping
from typing import Optional
from typing import Sequence

import torch
from torch import Tensor
from torch import nn

from . import autograd


def _normalised_node_weights(name: str, node_weights) -> Tensor:
    """``w / sum(w)`` as float32, for the class ``name``."""
    w = torch.as_tensor(node_weights).detach().double().reshape(-1)
    if w.numel() == 0 or not bool((w >= 0).all()) or float(w.sum()) <= 0:
        raise ValueError(f"{name}: node_weights must be non-negative with a positive sum")
    return (w / w.sum()).float()


class _NodeWeightedLoss(nn.Module):
    """Node weights ``w^ = w / sum(w)``, optional per-variable weights, and the per-variable form shared by the family."""

    kind = "mse"
    delta = 1.0

    def __init__(self, node_weights: Tensor, variable_weights: Optional[Tensor] = None) -> None:
        super().__init__()
        self.register_buffer("node_weights", _normalised_node_weights(type(self).__name__, node_weights), persistent=False)
        s = None if variable_weights is None else torch.as_tensor(variable_weights).detach().float().reshape(-1).clone()
        self.register_buffer("variable_weights", s, persistent=False)

    def _check(self, pred: Tensor, mask: Optional[Tensor]):
        name = type(self).__name__
        g, v = self.node_weights.numel(), pred.shape[-1]
        if pred.dim() < 2 or pred.shape[-2] != g:
            raise ValueError(f"{name}: pred {tuple(pred.shape)} does not end in [G = {g}, V]")
        s = self.variable_weights
        if s is not None and s.numel() != v:
            raise ValueError(f"{name}: {s.numel()} variable weights for {v} variables")
        if mask is not None and tuple(mask.shape) != (g, v):
            raise ValueError(f"{name}: mask must be [G = {g}, V = {v}], got {tuple(mask.shape)}")
        return g, v

    def per_variable(self, pred: Tensor, target: Tensor, mask: Optional[Tensor] = None, lead_dims: int = 0) -> Tensor:
        """``[*pred.shape[:lead_dims], V]``: summed over the grid, averaged over the leading axes that are not kept, variable
        weights applied, no ``1 / V`` -- anemoi-training's ``squash=False`` contract."""
        g, v = self._check(pred, mask)
        if not 0 <= lead_dims <= pred.dim() - 2:
            raise ValueError(f"{type(self).__name__}: lead_dims = {lead_dims} of a pred with {pred.dim() - 2} leading axes")
        lead = tuple(pred.shape[:lead_dims])
        n_groups = math.prod(lead)
        if n_groups == 0:
            return torch.zeros(lead + (v,), dtype=torch.float32, device=pred.device)
        n_avg = pred.numel() // max(n_groups * g * v, 1)
        s = self.variable_weights
        out = autograd.weighted_error(pred, target, self.node_weights.to(pred.device), self.kind, delta=self.delta,
                                      col_w=None if s is None else s.to(pred.device), mask=mask, n_groups=n_groups,
                                      scale=1.0 / max(n_avg, 1))
        return out.reshape(lead + (v,))

    def forward(self, pred: Tensor, target: Tensor, mask: Optional[Tensor] = None, squash: bool = True,
                lead_dims: int = 0) -> Tensor:
        out = self.per_variable(pred, target, mask, lead_dims)
        return out.mean(-1) if squash else out


class WeightedMSELoss(_NodeWeightedLoss):
    """``loss = 1 / (n_lead * V) * sum w^_g * s_v * keep * (pred - target)^2`` over ``pred`` ``[..., G, V]``: ``w^ = w /
    sum(w)`` the normalised node (area) weights, ``s`` the per-variable scaling (``None``: ones), ``n_lead`` the product of
    the leading dimensions (batch, ensemble, and a leading rollout axis where there is one) -- the node-weighted,
    variable-scaled squared error summed over the grid and averaged over the variables and every leading axis.

    ``mask`` ``[G, V]`` is an imputer's ``loss_mask_training`` as it is (1 = observed, 0 = imputed): masked values contribute
    exactly 0 to the loss and receive exactly 0 gradient, even where the target is NaN there."""

    def forward(self, pred: Tensor, target: Tensor, mask: Optional[Tensor] = None, squash: bool = True,
                lead_dims: int = 0) -> Tensor:
        """``squash=False``: the per-variable values ``[V]`` (no ``1 / V``); ``lead_dims = k``: the first ``k`` axes of ``pred``
        stay unreduced.  With the defaults: the scalar of the class docstring, on ``anemoi_weighted_mse`` as ever."""
        if not squash or lead_dims != 0:
            return super().forward(pred, target, mask, squash, lead_dims)
        g, v = self._check(pred, mask)
        s = self.variable_weights
        if s is None:
            s = torch.ones(v, dtype=torch.float32, device=pred.device)
        n_lead = pred.numel() // max(g * v, 1)
        return autograd.weighted_mse(pred, target, self.node_weights.to(pred.device), s.to(pred.device), mask,
                                     1.0 / (max(n_lead, 1) * v))


class WeightedMAELoss(_NodeWeightedLoss):
    """:class:`WeightedMSELoss` with ``|pred - target|`` for the square; the gradient is ``sign(pred - target)``, 0 where
    the two are equal (torch's convention)."""

    kind = "mae"


class WeightedHuberLoss(_NodeWeightedLoss):
    """:class:`WeightedMSELoss` with the Huber function: ``0.5 d^2`` for ``|d| <= delta``, ``delta (|d| - 0.5 delta)``
    beyond."""

    kind = "huber"

    def __init__(self, node_weights: Tensor, variable_weights: Optional[Tensor] = None, delta: float = 1.0) -> None:
        super().__init__(node_weights, variable_weights)
        if not float(delta) > 0:
            raise ValueError(f"WeightedHuberLoss: delta must be positive, got {delta}")
        self.delta = float(delta)


class WeightedLogCoshLoss(_NodeWeightedLoss):
    """:class:`WeightedMSELoss` with ``log cosh d`` for the square, in the overflow-free form ``|d| + log1p(exp(-2 |d|)) -
    ln 2``; the gradient is ``tanh d``."""

    kind = "logcosh"


class WeightedRMSELoss(_NodeWeightedLoss):
    """The square root of :class:`WeightedMSELoss`: per variable with ``squash=False``, of the squashed value with
    ``squash=True``.  The square root is plain torch on the small result; its gradient reaches the kernel as the upstream
    gradient."""

    kind = "mse"

    def forward(self, pred: Tensor, target: Tensor, mask: Optional[Tensor] = None, squash: bool = True,
                lead_dims: int = 0) -> Tensor:
        return super().forward(pred, target, mask, squash, lead_dims).sqrt()


METRIC_KINDS = ("mse", "mae", "huber", "logcosh", "rmse")


def _output_diff_scale(name: str, normalizer, n_vars: Optional[int] = None) -> Optional[Tensor]:
    """``1 / _norm_mul`` at the model-output variables of an ``InputNormalizer`` (or of a ``Processors`` container that holds
    nothing else): the scale that takes a difference of normalised values to physical units.  ``name``: the calling class."""
    from .preprocessing import Processors
    from .preprocessing.normalizer import InputNormalizer

    if normalizer is None:
        return None
    procs = list(normalizer.processors.values()) if isinstance(normalizer, Processors) else [normalizer]
    other = [type(p).__name__ for p in procs if not isinstance(p, InputNormalizer)]
    if other or len(procs) != 1:
        raise NotImplementedError(
            f"{name}: only one affine InputNormalizer can be folded into the metric kernel (its additive term "
            f"cancels in pred - target); got {[type(p).__name__ for p in procs]} -- an imputer or remapper is not affine")
    norm = procs[0]
    mul = norm._norm_mul.detach().double()
    if n_vars is None or n_vars == norm._output_idx.numel():
        mul = mul[norm._output_idx.long()]
    elif n_vars != mul.numel():
        raise ValueError(f"{name}: {n_vars} variables, the normaliser has {norm._output_idx.numel()} output and "
                         f"{mul.numel()} data variables")
    if bool((mul == 0).any()) or not bool(torch.isfinite(mul).all()):
        raise ValueError(f"{name}: the normaliser has a zero or non-finite _norm_mul: it cannot be inverted")
    return (1.0 / mul).float()


class _PhysicalMetrics(nn.Module):
    """What the metrics classes share: normalised node weights, ``1 / _norm_mul`` of the normaliser as the kernel's per-variable
    scale of the difference, and the variable groups with their means."""

    def __init__(self, node_weights: Tensor, normalizer, groups: Optional[Mapping[str, Sequence[int]]]) -> None:
        super().__init__()
        name = type(self).__name__
        self.register_buffer("node_weights", _normalised_node_weights(name, node_weights), persistent=False)
        self.register_buffer("diff_scale", _output_diff_scale(name, normalizer), persistent=False)
        self.groups = {str(k): [int(i) for i in idx] for k, idx in (groups or {}).items()}
        if any(len(idx) == 0 for idx in self.groups.values()):
            raise ValueError(f"{name}: an empty variable group")

    def _diff_scale_for(self, v: int, device) -> Optional[Tensor]:
        """``diff_scale`` on ``device``, after the per-call checks against the ``v`` variables of a ``pred``."""
        name, c = type(self).__name__, self.diff_scale
        if c is not None and c.numel() != v:
            raise ValueError(f"{name}: {v} variables, the normaliser has {c.numel()} output variables")
        if any(i < 0 or i >= v for idx in self.groups.values() for i in idx):
            raise ValueError(f"{name}: a group index is not one of the {v} output variables")
        return None if c is None else c.to(device)

    def _add_group_means(self, out: dict, key: str) -> None:
        for name, idx in self.groups.items():
            out[f"{key}/{name}"] = out[key][:, idx].mean(-1)


class ValidationMetrics(_PhysicalMetrics):
    """Per-variable validation metrics in physical (de-normalised) units for every rollout step.

    ``forward(pred, target, mask=None)`` takes the normalised ``[n_steps, B, Ens, G, V]`` model output and target (or ``[B,
    Ens, G, V]``: one step) and returns ``{kind: [n_steps, V]}`` -- the node-weighted (``w^ = w / sum(w)``) error of kind
    ``kind`` summed over the grid and averaged over batch and ensemble, of ``(pred - target) / _norm_mul`` -- and, with
    ``groups`` (name -> indices of output variables), ``{kind/name: [n_steps]}``, the mean over the group's variables.  One
    launch pair per kind and no de-normalised copy of either operand: the normaliser is affine, so its additive term cancels in
    the difference and ``1 / _norm_mul`` enters the kernel as the per-variable scale of the difference.  ``kinds`` from mse,
    mae, huber (``delta`` in physical units), logcosh, rmse (the square root of mse, per variable).  Runs without autograd."""

    def __init__(self, node_weights: Tensor, normalizer=None, groups: Optional[Mapping[str, Sequence[int]]] = None,
                 kinds: Sequence[str] = ("mse",), delta: float = 1.0) -> None:
        super().__init__(node_weights, normalizer, groups)
        bad = [k for k in kinds if k not in METRIC_KINDS]
        if bad or not kinds:
            raise ValueError(f"ValidationMetrics: unknown kinds {bad} (from {METRIC_KINDS})")
        if not float(delta) > 0:
            raise ValueError(f"ValidationMetrics: delta must be positive, got {delta}")
        self.kinds, self.delta = tuple(kinds), float(delta)

    @torch.no_grad()
    def forward(self, pred: Tensor, target: Tensor, mask: Optional[Tensor] = None) -> dict:
        if pred.dim() == 4:
            pred, target = pred[None], target[None]
        g = self.node_weights.numel()
        if pred.dim() != 5 or pred.shape != target.shape or pred.shape[-2] != g:
            raise ValueError(f"ValidationMetrics: pred {tuple(pred.shape)} / target {tuple(target.shape)} must be "
                             f"[n_steps, B, Ens, G = {g}, V] (or without the step axis)")
        n_steps, v = pred.shape[0], pred.shape[-1]
        c = self._diff_scale_for(v, pred.device)
        n_avg = max(pred.shape[1] * pred.shape[2], 1)
        out = {}
        for kind in self.kinds:
            per_var = autograd.weighted_error(pred, target, self.node_weights.to(pred.device),
                                              "mse" if kind == "rmse" else kind, delta=self.delta, mask=mask,
                                              diff_scale=c, n_groups=n_steps, scale=1.0 / n_avg)
            if kind == "rmse":
                per_var = per_var.sqrt()
            out[kind] = per_var
            self._add_group_means(out, kind)
        return out


class AlmostFairKernelCRPS(_NodeWeightedLoss):
    """The almost-fair kernel CRPS of AIFS-CRPS over ``pred`` ``[..., E, G, V]`` and ``target`` ``[..., G, V]`` (the same
    leading axes; the target has no ensemble axis): per point and variable

    ``1/E sum_j |x_j - y| - (1 - eps) / (2 E (E - 1)) sum_{j != k} |x_j - x_k|``, ``eps = (1 - alpha) / E``

    (``alpha = 1``: the fair CRPS, ``alpha = 0``: the ensemble CRPS with ``1 / (2 E^2)``), reduced as the family reduces:
    summed over the grid with ``w^ = w / sum(w)``, averaged over the leading axes that are not kept, variable weights applied;
    ``squash=False`` returns the per-variable values without ``1 / V``.  ``2 <= E <= 16``.  ``mask`` ``[G, V]`` is a select: a
    masked point contributes exactly 0 and its members receive exactly 0 gradient.  The gradient of ``|.|`` at 0 is 0; the
    target gets no gradient."""

    kind = "afcrps"

    def __init__(self, node_weights: Tensor, variable_weights: Optional[Tensor] = None, alpha: float = 1.0) -> None:
        super().__init__(node_weights, variable_weights)
        if not 0.0 <= float(alpha) <= 1.0:
            raise ValueError(f"{type(self).__name__}: alpha must lie in [0, 1], got {alpha}")
        self.alpha = float(alpha)

    def per_variable(self, pred: Tensor, target: Tensor, mask: Optional[Tensor] = None, lead_dims: int = 0) -> Tensor:
        """``[*pred.shape[:lead_dims], V]``; ``lead_dims <= pred.dim() - 3``: the ensemble axis is never a kept axis."""
        name = type(self).__name__
        g, v = self._check(pred, mask)
        if pred.dim() < 3:
            raise ValueError(f"{name}: pred {tuple(pred.shape)} must be [..., E, G = {g}, V]")
        if not 0 <= lead_dims <= pred.dim() - 3:
            raise ValueError(f"{name}: lead_dims = {lead_dims} of a pred with {pred.dim() - 3} leading axes before the "
                             f"ensemble axis")
        if tuple(target.shape) != tuple(pred.shape[:-3]) + (g, v):
            raise ValueError(f"{name}: target {tuple(target.shape)} must be pred {tuple(pred.shape)} without the ensemble axis")
        if target.requires_grad:
            raise ValueError(f"{name}: the target requires a gradient, and the ensemble scores have none for it")
        lead = tuple(pred.shape[:lead_dims])
        n_groups = math.prod(lead)
        if n_groups == 0:
            return torch.zeros(lead + (v,), dtype=torch.float32, device=pred.device)
        n_avg = target.numel() // max(n_groups * g * v, 1)
        s = self.variable_weights
        out = autograd.ensemble_score(pred, target, self.node_weights.to(pred.device), self.kind, alpha=self.alpha,
                                      col_w=None if s is None else s.to(pred.device), mask=mask, n_groups=n_groups,
                                      scale=1.0 / max(n_avg, 1))
        return out.reshape(lead + (v,))


class KernelCRPS(AlmostFairKernelCRPS):
    """:class:`AlmostFairKernelCRPS` at its two ends: ``fair=True`` is ``alpha = 1`` (pair coefficient ``1 / (2 E (E - 1))``),
    ``fair=False`` is ``alpha = 0`` (``1 / (2 E^2)``)."""

    def __init__(self, node_weights: Tensor, variable_weights: Optional[Tensor] = None, fair: bool = True) -> None:
        super().__init__(node_weights, variable_weights, alpha=1.0 if fair else 0.0)
        self.fair = bool(fair)


class EnsembleMetrics(_PhysicalMetrics):
    """Per-variable ensemble scores in physical (de-normalised) units for every rollout step.

    ``forward(pred, target, mask=None)`` takes the normalised ``[n_steps, B, E, G, V]`` ensemble and its ``[n_steps, B, G, V]``
    target (or both without the step axis) and returns ``[n_steps, V]`` each of

    * ``crps``: the almost-fair kernel CRPS (``alpha``), node-weighted (``w^ = w / sum(w)``), averaged over the batch;
    * ``ens_rmse``: the square root of the same reduction of ``(mean_j x_j - y)^2``;
    * ``spread``: the square root of the same reduction of the ensemble variance ``1 / (E - 1) sum_j (x_j - mean)^2``;
    * ``spread_skill``: ``sqrt((E + 1) / E) * spread / ens_rmse`` (1 for a statistically consistent ensemble),

    and with ``groups`` (name -> indices of output variables) ``{key/name: [n_steps]}``, the mean of the per-variable values
    over the group's variables.  Three launches of one kernel and no de-normalised copy: ``1 / _norm_mul`` of the (affine)
    ``InputNormalizer`` enters as the per-variable scale, as in :class:`ValidationMetrics`.  Runs without autograd."""

    KEYS = ("crps", "ens_rmse", "spread", "spread_skill")

    def __init__(self, node_weights: Tensor, normalizer=None, groups: Optional[Mapping[str, Sequence[int]]] = None,
                 alpha: float = 1.0) -> None:
        super().__init__(node_weights, normalizer, groups)
        if not 0.0 <= float(alpha) <= 1.0:
            raise ValueError(f"EnsembleMetrics: alpha must lie in [0, 1], got {alpha}")
        self.alpha = float(alpha)

    @torch.no_grad()
    def forward(self, pred: Tensor, target: Tensor, mask: Optional[Tensor] = None) -> dict:
        if pred.dim() == 4:
            pred, target = pred[None], target[None]
        g = self.node_weights.numel()
        if pred.dim() != 5 or target.dim() != 4 or pred.shape[-2] != g \
                or tuple(target.shape) != tuple(pred.shape[:2]) + tuple(pred.shape[3:]):
            raise ValueError(f"EnsembleMetrics: pred {tuple(pred.shape)} / target {tuple(target.shape)} must be "
                             f"[n_steps, B, E, G = {g}, V] / [n_steps, B, G, V] (or both without the step axis)")
        n_steps, e, v = pred.shape[0], pred.shape[2], pred.shape[-1]
        kw = dict(alpha=self.alpha, mask=mask, diff_scale=self._diff_scale_for(v, pred.device), n_groups=n_steps,
                  scale=1.0 / max(pred.shape[1], 1))
        w = self.node_weights.to(pred.device)
        out = {"crps": autograd.ensemble_score(pred, target, w, "afcrps", **kw),
               "ens_rmse": autograd.ensemble_score(pred, target, w, "mean_se", **kw).sqrt(),
               "spread": autograd.ensemble_score(pred, target, w, "variance", **kw).sqrt()}
        out["spread_skill"] = math.sqrt((e + 1) / e) * out["spread"] / out["ens_rmse"]
        for key in self.KEYS:
            self._add_group_means(out, key)
        return out
