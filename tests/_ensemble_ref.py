"""Plain-torch restatement of the ensemble scores (``csrc/ensemble.hip``, ``anemoi_models_amd.losses``), for the tests: any
dtype, CPU autograd.  Evaluated in float64 it is the reference of the GPU tests; evaluated in float32 it sets their bound.

* :func:`point_score` -- ``S(x_1 .. x_E, y)`` of the three kinds (the CRPS in anemoi-training's per-pair form);
* :func:`ensemble_score` -- the kernel contract ``[..., E, G, V], [..., G, V] -> [n_groups, V]``;
* :func:`closed_form_grad` -- the gradient of the CRPS written out, the contract of ``anemoi_ensemble_score_backward``;
* :func:`loss` -- the module contract of ``AlmostFairKernelCRPS`` / ``KernelCRPS`` (``squash``, ``lead_dims``);
* :func:`metrics` -- the contract of ``EnsembleMetrics``.
"""

import math

import torch

KINDS = ("afcrps", "mean_se", "variance")


def point_score(kind, x, y, alpha=1.0):
    """``x`` ``[..., E, G, V]``, ``y`` ``[..., G, V]`` -> ``[..., G, V]``.  afcrps: ``1 / (2 E (E - 1)) sum_{j != k} (|x_j - y| +
    |x_k - y| - (1 - eps) |x_j - x_k|)``, ``eps = (1 - alpha) / E``; mean_se: ``(mean_j x_j - y)^2``; variance: ``1 / (E - 1)
    sum_j (x_j - mean)^2``."""
    e = x.shape[-3]
    if kind == "afcrps":
        eps = (1.0 - alpha) / e
        ay = (x - y.unsqueeze(-3)).abs()  # [..., E, G, V]
        pair = ay.unsqueeze(-3) + ay.unsqueeze(-4) - (1.0 - eps) * (x.unsqueeze(-3) - x.unsqueeze(-4)).abs()  # [..., E, E, G, V]
        off = 1.0 - torch.eye(e, dtype=x.dtype).reshape(e, e, 1, 1)  # j != k
        return (pair * off).sum((-3, -4)) / (2.0 * e * (e - 1))
    mean = x.mean(-3)
    if kind == "mean_se":
        return (mean - y) ** 2
    if kind == "variance":
        return ((x - mean.unsqueeze(-3)) ** 2).sum(-3) / (e - 1)
    raise ValueError(kind)


def ensemble_score(pred, target, row_w, kind, alpha=1.0, col_w=None, mask=None, diff_scale=None, n_groups=1, scale=1.0):
    """``out[l, v] = scale * sum_{b, g} keep ? row_w[g] col_w[v] S(c x_1 .. c x_E, c y) : 0`` over ``pred`` ``[..., E, G, V]`` /
    ``target`` ``[..., G, V]`` cut into ``n_groups`` equal groups along the flattened leading axes.  The mask selects the
    OPERANDS (and then the term), so that a masked NaN / Inf reaches neither the sum nor the gradient."""
    v = pred.shape[-1]
    dt = pred.dtype
    x, y = pred, target
    if mask is not None:
        zero = torch.zeros((), dtype=dt)
        x, y = torch.where(mask != 0, x, zero), torch.where(mask != 0, y, zero)
    if diff_scale is not None:
        x, y = diff_scale.to(dt) * x, diff_scale.to(dt) * y
    term = row_w.to(dt)[:, None] * point_score(kind, x, y, alpha)
    if col_w is not None:
        term = term * col_w.to(dt)
    if mask is not None:
        term = torch.where(mask != 0, term, torch.zeros((), dtype=dt))
    return scale * term.reshape(n_groups, -1, v).sum(1)


def closed_form_grad(pred, target, row_w, upstream, alpha=1.0, col_w=None, mask=None, diff_scale=None, n_groups=1, scale=1.0,
                     target_term=True):
    """``d (sum upstream * out) / d pred`` of the afcrps :func:`ensemble_score`, written out:
    ``keep ? scale * upstream[l, v] * row_w[g] * col_w[v] * |c_v| * (sgn(x_e - y) / E - (1 - eps) / (E (E - 1)) sum_k sgn(x_e -
    x_k)) : 0`` with ``sgn(0) = 0``.  ``target_term=False`` leaves ``sgn(x_e - y) / E`` out."""
    dt = pred.dtype
    e, g, v = pred.shape[-3:]
    eps = (1.0 - alpha) / e
    x = pred if mask is None else torch.where(mask != 0, pred, torch.zeros((), dtype=dt))
    y = target if mask is None else torch.where(mask != 0, target, torch.zeros((), dtype=dt))
    inner = -(1.0 - eps) / (e * (e - 1)) * torch.sign(x.unsqueeze(-3) - x.unsqueeze(-4)).sum(-3)  # sum over k of sgn(x_e - x_k)
    if target_term:
        inner = inner + torch.sign(x - y.unsqueeze(-3)) / e
    coef = scale * upstream.to(dt).reshape(n_groups, 1, 1, 1, v) * row_w.to(dt).reshape(g, 1)
    if col_w is not None:
        coef = coef * col_w.to(dt)
    if diff_scale is not None:
        coef = coef * diff_scale.to(dt).abs()
    grad = (coef * inner.reshape(n_groups, -1, e, g, v)).reshape(pred.shape)
    if mask is not None:
        grad = torch.where(mask != 0, grad, torch.zeros((), dtype=dt))
    return grad


def loss(pred, target, node_weights, variable_weights=None, mask=None, alpha=1.0, squash=True, lead_dims=0):
    """The module contract.  Per variable: summed over the grid with ``w^ = w / sum(w)``, averaged over every leading axis
    that is not kept (the ensemble axis is inside the score), times the variable weight, no ``1 / V``; ``squash``: the mean of
    that over ``V``; ``lead_dims = k`` keeps the first ``k`` axes."""
    g, v = pred.shape[-2], pred.shape[-1]
    w = node_weights.to(pred.dtype)
    w = w / w.sum()
    lead = tuple(pred.shape[:lead_dims])
    n_groups = int(math.prod(lead))
    n_avg = target.numel() // max(n_groups * g * v, 1)
    out = ensemble_score(pred, target, w, "afcrps", alpha, variable_weights, mask, None, n_groups, 1.0 / n_avg)
    out = out.reshape(lead + (v,))
    return out.mean(-1) if squash else out


def metrics(pred, target, node_weights, diff_scale=None, mask=None, alpha=1.0, groups=None):
    """``pred`` ``[n_steps, B, E, G, V]``, ``target`` ``[n_steps, B, G, V]`` -> crps, ens_rmse, spread, spread_skill ``[n_steps,
    V]`` and ``key/group`` ``[n_steps]``."""
    n_steps, b, e = pred.shape[:3]
    w = node_weights.to(pred.dtype)
    w = w / w.sum()
    red = lambda kind: ensemble_score(pred, target, w, kind, alpha, None, mask, diff_scale, n_steps, 1.0 / b)  # noqa: E731
    out = {"crps": red("afcrps"), "ens_rmse": red("mean_se").sqrt(), "spread": red("variance").sqrt()}
    out["spread_skill"] = math.sqrt((e + 1) / e) * out["spread"] / out["ens_rmse"]
    for key in list(out):
        for name, cols in (groups or {}).items():
            out[f"{key}/{name}"] = out[key][:, cols].mean(-1)
    return out
