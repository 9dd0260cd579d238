"""Plain-torch restatement of the loss family (``csrc/losses.hip``, ``anemoi_models_amd.losses``), for the tests: any dtype,
CPU autograd.  Evaluated in float64 it is the reference of the GPU tests; evaluated in float32 it sets their bound.

* :func:`pointwise` -- ``f(d)`` of the four kinds;
* :func:`weighted_error` -- the kernel contract ``[..., G, V] -> [n_groups, V]``;
* :func:`loss` -- the module contract of ``Weighted{MSE,MAE,Huber,LogCosh,RMSE}Loss`` (``squash``, ``lead_dims``).
"""

import math

import torch

KINDS = ("mse", "mae", "huber", "logcosh")


def pointwise(kind, d, delta=1.0):
    """``f(d)``: d^2 | |d| | 0.5 d^2 if |d| <= delta else delta (|d| - 0.5 delta) | |d| + log1p(exp(-2 |d|)) - ln 2."""
    if kind == "mse":
        return d * d
    a = d.abs()
    if kind == "mae":
        return a
    if kind == "huber":
        return torch.where(a <= delta, 0.5 * d * d, delta * (a - 0.5 * delta))
    if kind == "logcosh":
        return a + torch.log1p(torch.exp(-2.0 * a)) - math.log(2.0)
    raise ValueError(kind)


def weighted_error(pred, target, row_w, kind, delta=1.0, col_w=None, mask=None, diff_scale=None, n_groups=1, scale=1.0):
    """``out[l, v] = scale * sum_{r in group l} keep ? row_w[g] col_w[v] f(c[v] (pred - target)) : 0`` over ``pred`` ``[..., G,
    V]`` cut into ``n_groups`` equal groups of consecutive rows.  The mask selects the DIFFERENCE, so that a masked NaN reaches
    neither the sum nor the gradient."""
    g, v = pred.shape[-2], pred.shape[-1]
    dt = pred.dtype
    d = pred - target
    if mask is not None:
        d = torch.where(mask != 0, d, torch.zeros((), dtype=dt))
    if diff_scale is not None:
        d = diff_scale.to(dt) * d
    term = row_w.to(dt)[:, None] * pointwise(kind, d, delta)
    if col_w is not None:
        term = term * col_w.to(dt)
    if mask is not None:  # (f(0) is 0 for every kind; the select keeps the exact zero explicit)
        term = torch.where(mask != 0, term, torch.zeros((), dtype=dt))
    return scale * term.reshape(n_groups, -1, v).sum(1)


def loss(kind, pred, target, node_weights, variable_weights=None, mask=None, delta=1.0, squash=True, lead_dims=0):
    """The module contract.  Per variable: summed over the grid with ``w^ = w / sum(w)``, averaged over every leading axis
    that is not kept, times the variable weight, no ``1 / V``; ``squash``: the mean of that over ``V``; ``lead_dims = k`` keeps
    the first ``k`` axes.  ``kind = "rmse"``: the square root of the mse result -- per variable, or of the squashed value."""
    g = pred.shape[-2]
    w = node_weights.to(pred.dtype)
    w = w / w.sum()
    lead = tuple(pred.shape[:lead_dims])
    n_groups = int(math.prod(lead))
    n_avg = pred.numel() // max(n_groups * g * pred.shape[-1], 1)
    out = weighted_error(pred, target, w, "mse" if kind == "rmse" else kind, delta, variable_weights, mask, None, n_groups,
                         1.0 / n_avg)
    out = out.reshape(lead + (pred.shape[-1],))
    if squash:
        out = out.mean(-1)
    return out.sqrt() if kind == "rmse" else out
