"""Plain-torch restatements of the rollout training pieces, for the tests: any dtype, CPU autograd.

* :func:`weighted_mse` -- the loss contract of ``anemoi_models_amd.losses.WeightedMSELoss``;
* :func:`advance` -- the state advance as ``roll`` + index writes, as in ``oracle.reference_path.rollout``;
* :func:`rollout` -- a normalised-space rollout on ``oracle.reference_path.model_forward``.
"""

import torch

from oracle import reference_path as ref


def weighted_mse(pred, target, node_weights, variable_weights=None, mask=None):
    """``1 / (n_lead * V) * sum w^_g s_v keep (pred - target)^2`` over ``pred`` ``[..., G, V]``, ``w^ = w / sum(w)``.  The mask
    selects the DIFFERENCE (not the product), so that a masked NaN neither reaches the sum nor the gradient."""
    g, v = pred.shape[-2], pred.shape[-1]
    w = node_weights.to(pred.dtype)
    w = w / w.sum()
    s = torch.ones(v, dtype=pred.dtype) if variable_weights is None else variable_weights.to(pred.dtype)
    d = pred - target
    if mask is not None:
        d = torch.where(mask != 0, d, torch.zeros((), dtype=pred.dtype))
    n_lead = pred.numel() // (g * v)
    return (w[:, None] * s[None, :] * d * d).sum() / (n_lead * v)


def advance(x, y, colmap, forcing=None):
    """Next input ``[B, T, Ens, G, V_in]`` from the current one and the prediction ``y`` ``[B, Ens, G, V_out]``: roll the time
    axis by one, keep the last slice, write ``y[..., m]`` where ``colmap[v] = m >= 0`` and ``forcing[..., -2 - m]`` where
    ``m <= -2`` (if forcing is given)."""
    cm = [int(m) for m in colmap]
    nxt = x.roll(-1, dims=1)
    nxt[:, -1] = x[:, -1]
    pin = [v for v, m in enumerate(cm) if m >= 0]
    if pin:
        nxt[:, -1, :, :, pin] = y[..., [cm[v] for v in pin]].to(x.dtype)
    fin = [v for v, m in enumerate(cm) if m <= -2]
    if forcing is not None and fin:
        nxt[:, -1, :, :, fin] = forcing[..., [-2 - cm[v] for v in fin]].to(x.dtype)
    return nxt


def rollout(sd, graph, x, n_steps, colmap, forcings=None, detach=False, **model_kwargs):
    """``[n_steps, B, Ens, G, V_out]``: ``ref.model_forward`` chained by :func:`advance` in normalised space (``forcings``
    ``[n_steps - 1, B, Ens, G, F]`` normalised, or None).  ``detach``: cut the gradient between the steps."""
    outs = []
    for s in range(n_steps):
        y = ref.model_forward(sd, graph, x, **model_kwargs)
        outs.append(y)
        if s + 1 < n_steps:
            x = advance(x.detach() if detach else x, y.detach() if detach else y, colmap,
                        None if forcings is None else forcings[s])
    return torch.stack(outs)
