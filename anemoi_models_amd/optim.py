"""The optimizer step on the project's own kernels (``csrc/optim.hip``, DESIGN.md section 7 "8f-10").

:class:`FusedAdamW` is a drop-in for ``torch.optim.AdamW`` whose whole step -- global gradient norm, clip, decoupled weight
decay, moments, update, step count -- is a fixed, small number of launches of multi-tensor kernels: ``ceil(T / 88)`` launches
for the sum of squares of ``T`` gradients plus one to finish it, one for the step's scalars, and ``ceil(T_g / 88)`` per
parameter group for the update.  Deterministic (no atomics, every sum in a fixed order), nothing read back to the host, and
capturable as it stands: the tensors' pointers travel by value in the kernel arguments, so there is no ``capturable=`` flag, no
per-parameter step tensor and no pointer table that a HIP graph would have to keep alive.

:func:`clip_grad_norm_` is the same norm for callers who keep a torch optimizer.
"""

from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from . import _lib
from . import ops

__all__ = ["FusedAdamW", "clip_grad_norm_"]


def _check_param(index: int, p: Tensor, grad: Optional[Tensor] = None) -> None:
    if p.dtype != torch.float32 or not p.is_cuda or p.is_sparse or not p.is_contiguous():
        raise NotImplementedError(f"FusedAdamW: parameter {index} is {p.dtype} on {p.device}"
                                  f"{'' if p.is_sparse or p.is_contiguous() else ' (not contiguous)'}; only dense contiguous "
                                  "float32 parameters on one GPU are supported")
    if grad is not None and (grad.dtype != torch.float32 or grad.is_sparse or grad.device != p.device
                             or not grad.is_contiguous()):
        raise NotImplementedError(f"FusedAdamW: the gradient of parameter {index} is {grad.dtype} on {grad.device}"
                                  f"{' (sparse)' if grad.is_sparse else ''}; only dense contiguous float32 gradients on "
                                  "the parameter's GPU are supported")


class FusedAdamW(torch.optim.Optimizer):
    """``torch.optim.AdamW`` with optional clipping by the global gradient norm, on the multi-tensor kernels.

    Per element, with ``g' = clip * g`` and ``clip = min(1, max_grad_norm / (norm + 1e-6))`` (``torch.nn.utils.
    clip_grad_norm_``'s formula; 1 without ``max_grad_norm``), in torch's order::

        p <- p (1 - lr wd);  m <- m + (g' - m)(1 - beta1);  v <- beta2 v + (1 - beta2) g'^2
        p <- p - (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)

    Differences from ``clip_grad_norm_`` + ``torch.optim.AdamW`` worth knowing:

    * ``.grad`` is NOT modified: the clip is applied as the gradient is loaded (that is the point of fusing it -- no
      read-and-write pass over the gradients).  Code that reads ``p.grad`` after the step sees the unclipped gradient;
      ``opt.grad_norm`` is the norm before clipping, as ``clip_grad_norm_`` returns it.
    * One norm runs over ALL parameter groups.
    * ``lr`` may be a float or a 0-dim float32 device tensor.  A tensor is read on the device at every step, so a scheduler
      that writes into it (``group["lr"].fill_(x)``) works under HIP-graph replay.  A float travels by value in the kernel
      arguments and is therefore FROZEN in a captured graph -- schedulers that assign ``group["lr"] = x`` only reach eager
      steps.
    * ``skip_nonfinite=True``: a step whose gradient norm is NaN or infinite changes nothing -- parameters, moments and the
      step count keep their bits -- and ``opt.skipped_steps`` (a device counter) is advanced, all on the device.
    * There is one step counter per parameter group (a float32 device tensor, as torch's capturable AdamW keeps per
      parameter); ``state[p]["step"]`` is that tensor.  ``state_dict()`` / ``load_state_dict()`` keep
      ``torch.optim.AdamW``'s layout (``step``, ``exp_avg``, ``exp_avg_sq`` per parameter), so checkpoints move in both
      directions; a loaded dict whose parameters of one group disagree on ``step`` is refused with ``ValueError``.
    * Parameter versions are bumped after the launches (``torch.autograd.graph.increment_version``), so weights derived
      from the parameters (``runtime.PackedWeights``, the split-bf16 planes, the stacked folds) are rebuilt as after a
      ``torch.optim`` step.

    ``amsgrad``, ``maximize`` and ``differentiable=True`` raise ``NotImplementedError``; ``foreach``, ``fused`` and
    ``capturable`` are accepted and ignored, so existing configurations load.  Parameters without a gradient are skipped, as
    torch does.  Anything but dense float32 parameters with float32 gradients on one GPU raises ``NotImplementedError`` at
    the step.
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2, *,
                 max_grad_norm: Optional[float] = None, skip_nonfinite: bool = False, amsgrad: bool = False,
                 maximize: bool = False, foreach=None, capturable: bool = False, differentiable: bool = False,
                 fused=None) -> None:
        if amsgrad or maximize or differentiable:
            raise NotImplementedError("FusedAdamW: amsgrad, maximize and differentiable=True are not supported")
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError(f"FusedAdamW: invalid max_grad_norm {max_grad_norm}")
        # torch.optim.AdamW's own group keys (whatever this torch has), so that state dicts are interchangeable
        defaults = dict(torch.optim.AdamW([torch.zeros(1)]).defaults)
        defaults.update(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.grad_norm: Optional[Tensor] = None
        self.skipped_steps: Optional[Tensor] = None
        self._steps: list = []  # one device counter per group
        self._consts = self._sumsq = self._workspace = None

    @staticmethod
    def _check_group(group) -> None:
        lr, (beta1, beta2) = group["lr"], group["betas"]
        if isinstance(lr, Tensor):
            if lr.numel() != 1 or lr.dtype != torch.float32:
                raise ValueError("FusedAdamW: a tensor lr must be a 0-dim float32 tensor")
        elif not float(lr) >= 0.0:
            raise ValueError(f"FusedAdamW: invalid learning rate {lr}")
        if not 0.0 <= beta1 < 1.0 or not 0.0 <= beta2 < 1.0:
            raise ValueError(f"FusedAdamW: invalid betas {group['betas']}")
        if not group["eps"] >= 0.0 or not group["weight_decay"] >= 0.0:
            raise ValueError(f"FusedAdamW: invalid eps {group['eps']} / weight_decay {group['weight_decay']}")
        if group.get("amsgrad") or group.get("maximize") or group.get("differentiable"):
            raise NotImplementedError("FusedAdamW: amsgrad, maximize and differentiable=True are not supported")

    def add_param_group(self, param_group) -> None:
        super().add_param_group(param_group)
        self._check_group(self.param_groups[-1])

    @property
    def step_count(self) -> Optional[Tensor]:
        """The step counter of the first parameter group: a 0-dim float32 device tensor (``None`` before any state exists)."""
        return self._steps[0] if self._steps else None

    def _group_step(self, gi: int, device) -> Tensor:
        while len(self._steps) <= gi:
            self._steps.append(None)
        if self._steps[gi] is None:
            self._steps[gi] = torch.zeros((), dtype=torch.float32, device=device)
        return self._steps[gi]

    def _ensure_state(self, gi: int, p: Tensor) -> dict:
        state = self.state[p]
        if "exp_avg" not in state:
            state["step"] = self._group_step(gi, p.device)
            state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return state

    def init_state(self) -> None:
        """Allocate ``step`` / ``exp_avg`` / ``exp_avg_sq`` of every parameter now (the first step does it for the parameters
        that have a gradient): for building a ``state_dict()`` before any step."""
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                self._ensure_state(gi, p)

    def _buffers(self, device, n_chunks: int) -> None:
        n_consts = (1 + len(self.param_groups)) * _lib.OPT_CONSTS
        if self._consts is None or self._consts.numel() < n_consts or self._consts.device != device:
            self._consts = torch.zeros(n_consts, dtype=torch.float32, device=device)
            self._sumsq = torch.zeros((), dtype=torch.float32, device=device)
        if self.skipped_steps is None or self.skipped_steps.device != device:
            self.skipped_steps = torch.zeros((), dtype=torch.int64, device=device)
        if self._workspace is None or self._workspace.numel() < n_chunks or self._workspace.device != device:
            self._workspace = torch.empty(max(n_chunks, 1), dtype=torch.float32, device=device)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        active = []  # (group index, group, params, grads, moments)
        device, index = None, 0
        for gi, group in enumerate(self.param_groups):
            ps, gs, ms, vs = [], [], [], []
            for p in group["params"]:
                g = p.grad
                index += 1
                if g is None:
                    continue
                _check_param(index - 1, p, g)
                if device is None:
                    device = p.device
                elif p.device != device:
                    raise NotImplementedError(f"FusedAdamW: parameter {index - 1} is on {p.device}, the others on {device}; "
                                              "only parameters on one GPU are supported")
                state = self._ensure_state(gi, p)
                ps.append(p)
                gs.append(g)
                ms.append(state["exp_avg"])
                vs.append(state["exp_avg_sq"])
            if ps:
                active.append((gi, group, ps, gs, ms, vs))
        if not active:
            return loss
        want_norm = self.max_grad_norm is not None or self.skip_nonfinite
        all_grads = [g for a in active for g in a[3]]
        self._buffers(device, ops.multi_tensor_chunks(g.numel() for g in all_grads) if want_norm else 0)
        consts = self._consts.view(-1, _lib.OPT_CONSTS)
        if want_norm:
            ops.multi_sumsq(all_grads, out=self._sumsq, workspace=self._workspace)
        ops.adamw_constants(self._consts[: (1 + len(active)) * _lib.OPT_CONSTS],
                            [self._group_step(a[0], device) for a in active], [a[1]["lr"] for a in active],
                            [a[1]["betas"] for a in active], [a[1]["weight_decay"] for a in active],
                            sumsq=self._sumsq if want_norm else None, max_norm=self.max_grad_norm,
                            skip_nonfinite=self.skip_nonfinite, skipped=self.skipped_steps)
        for k, (gi, group, ps, gs, ms, vs) in enumerate(active):
            beta1, beta2 = group["betas"]
            ops.multi_adamw(ps, gs, ms, vs, consts[1 + k], beta1, beta2, group["eps"])
        torch.autograd.graph.increment_version([p for a in active for p in a[2]])
        self.grad_norm = consts[0, 0] if want_norm else None
        return loss

    # ---- checkpoints in torch.optim.AdamW's layout
    def state_dict(self):
        sd = super().state_dict()
        # one `step` tensor per parameter, as torch writes them (here the parameters of a group share the group's counter)
        sd["state"] = {k: {name: (v.clone() if name == "step" and isinstance(v, Tensor) else v) for name, v in st.items()}
                       for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict) -> None:
        old = {p: dict(s) for p, s in self.state.items()}
        super().load_state_dict(state_dict)
        for gi, group in enumerate(self.param_groups):
            self._check_group(group)
            steps = {}
            for p in group["params"]:
                s = self.state.get(p)
                if s and "step" in s:
                    steps[float(s["step"])] = None
            if len(steps) > 1:
                raise ValueError(f"FusedAdamW.load_state_dict: the parameters of group {gi} disagree on `step` "
                                 f"({sorted(steps)}); this optimizer keeps one step count per parameter group")
            for p in group["params"]:
                s = self.state.get(p)
                if not s:
                    continue
                counter = self._group_step(gi, p.device)
                if steps:
                    counter.fill_(next(iter(steps)))
                s["step"] = counter
                for name in ("exp_avg", "exp_avg_sq"):  # written into the tensors a captured graph may hold
                    prev = old.get(p, {}).get(name)
                    if name in s and prev is not None and prev.shape == s[name].shape and prev.device == p.device:
                        prev.copy_(s[name])
                        s[name] = prev


def clip_grad_norm_(parameters, max_norm: float, norm_type: float = 2.0, error_if_nonfinite: bool = False,
                    foreach=None) -> Tensor:
    """``torch.nn.utils.clip_grad_norm_`` on the multi-tensor kernels, for callers who keep a torch optimizer: the
    deterministic global 2-norm of the gradients (``anemoi_multi_sumsq``), then every gradient multiplied IN PLACE by
    ``min(1, max_norm / (norm + 1e-6))`` -- always, also by a coefficient of exactly 1, as torch does.  Returns the norm as a
    0-dim device tensor; nothing is read back.  Only the 2-norm; ``error_if_nonfinite=True`` is refused (it needs the norm on
    the host).  ``foreach`` is accepted and ignored."""
    if float(norm_type) != 2.0:
        raise NotImplementedError(f"clip_grad_norm_: only the 2-norm is supported, got norm_type={norm_type}")
    if error_if_nonfinite:
        raise NotImplementedError("clip_grad_norm_: error_if_nonfinite=True needs the norm on the host (a synchronisation)")
    if isinstance(parameters, Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.zeros(())
    for i, g in enumerate(grads):
        if g.dtype != torch.float32 or not g.is_cuda or g.is_sparse or not g.is_contiguous() or g.device != grads[0].device:
            raise NotImplementedError(f"clip_grad_norm_: gradient {i} is {g.dtype} on {g.device}; only dense contiguous "
                                      "float32 gradients on one GPU are supported")
    consts = torch.empty(_lib.OPT_CONSTS, dtype=torch.float32, device=grads[0].device)
    sumsq = ops.multi_sumsq(grads)
    ops.adamw_constants(consts, sumsq=sumsq, max_norm=float(max_norm))
    ops.multi_scale(grads, consts[1:2])
    return consts[0]
