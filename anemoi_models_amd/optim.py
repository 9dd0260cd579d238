"""The optimizer step on the project's own kernels (``csrc/optim.hip``, DESIGN.md section 7 "8f-10"), and what sits next to it
in a training run (``csrc/average.hip``, "8f-11"): :class:`WeightAverager` (EMA / SWA of the weights) and
:class:`DeviceLRSchedule` (linear warm-up and cosine decay evaluated on the device), both capturable with the step.

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

__all__ = ["FusedAdamW", "clip_grad_norm_", "WeightAverager", "DeviceLRSchedule"]


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
      steps.  :class:`DeviceLRSchedule` evaluates warm-up + cosine on the device from this optimizer's own step counter, so it
      also advances inside a captured step.
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

    def group_step_count(self, gi: int) -> Tensor:
        """The step counter of parameter group ``gi`` (steps completed): a 0-dim float32 device tensor, allocated on the
        device of the group's first parameter if the group has not stepped yet.  ``step()`` advances it in place, so the
        tensor may be held across steps and graph replays."""
        return self._group_step(gi, self.param_groups[gi]["params"][0].device)

    @property
    def skip_flag(self) -> Optional[Tensor]:
        """One float32 element on the device: 1 if the last ``step()`` was skipped for a non-finite gradient norm, else 0
        (``None`` before the first step).  A view of the constants block, rewritten by every step."""
        return None if self._consts is None else self._consts[_lib.OPT_SKIP_ALL: _lib.OPT_SKIP_ALL + 1]

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


def _check_avg_param(index: int, p: Tensor, device) -> None:
    if not isinstance(p, Tensor):
        raise NotImplementedError(f"WeightAverager: parameter {index} is a {type(p).__name__}, not a tensor")
    if p.dtype != torch.float32 or not p.is_cuda or p.is_sparse or not p.is_contiguous():
        raise NotImplementedError(f"WeightAverager: parameter {index} is {p.dtype} on {p.device}"
                                  f"{'' if p.is_sparse or p.is_contiguous() else ' (not contiguous)'}; only dense contiguous "
                                  "float32 parameters on one GPU are supported")
    if p.device != device:
        raise NotImplementedError(f"WeightAverager: parameter {index} is on {p.device}, the others on {device}; only "
                                  "parameters on one GPU are supported")


class WeightAverager:
    """An exponential (``kind="ema"``) or equal-weight (``kind="swa"``) running average of a list of parameters, kept in one
    float32 shadow tensor per parameter and updated by one multi-tensor kernel (``csrc/average.hip``, DESIGN.md section 7
    "8f-11") -- what ``torch.optim.swa_utils.AveragedModel`` computes, without a copy of the module (and of every weight
    derived from its parameters) and in ``ceil(T / 88)`` launches for ``T`` tensors.  Per element, with ``n`` the updates
    counted so far::

        n == 0:  s <- p                     (bit for bit)
        EMA:     s <- s + (p - s) (1 - d)   d = min(decay, (1 + n) / (10 + n)) with ``warmup``, else decay
        SWA:     s <- s + (p - s) / (n + 1)

    ``source`` is a :class:`FusedAdamW` or an iterable of parameters.

    * With a ``FusedAdamW`` the averager registers a step post-hook: every ``optimizer.step()`` is followed by the update, also
      inside a ``runtime.GraphedTrainStep`` (which captures ``optimizer.step()``, hooks included).  ``start_step`` and
      ``every`` count OPTIMIZER steps, read from the optimizer's device counter of its first parameter group: the update runs
      after the steps ``start_step, start_step + every, ...`` have completed.  A step that ``skip_nonfinite`` skipped does not
      enter the average.  All of this is decided on the device; nothing is read back.  :meth:`detach` removes the hook.
    * With a plain list the caller calls :meth:`update`; every call counts.

    ``averaged`` are the shadow tensors in parameter order and ``n_averaged`` the device counter.  :meth:`swap` exchanges
    parameters and shadows exactly and bumps the parameters' versions, so weights derived from them (``runtime.PackedWeights``,
    the split-bf16 planes, the stacked folds) are rebuilt; :meth:`applied` is the context manager around two swaps for
    validating with the averaged weights.  Only dense contiguous float32 parameters on one GPU are accepted.
    """

    def __init__(self, source, kind: str = "ema", decay: float = 0.999, warmup: bool = False, start_step: int = 0,
                 every: int = 1) -> None:
        if kind not in ("ema", "swa"):
            raise ValueError(f"WeightAverager: kind must be 'ema' or 'swa', got {kind!r}")
        if not 0.0 <= float(decay) < 1.0:
            raise ValueError(f"WeightAverager: decay {decay} is not in [0, 1)")
        if int(every) != every or every < 1:
            raise ValueError(f"WeightAverager: every = {every} must be an integer >= 1")
        if int(start_step) != start_step or start_step < 0:
            raise ValueError(f"WeightAverager: start_step = {start_step} must be an integer >= 0")
        self.kind, self.decay, self.warmup = kind, float(decay), bool(warmup)
        self.start_step, self.every = int(start_step), int(every)
        self.optimizer = source if isinstance(source, FusedAdamW) else None
        if self.optimizer is not None:
            params = [p for group in source.param_groups for p in group["params"]]
        elif isinstance(source, torch.optim.Optimizer):
            raise NotImplementedError(f"WeightAverager: {type(source).__name__} has no device step counter; pass a FusedAdamW, "
                                      "or the parameters and call update() yourself")
        else:
            params = [source] if isinstance(source, Tensor) else list(source)
        if not params:
            raise ValueError("WeightAverager: no parameters")
        for i, p in enumerate(params):
            _check_avg_param(i, p, params[0].device)
        self.params = params
        self.averaged = [torch.zeros_like(p, memory_format=torch.preserve_format) for p in params]
        self.n_averaged = torch.zeros((), dtype=torch.float32, device=params[0].device)
        self._avg = torch.zeros(_lib.AVG_CONSTS, dtype=torch.float32, device=params[0].device)
        self._hook = None if self.optimizer is None else self.optimizer.register_step_post_hook(self._after_step)

    def _after_step(self, optimizer, args, kwargs) -> None:
        self.update()

    def update(self) -> None:
        """One update of the average from the parameters as they stand (two launches for up to 88 tensors).  With a
        ``FusedAdamW`` this is what the hook calls; ``start_step``, ``every`` and the skip flag are then honoured on the
        device."""
        step = skip = None
        if self.optimizer is not None:
            skip = self.optimizer.skip_flag
            if skip is None:  # no step() has launched anything yet (no parameter had a gradient)
                return
            step = self.optimizer.group_step_count(0)
        ops.average_constants(self._avg, self.n_averaged, kind=self.kind, decay=self.decay, warmup=self.warmup,
                              start_step=self.start_step, every=self.every, step=step, skip=skip)
        ops.multi_average(self.params, self.averaged, self._avg)

    def detach(self) -> None:
        """Remove the optimizer hook; the averages stay.  (A graph captured with the hook keeps averaging.)"""
        if self._hook is not None:
            self._hook.remove()
            self._hook = None

    def swap(self) -> None:
        """Exchange parameters and averages, bit for bit, in one multi-tensor pass; the parameters' versions are bumped.
        Twice restores every bit."""
        ops.multi_swap(self.params, self.averaged)
        torch.autograd.graph.increment_version(self.params)

    def applied(self):
        """``with averager.applied(): validate(model)`` -- the model runs with the averaged weights inside the block."""
        import contextlib

        @contextlib.contextmanager
        def swapped():
            self.swap()
            try:
                yield self
            finally:
                self.swap()

        return swapped()

    @torch.no_grad()
    def copy_to(self, params=None) -> None:
        """Write the averaged values into ``params`` (default: the averaged parameters themselves); ``copy_`` bumps their
        versions."""
        targets = self.params if params is None else ([params] if isinstance(params, Tensor) else list(params))
        if len(targets) != len(self.averaged):
            raise ValueError(f"WeightAverager.copy_to: {len(targets)} tensors for {len(self.averaged)} averages")
        for i, (t, s) in enumerate(zip(targets, self.averaged)):
            if t.shape != s.shape:
                raise ValueError(f"WeightAverager.copy_to: tensor {i} has shape {tuple(t.shape)}, the average {tuple(s.shape)}")
            t.copy_(s)

    def state_dict(self) -> dict:
        return {"kind": self.kind, "decay": self.decay, "warmup": self.warmup, "start_step": self.start_step,
                "every": self.every, "n_averaged": self.n_averaged.clone(),
                "averaged": {i: s.clone() for i, s in enumerate(self.averaged)}}

    @torch.no_grad()
    def load_state_dict(self, state_dict) -> None:
        """Values are copied INTO the existing shadow tensors and counter (a captured graph holds their addresses)."""
        shadows = state_dict["averaged"]
        if len(shadows) != len(self.averaged):
            raise ValueError(f"WeightAverager.load_state_dict: {len(shadows)} averages for {len(self.averaged)} parameters")
        for i, s in enumerate(self.averaged):
            if tuple(shadows[i].shape) != tuple(s.shape):
                raise ValueError(f"WeightAverager.load_state_dict: average {i} has shape {tuple(shadows[i].shape)}, the "
                                 f"parameter {tuple(s.shape)}")
        for name in ("kind", "decay", "warmup", "start_step", "every"):
            if name in state_dict and state_dict[name] != getattr(self, name):
                raise ValueError(f"WeightAverager.load_state_dict: the checkpoint has {name} = {state_dict[name]!r}, this "
                                 f"averager {getattr(self, name)!r}")
        for i, s in enumerate(self.averaged):
            s.copy_(shadows[i])
        self.n_averaged.copy_(torch.as_tensor(state_dict["n_averaged"], dtype=torch.float32))


class DeviceLRSchedule:
    """Linear warm-up followed by cosine decay, evaluated ON THE DEVICE from a :class:`FusedAdamW`'s own step counters
    (``anemoi_lr_schedule``, one tiny launch before every step), so the schedule also advances inside a captured
    ``runtime.GraphedTrainStep`` -- where a float ``lr`` is frozen.  With ``t`` the steps a group has completed, ``base`` the
    group's ``lr`` at construction (a float or a 0-dim device tensor) and ``T = total_steps``::

        t < warmup_steps:   warmup_start + t (base - warmup_start) / warmup_steps
        otherwise:          lr_min + 0.5 (base - lr_min) (1 + cos(pi tc / T))  while tc < T, then lr_min
                            tc = t - warmup_steps with ``warmup_prefix``, else t

    ``warmup_prefix=True`` is ``SequentialLR(LinearLR(start_factor=warmup_start / base), CosineAnnealingLR(T))``;
    ``warmup_prefix=False`` with ``warmup_start=0`` is timm's ``CosineLRScheduler`` as anemoi-training configures it.  The step
    that moves a group's counter from ``t`` to ``t + 1`` uses ``lr(t)``.

    ``group["lr"]`` becomes a 0-dim float32 device tensor (an existing one is kept) that the hook rewrites; there is no
    ``scheduler.step()`` to call.  The schedule is a function of the optimizer's counter alone: it has no state of its own
    (resume follows ``optimizer.load_state_dict``), a step skipped for a non-finite norm does not advance it, and it is right
    under graph replay by construction.  ``get_last_lr()`` returns the device tensors; nothing is synchronised.
    """

    def __init__(self, optimizer, *, warmup_steps: int, total_steps: int, lr_min: float = 0.0, warmup_start: float = 0.0,
                 warmup_prefix: bool = False) -> None:
        if not isinstance(optimizer, FusedAdamW):
            raise NotImplementedError(f"DeviceLRSchedule: needs the device step counters of a FusedAdamW, got "
                                      f"{type(optimizer).__name__}")
        if int(warmup_steps) != warmup_steps or warmup_steps < 0:
            raise ValueError(f"DeviceLRSchedule: warmup_steps = {warmup_steps} must be an integer >= 0")
        if int(total_steps) != total_steps or total_steps < 1:
            raise ValueError(f"DeviceLRSchedule: total_steps = {total_steps} must be an integer >= 1")
        if not float(lr_min) >= 0.0 or not float(warmup_start) >= 0.0:
            raise ValueError(f"DeviceLRSchedule: negative learning rate (lr_min {lr_min}, warmup_start {warmup_start})")
        if len(optimizer.param_groups) > _lib.LR_MAX_GROUPS:
            raise ValueError(f"DeviceLRSchedule: {len(optimizer.param_groups)} parameter groups, at most {_lib.LR_MAX_GROUPS}")
        self.optimizer = optimizer
        self.warmup_steps, self.total_steps = int(warmup_steps), int(total_steps)
        self.lr_min, self.warmup_start, self.warmup_prefix = float(lr_min), float(warmup_start), bool(warmup_prefix)
        self.base_lrs = [float(group["lr"]) for group in optimizer.param_groups]
        self._lrs = []
        for group, base in zip(optimizer.param_groups, self.base_lrs):
            if not isinstance(group["lr"], Tensor):
                group["lr"] = torch.full((), base, dtype=torch.float32, device=group["params"][0].device)
            optimizer._check_group(group)
            self._lrs.append(group["lr"])
        self._launch()  # get_last_lr() is lr(t) from now on
        self._hook = optimizer.register_step_pre_hook(self._before_step)

    def _launch(self) -> None:
        n = len(self._lrs)
        ops.lr_schedule(self._lrs, [self.optimizer.group_step_count(gi) for gi in range(n)], self.base_lrs,
                        warmup_steps=[self.warmup_steps] * n, total_steps=[self.total_steps] * n, lr_min=[self.lr_min] * n,
                        warmup_start=[self.warmup_start] * n, warmup_prefix=[self.warmup_prefix] * n)

    def _before_step(self, optimizer, args, kwargs) -> None:
        for group, lr in zip(optimizer.param_groups, self._lrs):
            if group["lr"] is not lr:  # (optimizer.load_state_dict installs the checkpoint's value)
                group["lr"] = lr
        self._launch()

    def get_last_lr(self) -> list:
        """The groups' learning-rate tensors (0-dim float32, on the device): the rate of the last step launched, or of the
        next one before any."""
        return list(self._lrs)

    def detach(self) -> None:
        """Remove the hook; ``group["lr"]`` stays the device tensor with the value it has."""
        if self._hook is not None:
            self._hook.remove()
            self._hook = None
