"""Noise conditioning of the ensemble model: Gaussian noise per member and mesh node, drawn on the device, and the small MLP
that embeds it.  The embedding conditions every LayerNorm of the processor (``layers.normalization.ConditionalLayerNorm``)."""

from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor
from torch import nn

from .. import ops
from .. import runtime
from .mlp import NativeSequential


class NoiseConditioning(nn.Module):
    """``forward(rows, device, dtype)``: ``[rows, noise_channels_dim]`` of ``noise_std * N(0, 1)`` from ``ops.gaussian_noise``
    (counter-based: one launch, no generator state on the device), through ``noise_mlp`` = Linear -> GELU -> Linear on the fused
    Linear in ``dtype``; returns the f32 embedding ``[rows, noise_channels_dim]``, or ``None`` with ``inject_noise=False``.

    The seed of a call is :meth:`next_seed`: eagerly a draw from torch's default CPU generator (``torch.manual_seed`` reproduces
    the noise), inside a ``runtime.DeviceDropout`` context a constant of this module (drawn once, the same way) to which the
    kernel adds the context's device word -- a captured training step then draws new noise on every replay.  A call while a
    stream is capturing and no such context is active raises: the captured seed would repeat on every replay."""

    def __init__(self, noise_std: float, noise_channels_dim: int, noise_mlp_hidden_dim: int, inject_noise: bool = True) -> None:
        super().__init__()
        self.noise_std, self.noise_channels_dim = float(noise_std), int(noise_channels_dim)
        self.inject_noise = bool(inject_noise)
        self.noise_mlp = nn.Sequential(nn.Linear(self.noise_channels_dim, int(noise_mlp_hidden_dim)), nn.GELU(),
                                       nn.Linear(int(noise_mlp_hidden_dim), self.noise_channels_dim))
        self._native: Optional[NativeSequential] = None

    def next_seed(self) -> int:
        dd = runtime.device_dropout()
        if dd is not None and self.__dict__.get("_layer_seed") is not None:
            return self.__dict__["_layer_seed"]
        seed = int(torch.randint(0, 2**31 - 1, (1,)).item())
        if dd is not None:
            self.__dict__["_layer_seed"] = seed
        return seed

    def draw(self, rows: int, device) -> Tensor:
        """The raw noise ``[rows, noise_channels_dim]`` (f32) of one call."""
        dd = runtime.device_dropout()
        if dd is None and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("NoiseConditioning: drawing noise while a stream is capturing needs a runtime.DeviceDropout "
                               "context (the captured seed would repeat the same noise on every replay)")
        return ops.gaussian_noise(rows, self.noise_channels_dim, self.noise_std, seed=self.next_seed(),
                                  seed_dev=None if dd is None else dd.word, device=device)

    def forward(self, rows: int, device, dtype: torch.dtype) -> Optional[Tensor]:
        if not self.inject_noise:
            return None
        from .. import training

        z = self.draw(int(rows), device).to(dtype)
        if training.wants_grad(self):
            return training.sequential(self.noise_mlp, z).float()
        if self._native is None:
            self._native = NativeSequential(self.noise_mlp)
        return self._native(z).float()
