"""Ensemble model: the encoder - processor - decoder network with noise-conditioned LayerNorms in the processor.

Members that start from the same state differ because each (member, mesh node) draws Gaussian noise, a small MLP embeds it,
and every LayerNorm of the Transformer processor is a ``ConditionalLayerNorm`` of that embedding -- how AIFS-CRPS and
anemoi-models' ``AnemoiEnsModelEncProcDec`` create spread.  The reference checkout this package mirrors predates that model:
this is a restatement of its published description, not a port, with the config key ``model.noise_injector`` (``noise_std``,
``noise_channels_dim``, ``noise_mlp_hidden_dim``, ``inject_noise``) and the parameter names as far as they are known.
"""

from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from .. import runtime
from ..layers.ensemble import NoiseConditioning
from .encoder_processor_decoder import AnemoiModelEncProcDec


class AnemoiEnsModelEncProcDec(AnemoiModelEncProcDec):
    """``forward(x)``: ``x [1, T, E, G, V_in]`` -> ``[1, E, G, V_out]``; one noise embedding ``[E * N_mesh, K]`` per call, drawn
    before the processor and handed to every block.  Transformer processor only; single device."""

    def __init__(self, *, model_config, data_indices, graph_data, truncation_data=None, statistics=None) -> None:
        target = str(model_config.model.processor.get("_target_", ""))
        if not target.endswith(".TransformerProcessor"):
            raise NotImplementedError(
                f"AnemoiEnsModelEncProcDec needs the Transformer processor, got {target.rsplit('.', 1)[-1] or 'none'}: the "
                "LayerNorms of the GraphTransformer and GNN processors are folded into their GEMMs and cannot be conditioned yet")
        cfg = model_config.model.get("noise_injector", None)
        if cfg is None:
            raise ValueError("AnemoiEnsModelEncProcDec: the config has no model.noise_injector")
        super().__init__(model_config=model_config, data_indices=data_indices, graph_data=graph_data,
                         truncation_data=truncation_data, statistics=statistics)  # (the members are slabs of one projection launch)
        self.noise_injector = NoiseConditioning(
            noise_std=cfg["noise_std"], noise_channels_dim=cfg["noise_channels_dim"],
            noise_mlp_hidden_dim=cfg["noise_mlp_hidden_dim"], inject_noise=cfg.get("inject_noise", True))

    def _processor_kwargs(self, model_config) -> dict:
        return {"cond_dim": int(model_config.model.noise_injector["noise_channels_dim"])}

    def _processor_condition(self, batch_size: int, x_latent: Tensor) -> Optional[Tensor]:
        inj = self.noise_injector
        cond = inj(x_latent.shape[0], x_latent.device, x_latent.dtype)
        if cond is None:  # inject_noise=False: a zero condition -- the LayerNorms keep their biases, the members stay equal
            cond = torch.zeros((x_latent.shape[0], inj.noise_channels_dim), dtype=torch.float32, device=x_latent.device)
        return cond

    def forward(self, x: Tensor, model_comm_group=None, *, input_affine=None, output_affine=None) -> Tensor:
        if model_comm_group is not None and model_comm_group.size() > 1:
            raise NotImplementedError("AnemoiEnsModelEncProcDec: a model communication group is not implemented (the noise "
                                      "and the conditional LayerNorms are single-device)")
        b, _, ens, _, _ = x.shape
        if ens != 1 and b != 1:
            raise NotImplementedError("an ensemble dimension > 1 only with batch size 1")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return super().forward(x, input_affine=input_affine, output_affine=output_affine)
        if ens == 1:
            return super().forward(x, input_affine=input_affine, output_affine=output_affine)
        # the inference route runs its rows as (batch, node): the members of the one batch entry become the batch
        y = super().forward(x.transpose(0, 2), input_affine=input_affine, output_affine=output_affine)
        return y.transpose(0, 1).contiguous()
