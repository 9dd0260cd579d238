"""``AnemoiModelInterface`` mirroring reference interface/__init__.py:20-123: the wrapper anemoi-inference /
anemoi-training hold -- pre-processors, the model, post-processors, ``predict_step``.  Same constructor kwargs, same
sub-module names (``pre_processors``, ``post_processors``, ``model``) and therefore the same ``state_dict``."""

from __future__ import annotations

import uuid

import torch

from .. import ops
from ..models.encoder_processor_decoder import instantiate
from ..preprocessing import Processors
from ..utils.config import target_accepts


class AnemoiModelInterface(torch.nn.Module):
    def __init__(self, *, config, graph_data, statistics: dict, data_indices, metadata: dict,
                 supporting_arrays: dict = None, truncation_data: dict = None) -> None:
        """``truncation_data``: ``{"down": A_down, "up": A_up}`` of the truncated skip connection, handed to the model as current
        anemoi-models does (``layers.truncation``); ``None``: the model is built without the argument, as before."""
        super().__init__()
        self.config = config
        self.id = str(uuid.uuid4())
        self.multi_step = self.config.training.multistep_input
        self.graph_data = graph_data
        self.statistics = statistics
        self.metadata = metadata
        self.supporting_arrays = supporting_arrays if supporting_arrays is not None else {}
        self.data_indices = data_indices
        self.truncation_data = truncation_data
        self._build_model()

    def _build_model(self) -> None:
        processors = [
            [name, instantiate(processor, data_indices=self.data_indices, statistics=self.statistics)]
            for name, processor in self.config.data.processors.items()
        ]
        self.pre_processors = Processors(processors)
        self.post_processors = Processors(processors, inverse=True)
        extra = {} if not self.truncation_data else {"truncation_data": self.truncation_data}
        if target_accepts(self.config.model.model, "statistics"):  # (the boundings that work in normalised space read them)
            extra["statistics"] = self.statistics
        self.model = instantiate(self.config.model.model, model_config=self.config, data_indices=self.data_indices,
                                 graph_data=self.graph_data, _recursive_=False, **extra)
        self.forward = self.model.forward

    def predict_step(self, batch: torch.Tensor) -> torch.Tensor:
        """``[batch, time, grid, variables]`` (physical values, input variables) -> de-normalised prediction
        ``[batch, ensemble = 1, grid, output variables]`` (reference interface/__init__.py:97-123)."""
        fused = self._fused_route(batch)
        if fused is not None:
            # the processors are an InputNormalizer, alone or with one NaN imputer: the per-variable affine maps, the
            # imputer's select and its NaN restore ride on the first and the last kernel of the forward (anemoi_assemble_nodes /
            # anemoi_finalize_output / anemoi_bound_output and their _imputed forms) -- no pass of its own over the grid
            # state or the prediction, same arithmetic.  With a remapper next to the normaliser its converters ride on
            # anemoi_assemble_nodes_remapped / anemoi_residual_remapped / anemoi_unmap_output in the same way
            with torch.no_grad():
                assert len(batch.shape) == 4, (
                    f"The input tensor has an incorrect shape: expected a 4-dimensional tensor, got {batch.shape}!")
                x = batch[:, 0 : self.multi_step, None, ...]
                return self.model(x, input_affine=fused[0], output_affine=fused[1])
        batch = self.pre_processors(batch, in_place=False)
        with torch.no_grad():
            assert len(batch.shape) == 4, (
                f"The input tensor has an incorrect shape: expected a 4-dimensional tensor, got {batch.shape}!")
            x = batch[:, 0 : self.multi_step, None, ...]  # dummy ensemble dimension as 3rd index
            y_hat = self(x)
        return self.post_processors(y_hat, in_place=False)

    def _normalizer_affines(self, batch: torch.Tensor):
        """``((mul_in, add_in), (mul_out, add_out))`` when pre / post-processing is exactly one ``InputNormalizer``
        acting on the model's input / output variable lists and the model accepts them; else ``None``.
        ``ANEMOI_AMD_FUSE_NORMALIZER=0`` turns the fusion off (A/B)."""
        from ..preprocessing.normalizer import InputNormalizer

        procs = list(self.pre_processors.processors.values())
        if len(procs) != 1 or type(procs[0]) is not InputNormalizer:
            return None
        return self._affines_of(procs[0], batch)

    def _affines_of(self, norm, batch: torch.Tensor):
        """The conditions every fused route shares, then the affine maps of ``norm`` on the model's variable lists."""
        import inspect
        import os

        mode = os.environ.get("ANEMOI_AMD_FUSE_NORMALIZER", "1")
        if mode == "0" or batch.dim() != 4 or not (batch.is_cuda or mode == "force"):
            return None
        if "input_affine" not in inspect.signature(self.model.forward).parameters:
            return None
        if batch.shape[-1] != norm._input_idx.numel():  # the full-variable layout is left to the generic route
            return None
        if self.pre_processors.first_run:  # keep the reference's one-off NaN check of the first processed batch
            return None
        i_in, i_out = norm._input_idx.long(), norm._output_idx.long()
        return ((norm._norm_mul[i_in], norm._norm_add[i_in]), (norm._norm_mul[i_out], norm._norm_add[i_out]))

    def _fused_route(self, batch: torch.Tensor):
        """Route query of :meth:`predict_step`: ``(input_affine, output_affine)`` for ``model(x, input_affine=...,
        output_affine=...)`` when pre / post-processing rides on the forward's I/O kernels, ``None`` for the generic route.

        Fused: exactly one ``InputNormalizer`` (:meth:`_normalizer_affines`), or one ``InputNormalizer`` and one NaN imputer of
        ``preprocessing.imputer`` in either order -- then ``input_affine`` is an ``ImputedAffine`` carrying the imputer's
        ``Imputation``.  With an imputer the model must have the plain residual and a bounding list that compiles, and a
        static imputer its ``nan_locations`` on a grid of the batch's size with every map column inside the map.  The first
        call is always generic: it fixes ``nan_locations`` / ``loss_mask_training``, which this route never touches.
        One ``InputNormalizer`` and one ``Monomapper`` / ``Multimapper``: :meth:`_remapped_route`."""
        from ..layers.bounding import compile_boundings
        from ..preprocessing import imputer as imp_mod
        from ..preprocessing.monomapper import Monomapper
        from ..preprocessing.multimapper import Multimapper
        from ..preprocessing.normalizer import InputNormalizer

        procs = list(self.pre_processors.processors.values())
        if len(procs) == 1:
            return self._normalizer_affines(batch)
        # (exact types: a subclass may redefine transform / inverse_transform; BaseImputer itself imputes nothing)
        kinds = (imp_mod.InputImputer, imp_mod.ConstantImputer, imp_mod.DynamicInputImputer, imp_mod.DynamicConstantImputer)
        if len(procs) != 2 or sorted(type(p) is InputNormalizer for p in procs) != [False, True]:
            return None
        imputer_first = type(procs[1]) is InputNormalizer
        imputer, norm = (procs[0], procs[1]) if imputer_first else (procs[1], procs[0])
        if type(imputer) in (Monomapper, Multimapper):
            return self._remapped_route(batch, imputer, norm, mapper_first=imputer_first)
        if not any(type(imputer) is k for k in kinds):
            return None
        affines = self._affines_of(norm, batch)
        if affines is None:
            return None
        if getattr(self.model, "_truncation", None) is not None:
            return None
        if len(getattr(self.model, "boundings", ())) > 0 and compile_boundings(self.model.boundings) is None:
            return None
        dynamic = isinstance(imputer, imp_mod.DynamicMixin)
        if not dynamic:
            nan_map = imputer.nan_locations
            if nan_map is None or nan_map.dim() != 2 or nan_map.shape[0] != batch.shape[-2]:
                return None
            if any(src >= nan_map.shape[1] for src in imputer.index_training_input):
                return None  # the generic route fails on it exactly as the reference does
        (mul_in, add_in), out_affine = affines
        key = (id(imputer), str(batch.device), imputer_first, self._version_of(norm),
               None if dynamic else (imputer.nan_locations.data_ptr(), tuple(imputer.nan_locations.shape)))
        cache = self.__dict__.setdefault("_imputation_cache", {})
        hit = cache.get("imputation")
        if hit is None or hit[0] != key:  # built once per (imputer, device), rebuilt when its sources change
            hit = (key, imputer.imputation(batch.device, (mul_in, add_in) if imputer_first else None))
            cache["imputation"] = hit
        return imp_mod.ImputedAffine(mul_in, add_in, hit[1]), out_affine

    def _remapped_route(self, batch: torch.Tensor, mapper, norm, mapper_first: bool):
        """The case of :meth:`_fused_route` with one remapper next to the normaliser: a ``Monomapper`` on either side of it, a
        ``Multimapper`` after it (before it the reference normaliser refuses the internal width, and so does the generic route).
        The model must be the flat ``AnemoiModelEncProcDec`` with the plain residual and a bounding list that compiles.
        ``input_affine`` is a ``RemappedAffine``: its ``ops.Remapping`` holds the remapper's and the normaliser's column tables
        for the assemble, residual and unmap kernels, built once per (remapper, normaliser version, device)."""
        from ..layers.bounding import compile_boundings
        from ..models.encoder_processor_decoder import AnemoiModelEncProcDec
        from ..preprocessing import remapper as rm_mod

        if mapper_first and type(mapper) is rm_mod.Multimapper:
            return None
        if type(self.model) is not AnemoiModelEncProcDec or getattr(self.model, "_truncation", None) is not None:
            return None
        if len(self.model.boundings) > 0 and compile_boundings(self.model.boundings) is None:
            return None
        affines = self._affines_of(norm, batch)
        if affines is None:
            return None
        (mul_in, add_in), out_affine = affines
        key = (id(mapper), str(batch.device), mapper_first, self._version_of(norm))
        cache = self.__dict__.setdefault("_remapping_cache", {})
        hit = cache.get("remapping")
        if hit is None or hit[0] != key:
            hit = (key, rm_mod.remapping(mapper, (mul_in, add_in), out_affine, mapper_first, batch.device))
            cache["remapping"] = hit
        return rm_mod.RemappedAffine(mul_in, add_in, hit[1]), out_affine

    @staticmethod
    def _version_of(norm) -> tuple:
        return (norm._norm_mul.data_ptr(), norm._norm_mul._version, norm._norm_add.data_ptr(), norm._norm_add._version)

    # ------------------------------------------------------------------ autoregressive rollout (BASELINE config 4)
    def _advance_map(self, device) -> torch.Tensor:
        """int32 ``[V_in]`` column map of ``anemoi_advance_input``: prognostic inputs <- their output column, forcing
        inputs <- their position in the forcing tensor (-2 - k), everything else persists (-1)."""
        from ..utils.indices import advance_colmap

        return advance_colmap(self.data_indices).to(device)

    def rollout(self, batch: torch.Tensor, n_steps: int, forcings: torch.Tensor = None, model_comm_group=None,
                gather: str = "all"):
        """``n_steps`` autoregressive forecasts from ``batch`` ``[batch, time, grid, input variables]`` (physical
        values).  ``forcings`` ``[n_steps, batch, grid, n_forcing]`` holds the physical forcing inputs valid at each
        step's output time (ordered like ``data_indices.internal_model.input.forcing``); without it the last forcing
        values persist.  Returns ``[n_steps, batch, 1, grid, output variables]`` de-normalised predictions.

        Not part of the reference repository (which stops at :meth:`predict_step`): the loop follows its caller,
        anemoi-training's ``advance_input``.  The state stays on the device in normalised model space; the time shift
        and the prognostic / forcing write-back are one in-place HIP kernel (``anemoi_advance_input``).

        With a model communication group, ``gather="last"`` keeps the state SHARDED between the steps: the intermediate
        forecasts are not all-gathered (each rank holds the grid rows it decodes plus the few its encoder reads, fetched
        by one small all-to-all-v per step) and only the last step's full prediction is returned, ``[1, batch, 1, grid,
        output variables]``.  ``gather="all"`` (default) returns every step, each all-gathered as the reference's decoder
        contract prescribes."""
        if gather not in ("all", "last"):
            raise ValueError(f"rollout: gather must be 'all' or 'last', got {gather!r}")
        keep_sharded = gather == "last" and model_comm_group is not None and model_comm_group.size() > 1
        from ..preprocessing.multimapper import Multimapper

        if any(isinstance(p, Multimapper) for p in self.pre_processors.processors.values()):
            # the forcing write-back below pre-processes slices of the INTERNAL width, which a Multimapper does not take
            raise NotImplementedError("rollout: a Multimapper in config.data.processors changes the width of the state; "
                                      "use predict_step")
        idx = self.data_indices.internal_model
        x = self.pre_processors(batch, in_place=False)
        assert len(x.shape) == 4, f"The input tensor has an incorrect shape: expected 4 dimensions, got {x.shape}!"
        x = x[:, 0 : self.multi_step, None, ...].float().contiguous().clone()
        cmap = self._advance_map(x.device)
        f_idx = idx.input.forcing.long().to(x.device)
        outs = []
        with torch.no_grad():
            for step in range(n_steps):
                last = step + 1 == n_steps
                y_local = None
                if keep_sharded:
                    from ..distributed.partition import advance_sharded_state, sharded_forward, sharded_state_output

                    y_local, shard_plan = sharded_forward(self.model, x, model_comm_group, local_output=True)
                    if last:  # the one all-gather of the rollout
                        y_hat = sharded_state_output(self.model, x, y_local, shard_plan, model_comm_group).to(x.dtype)
                        outs.append(self.post_processors(y_hat, in_place=False))
                else:
                    y_hat = self.model(x, model_comm_group) if model_comm_group is not None else self.model(x)
                    outs.append(self.post_processors(y_hat, in_place=False))
                if last:
                    break
                f_norm = None
                if forcings is not None and f_idx.numel() > 0:
                    # normalise the forcing columns with the same pre-processors: embed them in a full-width slice
                    full = x[:, -1, 0].clone()
                    full[..., f_idx] = forcings[step].to(full)
                    f_norm = self.pre_processors(full[:, None], in_place=False)[:, 0][..., f_idx][:, None].contiguous()
                if y_local is not None:
                    advance_sharded_state(self.model, x, y_local, shard_plan, cmap, f_norm)
                else:
                    ops.advance_input(x, y_hat.float().contiguous(), cmap, f_norm)
        return torch.stack(outs)
