"""``Multimapper`` mirroring reference preprocessing/multimapper.py:25-306: one variable -> several new variables and back
(``cos_sin``: a direction in degrees becomes its cosine and sine; the inverse is ``atan2`` in degrees, in ``[0, 360)``).  The
tensor changes its width: the kept variables move to the front, in their order, and the new ones stand at the end, where
``data_indices.internal_data`` / ``internal_model`` (``config.data.remapped``) list them.  Same config schema
(``{cos_sin: {variable: [cos name, sin name]}}``), attribute names (``index_*``, ``indices_keep_*``, ``num_*``) and
shape-driven choice of the layout; never in place.

One deviation, ``transform_loss_mask`` with a remapped FORCING: the reference indexes the mask with the variable's ``None``
output position, which adds an axis, and fails on the shapes (``RuntimeError: The expanded size of the tensor ...``); here
that configuration raises ``NotImplementedError`` naming it.  Every other configuration is pinned to the reference."""

from __future__ import annotations

import logging
from typing import Optional

import torch
from torch import Tensor

from . import BasePreprocessor
from . import mappings

LOGGER = logging.getLogger(__name__)


class Multimapper(BasePreprocessor):
    """Remap one variable to two or more variables, and back."""

    supported_methods = {"cos_sin": [[mappings.cos_converter, mappings.sin_converter], mappings.atan2_converter]}

    def __init__(self, config=None, data_indices=None, statistics: Optional[dict] = None) -> None:
        super().__init__(config, data_indices, statistics)
        self.printed_preprocessor_warning, self.printed_postprocessor_warning = False, False
        self._create_remapping_indices(statistics)
        self._validate_indices()

    def _validate_indices(self) -> None:
        n = len(self.remappers)
        assert len(self.index_training_input) == len(self.index_inference_input) <= n, (
            f"Error creating conversion indices {len(self.index_training_input)}, {len(self.index_inference_input)}, {n}")
        assert len(self.index_training_output) == len(self.index_inference_output) <= n, (
            f"Error creating conversion indices {len(self.index_training_output)}, {len(self.index_inference_output)}, {n}")
        assert len(set(self.index_training_input + self.indices_keep_training_input)) == self.num_training_input_vars, (
            "Error creating conversion indices: variables remapped in config.data.remapped that have no remapping function "
            "defined. Preprocessed tensors contains empty columns.")

    def _create_remapping_indices(self, statistics=None) -> None:
        """reference :86-183.  Per remapped variable of the training input, in its order: its column in the four raw
        layouts (``index_*``), and the columns of its new variables in the four internal layouts
        (``index_*_remapped_input`` / ``index_*_backmapped_output``); ``indices_keep_*``: raw columns that stay."""
        idx = self.data_indices
        raw = {"training_input": idx.data.input.name_to_index, "inference_input": idx.model.input.name_to_index,
               "training_output": idx.data.output.name_to_index, "inference_output": idx.model.output.name_to_index}
        internal = {"training_input": idx.internal_data.input.name_to_index,
                    "inference_input": idx.internal_model.input.name_to_index,
                    "training_output": idx.internal_data.output.name_to_index,
                    "inference_output": idx.internal_model.output.name_to_index}
        for layout in raw:
            setattr(self, f"num_{layout}_vars", len(raw[layout]))
            setattr(self, f"num_remapped_{layout}_vars", len(internal[layout]))
            setattr(self, f"indices_keep_{layout}", [pos for name, pos in raw[layout].items() if name in internal[layout]])
        self.index_training_input, self.index_training_remapped_input = [], []
        self.index_inference_input, self.index_inference_remapped_input = [], []
        self.index_training_output, self.index_training_backmapped_output = [], []
        self.index_inference_output, self.index_inference_backmapped_output = [], []
        self.remappers, self.backmappers = [], []
        for name in raw["training_input"]:
            method = self.methods.get(name, self.default)
            if method == "none":
                continue
            if method not in self.supported_methods:
                raise ValueError(f"Unknown remapping method for {name}: {method}")
            self.index_training_input.append(raw["training_input"][name])
            self.index_training_output.append(raw["training_output"][name])
            self.index_inference_input.append(raw["inference_input"][name])
            self.index_inference_output.append(raw["inference_output"].get(name))  # None: a forcing has no output column
            new_names = self.method_config[method][name]
            for name_dst in new_names:
                assert name_dst in internal["training_input"], (
                    f"Trying to remap {name} to {name_dst}, but {name_dst} not a variable. "
                    f"Remap {name} to {name_dst} in config.data.remapped. ")
            self.index_training_remapped_input.append([internal["training_input"][n] for n in new_names])
            self.index_training_backmapped_output.append([internal["training_output"][n] for n in new_names])
            self.index_inference_remapped_input.append([internal["inference_input"][n] for n in new_names])
            self.index_inference_backmapped_output.append([internal["inference_output"].get(n) for n in new_names])
            forward, backward = self.supported_methods[method]
            self.remappers.append(list(forward))
            self.backmappers.append(backward)
            LOGGER.info("Map %s to cosine and sine and save result in %s.", name, new_names)

    def _warn_in_place(self, in_place: bool, flag: str) -> None:
        if in_place and not getattr(self, flag):
            LOGGER.warning("Remapper called with in_place=True. This processor cannot be applied in_place as new columns "
                           "are added to the tensors.")
            setattr(self, flag, True)

    def transform(self, x: Tensor, in_place: bool = True) -> Tensor:
        """``[..., raw input variables]`` -> a NEW ``[..., internal input variables]``: kept columns first, then what the
        converters make of each remapped column."""
        if x.shape[-1] == self.num_training_input_vars:
            index, remapped, keep = self.index_training_input, self.index_training_remapped_input, self.indices_keep_training_input
            width = self.num_remapped_training_input_vars
        elif x.shape[-1] == self.num_inference_input_vars:
            index, remapped, keep = (self.index_inference_input, self.index_inference_remapped_input,
                                     self.indices_keep_inference_input)
            width = self.num_remapped_inference_input_vars
        else:
            raise ValueError(f"Input tensor ({x.shape[-1]}) does not match the training ({self.num_training_input_vars}) "
                             f"or inference shape ({self.num_inference_input_vars})")
        out = torch.zeros(x.shape[:-1] + (width,), dtype=x.dtype, device=x.device)
        self._warn_in_place(in_place, "printed_preprocessor_warning")
        out[..., : len(keep)] = x[..., keep]
        for dst, converters, src in zip(remapped, self.remappers, index):
            if src is not None:
                for converter, column in zip(converters, dst):
                    out[..., column] = converter(x[..., src])
        return out

    def inverse_transform(self, x: Tensor, in_place: bool = True) -> Tensor:
        """``[..., internal output variables]`` -> a NEW ``[..., raw output variables]``."""
        if x.shape[-1] == self.num_remapped_training_output_vars:
            index, remapped, keep = (self.index_training_output, self.index_training_backmapped_output,
                                     self.indices_keep_training_output)
            width = self.num_training_output_vars
        elif x.shape[-1] == self.num_remapped_inference_output_vars:
            index, remapped, keep = (self.index_inference_output, self.index_inference_backmapped_output,
                                     self.indices_keep_inference_output)
            width = self.num_inference_output_vars
        else:
            raise ValueError(f"Input tensor ({x.shape[-1]}) does not match the training "
                             f"({self.num_remapped_training_output_vars}) or inference shape "
                             f"({self.num_remapped_inference_output_vars})")
        out = torch.zeros(x.shape[:-1] + (width,), dtype=x.dtype, device=x.device)
        self._warn_in_place(in_place, "printed_postprocessor_warning")
        out[..., keep] = x[..., : len(keep)]
        for dst, backmapper, src in zip(index, self.backmappers, remapped):
            if dst is not None:
                out[..., dst] = backmapper(x[..., src])
        return out

    def transform_loss_mask(self, mask: Tensor) -> Tensor:
        """The loss mask ``[..., raw model outputs]`` on the internal model outputs: a remapped variable's mask column
        serves each of its new columns (reference :280-306)."""
        if any(i is None for i in self.index_inference_output):
            raise NotImplementedError("Multimapper.transform_loss_mask with a remapped forcing variable: the variable has no "
                                      "output column to take the mask from (the reference fails on the shapes here)")
        keep = self.indices_keep_inference_output
        out = torch.zeros(mask.shape[:-1] + (mask.shape[-1] + len(self.index_inference_output),), dtype=mask.dtype,
                          device=mask.device)
        out[..., : len(keep)] = mask[..., keep]
        for src, dst in zip(self.index_inference_output, self.index_inference_backmapped_output):
            for column in dst:
                out[..., column] = mask[..., src]
        return out
