"""``Monomapper`` mirroring reference preprocessing/monomapper.py:30-150: one variable -> one variable, in its own column
(``log1p``, ``sqrt``, ``boxcox``, ``none``), so the tensor keeps its width and its layout.  Same config schema
(``{method: [variables]}``), attribute names (``index_training_input``, ``index_training_out``, ``index_inference_input``,
``index_inference_output``, ``remappers``, ``backmappers``) and shape-driven choice of the layout."""

from __future__ import annotations

from typing import Optional

from torch import Tensor

from . import BasePreprocessor
from . import mappings


class Monomapper(BasePreprocessor):
    """Remap and convert single variables in place of themselves."""

    supported_methods = {
        "log1p": [mappings.log1p_converter, mappings.expm1_converter],
        "sqrt": [mappings.sqrt_converter, mappings.square_converter],
        "boxcox": [mappings.boxcox_converter, mappings.inverse_boxcox_converter],
        "none": [mappings.noop, mappings.noop],
    }

    def __init__(self, config=None, data_indices=None, statistics: Optional[dict] = None) -> None:
        super().__init__(config, data_indices, statistics)
        self._create_remapping_indices(statistics)
        self._validate_indices()

    def _validate_indices(self) -> None:
        n = len(self.remappers)
        assert (len(self.index_training_input) == len(self.index_inference_input) == len(self.index_inference_output)
                == len(self.index_training_out) == n), (
            f"Error creating conversion indices {len(self.index_training_input)}, {len(self.index_inference_input)}, "
            f"{len(self.index_inference_output)}, {len(self.index_training_out)}, {n}")

    def _create_remapping_indices(self, statistics=None) -> None:
        """One entry per variable of the training input, in its order (reference :65-117); ``None`` where a layout does
        not hold the variable (a forcing has no output column)."""
        train_in = self.data_indices.data.input.name_to_index
        infer_in = self.data_indices.model.input.name_to_index
        train_out = self.data_indices.data.output.name_to_index
        infer_out = self.data_indices.model.output.name_to_index
        self.num_training_input_vars, self.num_inference_input_vars = len(train_in), len(infer_in)
        self.num_training_output_vars, self.num_inference_output_vars = len(train_out), len(infer_out)
        self.remappers, self.backmappers, self.method_names = [], [], []
        self.index_training_input, self.index_training_out = [], []
        self.index_inference_input, self.index_inference_output = [], []
        for name, position in train_in.items():
            method = self.methods.get(name, self.default)
            if method not in self.supported_methods:
                raise KeyError(f"Unknown remapping method for {name}: {method}")
            forward, backward = self.supported_methods[method]
            self.remappers.append(forward)
            self.backmappers.append(backward)
            self.method_names.append(method)
            self.index_training_input.append(position)
            self.index_training_out.append(train_out.get(name))
            self.index_inference_input.append(infer_in.get(name))
            self.index_inference_output.append(infer_out.get(name))

    @staticmethod
    def _layout(width: int, train_n: int, infer_n: int, train_idx, infer_idx):
        if width == train_n:
            return train_idx
        if width == infer_n:
            return infer_idx
        raise ValueError(f"Input tensor ({width}) does not match the training ({train_n}) or inference shape ({infer_n})")

    def transform(self, x: Tensor, in_place: bool = True) -> Tensor:
        if not in_place:
            x = x.clone()
        idx = self._layout(x.shape[-1], self.num_training_input_vars, self.num_inference_input_vars,
                           self.index_training_input, self.index_inference_input)
        for i, remapper in zip(idx, self.remappers):
            if i is not None and remapper is not mappings.noop:
                x[..., i] = remapper(x[..., i])
        return x

    def inverse_transform(self, x: Tensor, in_place: bool = True) -> Tensor:
        if not in_place:
            x = x.clone()
        idx = self._layout(x.shape[-1], self.num_training_output_vars, self.num_inference_output_vars,
                           self.index_training_out, self.index_inference_output)
        for i, backmapper in zip(idx, self.backmappers):
            if i is not None and backmapper is not mappings.noop:
                x[..., i] = backmapper(x[..., i])
        return x
