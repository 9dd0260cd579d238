"""``Remapper`` mirroring reference preprocessing/remapper.py:23-47: the config's entry point for the remappers.  It is never
instantiated itself: ``Remapper(config, data_indices, statistics)`` returns a ``Monomapper`` when every method of the config
maps one variable to one (``log1p``, ``sqrt``, ``boxcox``, ``none``) and a ``Multimapper`` when every method maps one variable
to several (``cos_sin``).  A config that mixes the two kinds raises ``NotImplementedError`` (give each kind its own processor
entry), one without any known method ``ValueError``.

``remapping()`` turns a mapper and the normaliser next to it into the column tables of the fused I/O kernels
(``ops.Remapping``); ``RemappedAffine`` carries them from ``AnemoiModelInterface.predict_step`` to the model."""

from __future__ import annotations

from typing import Optional

import torch

from . import BasePreprocessor
from .monomapper import Monomapper
from .multimapper import Multimapper


class RemappedAffine(tuple):
    """``(mul, add)`` of the input normaliser, as ``model.forward(x, input_affine=...)`` takes it, that also carries the
    ``ops.Remapping`` of the state (``.remap``, whose tables already hold the pair): what ``preprocessing.imputer.ImputedAffine``
    is to an imputer."""

    def __new__(cls, mul, add, remap):
        self = super().__new__(cls, (mul, add))
        self.remap = remap
        return self


_FORWARD_OP = {"log1p": "log1p", "sqrt": "sqrt", "boxcox": "boxcox", "none": "copy"}
_INVERSE_OP = {"log1p": "expm1", "sqrt": "square", "boxcox": "inv_boxcox", "none": "copy"}


def remapping(mapper, in_affine, out_affine, mapper_first: bool, device):
    """The ``ops.Remapping`` of ``mapper`` (a ``Monomapper`` or ``Multimapper``) on the inference layouts, with the normaliser's
    ``in_affine = (mul, add)`` per RAW input column and ``out_affine`` per RAW output column folded in.  ``mapper_first``: the
    mapper runs before the normaliser, which then acts on what the mapper wrote (the post pair; on the way back the
    de-normalisation comes first); else the normaliser runs first on the raw columns (the pre pair).  A ``Multimapper`` changes
    the width, which the normaliser after it would refuse: ``ValueError``."""
    from ..ops import Remapping

    internal = mapper.data_indices.internal_model
    res = [-1] * len(internal.output.name_to_index)
    for c, j in zip(internal.output.prognostic.tolist(), internal.input.prognostic.tolist()):
        res[c] = j
    in_mul, in_add = (t.detach().float().cpu() for t in in_affine)
    if isinstance(mapper, Monomapper):
        n_in, n_out = mapper.num_inference_input_vars, mapper.num_inference_output_vars
        op, inv_op = ["copy"] * n_in, ["copy"] * n_out
        for method, j, c in zip(mapper.method_names, mapper.index_inference_input, mapper.index_inference_output):
            if j is not None:
                op[j] = _FORWARD_OP[method]
            if c is not None:
                inv_op[c] = _INVERSE_OP[method]
        side = {"post": in_affine, "inv_post": out_affine} if mapper_first else {"pre": in_affine, "inv_pre": out_affine}
        return Remapping(device, n_in, list(range(n_in)), op, res, list(range(n_out)), [-1] * n_out, inv_op, **side)
    if mapper_first:
        raise ValueError("a Multimapper before the normaliser hands it the internal width, which it refuses")
    keep_in, keep_out = mapper.indices_keep_inference_input, mapper.indices_keep_inference_output
    n_int, n_out = mapper.num_remapped_inference_input_vars, mapper.num_inference_output_vars
    src, op = [-1] * n_int, ["copy"] * n_int
    src[: len(keep_in)] = keep_in
    s0, s1, inv_op = [-1] * n_out, [-1] * n_out, ["copy"] * n_out
    for k, c in enumerate(keep_out):
        s0[c] = k
    for raw_in, new_in, raw_out, new_out in zip(mapper.index_inference_input, mapper.index_inference_remapped_input,
                                                 mapper.index_inference_output, mapper.index_inference_backmapped_output):
        for column, name in zip(new_in, ("cos", "sin")):
            src[column], op[column] = raw_in, name
        if raw_out is not None:
            s0[raw_out], s1[raw_out], inv_op[raw_out] = new_out[0], new_out[1], "atan2deg"
    if min(src) < 0 or min(s0) < 0:
        raise ValueError("Multimapper: an internal input or a raw output column is neither kept nor remapped")
    pick = torch.tensor(src, dtype=torch.long)
    return Remapping(device, mapper.num_inference_input_vars, src, op, res, s0, s1, inv_op,
                     pre=(in_mul[pick], in_add[pick]), inv_pre=out_affine)


class Remapper(BasePreprocessor):
    """Dispatches to :class:`Monomapper` or :class:`Multimapper` by the methods of its config."""

    def __new__(cls, config=None, data_indices=None, statistics: Optional[dict] = None):
        _, _, method_config = cls._process_config(config)
        mono = [method in Monomapper.supported_methods for method in method_config]
        multi = [method in Multimapper.supported_methods for method in method_config]
        if all(mono):
            return Monomapper(config, data_indices, statistics)
        if all(multi):
            return Multimapper(config, data_indices, statistics)
        if not any(mono) and not any(multi):
            raise ValueError("No valid remapping method found.")
        raise NotImplementedError("Not implemented: method_config contains a mix of monomapper and multimapper methods: "
                                  f"{list(method_config.keys())}")
