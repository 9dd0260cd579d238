"""Stand-in for the part of ``anemoi.models.data_indices.IndexCollection`` the forward path reads.

The model root only touches ``data_indices.internal_model.{input,output}`` for
``len()``, ``.prognostic``, ``.full``, ``.diagnostic`` and ``.name_to_index``
(reference models/encoder_processor_decoder.py:103,108-125).  A real
``IndexCollection`` can be passed instead; this class exists so tests and
``bench.py`` need no dataset configuration.

Variable layout: input = [prognostic..., forcing...], output = [prognostic..., diagnostic...].
"""

from __future__ import annotations

import torch


class _ModelIndex:
    def __init__(self, names, prognostic, diagnostic=(), forcing=()):
        self.name_to_index = {n: i for i, n in enumerate(names)}
        self.full = torch.arange(len(names), dtype=torch.int64)
        self.prognostic = torch.as_tensor(list(prognostic), dtype=torch.int64)
        self.diagnostic = torch.as_tensor(list(diagnostic), dtype=torch.int64)
        self.forcing = torch.as_tensor(list(forcing), dtype=torch.int64)

    def __len__(self) -> int:
        return len(self.name_to_index)


class _Internal:
    def __init__(self, inp, out):
        self.input = inp
        self.output = out


class _DataIndex:
    """Dataset-side view (reference data_indices/index.py:46-63): positions in the FULL variable list."""

    def __init__(self, name_to_index, full, prognostic, diagnostic=(), forcing=()):
        self.name_to_index = dict(name_to_index)
        self.full = torch.as_tensor(list(full), dtype=torch.int64)
        self.prognostic = torch.as_tensor(list(prognostic), dtype=torch.int64)
        self.diagnostic = torch.as_tensor(list(diagnostic), dtype=torch.int64)
        self.forcing = torch.as_tensor(list(forcing), dtype=torch.int64)

    def __len__(self) -> int:
        return int(self.full.numel())


class SimpleDataIndices:
    """Dataset layout ``[prognostic..., forcing..., diagnostic...]``; input = all but diagnostic, output = all but
    forcing (reference data_indices/collection.py:24-103).  ``remapped = {name: [new names]}`` (``config.data.remapped``, the
    variables a ``preprocessing.multimapper.Multimapper`` replaces): ``internal_data`` / ``internal_model`` drop those
    variables and append the new ones at the end, a remapped forcing hands its new names to ``forcing``; without it
    ``internal_*`` are the plain views."""

    def __init__(self, n_prognostic: int, n_forcing: int = 0, n_diagnostic: int = 0, names=None, remapped=None) -> None:
        prog = [f"prog_{i}" for i in range(n_prognostic)]
        forc = [f"forc_{i}" for i in range(n_forcing)]
        diag = [f"diag_{i}" for i in range(n_diagnostic)]
        if names is not None:  # variable names in dataset order (prognostic, forcing, diagnostic)
            names = list(names)
            assert len(names) == n_prognostic + n_forcing + n_diagnostic
            prog, forc = names[:n_prognostic], names[n_prognostic:n_prognostic + n_forcing]
            diag = names[n_prognostic + n_forcing:]
        inp = _ModelIndex(prog + forc, range(n_prognostic), forcing=range(n_prognostic, n_prognostic + n_forcing))
        out = _ModelIndex(prog + diag, range(n_prognostic),
                          diagnostic=range(n_prognostic, n_prognostic + n_diagnostic))
        self.internal_model = _Internal(inp, out)
        self.model = self.internal_model
        names = prog + forc + diag
        self.name_to_index = {n: i for i, n in enumerate(names)}
        np_, nf = n_prognostic, n_forcing
        d_in = _DataIndex(self.name_to_index, range(np_ + nf), range(np_), forcing=range(np_, np_ + nf))
        d_out = _DataIndex(self.name_to_index, list(range(np_)) + list(range(np_ + nf, len(names))), range(np_),
                           diagnostic=range(np_ + nf, len(names)))
        self.data = _Internal(d_in, d_out)
        self.internal_data = self.data
        self.num_input = len(inp)
        self.num_output = len(out)
        self.remapped = {k: list(v) for k, v in (remapped or {}).items()}
        if self.remapped:
            self._remap(prog + forc, prog + diag, forc, diag)

    def _remap(self, model_in, model_out, forcing, diagnostic) -> None:
        """The two internal views with ``self.remapped`` applied (reference data_indices/collection.py:40-103)."""
        assert set(self.remapped).isdisjoint(diagnostic), "Remapped variable overlap with diagnostic variables. Not implemented."
        assert set(self.remapped).issubset(self.name_to_index), (
            "Remapping a variable that does not exist in the dataset. Check for typos: "
            f"{set(self.remapped).difference(self.name_to_index)}")
        data_names = [n for n in self.name_to_index if n not in self.remapped]
        in_names = [n for n in model_in if n not in self.remapped]
        out_names = [n for n in model_out if n not in self.remapped]
        forcing = list(forcing)
        for key, new in self.remapped.items():
            in_names += new
            data_names += new
            if key in forcing:  # a forcing stays out of the output; its new names are forcings
                forcing += new
                forcing.remove(key)
            else:
                out_names += new

        def pick(names, chosen):
            return sorted(i for i, n in enumerate(names) if n in chosen)

        def without(names, *dropped):
            return sorted(i for i, n in enumerate(names) if not any(n in d for d in dropped))

        inp = _ModelIndex(in_names, without(in_names, forcing), forcing=pick(in_names, forcing))
        out = _ModelIndex(out_names, without(out_names, diagnostic), diagnostic=pick(out_names, diagnostic))
        self.internal_model = _Internal(inp, out)
        name_to_index = {n: i for i, n in enumerate(data_names)}
        d_in = _DataIndex(name_to_index, without(data_names, diagnostic), without(data_names, diagnostic, forcing),
                          diagnostic=pick(data_names, diagnostic), forcing=pick(data_names, forcing))
        d_out = _DataIndex(name_to_index, without(data_names, forcing), without(data_names, diagnostic, forcing),
                           diagnostic=pick(data_names, diagnostic), forcing=pick(data_names, forcing))
        self.internal_data = _Internal(d_in, d_out)


def advance_colmap(data_indices) -> torch.Tensor:
    """int32 ``[V_in]`` column map of the rollout's state advance (``anemoi_advance_input`` / ``anemoi_advance_state``), on
    the CPU: prognostic inputs <- their output column, forcing inputs <- their position in the forcing tensor (-2 - k),
    everything else persists (-1).  Shared by ``AnemoiModelInterface.rollout`` and ``training.RolloutModel``."""
    idx = data_indices.internal_model
    cmap = torch.full((len(idx.input),), -1, dtype=torch.int32)
    cmap[idx.input.prognostic.long()] = idx.output.prognostic.to(torch.int32)
    forcing = idx.input.forcing.long()
    cmap[forcing] = -2 - torch.arange(forcing.numel(), dtype=torch.int32)
    return cmap
