"""Output boundings mirroring reference layers/bounding.py:60-124 (in-place clamps on selected output variables).

Two routes, same arithmetic:

* ``module(x)`` -- the reference's own in-place index assignments in plain torch (any device); what a user calling a
  bounding module directly gets, and what the reference's exact-value tests exercise;
* inside the model (``AnemoiModelEncProcDec._finish``) the whole ``boundings`` list is compiled ONCE into an ordered op
  list (:func:`compile_boundings`) and applied by one kernel, ``anemoi_bound_output`` -- one pass over the touched
  columns instead of 3-5 indexing kernels per module, no host-resident index tensors on the hot path.  The training
  forward runs the same op list through a differentiable kernel pair (``autograd.bound_output``).

``NormalizedReluBounding`` and the four ``Leaky*`` classes restate the published behaviour of current anemoi-models (the
reference checkout predates them).  The leaky ones keep a small gradient outside the bounds: a hard clamp kills the gradient
of precipitation-like variables.
"""

from __future__ import annotations

import math
from abc import ABC
from abc import abstractmethod
from typing import List, Optional, Sequence, Tuple

import torch
from torch import nn

# negative slope of every Leaky* class (as upstream; not configurable)
LEAKY_SLOPE = 0.01


def _indices(variables, name_to_index) -> torch.Tensor:
    """Sorted output columns of ``variables`` (reference data_indices/tensor.py:91-94 ``_build_idx_from_includes``)."""
    missing = [v for v in variables if v not in name_to_index]
    assert not missing, f"Data indexing has invalid entries {missing}, not in dataset."
    return torch.tensor(sorted(name_to_index[v] for v in variables), dtype=torch.int64)


class BaseBounding(nn.Module, ABC):
    def __init__(self, *, variables: list, name_to_index: dict, statistics: Optional[dict] = None,
                 name_to_index_stats: Optional[dict] = None) -> None:
        """``statistics`` / ``name_to_index_stats``: accepted by every class (the models hand them to each bounding), used by
        the normalised ones only."""
        super().__init__()
        self.name_to_index = name_to_index
        self.variables = variables
        self.data_index = self._create_index(variables)

    def _create_index(self, variables: list) -> torch.Tensor:
        return _indices(variables, self.name_to_index)

    @abstractmethod
    def forward(self, x: torch.Tensor) -> torch.Tensor: ...


class ReluBounding(BaseBounding):
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x[..., self.data_index] = torch.nn.functional.relu(x[..., self.data_index])
        return x


class HardtanhBounding(BaseBounding):
    def __init__(self, *, variables: list, name_to_index: dict, min_val: float, max_val: float,
                 statistics: Optional[dict] = None, name_to_index_stats: Optional[dict] = None) -> None:
        super().__init__(variables=variables, name_to_index=name_to_index)
        self.min_val = min_val
        self.max_val = max_val

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x[..., self.data_index] = torch.nn.functional.hardtanh(x[..., self.data_index], min_val=self.min_val,
                                                               max_val=self.max_val)
        return x


class FractionBounding(HardtanhBounding):
    def __init__(self, *, variables: list, name_to_index: dict, min_val: float, max_val: float,
                 total_var: str, statistics: Optional[dict] = None, name_to_index_stats: Optional[dict] = None) -> None:
        super().__init__(variables=variables, name_to_index=name_to_index, min_val=min_val, max_val=max_val)
        self.total_variable = self._create_index([total_var])

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = super().forward(x)
        x[..., self.data_index] *= x[..., self.total_variable]
        return x


def _leaky_hardtanh(v: torch.Tensor, lo: float, hi: float) -> torch.Tensor:
    """``v`` inside ``[lo, hi]``, ``bound + LEAKY_SLOPE * (v - bound)`` outside (a NaN stays a NaN).  ``<=`` / ``>=`` change no
    value; they give autograd the slope AT a bound, as torch's relu / hardtanh / leaky_relu have it."""
    v = torch.where(v <= lo, lo + LEAKY_SLOPE * (v - lo), v)
    return torch.where(v >= hi, hi + LEAKY_SLOPE * (v - hi), v)


class LeakyReluBounding(BaseBounding):
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x[..., self.data_index] = torch.nn.functional.leaky_relu(x[..., self.data_index], negative_slope=LEAKY_SLOPE)
        return x


class LeakyHardtanhBounding(HardtanhBounding):
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x[..., self.data_index] = _leaky_hardtanh(x[..., self.data_index], self.min_val, self.max_val)
        return x


class LeakyFractionBounding(FractionBounding):
    """The leaky hardtanh, then the product with ``total_var`` (read before any write, as in ``FractionBounding``)."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x[..., self.data_index] = _leaky_hardtanh(x[..., self.data_index], self.min_val, self.max_val)
        x[..., self.data_index] *= x[..., self.total_variable]
        return x


NORMALIZERS = ("mean-std", "min-max", "max", "std")


class NormalizedReluBounding(BaseBounding):
    """``x[..., idx] = relu(x[..., idx] - t) + t`` with one threshold per variable: ``min_val[i]``, a physical value, taken
    into the normalised space the model output lives in by ``normalizer[i]`` and the dataset statistics of ``variables[i]``.

    Threshold ``i`` belongs to ``variables[i]`` BY NAME: ``data_index`` is built in ``variables`` order here (not sorted, as in
    the other classes), so ``data_index[i]`` and ``norm_min_val[i]`` speak of the same variable whatever order the config
    lists them in.  The thresholds are held as f32 (a plain attribute: no parameter, no buffer)."""

    def __init__(self, *, variables: list, name_to_index: dict, min_val: list, normalizer: list,
                 statistics: Optional[dict] = None, name_to_index_stats: Optional[dict] = None) -> None:
        super().__init__(variables=variables, name_to_index=name_to_index)
        min_val, normalizer = list(min_val), list(normalizer)
        if statistics is None or name_to_index_stats is None:
            raise ValueError(f"{type(self).__name__} needs statistics and name_to_index_stats")
        if not (len(variables) == len(min_val) == len(normalizer)):
            raise ValueError(f"{type(self).__name__}: variables ({len(variables)}), min_val ({len(min_val)}) and normalizer "
                             f"({len(normalizer)}) must have one entry per variable")
        if len(set(variables)) != len(variables):
            raise ValueError(f"{type(self).__name__}: a variable is listed twice in {list(variables)}")
        unknown = [n for n in normalizer if n not in NORMALIZERS]
        if unknown:
            raise ValueError(f"{type(self).__name__}: normalizer {unknown} not in {list(NORMALIZERS)}")
        self.min_val = min_val
        self.normalizer = normalizer
        stat = lambda name, j: float(torch.as_tensor(statistics[name]).reshape(-1)[j])  # noqa: E731
        thresholds = []
        for var, m, kind in zip(variables, min_val, normalizer):
            j = name_to_index_stats[var]
            if kind == "mean-std":
                t = (m - stat("mean", j)) / stat("stdev", j)
            elif kind == "min-max":
                t = (m - stat("minimum", j)) / (stat("maximum", j) - stat("minimum", j))
            elif kind == "max":
                t = m / stat("maximum", j)
            else:
                t = m / stat("stdev", j)
            thresholds.append(t)
        self.norm_min_val = torch.tensor(thresholds, dtype=torch.float32)

    def _create_index(self, variables: list) -> torch.Tensor:
        missing = [v for v in variables if v not in self.name_to_index]
        assert not missing, f"Data indexing has invalid entries {missing}, not in dataset."
        return torch.tensor([self.name_to_index[v] for v in variables], dtype=torch.int64)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        t = self.norm_min_val.to(device=x.device, dtype=x.dtype)
        x[..., self.data_index] = torch.nn.functional.relu(x[..., self.data_index] - t) + t
        return x


class LeakyNormalizedReluBounding(NormalizedReluBounding):
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        t = self.norm_min_val.to(device=x.device, dtype=x.dtype)
        x[..., self.data_index] = torch.nn.functional.leaky_relu(x[..., self.data_index] - t, negative_slope=LEAKY_SLOPE) + t
        return x


# one op = (column, lo, hi, multiplier column or -1), and beside it one slope; see include/anemoi_amd.h: anemoi_bound_output
# and anemoi_bound_output_leaky:  v < lo: lo + s (v - lo);  v > hi: hi + s (v - hi);  else v;  then * y[mul] when mul >= 0
Op = Tuple[int, float, float, int]


def _compile(boundings: Sequence[nn.Module]) -> Optional[Tuple[List[Op], List[float]]]:
    ops: List[Op] = []
    slopes: List[float] = []
    for b in boundings:
        kind = type(b)
        s = LEAKY_SLOPE if kind in (LeakyReluBounding, LeakyHardtanhBounding, LeakyFractionBounding,
                                    LeakyNormalizedReluBounding) else 0.0
        cols = sorted(set(int(c) for c in b.data_index))
        if kind in (NormalizedReluBounding, LeakyNormalizedReluBounding):
            # one op per variable in ``variables`` order, each with its own threshold (the f32 value the module route uses)
            ops += [(int(c), float(t), math.inf, -1) for c, t in zip(b.data_index, b.norm_min_val)]
        elif kind in (ReluBounding, LeakyReluBounding):
            ops += [(c, 0.0, math.inf, -1) for c in cols]
        elif kind in (HardtanhBounding, LeakyHardtanhBounding):
            ops += [(c, float(b.min_val), float(b.max_val), -1) for c in cols]
        elif kind in (FractionBounding, LeakyFractionBounding):
            total = int(b.total_variable[0])
            ops += [(c, float(b.min_val), float(b.max_val), -1) for c in cols]
            # ``x[..., idx] *= x[..., total]`` reads the total BEFORE any write: if the total is itself bounded by this
            # module its own product goes last.  (lo = -inf, hi = +inf: neither branch is taken, the slope plays no part)
            ops += [(c, -math.inf, math.inf, total) for c in cols if c != total]
            ops += [(c, -math.inf, math.inf, total) for c in cols if c == total]
        else:
            return None
        slopes += [s] * (len(ops) - len(slopes))
    return ops, slopes


def compile_boundings(boundings: Sequence[nn.Module]) -> Optional[List[Op]]:
    """The ordered op list equivalent to calling ``boundings`` one after the other, or ``None`` when the list holds a
    class this module does not know (a user subclass: the model then calls the modules themselves).  The slopes of a list
    with leaky classes travel beside it: :func:`bounding_slopes`."""
    compiled = _compile(boundings)
    return None if compiled is None else compiled[0]


def bounding_slopes(boundings: Sequence[nn.Module]) -> Optional[List[float]]:
    """One slope per op of :func:`compile_boundings` (0 for a hard op), or ``None`` when every op is hard -- the kernels of
    the hard classes are then launched exactly as before -- or the list does not compile."""
    compiled = _compile(boundings)
    if compiled is None or not any(compiled[1]):
        return None
    return compiled[1]


def bounded_columns(ops: Sequence[Op]) -> List[int]:
    """Columns an op list writes or reads: they must stay normalised until the boundings have run."""
    return sorted({c for c, _, _, _ in ops} | {m for _, _, _, m in ops if m >= 0})
