"""Truncated residual connection: the matrices of ``x_skip = A_up (A_down x[:, -1])`` and their device copies.

Current anemoi-models hands its models ``truncation_data = {"down": A_down, "up": A_up}``, two sparse interpolation matrices,
and adds the last input state projected to a coarser grid and back instead of the state itself: the network learns the small
scales, the residual carries the large ones.  The reference checkout this package mirrors predates that code: this is a
restatement of the published behaviour, not a port.

:class:`TruncationPlan` is NOT an ``nn.Module``: it has no parameters and no buffers, so the ``state_dict`` of a model with
truncation is key for key that of the model without.  It canonicalises the matrices once on the host (CSR, duplicates summed,
columns ascending within a row, indices checked) and caches their device copies and transposes per device
(:meth:`TruncationPlan.on`); ``csr_project`` of ``anemoi_models_amd.ops`` does the arithmetic.
"""

from __future__ import annotations

import os
from typing import NamedTuple
from typing import Optional

import numpy as np
import torch
from torch import Tensor

from .. import ops


class CsrMatrix(NamedTuple):
    """Canonical CSR: ``indptr`` int64 ``[rows + 1]``, ``idx`` int32 (ascending within a row, no repeats), ``val`` float32."""

    indptr: Tensor
    idx: Tensor
    val: Tensor
    shape: tuple

    def to(self, device) -> "CsrMatrix":
        return CsrMatrix(self.indptr.to(device), self.idx.to(device), self.val.to(device), self.shape)

    def transpose(self) -> "CsrMatrix":
        t = ops.csr_transpose(self.indptr, self.idx, self.val, self.shape[1])
        return CsrMatrix(t[0], t[1], t[2], (self.shape[1], self.shape[0]))

    def to_sparse_coo(self, device=None, dtype=torch.float32) -> Tensor:
        counts = self.indptr[1:] - self.indptr[:-1]
        rows = torch.repeat_interleave(torch.arange(self.shape[0], dtype=torch.int64), counts.cpu())
        m = torch.sparse_coo_tensor(torch.stack([rows, self.idx.cpu().long()]), self.val.cpu().to(dtype), self.shape)
        return m.coalesce().to(device) if device is not None else m.coalesce()


def _coo_to_canonical(rows, cols, vals, shape, name: str) -> CsrMatrix:
    rows = np.asarray(rows).astype(np.int64).reshape(-1)
    cols = np.asarray(cols).astype(np.int64).reshape(-1)
    vals = np.asarray(vals).astype(np.float64).reshape(-1)
    n_rows, n_cols = (int(s) for s in shape)
    if n_rows < 0 or n_cols < 0 or not (rows.size == cols.size == vals.size):
        raise ValueError(f"truncation matrix {name!r}: malformed sparse matrix of shape {tuple(shape)}")
    if rows.size and (rows.min() < 0 or rows.max() >= n_rows or cols.min() < 0 or cols.max() >= n_cols):
        raise ValueError(f"truncation matrix {name!r}: index out of range for shape ({n_rows}, {n_cols})")
    if n_cols >= 2 ** 31 or rows.size >= 2 ** 62:
        raise ValueError(f"truncation matrix {name!r}: {n_cols} columns do not fit int32 indices")
    order = np.lexsort((cols, rows))  # by row, then column (stable)
    rows, cols, vals = rows[order], cols[order], vals[order]
    if rows.size:
        first = np.ones(rows.size, dtype=bool)
        first[1:] = (rows[1:] != rows[:-1]) | (cols[1:] != cols[:-1])
        starts = np.flatnonzero(first)
        vals = np.add.reduceat(vals, starts)  # duplicates summed (f64, rounded once)
        rows, cols = rows[starts], cols[starts]
    indptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n_rows), out=indptr[1:])
    return CsrMatrix(torch.from_numpy(indptr), torch.from_numpy(cols.astype(np.int32)),
                     torch.from_numpy(vals.astype(np.float32)), (n_rows, n_cols))


def _compressed_to_coo(indptr, indices, n_major: int, name: str):
    indptr = np.asarray(indptr).astype(np.int64).reshape(-1)
    indices = np.asarray(indices).reshape(-1)
    if indptr.size != n_major + 1 or (indptr.size and (indptr[0] != 0 or indptr[-1] != indices.size)) or np.any(np.diff(indptr) < 0):
        raise ValueError(f"truncation matrix {name!r}: indptr does not match its shape / index list")
    return np.repeat(np.arange(n_major, dtype=np.int64), np.diff(indptr))


def load_npz(path) -> tuple:
    """``(rows, cols, values, shape)`` of an ``.npz`` in the layout of ``scipy.sparse.save_npz``, read with numpy only: keys
    ``format`` / ``shape`` / ``data`` and ``indices`` + ``indptr`` (csr, csc) or ``row`` + ``col`` (coo)."""
    with np.load(os.fspath(path), allow_pickle=False) as f:
        if "format" not in f.files or "shape" not in f.files or "data" not in f.files:
            raise ValueError(f"{path}: not a scipy.sparse.save_npz file (keys {sorted(f.files)})")
        fmt = f["format"].item()
        fmt = fmt.decode() if isinstance(fmt, bytes) else str(fmt)
        shape = tuple(int(s) for s in f["shape"])
        data = f["data"]
        if fmt in ("csr", "csc"):
            indices, indptr = f["indices"], f["indptr"]
            major = _compressed_to_coo(indptr, indices, shape[0] if fmt == "csr" else shape[1], os.fspath(path))
            rows, cols = (major, indices) if fmt == "csr" else (indices, major)
        elif fmt == "coo":
            rows, cols = f["row"], f["col"]
        else:
            raise ValueError(f"{path}: sparse format {fmt!r} is not supported (csr, csc, coo)")
        return np.asarray(rows), np.asarray(cols), np.asarray(data), shape


def canonical_csr(matrix, name: str = "matrix") -> CsrMatrix:
    """Any accepted form of one matrix -> :class:`CsrMatrix` on the host: a scipy sparse matrix (anything with ``.tocsr()``), a
    torch sparse COO / CSR tensor, an ``(indptr, indices, values, shape)`` tuple, or the path of a ``save_npz`` file."""
    if isinstance(matrix, CsrMatrix):
        matrix = tuple(matrix)
    if isinstance(matrix, (str, os.PathLike)):
        return _coo_to_canonical(*load_npz(matrix), name)
    if isinstance(matrix, Tensor):
        if matrix.layout == torch.sparse_coo:
            ind = matrix._indices().cpu().numpy()
            return _coo_to_canonical(ind[0], ind[1], matrix._values().detach().cpu().double().numpy(), matrix.shape, name)
        if matrix.layout == torch.sparse_csr:
            crow, col = matrix.crow_indices().cpu().numpy(), matrix.col_indices().cpu().numpy()
            rows = _compressed_to_coo(crow, col, matrix.shape[0], name)
            return _coo_to_canonical(rows, col, matrix.values().detach().cpu().double().numpy(), matrix.shape, name)
        raise TypeError(f"truncation matrix {name!r}: a dense tensor is not accepted (sparse COO / CSR)")
    if hasattr(matrix, "tocsr"):
        m = matrix.tocsr()
        rows = _compressed_to_coo(m.indptr, m.indices, m.shape[0], name)
        return _coo_to_canonical(rows, m.indices, m.data, m.shape, name)
    if isinstance(matrix, (tuple, list)) and len(matrix) == 4:
        indptr, indices, values, shape = matrix
        as_np = lambda t: t.detach().cpu().numpy() if isinstance(t, Tensor) else np.asarray(t)  # noqa: E731
        rows = _compressed_to_coo(as_np(indptr), as_np(indices), int(shape[0]), name)
        return _coo_to_canonical(rows, as_np(indices), as_np(values), shape, name)
    raise TypeError(f"truncation matrix {name!r}: unsupported type {type(matrix).__name__}")


class DeviceTruncation(NamedTuple):
    """The stages of one plan on one device, in the order the forward applies them, and their transposes (same order)."""

    stages: tuple    # CsrMatrix per stage: (down, up), or the one matrix present
    stages_t: tuple  # their transposes


class TruncationPlan:
    """``truncation_data`` of a model: ``{"down": A_down [G_c, G], "up": A_up [G, G_c]}``; either may be absent (the one left
    must then be ``[G, G]``), none at all is an empty plan (``bool(plan)`` is False: today's untruncated residual)."""

    def __init__(self, truncation_data=None, grid_size: Optional[int] = None) -> None:
        data = dict(truncation_data or {})
        unknown = set(data) - {"down", "up"}
        if unknown:
            raise ValueError(f"truncation_data: unknown keys {sorted(unknown)} (expected 'down' and / or 'up')")
        self.down = canonical_csr(data["down"], "down") if data.get("down") is not None else None
        self.up = canonical_csr(data["up"], "up") if data.get("up") is not None else None
        self.stages = tuple(m for m in (self.down, self.up) if m is not None)
        self._device: dict = {}
        if not self.stages:
            self.grid_size = grid_size
            return
        shapes = " , ".join(f"{n} {tuple(m.shape)}" for n, m in (("down", self.down), ("up", self.up)) if m is not None)
        if len(self.stages) == 2 and self.down.shape[0] != self.up.shape[1]:
            raise ValueError(f"truncation_data: up does not take what down gives: {shapes}")
        g_in, g_out = self.stages[0].shape[1], self.stages[-1].shape[0]
        if g_in != g_out or (grid_size is not None and g_in != int(grid_size)):
            want = f"G = {int(grid_size)}" if grid_size is not None else "one grid"
            raise ValueError(f"truncation_data: the composition must map {want} -> G, got {shapes}")
        self.grid_size = g_in

    def __bool__(self) -> bool:
        return bool(self.stages)

    def on(self, device, cache: Optional[dict] = None) -> DeviceTruncation:
        """Device copies and transposes, built once per device; ``cache``: the owner's per-device cache (a model's ``_idx_cache``)."""
        cache = self._device if cache is None else cache
        key = ("truncation", id(self), str(device))
        if key not in cache:
            cache[key] = DeviceTruncation(tuple(m.to(device) for m in self.stages),
                                          tuple(m.transpose().to(device) for m in self.stages))
        return cache[key]

    def sparse(self, device, dtype=torch.float32, cache: Optional[dict] = None) -> list:
        """torch sparse COO copies of the stages on ``device``, cached like :meth:`on` (the composed torch route of
        ``training._finish``, which restates upstream's ``torch.sparse.mm`` composition)."""
        cache = self._device if cache is None else cache
        key = ("truncation_sparse", id(self), str(device), dtype)
        if key not in cache:
            cache[key] = [m.to_sparse_coo(device, dtype) for m in self.stages]
        return cache[key]


REFUSAL = "the truncated residual connection is single-device: its projection is not row-local (no node partitioning)"


def project_add(y: Tensor, x_last: Tensor, dev: DeviceTruncation, out_idx: Tensor, in_idx: Tensor, in_affine=None) -> Tensor:
    """``y[..., out_idx] += A_up (A_down x'[..., in_idx])`` in place: ``y`` f32 ``[B, Ens, G, V_out]``, ``x_last`` f32 ``[B, Ens,
    G, V_in]`` (any slab strides), ``x' = x * mul + add`` with ``in_affine``.  Only the prognostic columns are projected."""
    if len(dev.stages) == 1:
        m = dev.stages[0]
        return ops.csr_project(x_last, y, m.indptr, m.idx, m.val, in_idx, out_idx, in_affine, accumulate=True)
    down, up = dev.stages
    mid = torch.empty((y.shape[0], y.shape[1], down.shape[0], in_idx.numel()), dtype=torch.float32, device=y.device)
    ops.csr_project(x_last, mid, down.indptr, down.idx, down.val, in_idx, None, in_affine)
    return ops.csr_project(mid, y, up.indptr, up.idx, up.val, None, out_idx, None, accumulate=True)


def project_add_backward(dy: Tensor, dev: DeviceTruncation, out_idx: Tensor, in_idx: Tensor, x_shape) -> Tensor:
    """Input gradient of :func:`project_add` (no affine): ``dx`` f32 ``[B, T, Ens, G, V_in]``, zero except ``dx[:, -1, ..., in_idx] =
    A_down^T (A_up^T dy[..., out_idx])``.  ``in_idx`` must not repeat a column (each is stored once)."""
    dx = torch.zeros(tuple(x_shape), dtype=torch.float32, device=dy.device)
    dx_last = dx[:, -1]
    if len(dev.stages) == 1:
        m = dev.stages_t[0]
        ops.csr_project(dy, dx_last, m.indptr, m.idx, m.val, out_idx, in_idx)
        return dx
    down_t, up_t = dev.stages_t
    mid = torch.empty((dy.shape[0], dy.shape[1], up_t.shape[0], out_idx.numel()), dtype=torch.float32, device=dy.device)
    ops.csr_project(dy, mid, up_t.indptr, up_t.idx, up_t.val, out_idx, None)
    ops.csr_project(mid, dx_last, down_t.indptr, down_t.idx, down_t.val, None, in_idx)
    return dx
