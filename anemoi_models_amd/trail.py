"""Launch trail: one digest record per output buffer of every kernel-library call, and a first-difference finder.

    with trail.record(capacity=4096) as t:
        y = model(x)
    t.entries                      # [TrailEntry(index, name, dtype, rows, cols, digest, nonfinite, absmax), ...]
    t.first_nonfinite()            # the first launch that produced a NaN / Inf, or None
    trail.first_difference(a, b)   # (index, entry_a, entry_b) of the first record that differs between two trails, or None

While a trail is armed, every entry point of ``include/anemoi_amd.h`` that writes device memory appends a 32-byte record per
output, computed on the device by ``csrc/trail.hip`` on the stream of the call (header section "Launch trail": the digest is
an integer sum, identical from run to run and reproducible on the host).  The block-level entry points run six to eight
kernels behind one C call; each of those appears with its own records.

Limits: eager execution only (no HIP-graph capture); the trail belongs to the host thread that armed it -- ``record()``
therefore runs autograd's backward on the calling thread for its duration -- and to this process (one trail per rank);
ATen ops between the launches are invisible unless their results are added with :func:`mark`.
"""

from __future__ import annotations

import contextlib
import ctypes
import json
import struct
from typing import List
from typing import NamedTuple
from typing import Optional
from typing import Tuple

import torch
from torch import Tensor

from . import _lib

RECORD_BYTES = 32
_DTYPE_NAMES = {_lib.F32: "f32", _lib.BF16: "bf16", _lib.I32: "i32", _lib.U8: "u8"}
_DTYPE_CODES = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.int32: _lib.I32, torch.uint8: _lib.U8}


class TrailEntry(NamedTuple):
    index: int
    name: str      # "<entry point>:<output>", or the name given to mark()
    dtype: str     # "f32" | "bf16" | "i32" | "u8"
    rows: int
    cols: int
    digest: int    # u64
    nonfinite: int
    absmax: float  # largest finite |x| (0.0 if there is none)

    def same_as(self, other: "TrailEntry") -> bool:
        """Name, dtype, shape and digest agree (the digest covers every bit of the buffer)."""
        return (self.name, self.dtype, self.rows, self.cols, self.digest) == (
            other.name, other.dtype, other.rows, other.cols, other.digest)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _decode(raw: Tensor, metas) -> List[TrailEntry]:
    """``raw``: int64 CPU tensor [n, 4] of the records; ``metas``: [(name, dtype code, rows, cols)]."""
    out = []
    words = raw.tolist()
    for i, (name, code, rows, cols) in enumerate(metas):
        w = words[i]
        absmax = struct.unpack("<f", struct.pack("<I", w[2] & 0xFFFFFFFF))[0]
        out.append(TrailEntry(i, name, _DTYPE_NAMES[code], rows, cols, w[0] & 0xFFFFFFFFFFFFFFFF,
                              w[1] & 0xFFFFFFFFFFFFFFFF, absmax))
    return out


class Trail:
    """The records of one :func:`record` block (filled when the block is left) or of :func:`load`."""

    def __init__(self, entries: Optional[List[TrailEntry]] = None, dropped: int = 0):
        self.entries: List[TrailEntry] = list(entries or [])
        self.dropped = dropped

    def __len__(self) -> int:
        return len(self.entries)

    def names(self) -> List[str]:
        return [e.name for e in self.entries]

    def first_nonfinite(self) -> Optional[TrailEntry]:
        return next((e for e in self.entries if e.nonfinite > 0), None)

    def save(self, path: str) -> None:
        with open(path, "w") as f:
            json.dump({"dropped": self.dropped,
                       "entries": [{**e._asdict(), "digest": f"{e.digest:016x}"} for e in self.entries]}, f, indent=1)


def load(path: str) -> Trail:
    with open(path) as f:
        doc = json.load(f)
    return Trail([TrailEntry(**{**e, "digest": int(e["digest"], 16)}) for e in doc["entries"]], doc["dropped"])


def first_difference(a: Trail, b: Trail) -> Optional[Tuple[int, Optional[TrailEntry], Optional[TrailEntry]]]:
    """``(index, entry_a, entry_b)`` of the first record whose name, shape or digest differ (the missing side is None where
    one trail is a strict prefix of the other), or None if the trails agree."""
    for ea, eb in zip(a.entries, b.entries):
        if not ea.same_as(eb):
            return ea.index, ea, eb
    if len(a.entries) != len(b.entries):
        i = min(len(a.entries), len(b.entries))
        return i, (a.entries[i] if i < len(a.entries) else None), (b.entries[i] if i < len(b.entries) else None)
    return None


def _armed_error() -> None:
    if torch.cuda.is_current_stream_capturing():
        raise NotImplementedError("a launch trail cannot record while the stream is being captured into a HIP graph "
                                  "(eager execution only)")


@contextlib.contextmanager
def record(capacity: int = 4096):
    """Arm a trail of at most ``capacity`` records on the current device for the duration of the block; the :class:`Trail`
    it yields is filled (after a device synchronisation) when the block is left, also on an exception."""
    lib = _lib.load()
    if capacity <= 0:
        raise ValueError(f"trail capacity {capacity} is not positive")
    _armed_error()
    buf = torch.empty(capacity * RECORD_BYTES // 8, dtype=torch.int64, device="cuda")
    t = Trail()
    _lib.check(lib.anemoi_trail_begin(buf.data_ptr(), capacity), "anemoi_trail_begin")
    try:
        # the trail is thread-local and autograd would run the backward kernels on its own device thread
        with torch.autograd.set_multithreading_enabled(False):
            yield t
    finally:
        n, dropped = ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(lib.anemoi_trail_end(ctypes.byref(n), ctypes.byref(dropped)), "anemoi_trail_end")
        metas = []
        name, code = ctypes.c_char_p(), ctypes.c_int(0)
        rows, cols = ctypes.c_int64(0), ctypes.c_int64(0)
        for i in range(n.value):
            _lib.check(lib.anemoi_trail_entry(i, ctypes.byref(name), ctypes.byref(code), ctypes.byref(rows),
                                              ctypes.byref(cols)), "anemoi_trail_entry")
            metas.append((name.value.decode(), code.value, rows.value, cols.value))
        torch.cuda.synchronize()
        t.entries = _decode(buf[: n.value * 4].cpu().view(-1, 4), metas)
        t.dropped = dropped.value


def _as_matrix(tensor: Tensor) -> Tuple[Tensor, int, int, int]:
    """(tensor, rows, cols, ld): a 2-D tensor with unit inner stride as it stands (slices keep their leading dimension),
    anything else flattened to one row of its elements in logical order."""
    if tensor.dtype not in _DTYPE_CODES:
        raise NotImplementedError(f"launch trail: dtype {tensor.dtype} is none of float32, bfloat16, int32, uint8")
    if not tensor.is_cuda:
        raise RuntimeError("launch trail: the digest kernel runs on the GPU (tests/_trail_ref.py has the host reference)")
    if tensor.dim() == 2 and (tensor.shape[1] <= 1 or tensor.stride(1) == 1) and (
            tensor.shape[0] <= 1 or tensor.stride(0) >= tensor.shape[1]):
        rows, cols = tensor.shape
        return tensor, rows, cols, (tensor.stride(0) if rows > 1 else max(cols, 1))
    flat = tensor.contiguous().view(1, -1)
    return flat, 1, flat.shape[1], max(flat.shape[1], 1)


def mark(name: str, tensor: Tensor) -> None:
    """Add ``tensor`` to the armed trail under ``name`` (the result of an ATen op between two launches); a no-op when no
    trail is armed."""
    lib = _lib.load()
    m, rows, cols, ld = _as_matrix(tensor)
    _lib.check(lib.anemoi_trail_note(name.encode(), _DTYPE_CODES[m.dtype], m.data_ptr(), ld, rows, cols, _stream()),
               "anemoi_trail_note")


def digest(tensor: Tensor, name: str = "digest") -> TrailEntry:
    """One record of one 2-D (or flattened) tensor: the digest kernel as a plain op.  Not to be called inside a
    :func:`record` block (use :func:`mark` there)."""
    with record(capacity=1) as t:
        mark(name, tensor)
    return t.entries[0]
