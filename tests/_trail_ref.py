"""Host references of the launch-trail record (include/anemoi_amd.h, "Launch trail"), independent of csrc/trail.hip.

    digest    = sum_i (b_i + 1) * m(i) mod 2^64,  i = r * cols + c,  m(i) = ((i + 1) * 0x9E3779B97F4A7C15 mod 2^64) | 1
    nonfinite = number of NaN / +-Inf elements (0 for the integer dtypes)
    absmax    = largest |x| over the finite elements (bf16 widened), 0 if there is none

``numpy_record`` works in uint64 (wrap-around = mod 2^64); ``torch_record`` works in int64 -- two's-complement wrap-around
is the same arithmetic -- in row chunks on the tensor's own device, so it also covers matrices of more than 2^32 elements.
Both take a 2-D tensor as the caller sees it (a strided slice included): only the logical elements enter.
"""

import numpy as np
import torch

GOLDEN = 0x9E3779B97F4A7C15
MASK = (1 << 64) - 1


def m(i: int) -> int:
    return (((i + 1) * GOLDEN) & MASK) | 1


def _bits_numpy(t: torch.Tensor) -> np.ndarray:
    """The elements' bit patterns, zero-extended to uint64, in logical (row-major) order."""
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy().view(np.uint32).astype(np.uint64).reshape(-1)
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).numpy().view(np.uint16).astype(np.uint64).reshape(-1)
    if t.dtype == torch.int32:
        return t.numpy().view(np.uint32).astype(np.uint64).reshape(-1)
    if t.dtype == torch.uint8:
        return t.numpy().astype(np.uint64).reshape(-1)
    raise TypeError(t.dtype)


def numpy_record(t: torch.Tensor):
    """(digest, nonfinite, absmax) of a 2-D tensor by the definition, in numpy uint64."""
    assert t.dim() == 2
    b = _bits_numpy(t)
    n = b.shape[0]
    with np.errstate(over="ignore"):
        idx = np.arange(1, n + 1, dtype=np.uint64)
        mult = (idx * np.uint64(GOLDEN)) | np.uint64(1)
        digest = int(((b + np.uint64(1)) * mult).sum(dtype=np.uint64)) if n else 0
    if t.dtype in (torch.float32, torch.bfloat16):
        f = t.detach().cpu().float().reshape(-1)
        finite = torch.isfinite(f)
        nonfinite = int((~finite).sum())
        absmax = float(f[finite].abs().max()) if bool(finite.any()) else 0.0
    else:
        nonfinite, absmax = 0, 0.0
    return digest & MASK, nonfinite, absmax


def _bits_torch(t: torch.Tensor) -> torch.Tensor:
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    if t.dtype == torch.bfloat16:
        return t.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF
    if t.dtype == torch.int32:
        return t.to(torch.int64) & 0xFFFFFFFF
    if t.dtype == torch.uint8:
        return t.to(torch.int64)
    raise TypeError(t.dtype)


def torch_record(t: torch.Tensor, chunk_rows: int = 0):
    """(digest, nonfinite, absmax) of a 2-D tensor in torch int64 arithmetic on ``t.device``, ``chunk_rows`` rows at a time
    (0: a chunk of about 2^24 elements)."""
    assert t.dim() == 2
    rows, cols = t.shape
    if chunk_rows <= 0:
        chunk_rows = max(1, (1 << 24) // max(cols, 1))
    golden = GOLDEN - (1 << 64)  # the same 64 bits as a signed value
    digest, nonfinite, absmax = 0, 0, 0.0
    col_idx = torch.arange(cols, dtype=torch.int64, device=t.device)
    for r0 in range(0, rows, chunk_rows):
        part = t[r0 : r0 + chunk_rows]
        nr = part.shape[0]
        idx = (torch.arange(r0, r0 + nr, dtype=torch.int64, device=t.device) * cols).unsqueeze(1) + col_idx + 1
        mult = (idx * golden) | 1
        digest = (digest + int(((_bits_torch(part) + 1) * mult).sum())) & MASK  # int64 sum wraps: mod 2^64
        if t.dtype in (torch.float32, torch.bfloat16):
            f = part.float()
            finite = torch.isfinite(f)
            nonfinite += int((~finite).sum())
            if bool(finite.any()):
                absmax = max(absmax, float(torch.where(finite, f.abs(), torch.zeros_like(f)).max()))
    return digest & MASK, nonfinite, absmax
