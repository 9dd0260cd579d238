"""Tensor-level wrappers over the C ABI (``include/anemoi_amd.h``).

Every function takes torch tensors that live on an MI355X, passes raw device pointers, sizes and the
current HIP stream to ``libanemoi_amd.so`` and returns torch tensors.  PyTorch is used for device
memory and streams only.  There is deliberately no CPU implementation behind these names: calling
them with CPU tensors raises.  (CPU tests of the host logic substitute this module's functions from
``tests/``; the package itself never does.)
"""

from __future__ import annotations

import ctypes
import os
from typing import NamedTuple
from typing import Optional

import torch
from torch import Tensor

from . import _lib

_DT = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16}

# Optional per-launch timing used by bench.py's roofline leg (never active inside a timed region):
# when PROFILE is a list, every wrapper appends (kernel name, start event, end event, work dict) with the
# events recorded on the stream the kernel is launched on.
PROFILE: Optional[list] = None


class _Timed:
    __slots__ = ("name", "work", "start", "launched")

    def __init__(self, name: str, **work) -> None:
        self.name, self.work, self.start = name, work, None
        self.launched = True  # set to False inside the block when the library refused the call and launched nothing

    def __enter__(self):
        if PROFILE is not None:
            self.start = torch.cuda.Event(enable_timing=True)
            self.start.record(torch.cuda.current_stream())
        return self

    def __exit__(self, *exc):
        if self.start is not None and self.launched:
            end = torch.cuda.Event(enable_timing=True)
            end.record(torch.cuda.current_stream())
            PROFILE.append((self.name, self.start, end, self.work))
        return False


def dtype_code(dtype: torch.dtype) -> int:
    try:
        return _DT[dtype]
    except KeyError:
        raise NotImplementedError(f"compute dtype {dtype} is not supported (float32 or bfloat16)") from None


def k_multiple(dtype: torch.dtype) -> int:
    """The K dimension of a Linear must be a multiple of this many elements (128-byte K-slabs)."""
    return 128 // torch.empty((), dtype=dtype).element_size()


def round_up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def _dev(*tensors: Optional[Tensor]) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                "anemoi_models_amd kernels run on an MI355X only: got a CPU tensor (there is no CPU fallback)"
            )


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream() -> int:
    """hipStream_t of torch's current stream on the current device (the raw getter skips the Stream object)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _rows(t: Tensor) -> Tensor:
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"expected a row-major 2-D tensor (unit inner stride), got shape {tuple(t.shape)} "
                         f"strides {t.stride()}")
    return t


def _ld(t: Tensor) -> int:
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def _ptr(t: Optional[Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def layer_norm(x: Tensor, weight: Tensor, bias: Tensor, eps: float = 1e-5, out: Optional[Tensor] = None,
               residual: Optional[Tensor] = None) -> Tensor:
    """``LayerNorm(x)`` (``+ residual`` in the same pass: the trailing LayerNorm of an MLP followed by its skip connection)."""
    _dev(x, weight, bias, out, residual)
    _rows(x)
    if out is None:
        out = torch.empty((x.shape[0], x.shape[1]), dtype=x.dtype, device=x.device)
    if residual is not None and (residual.dtype != x.dtype or residual.shape != x.shape):
        raise ValueError("layer_norm: the residual must have the shape and dtype of x")
    if x.shape[0] == 0:  # (an empty tensor has no storage: the library would see null pointers)
        return out
    if residual is not None:
        with _Timed("layer_norm", bytes=3 * x.shape[0] * x.shape[1] * x.element_size()):
            st = _lib.load().anemoi_layer_norm_residual(dtype_code(x.dtype), x.data_ptr(), _ld(x), weight.data_ptr(),
                                                        bias.data_ptr(), residual.data_ptr(), _ld(_rows(residual)),
                                                        out.data_ptr(), _ld(_rows(out)), x.shape[0], x.shape[1], eps, _stream())
        _lib.check(st, "anemoi_layer_norm_residual")
        return out
    with _Timed("layer_norm", bytes=2 * x.shape[0] * x.shape[1] * x.element_size()):
        st = _lib.load().anemoi_layer_norm(dtype_code(x.dtype), x.data_ptr(), _ld(x), weight.data_ptr(),
                                           bias.data_ptr(), out.data_ptr(), _ld(_rows(out)), x.shape[0], x.shape[1],
                                           eps, _stream())
    _lib.check(st, "anemoi_layer_norm")
    return out


def layer_norm_with_stats(x: Tensor, weight: Tensor, bias: Tensor, eps: float = 1e-5):
    """``(LayerNorm(x), row statistics [M, 2] f32 = (rstd, -mean * rstd))`` from ONE pass over ``x`` (the training forward
    keeps the statistics for the backward; ``row_stats`` + ``layer_norm`` read ``x`` twice)."""
    _dev(x, weight, bias)
    _rows(x)
    out = torch.empty((x.shape[0], x.shape[1]), dtype=x.dtype, device=x.device)
    stats = torch.empty((x.shape[0], 2), dtype=torch.float32, device=x.device)
    if x.shape[0] == 0:
        return out, stats
    st = _lib.load().anemoi_layer_norm_stats(dtype_code(x.dtype), x.data_ptr(), _ld(x), weight.data_ptr(), bias.data_ptr(),
                                             out.data_ptr(), _ld(out), stats.data_ptr(), x.shape[0], x.shape[1], eps,
                                             _stream())
    _lib.check(st, "anemoi_layer_norm_stats")
    return out, stats


def _carry_stats(y: Tensor, eps: float, stats: Tensor) -> None:
    """Attach the LayerNorm statistics the producing GEMM's epilogue computed to ``y``.  The record pins the storage
    pointer and torch's in-place version counter of ``y`` at this moment: any later in-place write (or a swapped
    ``.data``) makes :func:`_carried_stats` ignore it, so stale statistics cannot be consumed silently."""
    y._anemoi_row_stats = (eps, stats, y.data_ptr(), y._version)


def _carried_stats(x: Tensor, eps: float) -> Optional[Tensor]:
    rec = getattr(x, "_anemoi_row_stats", None)
    if rec is None:
        return None
    r_eps, stats, ptr, version = rec
    if r_eps != eps or stats.shape[0] != x.shape[0] or ptr != x.data_ptr() or version != x._version:
        return None
    return stats


def row_stats(x: Tensor, eps: float = 1e-5) -> Tensor:
    """LayerNorm statistics of the rows of ``x``: ``[M, 2]`` f32 = ``(rstd, -mean * rstd)`` (see ``linear(ln=...)``)."""
    _dev(x)
    _rows(x)
    carried = _carried_stats(x, eps)  # left by linear(..., stats_eps=eps), which produced x
    if carried is not None:
        return carried
    out = torch.empty((x.shape[0], 2), dtype=torch.float32, device=x.device)
    if x.shape[0] == 0:
        return out
    with _Timed("row_stats", bytes=x.shape[0] * x.shape[1] * x.element_size()):
        st = _lib.load().anemoi_row_stats(dtype_code(x.dtype), x.data_ptr(), _ld(x), out.data_ptr(), x.shape[0],
                                          x.shape[1], eps, _stream())
    _lib.check(st, "anemoi_row_stats")
    return out


def linear(x: Tensor, w: Tensor, bias: Optional[Tensor] = None, *, act: str = "Identity",
           residual: Optional[Tensor] = None, out: Optional[Tensor] = None, out_dtype: Optional[torch.dtype] = None,
           n_out: Optional[int] = None, ln=None, stats_eps: Optional[float] = None) -> Tensor:
    """``act(x @ w.T + bias) + residual``; ``w`` is ``[N, K]`` in x's dtype with K already padded like x.

    ``stats_eps``: the result is about to enter a LayerNorm with this epsilon -- its row statistics are produced by the
    GEMM's epilogue (``anemoi_linear_stats``) and travel with the returned tensor: ``row_stats(result, stats_eps)`` then
    costs nothing.  Identity activation, same dtype in and out; silently ignored otherwise.

    ``ln=(stats, colsum)`` folds the LayerNorm of ``x`` into the product: ``x`` is the un-normalised input,
    ``stats = row_stats(x)``, ``w`` / ``bias`` / ``colsum`` come from ``runtime.fold_layer_norm``.
    """
    _dev(x, w, bias, residual, out)
    _rows(x)
    if w.dtype != x.dtype or not w.is_contiguous():
        raise ValueError("linear: weight must be contiguous and in the activation dtype")
    n = w.shape[0] if n_out is None else n_out
    k = w.shape[1]
    if x.shape[1] != k:
        raise ValueError(f"linear: x has {x.shape[1]} columns, weight expects {k}")
    if out is None:
        out = torch.empty((x.shape[0], n), dtype=out_dtype or x.dtype, device=x.device)
    if act not in _lib.ACT_CODES:
        raise RuntimeError(f"activation {act} is not supported by the fused Linear kernel")
    if x.shape[0] == 0:  # (an edge set without edges, an empty shard: torch hands out null pointers for empty tensors)
        return out
    alg = (x.shape[0] * k + n * k) * x.element_size() + x.shape[0] * n * (out.element_size() + (
        0 if residual is None else residual.element_size()))
    fuse_stats = stats_eps is not None and act == "Identity" and out.dtype == x.dtype and _rows(out).shape[1] == n
    with _Timed("linear", flops=2 * x.shape[0] * n * k, bytes=alg, m=x.shape[0], n=n, k=k):
        if fuse_stats:
            stats_in = colsum = None
            if ln is not None:
                stats_in, colsum = ln
                _dev(stats_in, colsum)
            m_rows = x.shape[0]
            ws = torch.empty((m_rows * max(n // 128, 1), 2), dtype=torch.float32, device=x.device)
            stats_out = torch.empty((m_rows, 2), dtype=torch.float32, device=x.device)
            st = _lib.load().anemoi_linear_stats(
                dtype_code(x.dtype), x.data_ptr(), _ld(x), w.data_ptr(), _ptr(bias), _ptr(colsum), _ptr(stats_in),
                _ptr(residual), 0 if residual is None else _ld(_rows(residual)), out.data_ptr(), _ld(_rows(out)), m_rows,
                n, k, ws.data_ptr(), ws.numel() * 4, stats_eps, stats_out.data_ptr(), _stream())
            _carry_stats(out, stats_eps, stats_out)
        elif ln is None:
            st = _lib.load().anemoi_linear(
                dtype_code(x.dtype), dtype_code(out.dtype), x.data_ptr(), _ld(x), w.data_ptr(), _ptr(bias),
                _ptr(residual), 0 if residual is None else _ld(_rows(residual)), out.data_ptr(), _ld(_rows(out)),
                x.shape[0], n, k, _lib.ACT_CODES[act], _stream())
        else:
            stats, colsum = ln
            _dev(stats, colsum)
            if stats.shape != (x.shape[0], 2) or stats.dtype != torch.float32 or not stats.is_contiguous():
                raise ValueError("linear: ln stats must be the contiguous [M, 2] f32 result of row_stats(x)")
            if colsum.numel() < n or colsum.dtype != torch.float32 or not colsum.is_contiguous():
                raise ValueError("linear: ln colsum must be a contiguous f32 vector with one entry per output column")
            st = _lib.load().anemoi_linear_ln(
                dtype_code(x.dtype), dtype_code(out.dtype), x.data_ptr(), _ld(x), w.data_ptr(), _ptr(bias),
                colsum.data_ptr(), stats.data_ptr(), _ptr(residual),
                0 if residual is None else _ld(_rows(residual)), out.data_ptr(), _ld(_rows(out)), x.shape[0], n, k,
                _lib.ACT_CODES[act], _stream())
    _lib.check(st, "anemoi_linear" if ln is None else "anemoi_linear_ln")
    return out


class SplitWeight(NamedTuple):
    """The split-bf16 planes of an f32 ``[N, K]`` weight (``include/anemoi_amd.h``, "Split-bf16"): ``hi = bf16(w)``,
    ``lo = bf16(w - hi)``, both contiguous bf16 ``[N, K]``."""

    hi: Tensor
    lo: Tensor


def split_weight(w: Tensor) -> SplitWeight:
    """``(w_hi, w_lo)`` of the f32 weight ``w`` ``[N, K]`` (unit inner stride, K a multiple of ``k_multiple(float32)``)."""
    _dev(w)
    _rows(w)
    if w.dtype != torch.float32:
        raise ValueError("split_weight: the weight must be f32")
    n, k = w.shape
    hi = torch.empty((n, k), dtype=torch.bfloat16, device=w.device)
    lo = torch.empty((n, k), dtype=torch.bfloat16, device=w.device)
    if k % k_multiple(torch.float32) != 0:
        raise ValueError(f"split_weight: K={k} must be a multiple of {k_multiple(torch.float32)} (pad with zeros)")
    if n == 0:
        return SplitWeight(hi, lo)
    with _Timed("split_weight", bytes=n * k * 8, n=n, k=k):
        st = _lib.load().anemoi_split_weight(w.data_ptr(), _ld(w), hi.data_ptr(), lo.data_ptr(), n, k, _stream())
    _lib.check(st, "anemoi_split_weight")
    return SplitWeight(hi, lo)


def linear_split(x: Tensor, planes: SplitWeight, bias: Optional[Tensor] = None, *, act: str = "Identity",
                 residual: Optional[Tensor] = None, out: Optional[Tensor] = None, n_out: Optional[int] = None) -> Tensor:
    """``act(x @ w.T + bias) + residual`` in f32 storage with the split-bf16 product ``x_hi w_hi + x_hi w_lo + x_lo w_hi``
    on the bf16 MFMA (``planes = split_weight(w)``; ``x`` is split inside the kernel).  ~4e-6 relative error per Linear;
    finite inputs below 2^126 only (see the header)."""
    w_hi, w_lo = planes
    _dev(x, w_hi, w_lo, bias, residual, out)
    _rows(x)
    if x.dtype != torch.float32:
        raise ValueError("linear_split: activations must be f32")
    if (w_hi.dtype != torch.bfloat16 or w_lo.dtype != torch.bfloat16 or w_hi.shape != w_lo.shape or w_hi.dim() != 2
            or not w_hi.is_contiguous() or not w_lo.is_contiguous()):
        raise ValueError("linear_split: planes must be two contiguous bf16 [N, K] tensors (ops.split_weight)")
    n = w_hi.shape[0] if n_out is None else n_out
    k = w_hi.shape[1]
    if x.shape[1] != k:
        raise ValueError(f"linear_split: x has {x.shape[1]} columns, weight expects {k}")
    if not 0 < n <= w_hi.shape[0]:
        raise ValueError(f"linear_split: n_out={n} outside the weight's {w_hi.shape[0]} rows")
    if k % k_multiple(torch.float32) != 0:
        raise ValueError(f"linear_split: K={k} must be a multiple of {k_multiple(torch.float32)} (pad with zeros)")
    for name, t in (("bias", bias), ("residual", residual), ("out", out)):
        if t is not None and t.dtype != torch.float32:
            raise ValueError(f"linear_split: {name} must be f32")
    if out is None:
        out = torch.empty((x.shape[0], n), dtype=torch.float32, device=x.device)
    if act not in _lib.ACT_CODES:
        raise RuntimeError(f"activation {act} is not supported by the fused Linear kernel")
    if x.shape[0] == 0:
        return out
    alg = (x.shape[0] * k + n * k) * 4 + x.shape[0] * n * (4 + (0 if residual is None else 4))
    with _Timed("linear_split", flops=2 * x.shape[0] * n * k, bytes=alg, m=x.shape[0], n=n, k=k):
        st = _lib.load().anemoi_linear_split(
            x.data_ptr(), _ld(x), w_hi.data_ptr(), w_lo.data_ptr(), _ptr(bias), _ptr(residual),
            0 if residual is None else _ld(_rows(residual)), out.data_ptr(), _ld(_rows(out)), x.shape[0], n, k,
            _lib.ACT_CODES[act], _stream())
    _lib.check(st, "anemoi_linear_split")
    return out


class MXTensor(NamedTuple):
    """MXFP8 rows (format: ``include/anemoi_amd.h``, "MXFP8"): ``q`` e4m3 bytes ``[rows, Kp]``, ``scales`` E8M0 bytes
    ``[rows, Kp / 32]``, ``k`` the logical width (columns ``k .. Kp-1`` are zero padding)."""

    q: Tensor
    scales: Tensor
    k: int


def mx_quantize(x: Tensor, ln=None) -> MXTensor:
    """MXFP8 of the rows of ``x`` (bf16 or f32 ``[M, K]``), K padded to a multiple of 128.

    ``ln=(weight, bias, eps)`` quantises ``LayerNorm(x)`` instead, in the same row pass (statistics in f32)."""
    _dev(x)
    _rows(x)
    m, k = x.shape
    kp = round_up(k, 128)
    q = torch.empty((m, kp), dtype=torch.uint8, device=x.device)
    s = torch.empty((m, kp // 32), dtype=torch.uint8, device=x.device)
    gamma = beta = None
    eps = 0.0
    if ln is not None:
        gamma, beta, eps = ln
        _dev(gamma, beta)
        if gamma.dtype != torch.float32 or beta.dtype != torch.float32 or gamma.numel() != k or beta.numel() != k \
                or not gamma.is_contiguous() or not beta.is_contiguous():
            raise ValueError(f"mx_quantize: LayerNorm weight / bias must be contiguous f32 vectors of length {k}")
    if m == 0:
        return MXTensor(q, s, k)
    with _Timed("mx_quantize", bytes=m * k * x.element_size() + m * (kp + kp // 32), m=m, k=k):
        st = _lib.load().anemoi_mx_quantize(dtype_code(x.dtype), x.data_ptr(), _ld(x), _ptr(gamma), _ptr(beta),
                                            float(eps), q.data_ptr(), kp, s.data_ptr(), kp // 32, m, k, kp, _stream())
    _lib.check(st, "anemoi_mx_quantize")
    return MXTensor(q, s, k)


def linear_mx(xq: MXTensor, wq: MXTensor, bias: Optional[Tensor] = None, *, act: str = "Identity",
              residual: Optional[Tensor] = None, out: str = "bf16"):
    """``act(x @ w.T + bias) + residual`` from MXFP8 operands (``mx_quantize`` of the activations and of the ``[N, K]``
    weight), f32 accumulation.  ``out="bf16"``: a bf16 ``[M, N]`` tensor; ``out="mx"``: the result as an
    :class:`MXTensor` of width N, ready to be the next ``linear_mx``'s input.  ``residual`` is bf16 ``[M, N]``."""
    _dev(xq.q, wq.q, bias, residual)
    if out not in ("bf16", "mx"):
        raise ValueError(f"linear_mx: out must be 'bf16' or 'mx', got {out!r}")
    if act not in _lib.ACT_CODES:
        raise RuntimeError(f"activation {act} is not supported by the MXFP8 Linear kernel")
    if xq.k != wq.k or xq.q.shape[1] != wq.q.shape[1]:
        raise ValueError(f"linear_mx: activations have K={xq.k} ({xq.q.shape[1]} padded), weight K={wq.k} "
                         f"({wq.q.shape[1]} padded)")
    if not wq.q.is_contiguous() or not wq.scales.is_contiguous():
        raise ValueError("linear_mx: the weight's elements and scales must be contiguous")
    for name, t in (("activations", xq), ("weight", wq)):
        _dev(t.scales)
        _rows(t.q)
        _rows(t.scales)
        if t.q.dtype != torch.uint8 or t.scales.dtype != torch.uint8 or t.q.device != xq.q.device \
                or t.scales.device != xq.q.device:
            raise ValueError(f"linear_mx: {name} elements and scales must be uint8 tensors on the activations' device")
        if t.q.shape[1] % 128 or t.scales.shape != (t.q.shape[0], t.q.shape[1] // 32):
            raise ValueError(f"linear_mx: {name} must be [rows, Kp] elements (Kp a multiple of 128) with [rows, Kp / 32] "
                             f"scales, got {tuple(t.q.shape)} and {tuple(t.scales.shape)}")
    if residual is not None and residual.dtype != torch.bfloat16:
        raise ValueError("linear_mx: the residual must be bf16")
    if bias is not None and (bias.dtype != torch.float32 or not bias.is_contiguous()):
        raise ValueError("linear_mx: the bias must be a contiguous f32 vector")
    m, kp = xq.q.shape
    n = wq.q.shape[0]
    if residual is not None and (_rows(residual).shape != (m, n) or residual.device != xq.q.device):
        raise ValueError(f"linear_mx: residual must be [{m}, {n}] on the activations' device, got {tuple(residual.shape)}")
    if bias is not None and (bias.numel() < n or bias.device != xq.q.device):
        raise ValueError(f"linear_mx: bias needs {n} entries on the activations' device, got {bias.numel()}")
    if out == "mx":
        npad = round_up(n, 128)
        y = torch.empty((m, npad), dtype=torch.uint8, device=xq.q.device)
        ys = torch.empty((m, npad // 32), dtype=torch.uint8, device=xq.q.device)
    else:
        y = torch.empty((m, n), dtype=torch.bfloat16, device=xq.q.device)
        ys = None
    if m > 0:
        alg = m * kp * 33 // 32 + n * kp * 33 // 32 + m * n * (2 if out == "bf16" else 1) + (
            0 if residual is None else m * n * 2)
        with _Timed("linear_mx", flops=2 * m * n * kp, bytes=alg, m=m, n=n, k=kp):
            st = _lib.load().anemoi_linear_mx(
                xq.q.data_ptr(), _ld(_rows(xq.q)), xq.scales.data_ptr(), _ld(_rows(xq.scales)), wq.q.data_ptr(),
                wq.scales.data_ptr(), _ptr(bias), _ptr(residual), 0 if residual is None else _ld(_rows(residual)),
                int(out == "mx"), y.data_ptr(), _ld(y), _ptr(ys), 0 if ys is None else _ld(ys), m, n, kp,
                _lib.ACT_CODES[act], _stream())
        _lib.check(st, "anemoi_linear_mx")
    return MXTensor(y, ys, n) if out == "mx" else y


def edge_attr_csr(a0: Tensor, a1: Optional[Tensor], perm: Tensor, ld_out: Optional[int] = None,
                  one_col: int = -1) -> Tensor:
    """Edge attributes ``[a0 | a1]`` gathered into CSR order (rows ``perm[e] % a0.shape[0]``), f32, zero padded.

    ``one_col >= 0`` writes a constant 1 into that (padding) column: the bias carrier of the folded edge kernel.
    """
    _dev(a0, a1, perm)
    d0 = a0.shape[1]
    d1 = 0 if a1 is None else a1.shape[1]
    ld = round_up(d0 + d1, 4) if ld_out is None else ld_out
    a0 = a0.contiguous().float()
    a1 = None if a1 is None else a1.contiguous().float()
    out = torch.empty((perm.shape[0], ld), dtype=torch.float32, device=a0.device)
    if perm.shape[0] == 0:
        return out
    st = _lib.load().anemoi_edge_attr_csr(a0.data_ptr(), d0, _ptr(a1), d1, a0.shape[0], perm.data_ptr(),
                                          out.data_ptr(), ld, one_col, perm.shape[0], _stream())
    _lib.check(st, "anemoi_edge_attr_csr")
    return out


def gt_edge_attention(q: Tensor, k: Tensor, v: Tensor, x_r: Optional[Tensor], edge_attr: Tensor, edge_dim: int,
                      w_edge: Tensor, b_edge: Tensor, rowptr: Tensor, col: Tensor, num_heads: int,
                      out: Optional[Tensor] = None) -> Tensor:
    """Fused gather -> lin_edge -> score -> segment softmax -> weighted scatter-sum (+ x_r) over a dst-CSR graph."""
    _dev(q, k, v, x_r, edge_attr, w_edge, b_edge, rowptr, col, out)
    n_dst, c = _rows(q).shape
    if _ld(_rows(k)) != _ld(_rows(v)):
        raise ValueError("gt_edge_attention: k and v must share their leading dimension")
    if out is None:
        out = torch.empty((n_dst, c), dtype=q.dtype, device=q.device)
    if rowptr.dtype != torch.int32 or col.dtype != torch.int32 or rowptr.shape[0] != n_dst + 1:
        raise ValueError("gt_edge_attention: rowptr/col must be int32 with rowptr of length n_dst + 1")
    if col.shape[0] == 0:  # graph without edges: the C ABI still wants valid (never dereferenced) pointers
        col = torch.zeros(1, dtype=torch.int32, device=q.device)
        edge_attr = torch.zeros((1, max(4, round_up(edge_dim, 4))), dtype=torch.float32, device=q.device)
    # algorithmic bytes per SURVEY.md section 8d: q + out over the destinations, k + v over the sources (each once),
    # 48 B of raw attributes + 4 B column index per edge, the row pointers
    alg_bytes = (2 * n_dst + 2 * k.shape[0]) * c * q.element_size() + col.shape[0] * 52 + (n_dst + 1) * 4
    with _Timed("gt_edge_attention", bytes=alg_bytes, n_dst=n_dst, n_src=k.shape[0], edges=col.shape[0]):
        st = _lib.load().anemoi_gt_edge_attention(
            dtype_code(q.dtype), q.data_ptr(), _ld(q), k.data_ptr(), v.data_ptr(), _ld(k), _ptr(x_r),
            0 if x_r is None else _ld(_rows(x_r)), edge_attr.data_ptr(),
            edge_attr.stride(0) if edge_attr.shape[0] > 1 else edge_attr.shape[1], edge_dim, w_edge.data_ptr(),
            b_edge.data_ptr(), rowptr.data_ptr(), col.data_ptr(), out.data_ptr(), _ld(_rows(out)), n_dst, c,
            num_heads, _stream())
    _lib.check(st, "anemoi_gt_edge_attention")
    return out


def gt_edge_attention_folded(q: Tensor, k: Tensor, v: Tensor, x_r: Optional[Tensor], u: Tensor, edge_attr: Tensor,
                             rowptr: Tensor, col: Tensor, num_heads: int, up: int, out: Optional[Tensor] = None,
                             ld_out: Optional[int] = None, lse: Optional[Tensor] = None, runs=None, sched=None,
                             tiles=None) -> Tensor:
    """Edge phase with lin_edge folded away: returns ``[n_dst, ld_out]`` = ``[sum alpha v (+ x_r) | t (H*up) | 0-pad]``.

    ``u`` is ``[n_dst, H*up]`` (extra columns of the q/k/v GEMM), ``edge_attr`` ``[E, up]`` f32 in CSR order with the
    constant-1 column.  Columns beyond ``C + H*up`` (K padding for the projection GEMM) are zero filled.  ``lse``
    (optional f32 ``[n_dst, H]``, contiguous) receives the softmax normaliser per destination and head (training).
    ``runs`` (``EdgePlan.runs3()``, uniform-degree-3 graphs): destinations that share their three sources share one gather
    of them -- ``(grp_ptr, grp_perm, grp_dst)``: all destinations of a source triple (``anemoi_gt_edge_attention_folded_groups``),
    ``(run_ptr, perm)``: the consecutive ones (``anemoi_gt_edge_attention_folded_runs``).  ``sched`` (``EdgePlan.schedule()``: int32
    ``[8, slots, steps]``): the destination schedule of ``anemoi_gt_edge_attention_folded_sched`` -- balanced wave slots, index
    chain resolved one destination ahead; bit-identical to the plain kernel.  ``tiles`` (``EdgePlan.tiles()``: a
    ``runtime.EdgeTiles``): the LDS-tile kernel ``anemoi_gt_edge_attention_folded_tiles`` -- every source row staged once per
    tile of <= 32 destinations; bit-identical to the plain kernel.  ``runs`` wins over ``tiles`` wins over ``sched``.
    """
    _dev(q, k, v, x_r, u, edge_attr, rowptr, col, out, lse)
    if lse is not None and (lse.dtype != torch.float32 or not lse.is_contiguous()
                            or tuple(lse.shape) != (_rows(q).shape[0], num_heads)):
        raise ValueError("gt_edge_attention_folded: lse must be a contiguous f32 [n_dst, H] tensor")
    n_dst, c = _rows(q).shape
    if _ld(_rows(k)) != _ld(_rows(v)):
        raise ValueError("gt_edge_attention_folded: k and v must share their leading dimension")
    width = c + num_heads * up
    ld = width if ld_out is None else ld_out
    if out is None:
        out = torch.empty((n_dst, ld), dtype=q.dtype, device=q.device)
        if ld > width:
            out[:, width:].zero_()
    if rowptr.dtype != torch.int32 or col.dtype != torch.int32 or rowptr.shape[0] != n_dst + 1:
        raise ValueError("gt_edge_attention_folded: rowptr/col must be int32 with rowptr of length n_dst + 1")
    if edge_attr.shape[0] != col.shape[0] or (col.shape[0] > 0 and (edge_attr.shape[1] != up or
                                                                      not edge_attr.is_contiguous())):
        raise ValueError("gt_edge_attention_folded: edge_attr must be contiguous [E, up]")
    if col.shape[0] == 0:
        col = torch.zeros(1, dtype=torch.int32, device=q.device)
        edge_attr = torch.zeros((1, up), dtype=torch.float32, device=q.device)
    alg_bytes = (2 * n_dst + 2 * k.shape[0]) * c * q.element_size() + col.shape[0] * 52 + (n_dst + 1) * 4
    # (+ the operands this kernel moves because of its fusions -- x_r read, u read, t written -- which SURVEY 8d's figure does
    #  not count: reported beside the roofline fraction, never instead of it)
    fused_bytes = alg_bytes + n_dst * ((0 if x_r is None else c) + 2 * num_heads * up) * q.element_size()
    with _Timed("gt_edge_attention", bytes=alg_bytes, fused_bytes=fused_bytes, n_dst=n_dst, n_src=k.shape[0], edges=col.shape[0]):
        lib = _lib.load()
        head = (dtype_code(q.dtype), q.data_ptr(), _ld(q), k.data_ptr(), v.data_ptr(), _ld(_rows(k)), _ptr(x_r),
                0 if x_r is None else _ld(_rows(x_r)), u.data_ptr(), _ld(_rows(u)), edge_attr.data_ptr(), up,
                rowptr.data_ptr(), col.data_ptr())
        tail = (out.data_ptr(), _ld(_rows(out)), _ptr(lse), n_dst, c, num_heads, _stream())
        n_src, n_edges = _rows(k).shape[0], col.shape[0]
        if runs is not None and len(runs) == 3:  # groups of destinations that share their three sources
            grp_ptr, grp_perm, grp_dst = runs
            _dev(grp_ptr, grp_perm, grp_dst)
            if (grp_ptr.dtype != torch.int32 or grp_perm.dtype != torch.int32 or grp_dst.dtype != torch.int32
                    or grp_perm.shape[0] != n_dst or grp_dst.shape[0] != n_dst):
                raise ValueError("gt_edge_attention_folded: runs = (int32 grp_ptr [n_groups + 1], int32 grp_perm [n_dst], "
                                 "int32 grp_dst [n_dst])")
            st = lib.anemoi_gt_edge_attention_folded_groups(*head, grp_ptr.data_ptr(), grp_dst.data_ptr(), grp_perm.data_ptr(),
                                                            grp_ptr.shape[0] - 1, n_src, *tail)
        elif runs is not None:
            run_ptr, perm = runs
            _dev(run_ptr, perm)
            if run_ptr.dtype != torch.int32 or perm.dtype != torch.int32 or perm.shape[0] != run_ptr.shape[0] - 1:
                raise ValueError("gt_edge_attention_folded: runs = (int32 run_ptr [n_runs + 1], int32 perm [n_runs])")
            st = lib.anemoi_gt_edge_attention_folded_runs(*head, run_ptr.data_ptr(), perm.data_ptr(), run_ptr.shape[0] - 1, *tail)
        elif tiles is not None:
            _dev(tiles.hdr, tiles.dst, tiles.src, tiles.slot, tiles.xcd)
            st = lib.anemoi_gt_edge_attention_folded_tiles(
                *head, tiles.hdr.data_ptr(), tiles.dst.data_ptr(), tiles.src.data_ptr(), tiles.slot.data_ptr(),
                tiles.xcd.data_ptr(), tiles.max_tiles_per_xcd, tiles.src_cap, tiles.edge_cap, n_src, n_edges, *tail)
        elif sched is not None:  # (the entry point itself falls back to the plain kernel beyond 32-bit row offsets)
            _dev(sched)
            if sched.dtype != torch.int32 or sched.dim() != 3 or sched.shape[0] != 8 or not sched.is_contiguous():
                raise ValueError("gt_edge_attention_folded: sched = contiguous int32 [8, slots, steps]")
            st = lib.anemoi_gt_edge_attention_folded_sched(*head, sched.data_ptr(), sched.shape[1], sched.shape[2], n_src,
                                                           n_edges, *tail)
        else:
            st = lib.anemoi_gt_edge_attention_folded(*head, *tail)
    _lib.check(st, "anemoi_gt_edge_attention_folded")
    return out


def linear_heads(x: Tensor, w: Tensor, out: Optional[Tensor] = None, residual: Optional[Tensor] = None) -> Tensor:
    """``H`` independent products ``out[:, h*N:(h+1)*N] = x[:, h*K:(h+1)*K] @ w[h].T`` (``+ residual[:, h*N:(h+1)*N]``) as
    ONE launch (no bias / activation).  ``w`` is contiguous ``[H, N, K]`` in x's dtype; ``x`` / ``out`` / ``residual`` are
    row-major ``[M, >= H*K]`` / ``[M, >= H*N]`` slices.  The small products on either side of the raw-row edge phase: per-head
    shapes the thin kernel holds in registers run on it (``linear_thin``, residual fused); everything else, and everything
    under ``ANEMOI_AMD_THIN=0``, is ``anemoi_linear_batched`` followed by ``add`` for the residual."""
    _dev(x, w, out, residual)
    if thin_enabled() and w.dim() == 3:
        y = linear_thin(x, w, out=out, residual=residual)
        if y is not None:
            return y
    _rows(x)
    if w.dim() != 3 or w.dtype != x.dtype or not w.is_contiguous():
        raise ValueError("linear_heads: weight must be contiguous [H, N, K] in the activation dtype")
    h, n, k = w.shape
    if x.shape[1] < h * k:
        raise ValueError(f"linear_heads: x has {x.shape[1]} columns, {h} heads of {k} expected")
    if out is None:
        out = torch.empty((x.shape[0], h * n), dtype=x.dtype, device=x.device)
    if _rows(out).shape[1] < h * n or out.dtype != x.dtype or out.shape[0] != x.shape[0]:
        raise ValueError("linear_heads: out must be [M, >= H*N] in the activation dtype")
    m = x.shape[0]
    if m == 0:
        return out
    code = dtype_code(x.dtype)
    with _Timed("linear", flops=2 * m * h * n * k, bytes=(m * h * (k + n) + h * n * k) * x.element_size(), m=m, n=h * n,
                k=k, heads=h):
        st = _lib.load().anemoi_linear_batched(code, code, x.data_ptr(), _ld(x), k, w.data_ptr(), n * k, out.data_ptr(),
                                               _ld(out), n, h, m, n, k, _stream())
    _lib.check(st, "anemoi_linear_batched")
    if residual is not None:
        add(out[:, :h * n], residual[:, :h * n], out=out[:, :h * n])
    return out


def thin_enabled() -> bool:
    """The thin-Linear route (``anemoi_linear_thin``) is taken where a call site asks for it; ``ANEMOI_AMD_THIN=0`` keeps the
    fused Linear family's launches at every such site."""
    return os.environ.get("ANEMOI_AMD_THIN", "1") != "0"


def linear_thin(x: Tensor, w: Tensor, bias: Optional[Tensor] = None, *, residual: Optional[Tensor] = None,
                out: Optional[Tensor] = None, out_dtype: Optional[torch.dtype] = None, ln=None,
                stats_eps: Optional[float] = None) -> Optional[Tensor]:
    """``x @ w.T (+ bias) (+ residual)`` on the register-resident thin kernel (``csrc/gemm_thin.hip``), or ``None`` when the
    library does not take the call (shape outside its table, an unsupported combination): NOTHING is launched then and the
    caller keeps its route through the fused Linear family.  bf16 ``x`` and ``w`` only.

    ``w [N, K]``: one product.  ``w [H, N, K]``: ``H`` products over the column blocks of ``x [M, >= H K]``, ``out`` and
    ``residual [M, >= H N]`` and ``bias [H N]``, as ``linear_heads``.  ``ln=(stats, colsum)``: the LayerNorm fold of
    ``linear(ln=)``.  ``stats_eps``: statistics only -- returns ``row_stats(x @ w.T + bias, stats_eps)`` ``[M, 2]`` of the
    product as ``out_dtype`` (default bf16) would store it, and stores no product."""
    if not x.is_cuda:  # (host-logic tests substitute the fused family's functions: their tensors keep that route)
        return None
    _dev(x, w, bias, residual, out)
    _rows(x)
    if x.dtype != torch.bfloat16 or w.dtype != torch.bfloat16 or not w.is_contiguous() or w.dim() not in (2, 3):
        return None
    h = w.shape[0] if w.dim() == 3 else 1
    n, k = w.shape[-2], w.shape[-1]
    m = x.shape[0]
    if (n, k) not in _lib.THIN_SHAPES or m == 0 or x.shape[1] < h * k:
        return None
    odt = out.dtype if out is not None else (out_dtype or x.dtype)
    if odt not in _DT:
        return None
    # operands the kernel's 16-byte accesses cannot take are a refusal, not an error: the fused family may take them
    mult = 8 if odt == torch.bfloat16 else 4
    for t, md in ((x, 8), (w, 8), (out, mult), (residual, 8)):
        if t is not None and (t.data_ptr() % 16 != 0 or (t.dim() == 2 and _ld(_rows(t)) % md != 0)):
            return None
    for t in (bias,) + (tuple(ln) if ln is not None else ()):
        if t is not None and t.data_ptr() % 16 != 0:
            return None
    a = _lib.LinearThinArgs()
    a.struct_bytes = ctypes.sizeof(_lib.LinearThinArgs)
    a.out_dtype, a.batch = _DT[odt], h
    a.x, a.w, a.bias = x.data_ptr(), w.data_ptr(), _ptr(bias)
    a.ldx, a.M, a.N, a.K = _ld(x), m, n, k
    a.stride_x, a.stride_w, a.stride_y, a.stride_r = k, n * k, n, n
    if bias is not None and (bias.dtype != torch.float32 or not bias.is_contiguous() or bias.numel() < h * n):
        raise ValueError("linear_thin: bias must be a contiguous f32 vector with one entry per output column")
    if ln is not None:
        stats, colsum = ln
        _dev(stats, colsum)
        if stats.shape != (m, 2) or stats.dtype != torch.float32 or not stats.is_contiguous():
            raise ValueError("linear_thin: ln stats must be the contiguous [M, 2] f32 result of row_stats(x)")
        if colsum.numel() < n or colsum.dtype != torch.float32 or not colsum.is_contiguous():
            raise ValueError("linear_thin: ln colsum must be a contiguous f32 vector with one entry per output column")
        a.stats, a.colsum = stats.data_ptr(), colsum.data_ptr()
    if residual is not None:
        if residual.dtype != torch.bfloat16 or _rows(residual).shape[0] != m or residual.shape[1] < h * n:
            raise ValueError("linear_thin: the residual must be bf16 [M, >= H*N]")
        a.residual, a.ldr = residual.data_ptr(), _ld(residual)
    result = None
    if stats_eps is not None:
        result = torch.empty((m, 2), dtype=torch.float32, device=x.device)
        a.stats_out, a.eps = result.data_ptr(), stats_eps
        moved = (m * h * k + h * n * k) * 2 + m * 8
    else:
        if out is None:
            out = torch.empty((m, h * n), dtype=odt, device=x.device)
        if _rows(out).shape[0] != m or out.shape[1] < h * n:
            raise ValueError("linear_thin: out must be [M, >= H*N]")
        result = out
        a.y, a.ldy = out.data_ptr(), _ld(out)
        moved = (m * h * k + h * n * k) * 2 + m * h * n * (out.element_size() + (0 if residual is None else 2))
    with _Timed("linear", flops=2 * m * h * n * k, bytes=moved, m=m, n=h * n, k=k, thin=True) as timed:
        st = _lib.load().anemoi_linear_thin(ctypes.byref(a), _stream())
        timed.launched = st == _lib.ANEMOI_OK
    if st == _lib.ANEMOI_ERR_UNSUPPORTED:
        return None
    _lib.check(st, "anemoi_linear_thin")
    return result


def gt_edge_attention_raw(qt: Tensor, x_raw: Tensor, src_stats: Tensor, u: Tensor, edge_attr: Tensor, rowptr: Tensor,
                          col: Tensor, num_heads: int, head_dim: int, up: int, sum_col: int, t_out: Tensor,
                          g: Optional[Tensor] = None) -> Tensor:
    """Folded edge phase on RAW source rows (``anemoi_gt_edge_attention_raw``, bf16): returns ``g [n_dst, H*Ks]`` with
    ``g[i, h] = sum_j alpha_ij,h rstd_j x_j`` (column ``sum_col`` of every head: ``sum_j alpha_ij,h``) and writes
    ``t [n_dst, H*up]`` into ``t_out``.  ``qt [n_dst, H*Ks]`` are the queries carried to the raw space
    (``linear_heads(q, A_k^T)``), ``x_raw [n_src, Ks]`` the raw rows, ``src_stats = row_stats`` of their embedding."""
    _dev(qt, x_raw, src_stats, u, edge_attr, rowptr, col, t_out, g)
    n_dst, ks = _rows(qt).shape[0], _rows(x_raw).shape[1]
    if qt.dtype != torch.bfloat16 or x_raw.dtype != torch.bfloat16 or u.dtype != torch.bfloat16 or t_out.dtype != torch.bfloat16:
        raise NotImplementedError("gt_edge_attention_raw: bf16 only")
    if qt.shape[1] != num_heads * ks:
        raise ValueError(f"gt_edge_attention_raw: qt has {qt.shape[1]} columns, {num_heads} heads of {ks} expected")
    if (src_stats.shape != (x_raw.shape[0], 2) or src_stats.dtype != torch.float32 or not src_stats.is_contiguous()):
        raise ValueError("gt_edge_attention_raw: src_stats must be the contiguous [n_src, 2] f32 result of row_stats")
    if rowptr.dtype != torch.int32 or col.dtype != torch.int32 or rowptr.shape[0] != n_dst + 1:
        raise ValueError("gt_edge_attention_raw: rowptr/col must be int32 with rowptr of length n_dst + 1")
    if edge_attr.shape[0] != col.shape[0] or (col.shape[0] > 0 and (edge_attr.shape[1] != up or
                                                                      not edge_attr.is_contiguous())):
        raise ValueError("gt_edge_attention_raw: edge_attr must be contiguous [E, up]")
    if _rows(u).shape != (n_dst, num_heads * up) or _rows(t_out).shape[0] != n_dst or t_out.shape[1] < num_heads * up:
        raise ValueError("gt_edge_attention_raw: u / t_out must be [n_dst, H*up]")
    if g is None:
        g = torch.empty((n_dst, num_heads * ks), dtype=qt.dtype, device=qt.device)
    if col.shape[0] == 0:
        col = torch.zeros(1, dtype=torch.int32, device=qt.device)
        edge_attr = torch.zeros((1, up), dtype=torch.float32, device=qt.device)
    # algorithmic bytes: every edge gathers one raw row, its source's rstd, its attribute row and its source id; qt in,
    # g out, the row pointers.  (+ u read, t written: the operands of the lin_edge fusion, as the other folded kernels)
    alg_bytes = (col.shape[0] * (ks * 2 + 4 + up * 4 + 4) + 2 * n_dst * num_heads * ks * 2 + (n_dst + 1) * 4)
    fused_bytes = alg_bytes + n_dst * 2 * num_heads * up * 2
    with _Timed("gt_edge_attention", bytes=alg_bytes, fused_bytes=fused_bytes, n_dst=n_dst, n_src=x_raw.shape[0],
                edges=col.shape[0], raw_rows=ks):
        st = _lib.load().anemoi_gt_edge_attention_raw(
            qt.data_ptr(), _ld(qt), x_raw.data_ptr(), _ld(x_raw), src_stats.data_ptr(), u.data_ptr(), _ld(u),
            edge_attr.data_ptr(), up, rowptr.data_ptr(), col.data_ptr(), g.data_ptr(), _ld(_rows(g)), t_out.data_ptr(),
            _ld(t_out), n_dst, num_heads, ks, head_dim, sum_col, _stream())
    _lib.check(st, "anemoi_gt_edge_attention_raw")
    return g


def gt_conv(q: Tensor, k: Tensor, v: Tensor, edges_csr: Tensor, rowptr: Tensor, col: Tensor, num_heads: int,
            x_r: Optional[Tensor] = None, lse: Optional[Tensor] = None, dropout_p: float = 0.0, dropout_seed: int = 0,
            seed_dev: Optional[Tensor] = None) -> Tensor:
    """``GraphTransformerConv`` with explicit per-edge features (reference layers/conv.py:98-142): ``q [n_dst, C]``,
    ``k, v [n_src, C]``, ``edges_csr [E, C]`` in the CSR order of ``(rowptr, col)``; returns ``[n_dst, C]`` (``+ x_r``).
    ``lse`` (optional f32 ``[n_dst, H]``) receives the softmax normaliser (training).  ``dropout_p`` / ``dropout_seed`` /
    ``seed_dev``: the conv's dropout of the attention weights in training mode (layers/conv.py:140), mask = hash(CSR edge
    position, head, seed) as for :func:`mhsa`."""
    if not 0.0 <= dropout_p <= 1.0:
        raise ValueError(f"dropout probability has to be between 0 and 1, but got {dropout_p}")
    _dev(q, k, v, edges_csr, rowptr, col, x_r, lse)
    n_dst, c = _rows(q).shape
    if _ld(_rows(k)) != _ld(_rows(v)):
        raise ValueError("gt_conv: k and v must share their leading dimension")
    if rowptr.dtype != torch.int32 or col.dtype != torch.int32 or rowptr.shape[0] != n_dst + 1:
        raise ValueError("gt_conv: rowptr/col must be int32 with rowptr of length n_dst + 1")
    if edges_csr.shape[0] != col.shape[0] or edges_csr.dtype != q.dtype:
        raise ValueError("gt_conv: edges must be [E, C] in the activation dtype")
    out = torch.empty((n_dst, c), dtype=q.dtype, device=q.device)
    if col.shape[0] == 0:
        if lse is not None:
            lse.fill_(float("-inf"))
        return out.zero_() if x_r is None else out.copy_(x_r)
    alg_bytes = (2 * n_dst + 2 * k.shape[0] + col.shape[0]) * c * q.element_size() + col.shape[0] * 4 + (n_dst + 1) * 4
    with _Timed("gt_conv", bytes=alg_bytes, n_dst=n_dst, n_src=k.shape[0], edges=col.shape[0]):
        st = _lib.load().anemoi_gt_conv(dtype_code(q.dtype), q.data_ptr(), _ld(q), k.data_ptr(), v.data_ptr(), _ld(_rows(k)),
                                        edges_csr.data_ptr(), _ld(_rows(edges_csr)), _ptr(x_r),
                                        0 if x_r is None else _ld(_rows(x_r)), rowptr.data_ptr(), col.data_ptr(),
                                        out.data_ptr(), _ld(out), _ptr(lse), n_dst, c, num_heads, float(dropout_p),
                                        int(dropout_seed) & 0xFFFFFFFF, _seed_dev_ptr(seed_dev, q), _stream())
    _lib.check(st, "anemoi_gt_conv")
    return out


def gather_add_act(t: Tensor, p_dst: Tensor, p_src: Tensor, dst: Tensor, src: Tensor, act: str = "Identity",
                   out: Optional[Tensor] = None) -> Tensor:
    """``act(t[e] + p_dst[dst[e]] + p_src[src[e]])`` per edge row (first edge-MLP layer of the GNN block)."""
    _dev(t, p_dst, p_src, dst, src, out)
    e, c = _rows(t).shape
    if out is None:
        out = torch.empty((e, c), dtype=t.dtype, device=t.device)
    if e == 0:
        return out
    if dst.dtype != torch.int32 or src.dtype != torch.int32 or dst.shape[0] != e or src.shape[0] != e:
        raise ValueError("gather_add_act: dst / src must be int32 [E]")
    # compulsory bytes: t read + result written per edge, each node table once, the two index lists
    with _Timed("gather_add_act", bytes=(2 * e + p_dst.shape[0] + p_src.shape[0]) * c * t.element_size() + 8 * e):
        st = _lib.load().anemoi_gather_add_act(dtype_code(t.dtype), t.data_ptr(), _ld(t), p_dst.data_ptr(),
                                               _ld(_rows(p_dst)), p_src.data_ptr(), _ld(_rows(p_src)), dst.data_ptr(),
                                               src.data_ptr(), out.data_ptr(), _ld(_rows(out)), e, c,
                                               _lib.ACT_CODES[act], _stream())
    _lib.check(st, "anemoi_gather_add_act")
    return out


def segment_sum(v: Tensor, rowptr: Tensor, out: Optional[Tensor] = None, cat_with: Optional[Tensor] = None) -> Tensor:
    """Sum of the rows of every CSR segment: ``out[i] = v[rowptr[i]:rowptr[i+1]].sum(0)`` (scatter-sum over dst).
    ``cat_with`` = ``x [n_dst, C]``: returns ``[n_dst, 2C] = [x | sums]`` -- the node MLP's input -- from the same pass."""
    _dev(v, rowptr, out, cat_with)
    n_dst = rowptr.shape[0] - 1
    c = _rows(v).shape[1]
    if cat_with is not None:
        x = _rows(cat_with)
        if x.shape != (n_dst, c) or x.dtype != v.dtype or out is not None:
            raise ValueError("segment_sum: cat_with must be [n_dst, C] of v's dtype (and no out=)")
        out = torch.empty((n_dst, 2 * c), dtype=v.dtype, device=v.device)
        if v.shape[0] == 0:
            out[:, :c].copy_(x)
            out[:, c:].zero_()
            return out
        with _Timed("segment_sum", bytes=(v.shape[0] + 3 * n_dst) * c * v.element_size()):
            st = _lib.load().anemoi_segment_sum_cat(dtype_code(v.dtype), v.data_ptr(), _ld(v), rowptr.data_ptr(),
                                                    x.data_ptr(), _ld(x), out.data_ptr(), 2 * c, n_dst, c, _stream())
        _lib.check(st, "anemoi_segment_sum_cat")
        return out
    if out is None:
        out = torch.empty((n_dst, c), dtype=v.dtype, device=v.device)
    if v.shape[0] == 0:
        return out.zero_()
    with _Timed("segment_sum", bytes=(v.shape[0] + n_dst) * c * v.element_size()):
        st = _lib.load().anemoi_segment_sum(dtype_code(v.dtype), v.data_ptr(), _ld(v), rowptr.data_ptr(),
                                            out.data_ptr(), _ld(_rows(out)), n_dst, c, _stream())
    _lib.check(st, "anemoi_segment_sum")
    return out


def _seed_dev_ptr(seed_dev: Optional[Tensor], like: Tensor):
    if seed_dev is None:
        return None
    if not seed_dev.is_cuda or seed_dev.device != like.device or seed_dev.numel() < 1 or seed_dev.element_size() < 4:
        raise ValueError("dropout seed_dev must be an integer tensor (>= 32 bits per element) on the input's device")
    return seed_dev.data_ptr()


def _mhsa_shape(who: str, qkv: Tensor, batch_size: int, num_heads: int):
    """(rows, C, S, D) of a fused ``q | k | v`` matrix, or ValueError: nothing is launched on operands that do not fit."""
    rows, c3 = _rows(qkv).shape
    if batch_size <= 0 or num_heads <= 0 or rows % batch_size != 0:
        raise ValueError(f"{who}: {rows} rows are no whole number of batch_size = {batch_size} sequences")
    if c3 % 3 != 0 or (c3 // 3) % num_heads != 0:
        raise ValueError(f"{who}: {c3} columns are not 3 x num_heads = {num_heads} x head size")
    return rows, c3 // 3, rows // batch_size, c3 // 3 // num_heads


def _mhsa_operand(who: str, name: str, t: Tensor, qkv: Tensor, rows: int, c: int) -> None:
    if _rows(t).shape != (rows, c) or t.dtype != qkv.dtype:
        raise ValueError(f"{who}: {name} must be [{rows}, {c}] {qkv.dtype} like qkv implies, got {tuple(t.shape)} {t.dtype}")


def mhsa(qkv: Tensor, batch_size: int, num_heads: int, window: int = -1, out: Optional[Tensor] = None,
         return_lse: bool = False, dropout_p: float = 0.0, dropout_seed: int = 0, head_offset: int = 0,
         heads_total: int = 0, seed_dev: Optional[Tensor] = None):
    """Multi-head self attention on the fused ``lin_qkv`` output ``[B*S, 3C]`` -> ``[B*S, C]`` (heads concatenated).
    ``return_lse``: also the f32 ``[B, H, S]`` log-sum-exp of the scaled scores (the backward's input).
    ``dropout_p`` / ``dropout_seed``: attention dropout (training mode of the reference), mask = hash(index, seed);
    ``head_offset`` / ``heads_total``: this call holds the heads ``head_offset ... + num_heads`` of ``heads_total`` (a head
    shard of a model group draws the mask of the unsharded attention; 0 = all heads).  ``seed_dev``: a device integer
    whose low 32 bits the kernels add to ``dropout_seed`` when they run (``runtime.DeviceDropout``: the part of the seed a
    captured HIP graph advances between replays)."""
    rows, c, s_len, d = _mhsa_shape("mhsa", qkv, batch_size, num_heads)
    if out is not None:
        _mhsa_operand("mhsa", "out", out, qkv, rows, c)
    _dev(qkv, out)
    if out is None:
        out = torch.empty((rows, c), dtype=qkv.dtype, device=qkv.device)
    lib = _lib.load()
    code = dtype_code(qkv.dtype)
    ws_bytes = lib.anemoi_mhsa_workspace_bytes(code, batch_size, s_len, num_heads, d)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=qkv.device) if ws_bytes > 0 else None
    lse = torch.empty((batch_size, num_heads, s_len), dtype=torch.float32, device=qkv.device) if return_lse else None
    with _Timed("mhsa", flops=4 * batch_size * num_heads * s_len * s_len * d, s=s_len, h=num_heads, d=d):
        st = lib.anemoi_mhsa(code, qkv.data_ptr(), _ld(qkv), out.data_ptr(), _ld(_rows(out)), _ptr(ws), _ptr(lse),
                             batch_size, s_len, num_heads, d, window, float(dropout_p), int(dropout_seed) & 0xFFFFFFFF,
                             _seed_dev_ptr(seed_dev, qkv), int(head_offset), int(heads_total), _stream())
    _lib.check(st, "anemoi_mhsa")
    return (out, lse) if return_lse else out


def mhsa_backward(qkv: Tensor, out: Tensor, dout: Tensor, lse: Tensor, batch_size: int, num_heads: int,
                  window: int = -1, dropout_p: float = 0.0, dropout_seed: int = 0, head_offset: int = 0,
                  heads_total: int = 0, use_mfma: bool = True, seed_dev: Optional[Tensor] = None) -> Tensor:
    """``d qkv`` ``[B*S, 3C]`` of :func:`mhsa` from the forward's output and log-sum-exp (``anemoi_mhsa_backward``).
    ``use_mfma=False`` withholds the workspace: the call then takes the VALU kernels (plain HIP, any head size / dtype) --
    the yardstick the MFMA route's hand-scheduled kernels are held against in the tests."""
    rows, c, s_len, _ = _mhsa_shape("mhsa_backward", qkv, batch_size, num_heads)
    c3 = 3 * c
    _mhsa_operand("mhsa_backward", "out", out, qkv, rows, c)
    _mhsa_operand("mhsa_backward", "dout", dout, qkv, rows, c)
    if lse.dtype != torch.float32 or not lse.is_contiguous() or tuple(lse.shape) != (batch_size, num_heads, s_len):
        raise ValueError("mhsa_backward: lse must be the contiguous f32 [B, H, S] output of mhsa(return_lse=True)")
    _dev(qkv, out, dout, lse)
    dqkv = torch.empty((rows, c3), dtype=qkv.dtype, device=qkv.device)
    delta = torch.empty((batch_size, num_heads, s_len), dtype=torch.float32, device=qkv.device)
    lib = _lib.load()
    ws_bytes = lib.anemoi_mhsa_backward_workspace_bytes(dtype_code(qkv.dtype), batch_size, s_len, num_heads, c // num_heads)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=qkv.device) if ws_bytes > 0 and use_mfma else None
    st = lib.anemoi_mhsa_backward(dtype_code(qkv.dtype), qkv.data_ptr(), _ld(qkv), out.data_ptr(), _ld(_rows(out)),
                                  dout.data_ptr(), _ld(_rows(dout)), lse.data_ptr(), delta.data_ptr(), dqkv.data_ptr(), c3,
                                  _ptr(ws), batch_size, s_len, num_heads, c // num_heads, window, float(dropout_p),
                                  int(dropout_seed) & 0xFFFFFFFF, _seed_dev_ptr(seed_dev, qkv), int(head_offset),
                                  int(heads_total), _stream())
    _lib.check(st, "anemoi_mhsa_backward")
    return dqkv


def _impute_args(who: str, impute, x: Tensor, n_out: Optional[int] = None):
    """``(fill_val, fill_src, nan_map | None, W, out_nan_src | None)`` of an imputation (``preprocessing.imputer.Imputation``:
    device tensors ``fill_val`` f32 ``[V]``, ``fill_src`` int32 ``[V]``, ``nan_map`` bool / uint8 ``[G, W]`` or ``None`` for a
    dynamic imputer, ``out_nan_src`` int32 or ``None``, and ``W``) checked against the state ``x`` ``[B, T, Ens, G, V]``."""
    v, g = x.shape[-1], x.shape[-2]
    fv, fs, nm, ons = impute.fill_val, impute.fill_src, impute.nan_map, impute.out_nan_src
    _dev(fv, fs, nm, ons)
    if fv.dtype != torch.float32 or fs.dtype != torch.int32 or fv.shape != (v,) or fs.shape != (v,) or \
            not fv.is_contiguous() or not fs.is_contiguous():
        raise ValueError(f"{who}: impute needs f32 fill_val and int32 fill_src with one entry per input variable ({v})")
    w = int(impute.W)
    if nm is not None:
        if nm.dtype not in (torch.bool, torch.uint8) or not nm.is_contiguous() or tuple(nm.shape) != (g, w) or w <= 0:
            raise ValueError(f"{who}: impute.nan_map must be a contiguous bool / uint8 [{g}, W = {w}] tensor, got "
                             f"{nm.dtype} {tuple(nm.shape)}")
    if ons is not None and n_out is not None:
        if ons.dtype != torch.int32 or ons.shape != (n_out,) or not ons.is_contiguous():
            raise ValueError(f"{who}: impute.out_nan_src must be int32 with {n_out} entries")
    return fv, fs, nm, w, ons


REMAP_OPS = {"copy": 0, "log1p": 1, "sqrt": 2, "boxcox": 3, "cos": 4, "sin": 5, "expm1": 6, "square": 7, "inv_boxcox": 8,
             "atan2deg": 9}  # ANEMOI_REMAP_* of include/anemoi_amd.h
REMAP_FORWARD_OPS = ("copy", "log1p", "sqrt", "boxcox", "cos", "sin")
REMAP_INVERSE_OPS = ("copy", "expm1", "square", "inv_boxcox", "atan2deg")


class Remapping:
    """The column tables of a remapper (and the normaliser next to it) for ``assemble_nodes(remap=)``, ``residual_remapped``
    and ``unmap_output``, on one device (include/anemoi_amd.h "Remappers folded into predict_step's I/O kernels").

    Forward, one entry per internal input column ``j``: ``src`` (raw input column), ``op`` (name in ``REMAP_FORWARD_OPS``),
    ``pre`` / ``post`` = ``(mul, add)`` f32 ``[V_int]`` or ``None`` (identity):  ``f_j(x) = post_mul * op(pre_mul * x + pre_add) +
    post_add``.  ``res``: internal input column whose ``f_j`` of the last state is added to internal output column ``c``, -1
    = none.  Inverse, one entry per raw output column ``c``: ``s0`` / ``s1`` (internal output columns; ``s1`` is the sine
    column of ``atan2deg``, else -1), ``inv_op`` (name in ``REMAP_INVERSE_OPS``), ``inv_post`` ``[V_int_out]`` / ``inv_pre``
    ``[V_out]``:  ``z = (inv((y - post_add) / post_mul) - pre_add) / pre_mul``.

    The integer tables are kept twice, on the device for the kernels and on the host for the entry points' range checks; the
    constructor makes the same checks and raises ``ValueError``."""

    __slots__ = ("v_raw", "v_int", "v_int_out", "v_out", "src", "op", "res", "s0", "s1", "inv_op", "h_src", "h_op", "h_res",
                 "h_s0", "h_s1", "h_inv_op", "pre", "post", "inv_pre", "inv_post")

    def __init__(self, device, v_raw: int, src, op, res, s0, s1, inv_op, pre=None, post=None, inv_pre=None,
                 inv_post=None) -> None:
        src, res, s0, s1 = ([int(i) for i in t] for t in (src, res, s0, s1))
        self.v_raw, self.v_int, self.v_int_out, self.v_out = int(v_raw), len(src), len(res), len(s0)
        if len(op) != self.v_int or len(s1) != self.v_out or len(inv_op) != self.v_out:
            raise ValueError("Remapping: one op per src entry, one s1 and one inverse op per s0 entry")
        if any(o not in REMAP_FORWARD_OPS for o in op) or any(o not in REMAP_INVERSE_OPS for o in inv_op):
            raise ValueError(f"Remapping: forward ops are {REMAP_FORWARD_OPS}, inverse ops {REMAP_INVERSE_OPS}")
        if any(not 0 <= i < self.v_raw for i in src) or any(not -1 <= i < self.v_int for i in res):
            raise ValueError("Remapping: src outside the raw input columns or res outside the internal input columns")
        if any(not 0 <= i < self.v_int_out for i in s0) or \
                any(o == "atan2deg" and not 0 <= i < self.v_int_out for o, i in zip(inv_op, s1)):
            raise ValueError("Remapping: s0 / s1 outside the internal output columns")

        def table(values):
            host = torch.tensor(values, dtype=torch.int32)
            return host, host.to(device)

        self.h_src, self.src = table(src)
        self.h_op, self.op = table([REMAP_OPS[o] for o in op])
        self.h_res, self.res = table(res)
        self.h_s0, self.s0 = table(s0)
        self.h_s1, self.s1 = table(s1)
        self.h_inv_op, self.inv_op = table([REMAP_OPS[o] for o in inv_op])

        def pair(p, n, name):
            if p is None:
                return None
            mul, add = (t.detach().to(device=device, dtype=torch.float32).contiguous() for t in p)
            if mul.shape != (n,) or add.shape != (n,):
                raise ValueError(f"Remapping: {name} needs (mul, add) with {n} entries each")
            return mul, add

        self.pre, self.post = pair(pre, self.v_int, "pre"), pair(post, self.v_int, "post")
        self.inv_pre, self.inv_post = pair(inv_pre, self.v_out, "inv_pre"), pair(inv_post, self.v_int_out, "inv_post")


def _remap_forward_args(who: str, remap: Remapping, x: Tensor):
    """Table arguments shared by ``anemoi_assemble_nodes_remapped`` and ``anemoi_residual_remapped``, checked against ``x``."""
    _dev(remap.src, remap.op, *(remap.pre or ()), *(remap.post or ()))
    if x.shape[-1] != remap.v_raw:
        raise ValueError(f"{who}: the state has {x.shape[-1]} variables, the remapping reads {remap.v_raw}")
    pre, post = remap.pre or (None, None), remap.post or (None, None)
    return (remap.src.data_ptr(), remap.op.data_ptr(), _ptr(pre[0]), _ptr(pre[1]), _ptr(post[0]), _ptr(post[1]))


def residual_remapped(y: Tensor, x: Tensor, remap: Remapping) -> Tensor:
    """In place on the f32 internal output ``y`` ``[B, Ens, G, V_int_out]``: ``y[..., c] += f_j(x[b, T - 1, ens, g, src[j]])``
    for ``j = remap.res[c] >= 0`` -- the prognostic residual on the remapped, normalised last state of the RAW ``x``
    ``[B, T, Ens, G, V_raw]``.  Nothing is de-normalised."""
    _dev(y, x, remap.res)
    if y.dtype != torch.float32 or not y.is_contiguous():
        raise ValueError("residual_remapped: y must be contiguous float32")
    x = x.contiguous().float()
    b, t, ens, g, v_raw = x.shape
    if y.shape[-1] != remap.v_int_out or y.numel() != b * ens * g * remap.v_int_out:
        raise ValueError(f"residual_remapped: y {tuple(y.shape)} does not hold [B, Ens, G, {remap.v_int_out}] of x {tuple(x.shape)}")
    tables = _remap_forward_args("residual_remapped", remap, x)
    st = _lib.load().anemoi_residual_remapped(y.data_ptr(), remap.v_int_out, x.data_ptr(), b, t, ens, g, v_raw, remap.v_int,
                                              remap.res.data_ptr(), *tables, remap.h_res.data_ptr(), remap.h_src.data_ptr(),
                                              remap.h_op.data_ptr(), _stream())
    _lib.check(st, "anemoi_residual_remapped")
    return y


def unmap_output(y: Tensor, remap: Remapping) -> Tensor:
    """The f32 internal output ``y`` ``[..., V_int_out]`` -> a new ``[..., V_out]`` in the raw output layout: kept columns, the
    mono inverses and ``atan2`` in degrees of a (cos, sin) column pair, the normaliser's inverse folded in (see
    :class:`Remapping`)."""
    _dev(y, remap.s0, remap.s1, remap.inv_op, *(remap.inv_pre or ()), *(remap.inv_post or ()))
    if y.dtype != torch.float32 or not y.is_contiguous() or y.shape[-1] != remap.v_int_out:
        raise ValueError(f"unmap_output: y must be contiguous float32 [..., {remap.v_int_out}]")
    out = torch.empty(tuple(y.shape[:-1]) + (remap.v_out,), dtype=torch.float32, device=y.device)
    pre, post = remap.inv_pre or (None, None), remap.inv_post or (None, None)
    st = _lib.load().anemoi_unmap_output(y.data_ptr(), remap.v_int_out, out.data_ptr(), remap.v_out,
                                         y.numel() // remap.v_int_out, remap.s0.data_ptr(), remap.s1.data_ptr(),
                                         remap.inv_op.data_ptr(), _ptr(pre[0]), _ptr(pre[1]), _ptr(post[0]), _ptr(post[1]),
                                         remap.h_s0.data_ptr(), remap.h_s1.data_ptr(), remap.h_inv_op.data_ptr(), _stream())
    _lib.check(st, "anemoi_unmap_output")
    return out


def assemble_nodes(x: Optional[Tensor], latlons: Tensor, trainable: Optional[Tensor], batch_size: int,
                   dtype: torch.dtype, ld_out: Optional[int] = None, ensemble: int = 1, in_affine=None,
                   rows: Optional[Tensor] = None, impute=None, remap: Optional[Remapping] = None) -> Tensor:
    """Rows ``(b, ens, g)`` of ``[x (time-major) | latlons | trainable | 0-pad]`` in ``dtype``.  ``in_affine`` =
    ``(mul, add)`` f32 ``[V]``: ``x`` is the raw state, normalised as ``x * mul + add`` while it is read.
    ``rows`` (int64 node ids; batch 1, ensemble 1): only those nodes' rows, in that order (``anemoi_assemble_node_rows``).
    ``impute`` (``preprocessing.imputer.Imputation``): NaN imputation as a select on the read
    (``anemoi_assemble_nodes_imputed``); not with ``rows``.
    ``remap`` (:class:`Remapping`): ``x`` holds the RAW variables and the feature columns are the internal ones, ``f_j`` of the
    raw column ``remap.src[j]`` (``anemoi_assemble_nodes_remapped``); its tables hold the normaliser, so not with
    ``in_affine``, ``impute`` or ``rows``."""
    if remap is not None:
        if x is None or in_affine is not None or impute is not None or rows is not None:
            raise ValueError("assemble_nodes: remap= needs a state x and takes no in_affine, impute or rows")
        _dev(x, latlons, trainable)
        b, t, ens, gx, v_raw = x.shape
        g, n_ll = latlons.shape
        n_tr = 0 if trainable is None else trainable.shape[1]
        if gx != g or b != batch_size:
            raise ValueError(f"assemble_nodes: x has shape {tuple(x.shape)} but the graph has {g} nodes")
        x = x.contiguous().float()
        tables = _remap_forward_args("assemble_nodes", remap, x)
        width = t * remap.v_int + n_ll + n_tr
        ld = width if ld_out is None else ld_out
        latlons = latlons.contiguous().float()
        trainable = None if trainable is None else trainable.contiguous().float()
        out = torch.empty((b * ens * g, ld), dtype=dtype, device=latlons.device)
        st = _lib.load().anemoi_assemble_nodes_remapped(dtype_code(dtype), x.data_ptr(), b, t, ens, g, v_raw, remap.v_int,
                                                        latlons.data_ptr(), n_ll, _ptr(trainable), n_tr, out.data_ptr(), ld,
                                                        *tables, remap.h_src.data_ptr(), remap.h_op.data_ptr(), _stream())
        _lib.check(st, "anemoi_assemble_nodes_remapped")
        return out
    if impute is not None and rows is not None:
        raise ValueError("assemble_nodes: the row-list kernel takes no imputation (rows= with impute=)")
    if impute is not None and x is None:
        raise ValueError("assemble_nodes: impute= needs a state x")
    _dev(x, latlons, trainable, rows)
    mul = add = None
    if in_affine is not None and x is not None:
        mul, add = (t.contiguous().float() for t in in_affine)
        _dev(mul, add)
        if mul.numel() != x.shape[-1] or add.numel() != x.shape[-1]:
            raise ValueError("assemble_nodes: in_affine needs one (mul, add) pair per input variable")
    g = latlons.shape[0]
    n_ll = latlons.shape[1]
    n_tr = 0 if trainable is None else trainable.shape[1]
    if x is not None:
        b, t, ens, gx, v = x.shape
        if gx != g or b != batch_size:
            raise ValueError(f"assemble_nodes: x has shape {tuple(x.shape)} but the graph has {g} nodes")
        x = x.contiguous().float()
    else:
        b, t, ens, v = batch_size, 0, ensemble, 0
    width = t * v + n_ll + n_tr
    ld = width if ld_out is None else ld_out
    latlons = latlons.contiguous().float()
    trainable = None if trainable is None else trainable.contiguous().float()
    if rows is not None:
        if b != 1 or ens != 1 or rows.dtype != torch.int64 or rows.dim() != 1:
            raise ValueError("assemble_nodes: rows needs batch 1, ensemble 1 and a 1-d int64 id list")
        rows = rows.contiguous()
        out = torch.empty((rows.shape[0], ld), dtype=dtype, device=latlons.device)
        st = _lib.load().anemoi_assemble_node_rows(dtype_code(dtype), _ptr(x), t, g, v, latlons.data_ptr(), n_ll,
                                                   _ptr(trainable), n_tr, rows.data_ptr(), rows.shape[0], out.data_ptr(),
                                                   ld, _ptr(mul), _ptr(add), _stream())
        _lib.check(st, "anemoi_assemble_node_rows")
        return out
    out = torch.empty((b * ens * g, ld), dtype=dtype, device=latlons.device)
    if impute is not None:
        fv, fs, nm, w, _ = _impute_args("assemble_nodes", impute, x)
        st = _lib.load().anemoi_assemble_nodes_imputed(dtype_code(dtype), _ptr(x), b, t, ens, g, v, latlons.data_ptr(), n_ll,
                                                       _ptr(trainable), n_tr, out.data_ptr(), ld, _ptr(mul), _ptr(add),
                                                       fv.data_ptr(), fs.data_ptr(), _ptr(nm), w, _stream())
        _lib.check(st, "anemoi_assemble_nodes_imputed")
        return out
    st = _lib.load().anemoi_assemble_nodes(dtype_code(dtype), _ptr(x), b, t, ens, g, v, latlons.data_ptr(), n_ll,
                                           _ptr(trainable), n_tr, out.data_ptr(), ld, _ptr(mul), _ptr(add), _stream())
    _lib.check(st, "anemoi_assemble_nodes")
    return out


def finalize_output(y: Tensor, x: Tensor, src: Tensor, in_affine=None, out_affine=None,
                    rows: Optional[Tensor] = None, impute=None) -> Tensor:
    """In place on the f32 output ``y`` ``[B, Ens, G, V_out]``: prognostic residual from the last time slice of ``x``
    (``src`` int32 ``[V_out]``: input column per output column, -1 = none; ``in_affine`` normalises a raw ``x`` on the
    fly) and, with ``out_affine = (mul, add)``, the de-normalisation ``(y - add) / mul``.  ``rows`` (int64 node ids; batch
    1, ensemble 1): ``y`` holds only those nodes' rows ``[..., len(rows), V_out]`` (``anemoi_finalize_output_rows``).
    ``impute`` (``preprocessing.imputer.Imputation``): the residual adds the imputed value of the raw state, and after the
    de-normalisation the columns of ``impute.out_nan_src`` (int32 ``[V_out]``, -1 = none) get the NaNs of the static map back
    (``anemoi_finalize_output_imputed``); not with ``rows``."""
    if impute is not None and rows is not None:
        raise ValueError("finalize_output: the row-list kernel takes no imputation (rows= with impute=)")
    _dev(y, x, src, rows)
    if y.dtype != torch.float32 or not y.is_contiguous():
        raise ValueError("finalize_output: y must be contiguous float32")
    x = x.contiguous().float()
    b, t, ens, g, v_in = x.shape
    if src.dtype != torch.int32 or src.numel() != y.shape[-1]:
        raise ValueError("finalize_output: src must be int32 with one entry per output column")
    im = ia = om = oa = None
    if in_affine is not None:
        im, ia = (t_.contiguous().float() for t_ in in_affine)
    if out_affine is not None:
        om, oa = (t_.contiguous().float() for t_ in out_affine)
    _dev(im, ia, om, oa)
    if rows is not None:
        if b != 1 or ens != 1 or rows.dtype != torch.int64 or rows.dim() != 1 or y.numel() != rows.shape[0] * y.shape[-1]:
            raise ValueError("finalize_output: rows needs batch 1, ensemble 1, a 1-d int64 id list and one y row per id")
        rows = rows.contiguous()
        st = _lib.load().anemoi_finalize_output_rows(y.data_ptr(), y.shape[-1], x.data_ptr(), t, g, v_in, src.data_ptr(),
                                                     rows.data_ptr(), rows.shape[0], _ptr(im), _ptr(ia), _ptr(om), _ptr(oa),
                                                     _stream())
        _lib.check(st, "anemoi_finalize_output_rows")
        return y
    if impute is not None:
        fv, fs, nm, w, ons = _impute_args("finalize_output", impute, x, y.shape[-1])
        if y.numel() != b * ens * g * y.shape[-1]:
            raise ValueError("finalize_output: y does not hold one row per (batch, member, grid node) of x")
        st = _lib.load().anemoi_finalize_output_imputed(y.data_ptr(), y.shape[-1], x.data_ptr(), b, t, ens, g, v_in,
                                                        src.data_ptr(), _ptr(im), _ptr(ia), _ptr(om), _ptr(oa),
                                                        fv.data_ptr(), fs.data_ptr(), _ptr(nm), w, _ptr(ons), _stream())
        _lib.check(st, "anemoi_finalize_output_imputed")
        return y
    st = _lib.load().anemoi_finalize_output(y.data_ptr(), y.shape[-1], x.data_ptr(), b, t, ens, g, v_in, src.data_ptr(),
                                            _ptr(im), _ptr(ia), _ptr(om), _ptr(oa), _stream())
    _lib.check(st, "anemoi_finalize_output")
    return y


def bound_output(y: Tensor, op_col: Tensor, op_lo: Tensor, op_hi: Tensor, op_mul: Tensor,
                 fin: Optional[tuple] = None, impute=None, slope: Optional[Tensor] = None) -> Tensor:
    """In place on the f32 output ``y`` ``[..., V_out]``: the ordered bounding ops (see ``layers.bounding.compile_boundings``)
    and, with ``fin = (cols int32, mul f32, add f32)``, the de-normalisation of those columns afterwards.
    ``impute`` (``preprocessing.imputer.Imputation`` whose ``out_nan_src`` holds ONE ENTRY PER ``fin`` COLUMN, -1 = none; ``y``
    is ``[..., G, V_out]`` with the map's ``G``): those columns get the NaNs of the static map back after their
    de-normalisation (``anemoi_bound_output_imputed``).
    ``slope`` (f32, one entry per op; ``layers.bounding.bounding_slopes``): a list with leaky classes -- every variant above on
    ``anemoi_bound_output_leaky``; ``None``: exactly the launches of the hard classes."""
    _dev(y, op_col, op_lo, op_hi, op_mul, slope)
    if y.dtype != torch.float32 or not y.is_contiguous():
        raise ValueError("bound_output: y must be contiguous float32")
    n_ops = op_col.numel()
    if op_col.dtype != torch.int32 or op_mul.dtype != torch.int32 or op_lo.dtype != torch.float32 or \
            op_hi.dtype != torch.float32 or op_lo.numel() != n_ops or op_hi.numel() != n_ops or op_mul.numel() != n_ops:
        raise ValueError("bound_output: op lists must be int32 / float32 vectors of one length")
    if slope is not None and (slope.dtype != torch.float32 or slope.numel() != n_ops or not slope.is_contiguous()):
        raise ValueError("bound_output: slope must be a contiguous float32 vector with one entry per op")
    fc = fm = fa = None
    if fin is not None:
        fc, fm, fa = fin
        _dev(fc, fm, fa)
        if fc.dtype != torch.int32 or fm.dtype != torch.float32 or fa.dtype != torch.float32 or \
                fm.numel() != fc.numel() or fa.numel() != fc.numel():
            raise ValueError("bound_output: fin = (int32 columns, f32 mul, f32 add) of one length")
    v_out = y.shape[-1]
    if impute is not None and impute.nan_map is not None:
        nm, ons, n_fin = impute.nan_map, impute.out_nan_src, 0 if fc is None else fc.numel()
        _dev(nm, ons)
        if y.dim() < 2 or nm.dtype not in (torch.bool, torch.uint8) or not nm.is_contiguous() or \
                tuple(nm.shape) != (y.shape[-2], int(impute.W)) or int(impute.W) <= 0:
            raise ValueError(f"bound_output: impute.nan_map must be a contiguous bool / uint8 [G = {y.shape[-2]}, W] tensor")
        if n_fin and (ons is None or ons.dtype != torch.int32 or ons.shape != (n_fin,) or not ons.is_contiguous()):
            raise ValueError(f"bound_output: impute.out_nan_src must be int32 with one entry per fin column ({n_fin})")
        if slope is not None:
            st = _lib.load().anemoi_bound_output_leaky(y.data_ptr(), v_out, y.numel() // max(v_out, 1), n_ops, _ptr(op_col),
                                                       _ptr(op_lo), _ptr(op_hi), _ptr(op_mul), n_fin, _ptr(fc), _ptr(fm),
                                                       _ptr(fa), y.shape[-2], nm.data_ptr(), int(impute.W),
                                                       _ptr(ons) if n_fin else None, slope.data_ptr(), _stream())
            _lib.check(st, "anemoi_bound_output_leaky")
            return y
        st = _lib.load().anemoi_bound_output_imputed(y.data_ptr(), v_out, y.numel() // max(v_out, 1), n_ops, _ptr(op_col),
                                                     _ptr(op_lo), _ptr(op_hi), _ptr(op_mul), n_fin, _ptr(fc), _ptr(fm),
                                                     _ptr(fa), y.shape[-2], nm.data_ptr(), int(impute.W),
                                                     _ptr(ons) if n_fin else None, _stream())
        _lib.check(st, "anemoi_bound_output_imputed")
        return y
    if slope is not None:
        st = _lib.load().anemoi_bound_output_leaky(y.data_ptr(), v_out, y.numel() // max(v_out, 1), n_ops, _ptr(op_col),
                                                   _ptr(op_lo), _ptr(op_hi), _ptr(op_mul), 0 if fc is None else fc.numel(),
                                                   _ptr(fc), _ptr(fm), _ptr(fa), 0, None, 0, None, slope.data_ptr(), _stream())
        _lib.check(st, "anemoi_bound_output_leaky")
        return y
    st = _lib.load().anemoi_bound_output(y.data_ptr(), v_out, y.numel() // max(v_out, 1), n_ops, _ptr(op_col),
                                         _ptr(op_lo), _ptr(op_hi), _ptr(op_mul), 0 if fc is None else fc.numel(),
                                         _ptr(fc), _ptr(fm), _ptr(fa), _stream())
    _lib.check(st, "anemoi_bound_output")
    return y


def _bound_train_lists(who: str, t: Tensor, op_col: Tensor, op_lo: Tensor, op_hi: Tensor, op_mul: Tensor, slope: Tensor) -> int:
    _dev(t, op_col, op_lo, op_hi, op_mul, slope)
    if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() < 1:
        raise ValueError(f"{who}: the [..., V_out] tensor must be contiguous float32")
    n_ops = op_col.numel()
    if op_col.dtype != torch.int32 or op_mul.dtype != torch.int32 or \
            any(v.dtype != torch.float32 or v.numel() != n_ops or not v.is_contiguous() for v in (op_lo, op_hi, slope)) or \
            op_mul.numel() != n_ops or not op_col.is_contiguous() or not op_mul.is_contiguous():
        raise ValueError(f"{who}: op lists must be contiguous int32 / float32 vectors of one length")
    return n_ops


def bound_output_train(y: Tensor, op_col: Tensor, op_lo: Tensor, op_hi: Tensor, op_mul: Tensor, slope: Tensor,
                       n_tape: int) -> Tensor:
    """The bounding ops in place on the f32 ``y`` ``[..., V_out]`` as ``bound_output(slope=)`` applies them, and the tape of
    ``anemoi_bound_output_train`` (returned; f32 ``[n_tape, rows]``: what every op read) for :func:`bound_output_backward`.
    ``n_tape``: the number of ops plus the number of ops with a multiplier."""
    n_ops = _bound_train_lists("bound_output_train", y, op_col, op_lo, op_hi, op_mul, slope)
    v_out = y.shape[-1]
    rows = y.numel() // max(v_out, 1)
    tape = torch.empty((n_tape, rows), dtype=torch.float32, device=y.device)
    st = _lib.load().anemoi_bound_output_train(y.data_ptr(), v_out, rows, n_ops, _ptr(op_col), _ptr(op_lo), _ptr(op_hi),
                                               _ptr(op_mul), _ptr(slope), _ptr(tape), n_tape, _stream())
    _lib.check(st, "anemoi_bound_output_train")
    return tape


def bound_output_backward(g: Tensor, tape: Tensor, op_col: Tensor, op_lo: Tensor, op_hi: Tensor, op_mul: Tensor,
                          slope: Tensor) -> Tensor:
    """The gradient with respect to the input of :func:`bound_output_train` from the gradient ``g`` (f32 ``[..., V_out]``, left
    as it is) of its output and its tape: a new tensor (``anemoi_bound_output_backward``)."""
    n_ops = _bound_train_lists("bound_output_backward", g, op_col, op_lo, op_hi, op_mul, slope)
    _dev(g, tape)
    v_out = g.shape[-1]
    rows = g.numel() // max(v_out, 1)
    if tape.dtype != torch.float32 or not tape.is_contiguous() or tape.dim() != 2 or tape.shape[1] != rows:
        raise ValueError(f"bound_output_backward: the tape must be contiguous float32 [n_tape, rows = {rows}]")
    dx = torch.empty_like(g)
    st = _lib.load().anemoi_bound_output_backward(g.data_ptr(), dx.data_ptr(), v_out, rows, n_ops, _ptr(op_col), _ptr(op_lo),
                                                  _ptr(op_hi), _ptr(op_mul), _ptr(slope), _ptr(tape), tape.shape[0], _stream())
    _lib.check(st, "anemoi_bound_output_backward")
    return dx


def advance_input(x: Tensor, y: Tensor, colmap: Tensor, forcing: Optional[Tensor] = None) -> Tensor:
    """Autoregressive input update in place on ``x`` ``[B, T, Ens, G, V_in]`` (f32): shift the time axis by one and
    fill the last slice from the prediction ``y`` ``[B, Ens, G, V_out]`` / the new ``forcing`` ``[B, Ens, G, F]``
    according to ``colmap`` (int32 ``[V_in]``; see include/anemoi_amd.h: anemoi_advance_input)."""
    _dev(x, y, colmap, forcing)
    if x.dtype != torch.float32 or y.dtype != torch.float32 or not x.is_contiguous() or not y.is_contiguous():
        raise ValueError("advance_input: x and y must be contiguous float32")
    b, t, ens, g, v_in = x.shape
    if tuple(y.shape[:3]) != (b, ens, g) or colmap.dtype != torch.int32 or colmap.numel() != v_in:
        raise ValueError(f"advance_input: y {tuple(y.shape)} / colmap do not match x {tuple(x.shape)}")
    f = 0
    if forcing is not None:
        if forcing.dtype != torch.float32 or not forcing.is_contiguous() or tuple(forcing.shape[:3]) != (b, ens, g):
            raise ValueError("advance_input: forcing must be contiguous float32 [B, Ens, G, F]")
        f = forcing.shape[-1]
    st = _lib.load().anemoi_advance_input(x.data_ptr(), b, t, ens, g, v_in, y.data_ptr(), y.shape[-1], _ptr(forcing), f,
                                          colmap.data_ptr(), _stream())
    _lib.check(st, "anemoi_advance_input")
    return x


# ------------------------------------------------------------------------------------------ rollout training
def inverse_colmap(colmap: Tensor, v_out: int) -> Tensor:
    """int32 ``[v_out]``: the input column ``v`` with ``colmap[v] == m``, or -1 -- what ``advance_state_backward`` reads.
    Host work (one copy of the small map to the CPU): build it once per map.  A ``colmap`` whose non-negative entries
    repeat (two input columns fed by one output column: their gradients would have to meet) is refused."""
    cm = colmap.detach().to("cpu", torch.int64)
    inv = torch.full((v_out,), -1, dtype=torch.int32)
    for v, m in enumerate(cm.tolist()):
        if m < 0:
            continue
        if m >= v_out:
            raise ValueError(f"inverse_colmap: colmap[{v}] = {m} is not one of the {v_out} output columns")
        if inv[m] >= 0:
            raise ValueError(f"inverse_colmap: output column {m} feeds input columns {int(inv[m])} and {v}")
        inv[m] = v
    return inv.to(colmap.device)


def _state_args(who: str, x: Tensor, y_shape, colmap: Tensor):
    if x.dtype != torch.float32 or not x.is_contiguous() or x.dim() != 5:
        raise ValueError(f"{who}: the state must be contiguous float32 [B, T, Ens, G, V_in]")
    b, t, ens, g, v_in = x.shape
    if tuple(y_shape[:3]) != (b, ens, g) or len(y_shape) != 4 or colmap.dtype != torch.int32 or colmap.numel() != v_in:
        raise ValueError(f"{who}: y {tuple(y_shape)} / colmap do not match the state {tuple(x.shape)}")
    return b, t, ens, g, v_in


def advance_state(x: Tensor, y: Tensor, colmap: Tensor, forcing: Optional[Tensor] = None) -> Tensor:
    """Out-of-place :func:`advance_input`: a NEW state with the bits ``advance_input`` would leave in a copy of ``x``
    (include/anemoi_amd.h: anemoi_advance_state)."""
    _dev(x, y, colmap, forcing)
    b, t, ens, g, v_in = _state_args("advance_state", x, y.shape, colmap)
    if y.dtype != torch.float32 or not y.is_contiguous():
        raise ValueError("advance_state: y must be contiguous float32")
    f = 0
    if forcing is not None:
        if forcing.dtype != torch.float32 or not forcing.is_contiguous() or tuple(forcing.shape[:3]) != (b, ens, g):
            raise ValueError("advance_state: forcing must be contiguous float32 [B, Ens, G, F]")
        f = forcing.shape[-1]
    out = torch.empty_like(x)
    st = _lib.load().anemoi_advance_state(x.data_ptr(), out.data_ptr(), b, t, ens, g, v_in, y.data_ptr(), y.shape[-1],
                                          _ptr(forcing), f, colmap.data_ptr(), _stream())
    _lib.check(st, "anemoi_advance_state")
    return out


def advance_state_backward(dx_out: Tensor, v_out: int, colmap: Tensor, inv_colmap: Tensor, has_forcing: bool):
    """``(dx_in, dy)`` of :func:`advance_state` from the gradient of its result; ``inv_colmap`` = :func:`inverse_colmap`."""
    _dev(dx_out, colmap, inv_colmap)
    b, t, ens, g, v_in = _state_args("advance_state_backward", dx_out, (dx_out.shape[0], dx_out.shape[2], dx_out.shape[3], v_out),
                                     colmap)
    if inv_colmap.dtype != torch.int32 or inv_colmap.numel() != v_out:
        raise ValueError("advance_state_backward: inv_colmap must be int32 with one entry per output column")
    dx = torch.empty_like(dx_out)
    dy = torch.empty((b, ens, g, v_out), dtype=torch.float32, device=dx_out.device)
    st = _lib.load().anemoi_advance_state_backward(dx_out.data_ptr(), dx.data_ptr(), dy.data_ptr(), b, t, ens, g, v_in, v_out,
                                                   colmap.data_ptr(), inv_colmap.data_ptr(), int(bool(has_forcing)), _stream())
    _lib.check(st, "anemoi_advance_state_backward")
    return dx, dy


def assemble_nodes_backward(grad: Tensor, shape) -> Tensor:
    """Input gradient of :func:`assemble_nodes`: ``dx`` f32 ``[B, T, Ens, G, V]`` (= ``shape``) from the leading ``T * V``
    columns of ``grad``, the gradient of its ``[B * Ens * G, ld]`` result (f32 or bf16, any row pitch)."""
    _dev(grad)
    _rows(grad)
    b, t, ens, g, v = (int(s) for s in shape)
    if grad.shape[0] != b * ens * g or grad.shape[1] < t * v:
        raise ValueError(f"assemble_nodes_backward: gradient {tuple(grad.shape)} does not belong to an input {tuple(shape)}")
    dx = torch.empty((b, t, ens, g, v), dtype=torch.float32, device=grad.device)
    if dx.numel() == 0:
        return dx
    st = _lib.load().anemoi_assemble_nodes_backward(dtype_code(grad.dtype), grad.data_ptr(), _ld(grad), dx.data_ptr(), b, t,
                                                    ens, g, v, _stream())
    _lib.check(st, "anemoi_assemble_nodes_backward")
    return dx


def prognostic_residual_backward(dy: Tensor, src: Tensor, shape) -> Tensor:
    """Input gradient of the prognostic residual of :func:`finalize_output` (no affine maps): ``dx`` f32 ``[B, T, Ens, G,
    V_in]`` (= ``shape``), zero except ``dx[:, -1, ..., src[c]] = dy[..., c]``."""
    _dev(dy, src)
    b, t, ens, g, v_in = (int(s) for s in shape)
    if dy.dtype != torch.float32 or not dy.is_contiguous() or tuple(dy.shape[:3]) != (b, ens, g) or dy.dim() != 4:
        raise ValueError(f"prognostic_residual_backward: dy must be contiguous float32 [B, Ens, G, V_out], got {tuple(dy.shape)}")
    if src.dtype != torch.int32 or src.numel() != dy.shape[-1]:
        raise ValueError("prognostic_residual_backward: src must be int32 with one entry per output column")
    dx = torch.empty((b, t, ens, g, v_in), dtype=torch.float32, device=dy.device)
    if dx.numel() == 0:
        return dx
    st = _lib.load().anemoi_prognostic_residual_backward(dy.data_ptr(), dy.shape[-1], dx.data_ptr(), b, t, ens, g, v_in,
                                                         src.data_ptr(), _stream())
    _lib.check(st, "anemoi_prognostic_residual_backward")
    return dx


def csr_transpose(indptr, idx, val, n_cols: int):
    """``(indptr, idx, val)`` of the transpose of a CSR matrix with ``n_cols`` columns, built on the HOST (CPU tensors in and
    out; int64 / int32 / the dtype of ``val``) by a stable counting sort over the column index: every transposed row lists its
    entries in ascending source-row order -- the order in which :func:`csr_project` adds them.  Runs once per matrix."""
    indptr = torch.as_tensor(indptr).to(device="cpu", dtype=torch.int64)
    idx = torch.as_tensor(idx).to(device="cpu", dtype=torch.int64)
    val = torch.as_tensor(val).to(device="cpu")
    n_rows, n_cols = indptr.numel() - 1, int(n_cols)
    if n_rows < 0 or n_cols < 0 or idx.numel() != val.numel() or (n_rows >= 0 and int(indptr[-1]) != idx.numel()):
        raise ValueError("csr_transpose: indptr / idx / val do not describe one CSR matrix")
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n_cols):
        raise ValueError(f"csr_transpose: column index out of range [0, {n_cols})")
    rows = torch.repeat_interleave(torch.arange(n_rows, dtype=torch.int64), indptr[1:] - indptr[:-1])
    order = torch.argsort(idx, stable=True)  # (rows ascend along the CSR: a stable sort by column keeps them ascending)
    t_indptr = torch.zeros(n_cols + 1, dtype=torch.int64)
    t_indptr[1:] = torch.cumsum(torch.bincount(idx, minlength=n_cols), 0)
    return t_indptr, rows[order].to(torch.int32), val[order].contiguous()


_CHECKED_COLUMNS: set = set()


def _check_columns(name: str, cols: Optional[Tensor], width: int, unique: bool) -> None:
    """Values of a column list inside ``[0, width)`` (and, for the output side, without repeats: two lanes on one element would
    end the one-owner property).  Reading a device list back synchronises, so a list is checked once -- remembered by its
    storage, version and the width -- and never while its stream is capturing (warm-up calls come first)."""
    if cols is None:
        return
    key = (cols.data_ptr(), cols._version, cols.numel(), int(width), unique, str(cols.device))
    if key in _CHECKED_COLUMNS or (cols.is_cuda and torch.cuda.is_current_stream_capturing()):
        return
    host = cols.detach().cpu()
    if host.numel() and (int(host.min()) < 0 or int(host.max()) >= width):
        raise ValueError(f"csr_project: {name} holds a column outside [0, {width})")
    if unique and torch.unique(host).numel() != host.numel():
        raise ValueError(f"csr_project: {name} repeats a column (every output element is owned by one thread)")
    if len(_CHECKED_COLUMNS) > 4096:
        _CHECKED_COLUMNS.clear()
    _CHECKED_COLUMNS.add(key)


def _byte_span(t: Tensor):
    """[first, last + 1) byte addresses that the elements of a (strided) tensor lie in."""
    if t.numel() == 0:
        return 0, 0
    reach = sum((n - 1) * abs(st) for n, st in zip(t.shape, t.stride()))
    return t.data_ptr(), t.data_ptr() + (reach + 1) * t.element_size()


def csr_project(x: Tensor, out: Tensor, indptr: Tensor, idx: Tensor, val: Tensor, cols_in: Optional[Tensor] = None,
                cols_out: Optional[Tensor] = None, in_affine=None, accumulate: bool = False, p: Optional[int] = None) -> Tensor:
    """``out[a, b, i, cols_out[q]] (= or +=) sum_k val[k] * x'[a, b, idx[k], cols_in[q]]`` over the entries ``k`` of CSR row ``i``
    (``anemoi_csr_project``), for ``q < P``.  ``x`` ``[A, B, n_in, W_in]`` and ``out`` ``[A, B, n_out, W_out]`` are f32 with
    unit-stride columns; the other dimensions may be strided views (a time slice of the state, a transposed ensemble view).
    ``indptr`` int64 ``[n_out + 1]``, ``idx`` int32, ``val`` f32; ``cols_in`` / ``cols_out`` int32 ``[P]`` or ``None`` (the
    identity ``0..P-1``; ``P`` then comes from the other list, from ``p``, or is the width of ``x``).  ``in_affine = (mul, add)``
    per INPUT column: ``x' = x * mul + add``.  Checked here: shapes, dtypes, strides, the values of ``cols_in`` / ``cols_out``
    (inside the widths; ``cols_out`` without repeats; each list once, see :func:`_check_columns`) and that ``x`` and ``out`` do not
    overlap.  NOT checked here: the values of ``idx`` (``< n_in``) and ``indptr`` -- ``layers.truncation`` checks them once on the
    host when it builds a plan, and a caller with matrices of its own must do the same.  Returns ``out``."""
    _dev(x, out, indptr, idx, val, cols_in, cols_out)
    if x.dim() != 4 or out.dim() != 4 or x.dtype != torch.float32 or out.dtype != torch.float32:
        raise ValueError(f"csr_project: x and out must be float32 [A, B, rows, columns], got {tuple(x.shape)} {x.dtype} and "
                         f"{tuple(out.shape)} {out.dtype}")
    if tuple(x.shape[:2]) != tuple(out.shape[:2]):
        raise ValueError(f"csr_project: slab dimensions differ, {tuple(x.shape[:2])} and {tuple(out.shape[:2])}")
    if (x.shape[3] > 1 and x.stride(3) != 1) or (out.shape[3] > 1 and out.stride(3) != 1):
        raise ValueError("csr_project: the columns of x and out must have unit stride")
    n_in, n_out = x.shape[2], out.shape[2]
    if (indptr.dtype != torch.int64 or idx.dtype != torch.int32 or val.dtype != torch.float32 or indptr.numel() != n_out + 1
            or idx.numel() != val.numel() or not (indptr.is_contiguous() and idx.is_contiguous() and val.is_contiguous())):
        raise ValueError("csr_project: indptr int64 [n_out + 1], idx int32 and val float32 of one length, all contiguous")
    for name, c in (("cols_in", cols_in), ("cols_out", cols_out)):
        if c is not None and (c.dtype != torch.int32 or c.dim() != 1 or not c.is_contiguous()):
            raise ValueError(f"csr_project: {name} must be a contiguous 1-d int32 tensor")
    counts = {int(c.numel()) for c in (cols_in, cols_out) if c is not None} | ({int(p)} if p is not None else set())
    if len(counts) > 1:
        raise ValueError(f"csr_project: column counts differ: {sorted(counts)}")
    n_p = counts.pop() if counts else int(x.shape[3])
    if n_p <= 0 or (cols_in is None and n_p > x.shape[3]) or (cols_out is None and n_p > out.shape[3]):
        raise ValueError(f"csr_project: P = {n_p} columns do not fit x / out of widths {x.shape[3]} / {out.shape[3]}")
    _check_columns("cols_in", cols_in, x.shape[3], unique=False)
    _check_columns("cols_out", cols_out, out.shape[3], unique=True)
    (x0, x1), (o0, o1) = _byte_span(x), _byte_span(out)
    if x0 < o1 and o0 < x1:
        raise ValueError("csr_project: x and out overlap in memory")
    mul = add = None
    if in_affine is not None:
        mul, add = (t_.contiguous().float() for t_ in in_affine)
        _dev(mul, add)
        if mul.numel() != x.shape[3] or add.numel() != x.shape[3]:
            raise ValueError("csr_project: in_affine needs one (mul, add) pair per column of x")
    if out.numel() == 0:
        return out
    if idx.numel() == 0:  # no entries at all: nothing to add; the store writes its zeros (two words the kernel never reads
        if accumulate:    # stand in for the empty arrays, whose pointers are null)
            return out
        idx, val = torch.zeros(1, dtype=torch.int32, device=out.device), torch.zeros(1, dtype=torch.float32, device=out.device)
    ldx = max(x.stride(2), x.shape[3]) if n_in <= 1 else x.stride(2)
    ldo = max(out.stride(2), out.shape[3]) if n_out <= 1 else out.stride(2)
    st = _lib.load().anemoi_csr_project(x.data_ptr(), ldx, x.stride(0), x.stride(1), out.data_ptr(), ldo, out.stride(0),
                                        out.stride(1), out.shape[0], out.shape[1], n_in, n_out, indptr.data_ptr(),
                                        idx.data_ptr(), val.data_ptr(), _ptr(cols_in), _ptr(cols_out), n_p, _ptr(mul), _ptr(add),
                                        int(bool(accumulate)), _stream())
    _lib.check(st, "anemoi_csr_project")
    return out


def _loss_operands(who: str, pred: Tensor, target: Tensor, row_w: Tensor, col_w: Optional[Tensor], mask: Optional[Tensor],
                   diff_scale: Optional[Tensor] = None, n_groups: Optional[int] = None, *, ensemble: bool = False,
                   upstream: Optional[Tensor] = None):
    """The operand check of the loss entry points: every operand on the device, float32 and contiguous, ``pred`` / ``target``
    ``[rows, V]`` (``ensemble``: only ``target``; its caller relates ``pred`` to it), ``col_w`` / ``diff_scale`` ``[V]``, ``mask``
    ``[G, V]``, ``rows`` in ``n_groups >= 1`` groups of a multiple of ``G = len(row_w) >= 1`` and ``upstream`` ``[n_groups, V]``.
    ``n_groups = None`` is the scalar ``weighted_mse``: no groups, ``upstream`` one value.  Returns ``rows, V, G, n_groups``."""
    _dev(pred, target, row_w, col_w, mask, diff_scale)
    _rows(pred)
    if ensemble:
        _rows(target)
    elif pred.shape != target.shape or not pred.is_contiguous() or not target.is_contiguous():
        raise ValueError(f"{who}: pred and target must be contiguous [rows, V] of one shape")
    tensors = [t for t in (pred, target, row_w, col_w, mask, diff_scale) if t is not None]
    if any(t.dtype != torch.float32 or not t.is_contiguous() for t in tensors):
        raise ValueError(f"{who}: every operand must be contiguous float32")
    rows, v = target.shape
    g = row_w.numel()
    if any(t is not None and t.numel() != v for t in (col_w, diff_scale)) or (mask is not None and tuple(mask.shape) != (g, v)):
        names = "col_w [V] / mask [G, V]" if n_groups is None else "col_w [V] / diff_scale [V] / mask [G, V]"
        raise ValueError(f"{who}: {names} do not match {'target' if ensemble else 'pred'} {tuple(target.shape)} and row_w [{g}]")
    if n_groups is not None:
        n_groups = int(n_groups)
        if n_groups < 1 or g < 1 or rows % (n_groups * g) != 0:
            raise ValueError(f"{who}: {rows} {'target ' if ensemble else ''}rows are not {n_groups} groups of a multiple of "
                             f"G = {g} rows")
    if upstream is not None:
        _dev(upstream)
        if n_groups is None and (upstream.dtype != torch.float32 or upstream.numel() != 1):
            raise ValueError(f"{who}: upstream must be one float32 value on the device")
        if n_groups is not None and (upstream.dtype != torch.float32 or not upstream.is_contiguous()
                                     or tuple(upstream.shape) != (n_groups, v)):
            raise ValueError(f"{who}: upstream must be contiguous float32 [{n_groups}, {v}] on the device")
    return rows, v, g, n_groups


def _loss_forward(name: str, ws_args: tuple, head: tuple, pred: Tensor, target: Tensor, tail: tuple, out: Tensor) -> Tensor:
    """The forward launch of the loss entry points ``anemoi_<name>(*head, pred, target, *tail, out, workspace, workspace_floats,
    stream)``: ask the library for the workspace size, allocate it, run, check.  (The workspace stands in for an empty
    operand, whose pointer is null.)"""
    lib = _lib.load()
    n_ws = getattr(lib, f"anemoi_{name}_workspace_floats")(*ws_args)
    ws = torch.empty(max(n_ws, 1), dtype=torch.float32, device=out.device)
    with _Timed(name, bytes=(pred.numel() + target.numel()) * 4):
        st = getattr(lib, f"anemoi_{name}")(*head, _ptr(pred) or ws.data_ptr(), _ptr(target) or ws.data_ptr(), *tail,
                                            out.data_ptr(), ws.data_ptr(), n_ws, _stream())
    _lib.check(st, f"anemoi_{name}")
    return out


def weighted_mse(pred: Tensor, target: Tensor, row_w: Tensor, col_w: Tensor, mask: Optional[Tensor] = None,
                 scale: float = 1.0) -> Tensor:
    """``scale * sum keep * row_w[r % G] * col_w[v] * (pred - target)^2`` as an f32 device scalar (``[rows, V]`` operands,
    ``rows`` a multiple of ``G = len(row_w)``; ``mask`` ``[G, V]``, kept where non-zero): deterministic two-stage reduction."""
    rows, v, g, _ = _loss_operands("weighted_mse", pred, target, row_w, col_w, mask)
    loss = torch.empty((), dtype=torch.float32, device=pred.device)
    return _loss_forward("weighted_mse", (rows, v), (), pred, target,
                         (rows, v, g, row_w.data_ptr(), col_w.data_ptr(), _ptr(mask), float(scale)), loss)


def weighted_mse_backward(pred: Tensor, target: Tensor, row_w: Tensor, col_w: Tensor, mask: Optional[Tensor], scale: float,
                          upstream: Tensor) -> Tensor:
    """``d loss / d pred`` of :func:`weighted_mse`; ``upstream`` is the f32 DEVICE scalar gradient of the loss (read by the
    kernel: no host synchronisation)."""
    rows, v, g, _ = _loss_operands("weighted_mse_backward", pred, target, row_w, col_w, mask, upstream=upstream)
    dpred = torch.empty_like(pred)
    if rows == 0:
        return dpred
    st = _lib.load().anemoi_weighted_mse_backward(pred.data_ptr(), target.data_ptr(), rows, v, g, row_w.data_ptr(),
                                                  col_w.data_ptr(), _ptr(mask), float(scale), upstream.data_ptr(),
                                                  dpred.data_ptr(), _stream())
    _lib.check(st, "anemoi_weighted_mse_backward")
    return dpred


def _werr_args(who: str, pred: Tensor, target: Tensor, row_w: Tensor, kind: str, delta: float, col_w: Optional[Tensor],
               mask: Optional[Tensor], diff_scale: Optional[Tensor], n_groups: int, upstream: Optional[Tensor] = None):
    shape = _loss_operands(who, pred, target, row_w, col_w, mask, diff_scale, n_groups, upstream=upstream)
    if kind not in _lib.LOSS_KINDS:
        raise ValueError(f"{who}: unknown kind {kind!r} (one of {sorted(_lib.LOSS_KINDS)})")
    if kind == "huber" and not float(delta) > 0:
        raise ValueError(f"{who}: the Huber delta must be positive, got {delta}")
    return (*shape, _lib.LOSS_KINDS[kind])


def weighted_error(pred: Tensor, target: Tensor, row_w: Tensor, kind: str, *, delta: float = 1.0,
                   col_w: Optional[Tensor] = None, mask: Optional[Tensor] = None, diff_scale: Optional[Tensor] = None,
                   n_groups: int = 1, scale: float = 1.0) -> Tensor:
    """``out[l, v] = scale * sum_{r in group l} keep * row_w[r % G] * col_w[v] * f(diff_scale[v] * (pred - target))`` as f32
    ``[n_groups, V]`` (``[rows, V]`` operands in ``n_groups`` equal groups of consecutive rows, each a multiple of ``G =
    len(row_w)``; ``kind`` one of mse / mae / huber / logcosh): deterministic two-stage reduction, no atomics."""
    rows, v, g, n_groups, code = _werr_args("weighted_error", pred, target, row_w, kind, delta, col_w, mask, diff_scale, n_groups)
    out = torch.empty((n_groups, v), dtype=torch.float32, device=pred.device)
    return _loss_forward("weighted_error", (n_groups, rows // n_groups, v), (code, float(delta)), pred, target,
                         (rows, v, g, n_groups, row_w.data_ptr(), _ptr(col_w), _ptr(mask), _ptr(diff_scale), float(scale)), out)


def weighted_error_backward(pred: Tensor, target: Tensor, row_w: Tensor, kind: str, *, delta: float = 1.0,
                            col_w: Optional[Tensor] = None, mask: Optional[Tensor] = None,
                            diff_scale: Optional[Tensor] = None, n_groups: int = 1, scale: float = 1.0,
                            upstream: Tensor) -> Tensor:
    """``d (sum upstream * out) / d pred`` of :func:`weighted_error`; ``upstream`` is the f32 DEVICE ``[n_groups, V]`` gradient
    of its result (read by the kernel: no host synchronisation)."""
    rows, v, g, n_groups, code = _werr_args("weighted_error_backward", pred, target, row_w, kind, delta, col_w, mask,
                                            diff_scale, n_groups, upstream)
    dpred = torch.empty_like(pred)
    if rows == 0:
        return dpred
    with _Timed("weighted_error_backward", bytes=3 * pred.numel() * 4):
        st = _lib.load().anemoi_weighted_error_backward(code, float(delta), pred.data_ptr(), target.data_ptr(), rows, v, g,
                                                        n_groups, row_w.data_ptr(), _ptr(col_w), _ptr(mask), _ptr(diff_scale),
                                                        float(scale), upstream.data_ptr(), dpred.data_ptr(), _stream())
    _lib.check(st, "anemoi_weighted_error_backward")
    return dpred


def _ens_args(who: str, pred: Tensor, target: Tensor, row_w: Tensor, kind: str, n_members: int, alpha: float,
              col_w: Optional[Tensor], mask: Optional[Tensor], diff_scale: Optional[Tensor], n_groups: int,
              upstream: Optional[Tensor] = None):
    rows, v, g, n_groups = _loss_operands(who, pred, target, row_w, col_w, mask, diff_scale, n_groups, ensemble=True,
                                          upstream=upstream)
    if kind not in _lib.ENS_KINDS:
        raise ValueError(f"{who}: unknown kind {kind!r} (one of {sorted(_lib.ENS_KINDS)})")
    e = int(n_members)
    if e < 2:
        raise ValueError(f"{who}: an ensemble score needs at least 2 members, got n_members = {e}")
    if e > _lib.ENS_MAX_MEMBERS:
        raise NotImplementedError(f"{who}: n_members = {e}, at most {_lib.ENS_MAX_MEMBERS}")
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError(f"{who}: alpha must lie in [0, 1], got {alpha}")
    if pred.shape[1] != v or pred.shape[0] != rows * e:
        raise ValueError(f"{who}: pred {tuple(pred.shape)} is not [rows * n_members, V] of target {tuple(target.shape)} with "
                         f"n_members = {e}")
    return rows, v, g, e, n_groups, _lib.ENS_KINDS[kind]


def ensemble_score(pred: Tensor, target: Tensor, row_w: Tensor, kind: str, *, n_members: int, alpha: float = 1.0,
                   col_w: Optional[Tensor] = None, mask: Optional[Tensor] = None, diff_scale: Optional[Tensor] = None,
                   n_groups: int = 1, scale: float = 1.0) -> Tensor:
    """``out[l, v] = scale * sum_{b, g} keep * row_w[g] * col_w[v] * S(members, target)`` as f32 ``[n_groups, V]``: ``target``
    ``[n_groups * B * G, V]``, ``pred`` ``[n_groups * B * n_members * G, V]`` (member ``e`` of point ``(l, b, g)`` in row ``((l B +
    b) E + e) G + g``), ``kind`` one of afcrps (with ``alpha``) / mean_se / variance, ``2 <= n_members <= 16``: deterministic
    two-stage reduction, no atomics, every member read once."""
    rows, v, g, e, n_groups, code = _ens_args("ensemble_score", pred, target, row_w, kind, n_members, alpha, col_w, mask,
                                              diff_scale, n_groups)
    out = torch.empty((n_groups, v), dtype=torch.float32, device=target.device)
    return _loss_forward("ensemble_score", (n_groups, rows // n_groups, v, e), (code, float(alpha)), pred, target,
                         (rows, v, g, e, n_groups, row_w.data_ptr(), _ptr(col_w), _ptr(mask), _ptr(diff_scale), float(scale)), out)


def ensemble_score_backward(pred: Tensor, target: Tensor, row_w: Tensor, kind: str, *, n_members: int, alpha: float = 1.0,
                            col_w: Optional[Tensor] = None, mask: Optional[Tensor] = None,
                            diff_scale: Optional[Tensor] = None, n_groups: int = 1, scale: float = 1.0,
                            upstream: Tensor) -> Tensor:
    """``d (sum upstream * out) / d pred`` of :func:`ensemble_score` (afcrps only); ``upstream`` is the f32 DEVICE ``[n_groups,
    V]`` gradient of its result (read by the kernel: no host synchronisation).  The target gets no gradient."""
    rows, v, g, e, n_groups, code = _ens_args("ensemble_score_backward", pred, target, row_w, kind, n_members, alpha, col_w,
                                              mask, diff_scale, n_groups, upstream)
    dpred = torch.empty_like(pred)
    if rows == 0 and code == _lib.ENS_AFCRPS:
        return dpred
    with _Timed("ensemble_score_backward", bytes=(2 * pred.numel() + target.numel()) * 4):
        st = _lib.load().anemoi_ensemble_score_backward(code, float(alpha), _ptr(pred) or upstream.data_ptr(),
                                                        _ptr(target) or upstream.data_ptr(), rows, v, g, e, n_groups,
                                                        row_w.data_ptr(), _ptr(col_w), _ptr(mask), _ptr(diff_scale),
                                                        float(scale), upstream.data_ptr(), dpred.data_ptr(), _stream())
    _lib.check(st, "anemoi_ensemble_score_backward")
    return dpred


def prognostic_residual(y: Tensor, x: Tensor, out_idx: Tensor, in_idx: Tensor) -> Tensor:
    """In place: ``y[..., out_idx] += x[:, -1, :, :, in_idx]`` (y f32 ``[B, Ens, G, V_out]`` contiguous)."""
    _dev(y, x, out_idx, in_idx)
    if y.dtype != torch.float32 or not y.is_contiguous():
        raise ValueError("prognostic_residual: y must be contiguous float32")
    b, t, ens, g, v_in = x.shape
    x = x.contiguous().float()
    st = _lib.load().anemoi_prognostic_residual(y.data_ptr(), y.shape[-1], x.data_ptr(), b, t, ens, g, v_in,
                                                out_idx.data_ptr(), in_idx.data_ptr(), out_idx.shape[0], _stream())
    _lib.check(st, "anemoi_prognostic_residual")
    return y


def convert_pad(src: Tensor, dtype: torch.dtype, ld_out: Optional[int] = None) -> Tensor:
    """Copy ``src`` ([rows, cols]) into a ``dtype`` buffer whose rows are zero padded to ``ld_out`` columns."""
    _dev(src)
    _rows(src)
    rows, cols = src.shape
    ld = cols if ld_out is None else ld_out
    out = torch.empty((rows, ld), dtype=dtype, device=src.device)
    if rows == 0:  # (an edge set without edges: torch hands out a null pointer for the empty tensor)
        return out
    st = _lib.load().anemoi_convert_pad(dtype_code(src.dtype), src.data_ptr(), _ld(src), dtype_code(dtype),
                                        out.data_ptr(), ld, rows, cols, _stream())
    _lib.check(st, "anemoi_convert_pad")
    return out


def add(a: Tensor, b: Tensor, out: Optional[Tensor] = None) -> Tensor:
    _dev(a, b, out)
    if a.shape != b.shape or a.dtype != b.dtype:
        raise ValueError("add: shape / dtype mismatch")
    if out is None:
        out = torch.empty(a.shape, dtype=a.dtype, device=a.device)
    with _Timed("add", bytes=3 * a.shape[0] * a.shape[1] * a.element_size(), m=a.shape[0], n=a.shape[1]):
        st = _lib.load().anemoi_add(dtype_code(a.dtype), a.data_ptr(), _ld(_rows(a)), b.data_ptr(), _ld(_rows(b)),
                                    out.data_ptr(), _ld(_rows(out)), a.shape[0], a.shape[1], _stream())
    _lib.check(st, "anemoi_add")
    return out


# ------------------------------------------------------------------------------------------ backward pass, dense half
def transpose(x: Tensor, ld_out: Optional[int] = None) -> Tensor:
    """``x.T`` as a new row-major matrix ``[cols, ld_out]`` (``ld_out >= rows``, extra columns zero): the K-contiguous
    operand of a GEMM that reduces over the rows of ``x``."""
    _dev(x)
    rows, cols = _rows(x).shape
    ld = rows if ld_out is None else ld_out
    out = torch.empty((cols, ld), dtype=x.dtype, device=x.device)
    st = _lib.load().anemoi_transpose(dtype_code(x.dtype), x.data_ptr(), _ld(x), out.data_ptr(), ld, rows, cols, _stream())
    _lib.check(st, "anemoi_transpose")
    return out


def col_sum(x: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """f32 column sums of a row-major matrix (bias gradient), deterministic two-stage reduction."""
    _dev(x)
    rows, cols = _rows(x).shape
    lib = _lib.load()
    if out is None:
        out = torch.empty(cols, dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or out.numel() != cols or not out.is_contiguous():
        raise ValueError("col_sum: out must be a contiguous f32 vector of the column count")
    if rows == 0:  # (an empty tensor has no storage: the library would see a null pointer)
        return out.zero_()
    n_ws = lib.anemoi_col_sum_workspace_floats(rows, cols)
    ws = torch.empty(max(n_ws, 1), dtype=torch.float32, device=x.device)
    st = lib.anemoi_col_sum(dtype_code(x.dtype), x.data_ptr(), _ld(x), rows, cols, out.data_ptr(), ws.data_ptr(), n_ws,
                            _stream())
    _lib.check(st, "anemoi_col_sum")
    return out


def row_dot(a: Tensor, b: Tensor, shift: Optional[Tensor] = None) -> Tensor:
    """``out[r] = sum_c a[r, c] * (b[r, c] - shift[c])`` in f32 (``shift``: optional f32 ``[cols]``)."""
    _dev(a, b, shift)
    rows, cols = _rows(a).shape
    if tuple(_rows(b).shape) != (rows, cols) or a.dtype != b.dtype:
        raise ValueError("row_dot: a and b must have the same shape and dtype")
    if shift is not None and (shift.dtype != torch.float32 or shift.numel() < cols or not shift.is_contiguous()):
        raise ValueError("row_dot: shift must be a contiguous f32 vector with one entry per column")
    out = torch.empty(rows, dtype=torch.float32, device=a.device)
    with _Timed("row_dot", bytes=2 * rows * cols * a.element_size()):
        st = _lib.load().anemoi_row_dot(dtype_code(a.dtype), a.data_ptr(), _ld(_rows(a)), b.data_ptr(), _ld(_rows(b)),
                                        _ptr(shift), out.data_ptr(), rows, cols, _stream())
    _lib.check(st, "anemoi_row_dot")
    return out


def row_scale(x: Tensor, s: Tensor, alpha: float = 1.0, out: Optional[Tensor] = None) -> Tensor:
    """``alpha * s[:, None] * x`` in x's dtype (``s``: contiguous f32 ``[rows]``)."""
    _dev(x, s, out)
    rows, cols = _rows(x).shape
    if s.dtype != torch.float32 or s.numel() != rows or not s.is_contiguous():
        raise ValueError("row_scale: s must be a contiguous f32 vector with one entry per row")
    if out is None:
        out = torch.empty((rows, cols), dtype=x.dtype, device=x.device)
    with _Timed("row_scale", bytes=2 * rows * cols * x.element_size()):
        st = _lib.load().anemoi_row_scale(dtype_code(x.dtype), x.data_ptr(), _ld(_rows(x)), s.data_ptr(), float(alpha),
                                          out.data_ptr(), _ld(_rows(out)), rows, cols, _stream())
    _lib.check(st, "anemoi_row_scale")
    return out


def raw_row_tail(x: Tensor, stats: Tensor, out: Tensor) -> Tensor:
    """``out[:, :K] = stats[:, 0, None] * x`` (f32 product, one rounding) and ``out[:, K:2K] = x`` -- the two raw-row blocks of
    the decoder fold's projection operand (``out``: a ``[rows, 2K]`` column view of the attention buffer).  ``stats``: the
    contiguous f32 ``[rows, 2]`` LayerNorm statistics of the rows.  Recorded as a ``row_scale`` launch."""
    _dev(x, stats, out)
    rows, cols = _rows(x).shape
    if stats.dtype != torch.float32 or tuple(stats.shape) != (rows, 2) or not stats.is_contiguous():
        raise ValueError("raw_row_tail: stats must be the contiguous [rows, 2] f32 result of row_stats")
    if out.dtype != x.dtype or tuple(_rows(out).shape) != (rows, 2 * cols):
        raise ValueError("raw_row_tail: out must be a [rows, 2 * cols] view in x's dtype")
    if rows == 0:
        return out
    with _Timed("row_scale", bytes=3 * rows * cols * x.element_size(), raw_tail=True):
        st = _lib.load().anemoi_raw_row_tail(dtype_code(x.dtype), x.data_ptr(), _ld(x), stats.data_ptr(), out.data_ptr(),
                                             _ld(out), rows, cols, _stream())
    _lib.check(st, "anemoi_raw_row_tail")
    return out


def _fused_epilogue_rows(dtype, m: int, n: int, k: int, ldx: int, ldp: int = 0) -> int:
    """Rows that ``linear_dual`` / ``linear_actgrad`` hand to the persistent kernel's DUAL / GMUL epilogue (``ldp``: pitch of the
    saved pre-activation, 0 where the call allocates it): the whole 256-row tiles of a bf16 product the library takes, from
    1024 of them on, and up to 8 ragged rows behind them (the launch's skinny pass).  0: the two-pass pair does it all."""
    if not (dtype == torch.bfloat16 and n >= 256 and n % 8 == 0 and k >= 128 and k % 64 == 0 and ldx % 8 == 0 and ldp % 8 == 0):
        return 0
    m_main = (m // 256) * 256
    if m_main < 1024:
        return 0
    return m if m - m_main <= 8 else m_main


def linear_dual(x: Tensor, w: Tensor, bias: Optional[Tensor], act: str):
    """``(pre, y) = (x @ w.T + bias, act(pre))``: the training forward of Linear + activation.  One launch
    (``anemoi_linear_dual``) for the whole 256-row tiles of a bf16 product and up to 8 rows behind them, the GEMM +
    activation pass pair for a longer remainder."""
    _dev(x, w, bias)
    m, k = _rows(x).shape
    n = w.shape[0]
    if w.dtype != x.dtype or not w.is_contiguous() or w.shape[1] != k:
        raise ValueError("linear_dual: weight must be contiguous [N, K] in the activation dtype, K as x")
    m_main = _fused_epilogue_rows(x.dtype, m, n, k, _ld(x))
    if m_main == 0:
        pre = linear(x, w, bias)
        return pre, act_forward(pre, act)
    pre = torch.empty((m, n), dtype=x.dtype, device=x.device)
    y = torch.empty((m, n), dtype=x.dtype, device=x.device)
    with _Timed("linear", flops=2 * m_main * n * k, bytes=(m_main * k + n * k + 2 * m_main * n) * 2, m=m_main, n=n, k=k):
        st = _lib.load().anemoi_linear_dual(dtype_code(x.dtype), x.data_ptr(), _ld(x), w.data_ptr(), _ptr(bias),
                                            pre.data_ptr(), n, y.data_ptr(), n, m_main, n, k, _lib.ACT_CODES[act], _stream())
    _lib.check(st, "anemoi_linear_dual")
    if m_main < m:  # the ragged rows
        linear(x[m_main:], w, bias, out=pre[m_main:])
        y[m_main:].copy_(act_forward(pre[m_main:], act))
    return pre, y


def linear_actgrad(x: Tensor, w: Tensor, pre: Tensor, act: str) -> Tensor:
    """``(x @ w.T) * act'(pre)``: the dX GEMM of the Linear behind an activation with the activation's derivative in its
    epilogue (``anemoi_linear_actgrad``; whole 256-row tiles of a bf16 product, GEMM + ``act_backward`` for the rest)."""
    _dev(x, w, pre)
    m, k = _rows(x).shape
    n = w.shape[0]
    if w.dtype != x.dtype or not w.is_contiguous() or w.shape[1] != k or tuple(_rows(pre).shape) != (m, n):
        raise ValueError("linear_actgrad: w must be contiguous [N, K] in the activation dtype, pre [M, N]")
    m_main = _fused_epilogue_rows(x.dtype, m, n, k, _ld(x), _ld(_rows(pre)))
    if m_main == 0:
        return act_backward(pre, linear(x, w), act)
    out = torch.empty((m, n), dtype=x.dtype, device=x.device)
    with _Timed("linear", flops=2 * m_main * n * k, bytes=(m_main * k + n * k + 2 * m_main * n) * 2, m=m_main, n=n, k=k):
        st = _lib.load().anemoi_linear_actgrad(dtype_code(x.dtype), x.data_ptr(), _ld(x), w.data_ptr(), pre.data_ptr(),
                                               _ld(_rows(pre)), out.data_ptr(), n, m_main, n, k, _lib.ACT_CODES[act],
                                               _stream())
    _lib.check(st, "anemoi_linear_actgrad")
    if m_main < m:
        out[m_main:].copy_(act_backward(pre[m_main:], linear(x[m_main:], w), act))
    return out


def act_forward(pre: Tensor, act: str, residual: Optional[Tensor] = None) -> Tensor:
    """``act(pre) + residual`` in one pass (the differentiable Linear keeps ``pre`` for the backward)."""
    _dev(pre, residual)
    rows, cols = _rows(pre).shape
    out = torch.empty((rows, cols), dtype=pre.dtype, device=pre.device)
    if rows == 0:  # (an empty tensor has no storage: the library would see null pointers)
        return out
    st = _lib.load().anemoi_act_forward(dtype_code(pre.dtype), _lib.ACT_CODES[act], pre.data_ptr(), _ld(pre),
                                        _ptr(residual), 0 if residual is None else _ld(_rows(residual)), out.data_ptr(),
                                        cols, rows, cols, _stream())
    _lib.check(st, "anemoi_act_forward")
    return out


def act_backward(pre: Tensor, dy: Tensor, act: str) -> Tensor:
    """``dy * act'(pre)`` (``pre`` = the Linear's result before its activation)."""
    _dev(pre, dy)
    rows, cols = _rows(pre).shape
    if tuple(_rows(dy).shape) != (rows, cols) or dy.dtype != pre.dtype:
        raise ValueError("act_backward: pre and dy must have the same shape and dtype")
    out = torch.empty((rows, cols), dtype=pre.dtype, device=pre.device)
    if rows == 0:  # (an edge phase without edges: an empty tensor has no storage, the library would see null pointers)
        return out
    st = _lib.load().anemoi_act_backward(dtype_code(pre.dtype), _lib.ACT_CODES[act], pre.data_ptr(), _ld(pre),
                                         dy.data_ptr(), _ld(dy), out.data_ptr(), cols, rows, cols, _stream())
    _lib.check(st, "anemoi_act_backward")
    return out


def layer_norm_backward(x: Tensor, stats: Tensor, gamma: Tensor, dy: Tensor, dres: Optional[Tensor] = None):
    """``(dx, dgamma, dbeta)`` of ``layer_norm(x) * gamma + beta`` from the forward's ``row_stats(x)``; ``dres`` (optional,
    x's shape and dtype) is added to ``dx`` in the same pass (the skip connection's gradient)."""
    _dev(x, stats, gamma, dy, dres)
    rows, c = _rows(x).shape
    if tuple(_rows(dy).shape) != (rows, c) or dy.dtype != x.dtype or stats.shape != (rows, 2):
        raise ValueError("layer_norm_backward: shapes of x, dy, stats do not match")
    lib = _lib.load()
    dx = torch.empty((rows, c), dtype=x.dtype, device=x.device)
    dgamma = torch.empty(c, dtype=torch.float32, device=x.device)
    dbeta = torch.empty(c, dtype=torch.float32, device=x.device)
    if dres is not None and (tuple(_rows(dres).shape) != (rows, c) or dres.dtype != x.dtype):
        raise ValueError("layer_norm_backward: dres must have x's shape and dtype")
    if rows == 0:  # (no rows: nothing to launch, and an empty tensor has no storage to point the library at)
        return dx, dgamma.zero_(), dbeta.zero_()
    n_ws = lib.anemoi_layer_norm_backward_workspace_floats(rows, c)
    ws = torch.empty(n_ws, dtype=torch.float32, device=x.device)
    gamma = gamma.detach().float().contiguous()
    st = lib.anemoi_layer_norm_backward(dtype_code(x.dtype), x.data_ptr(), _ld(x), stats.data_ptr(), gamma.data_ptr(),
                                        dy.data_ptr(), _ld(dy), _ptr(dres), 0 if dres is None else _ld(_rows(dres)),
                                        dx.data_ptr(), c, rows, c, dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(),
                                        n_ws, _stream())
    _lib.check(st, "anemoi_layer_norm_backward")
    return dx, dgamma, dbeta


def _pad_k(t: Tensor, kp: int) -> Tensor:
    """f32, contiguous, the last axis zero-padded to ``kp`` columns (the layout the conditional LayerNorm kernels read)."""
    t = t.detach().float()
    if t.shape[1] == kp:
        return t.contiguous()
    out = torch.zeros((t.shape[0], kp), dtype=torch.float32, device=t.device)
    out[:, :t.shape[1]] = t
    return out


def _cond_ln_args(who: str, x: Tensor, cond: Tensor, w_scale: Tensor, w_bias: Tensor):
    rows, c = _rows(x).shape
    k = w_scale.shape[1]
    if tuple(w_scale.shape) != (c, k) or tuple(w_bias.shape) != (c, k) or tuple(cond.shape) != (rows, k):
        raise ValueError(f"{who}: x {tuple(x.shape)}, cond {tuple(cond.shape)} and the weights {tuple(w_scale.shape)} / "
                         f"{tuple(w_bias.shape)} do not fit ([rows, C], [rows, K], [C, K])")
    return rows, c, k


def cond_layer_norm(x: Tensor, cond: Tensor, w_scale: Tensor, b_scale: Tensor, w_bias: Tensor, b_bias: Tensor,
                    eps: float = 1e-5, with_stats: bool = False):
    """``xhat * (1 + cond @ w_scale.T + b_scale) + (cond @ w_bias.T + b_bias)`` in one pass over ``x [rows, C]`` (f32 or bf16;
    ``cond [rows, K]``, the weights ``[C, K]`` and the biases ``[C]`` are taken in f32), ``K <= 32`` -- a wider condition raises
    ``NotImplementedError`` (``autograd.cond_layer_norm`` then composes the operation).  ``with_stats``: also the row
    statistics ``[rows, 2]`` of :func:`row_stats`, for :func:`cond_layer_norm_backward`."""
    _dev(x, cond, w_scale, b_scale, w_bias, b_bias)
    rows, c, k = _cond_ln_args("cond_layer_norm", x, cond, w_scale, w_bias)
    if k > _lib.COND_LN_MAX_K:
        raise NotImplementedError(f"cond_layer_norm: K = {k} condition columns, at most {_lib.COND_LN_MAX_K} on the fused kernel")
    kp = _lib.cond_ln_padded_k(k)
    cond, w_scale, w_bias = (_pad_k(t, kp) for t in (cond, w_scale, w_bias))
    b_scale, b_bias = (t.detach().float().contiguous() for t in (b_scale, b_bias))
    y = torch.empty((rows, c), dtype=x.dtype, device=x.device)
    stats = torch.empty((rows, 2), dtype=torch.float32, device=x.device) if with_stats else None
    with _Timed("cond_layer_norm", bytes=2 * rows * c * x.element_size() + rows * k * 4, flops=4 * rows * c * k):
        st = _lib.load().anemoi_cond_layer_norm(dtype_code(x.dtype), x.data_ptr(), _ld(x), cond.data_ptr(), kp, k,
                                                w_scale.data_ptr(), kp, b_scale.data_ptr(), w_bias.data_ptr(), b_bias.data_ptr(),
                                                y.data_ptr(), c, _ptr(stats), rows, c, eps, _stream())
    _lib.check(st, "anemoi_cond_layer_norm")
    return (y, stats) if with_stats else y


def cond_layer_norm_backward(dy: Tensor, x: Tensor, stats: Tensor, cond: Tensor, w_scale: Tensor, b_scale: Tensor,
                             w_bias: Tensor):
    """``(dx, dcond, dw_scale, db_scale, dw_bias, db_bias)`` of :func:`cond_layer_norm` from the forward's statistics; everything
    but ``dx`` in f32.  Deterministic (fixed row chunks, partials added in ascending order)."""
    _dev(dy, x, stats, cond, w_scale, b_scale, w_bias)
    rows, c, k = _cond_ln_args("cond_layer_norm_backward", x, cond, w_scale, w_bias)
    if tuple(_rows(dy).shape) != (rows, c) or dy.dtype != x.dtype or tuple(stats.shape) != (rows, 2):
        raise ValueError("cond_layer_norm_backward: shapes of x, dy, stats do not match")
    if k > _lib.COND_LN_MAX_K:
        raise NotImplementedError(f"cond_layer_norm_backward: K = {k} condition columns, at most {_lib.COND_LN_MAX_K}")
    kp = _lib.cond_ln_padded_k(k)
    cond, w_scale, w_bias = (_pad_k(t, kp) for t in (cond, w_scale, w_bias))
    b_scale = b_scale.detach().float().contiguous()
    dev = x.device
    dx = torch.empty((rows, c), dtype=x.dtype, device=dev)
    dcond = torch.empty((rows, k), dtype=torch.float32, device=dev)
    dws, dwb = (torch.empty((c, k), dtype=torch.float32, device=dev) for _ in range(2))
    dbs, dbb = (torch.empty(c, dtype=torch.float32, device=dev) for _ in range(2))
    lib = _lib.load()
    if rows == 0:
        return dx, dcond, dws.zero_(), dbs.zero_(), dwb.zero_(), dbb.zero_()
    n_ws = lib.anemoi_cond_layer_norm_backward_workspace_floats(rows, c, k)
    ws = torch.empty(max(n_ws, 1), dtype=torch.float32, device=dev)
    with _Timed("cond_layer_norm_backward", bytes=5 * rows * c * x.element_size() + 2 * rows * k * 4, flops=10 * rows * c * k):
        st = lib.anemoi_cond_layer_norm_backward(dtype_code(x.dtype), dy.data_ptr(), _ld(dy), x.data_ptr(), _ld(x),
                                                 stats.data_ptr(), cond.data_ptr(), kp, k, w_scale.data_ptr(), kp, b_scale.data_ptr(),
                                                 w_bias.data_ptr(), dx.data_ptr(), c, dcond.data_ptr(), dws.data_ptr(),
                                                 dbs.data_ptr(), dwb.data_ptr(), dbb.data_ptr(), rows, c, ws.data_ptr(), n_ws,
                                                 _stream())
    _lib.check(st, "anemoi_cond_layer_norm_backward")
    return dx, dcond, dws, dbs, dwb, dbb


def gaussian_noise(rows: int, k: int, std: float = 1.0, *, seed: int, seed_dev: Optional[Tensor] = None, device=None,
                   out: Optional[Tensor] = None) -> Tensor:
    """f32 ``[rows, k]`` of ``std * z``, ``z ~ N(0, 1)``: element ``i = row * k + col`` is a function of ``(seed + seed_dev[0], i)``
    alone (Philox4x32-10 and Box-Muller, ``anemoi_gaussian_noise``), so the first ``n`` rows of a longer draw are the ``n``-row
    draw.  ``seed_dev``: a device integer word the kernel adds to the seed (``runtime.DeviceDropout``: a captured step draws new
    noise on every replay)."""
    if out is None:
        out = torch.empty((int(rows), int(k)), dtype=torch.float32,
                          device=device if device is not None else (seed_dev.device if seed_dev is not None else "cuda"))
    _dev(out)
    if out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (int(rows), int(k)):
        raise ValueError("gaussian_noise: out must be contiguous float32 [rows, k]")
    if out.numel() == 0:  # (torch hands out a null pointer for an empty tensor)
        return out
    with _Timed("gaussian_noise", bytes=out.numel() * 4):
        st = _lib.load().anemoi_gaussian_noise(out.data_ptr(), int(rows), int(k), float(std), int(seed) & 0xFFFFFFFF,
                                               _seed_dev_ptr(seed_dev, out), _stream())
    _lib.check(st, "anemoi_gaussian_noise")
    return out


def _head_norm_args(who: str, x: Tensor, weight: Tensor, num_heads: int, groups: int):
    """``(rows, width, head size, f32 [groups, D] weight)`` of a ``[rows, groups * H * D]`` view and its norm weights."""
    rows, width = _rows(x).shape
    if groups < 1 or num_heads < 1 or width % (groups * num_heads) != 0 or width == 0:
        raise ValueError(f"{who}: {width} columns do not split into {groups} group(s) of {num_heads} heads")
    d = width // (groups * num_heads)
    if weight.numel() != groups * d or weight.shape[-1] != d:
        raise ValueError(f"{who}: weight {tuple(weight.shape)} does not fit [groups = {groups}, D = {d}]")
    if d > _lib.HEAD_NORM_MAX_D:
        raise NotImplementedError(f"{who}: head size {d}, at most {_lib.HEAD_NORM_MAX_D}")
    return rows, width, d, weight.detach().float().contiguous()


def head_norm(x: Tensor, weight: Tensor, num_heads: int, groups: int = 1, eps: float = 1e-5, out: Optional[Tensor] = None,
              with_stats: bool = False):
    """``qk_norm``: the bias-free LayerNorm over every head of ``x [rows, groups * H * D]`` (a row-major view, e.g. the ``q | k``
    columns of a ``q | k | v`` product: ``groups = 2``), scaled by ``weight [groups, D]`` (f32; ``[D]`` for one group).  Statistics
    in f32, the result in ``x``'s dtype.  ``out=x`` normalises in place (no copy of the product's output); any other ``out`` is
    a view of the same shape and dtype that does not overlap ``x``.  ``with_stats``: also the f32 ``[rows, groups * H, 2]``
    statistics ``(rstd, -mean * rstd)`` for :func:`head_norm_backward`."""
    _dev(x, weight, out)
    rows, width, d, w = _head_norm_args("head_norm", x, weight, num_heads, groups)
    if out is None:
        out = torch.empty((rows, width), dtype=x.dtype, device=x.device)
    elif tuple(_rows(out).shape) != (rows, width) or out.dtype != x.dtype:
        raise ValueError("head_norm: out must have x's shape and dtype")
    stats = torch.empty((rows, groups * num_heads, 2), dtype=torch.float32, device=x.device) if with_stats else None
    if rows > 0:
        with _Timed("head_norm", bytes=2 * rows * width * x.element_size()):
            st = _lib.load().anemoi_head_norm(dtype_code(x.dtype), x.data_ptr(), _ld(x), w.data_ptr(), out.data_ptr(), _ld(out),
                                              _ptr(stats), rows, groups, num_heads, d, eps, _stream())
        _lib.check(st, "anemoi_head_norm")
    return (out, stats) if with_stats else out


def head_norm_backward(dy: Tensor, x: Tensor, stats: Tensor, weight: Tensor, num_heads: int, groups: int = 1,
                       out: Optional[Tensor] = None):
    """``(dx, dweight [groups, D] f32)`` of :func:`head_norm` from the pre-norm ``x`` and the forward's statistics (``dy``, ``x``
    and the optional ``out`` for ``dx`` are ``[rows, groups * H * D]`` views).  Deterministic: fixed row chunks, partials added
    in ascending order; a zero weight is legal (nothing divides by it)."""
    _dev(dy, x, stats, weight, out)
    rows, width, d, w = _head_norm_args("head_norm_backward", x, weight, num_heads, groups)
    if (tuple(_rows(dy).shape) != (rows, width) or dy.dtype != x.dtype
            or tuple(stats.shape) != (rows, groups * num_heads, 2) or stats.dtype != torch.float32 or not stats.is_contiguous()):
        raise ValueError("head_norm_backward: shapes of x, dy, stats do not match")
    if out is None:
        out = torch.empty((rows, width), dtype=x.dtype, device=x.device)
    elif tuple(_rows(out).shape) != (rows, width) or out.dtype != x.dtype:
        raise ValueError("head_norm_backward: out must have x's shape and dtype")
    dw = torch.empty((groups, d), dtype=torch.float32, device=x.device)
    if rows == 0:
        return out, dw.zero_()
    lib = _lib.load()
    n_ws = lib.anemoi_head_norm_backward_workspace_floats(rows, groups, num_heads, d)
    ws = torch.empty(max(n_ws, 1), dtype=torch.float32, device=x.device)
    with _Timed("head_norm_backward", bytes=5 * rows * width * x.element_size()):
        st = lib.anemoi_head_norm_backward(dtype_code(x.dtype), dy.data_ptr(), _ld(dy), x.data_ptr(), _ld(x), stats.data_ptr(),
                                           w.data_ptr(), out.data_ptr(), _ld(out), dw.data_ptr(), rows, groups, num_heads, d,
                                           ws.data_ptr(), n_ws, _stream())
    _lib.check(st, "anemoi_head_norm_backward")
    return out, dw


def weight_grad(dpre: Tensor, x: Tensor, k: int, want_bias: bool = False, transposed_route: bool = False,
                out: Optional[Tensor] = None):
    """``dW [N, k] = dpre^T @ x[:, :k]`` in f32 (``dpre [M, N]``, ``x [M, >= k]`` in the compute dtype): the reduction
    over the M rows is cut into chunks -- chunked transposes, one batched GEMM on the 128 x 128 kernel, a deterministic
    sum of the partial results -- so that a small ``[N, k]`` result still fills the chip (a 1024 x 192 gradient over
    542 080 rows took 7 ms on 16 workgroups without the split).  ``want_bias``: returns ``(dW, db)`` with
    ``db = dpre.sum(0)`` (f32); for bf16 the column sums come out of the transpose of ``dpre`` (per-tile partials), not
    out of a second pass over it.  ``transposed_route=True`` (tests, tools/dw_bench.py) takes the transposes + NT route even
    where the TN kernel applies (bf16, 16-byte aligned operands, M >= 128), which otherwise runs.  ``out`` (optional, f32
    ``[N * k (+ N)]`` contiguous): where the TN route leaves ``dW`` (and ``db`` behind it) -- the results are then views of
    it (a caller's stacked gradient buffer, autograd.GradSink); ignored by the other route."""
    _dev(dpre, x)
    m, n = _rows(dpre).shape
    kmul = k_multiple(dpre.dtype)
    # bf16: partial results in bf16 from the persistent 256 x 256 kernel (f32 accumulation inside, as an autocast matmul
    # rounds them), summed in f32; f32: the exact 128 x 128 kernel
    fast = dpre.dtype == torch.bfloat16 and k % 8 == 0
    xr = _rows(x)
    if (fast and n % 8 == 0 and _ld(dpre) % 8 == 0 and _ld(xr) % 8 == 0 and dpre.data_ptr() % 16 == 0
            and xr.data_ptr() % 16 == 0 and m >= 128 and not transposed_route):
        # no transposed copies: the TN kernel reads dpre and x as they lie (ds_read_b64_tr_b16 fragments), f32 partials
        tiles = ((n + 255) // 256) * ((k + 255) // 256)
        chunks = max(1, min(256 // tiles if tiles <= 256 else 1, m // 2048))
        ld_max = max(_ld(dpre), _ld(xr))
        row_cap = ((1 << 31) - 1) // (2 * ld_max) // 64 * 64  # descriptor range of one chunk
        chunk_rows = max(128, min(round_up((m + chunks - 1) // chunks, 64), row_cap))
        chunks = (m + chunk_rows - 1) // chunk_rows
        # one buffer [chunks, n * k (+ n)]: the weight partials and, behind them, the bias partials of a chunk -- ONE column
        # sum over the chunks finishes both
        width = n * k + (n if want_bias else 0)
        if out is not None and (out.dtype != torch.float32 or out.numel() != width or not out.is_contiguous()):
            raise ValueError(f"weight_grad: out must be a contiguous f32 vector of {width} elements")
        if out is not None and chunks == 1:
            part = out.view(1, width)
        else:
            part = torch.empty((chunks, width), dtype=torch.float32, device=dpre.device)
        st = _lib.load().anemoi_weight_grad_tn(dpre.data_ptr(), _ld(dpre), xr.data_ptr(), _ld(xr), part.data_ptr(), width,
                                               part[:, n * k:].data_ptr() if want_bias else None, width, m, n, k, chunk_rows,
                                               _stream())
        _lib.check(st, "anemoi_weight_grad_tn")
        total = part[0] if chunks == 1 else col_sum(part, out=None if out is None else out.view(width))
        dw = total[: n * k].view(n, k)
        return (dw, total[n * k:]) if want_bias else dw
    tile = 256 if fast else 128
    tiles = ((n + tile - 1) // tile) * ((k + tile - 1) // tile)
    chunks = max(1, min(256 // tiles if tiles <= 256 else 1, m // 2048))
    chunk_rows = round_up((m + chunks - 1) // chunks, max(kmul, 128 if fast else kmul))
    chunks = (m + chunk_rows - 1) // chunk_rows
    lib = _lib.load()
    code = dtype_code(dpre.dtype)
    at = torch.empty((chunks, n, chunk_rows), dtype=dpre.dtype, device=dpre.device)
    bt = torch.empty((chunks, k, chunk_rows), dtype=dpre.dtype, device=dpre.device)
    partial = None
    if want_bias and fast and n % 4 == 0:
        partial = torch.empty((lib.anemoi_transpose_colsum_rows(m, chunk_rows), n), dtype=torch.float32, device=dpre.device)
    st = lib.anemoi_transpose_chunked(code, dpre.data_ptr(), _ld(dpre), at.data_ptr(), chunk_rows, m, n, chunk_rows,
                                      _ptr(partial), _stream())
    _lib.check(st, "anemoi_transpose_chunked")
    st = lib.anemoi_transpose_chunked(code, x.data_ptr(), _ld(_rows(x)), bt.data_ptr(), chunk_rows, m, k, chunk_rows, None,
                                      _stream())
    _lib.check(st, "anemoi_transpose_chunked")
    part = torch.empty((chunks, n, k), dtype=dpre.dtype if fast else torch.float32, device=dpre.device)
    st = lib.anemoi_linear_batched(code, dtype_code(part.dtype), at.data_ptr(), chunk_rows, n * chunk_rows, bt.data_ptr(),
                                   k * chunk_rows, part.data_ptr(), k, n * k, chunks, n, k, chunk_rows, _stream())
    _lib.check(st, "anemoi_linear_batched")
    if part.dtype != torch.float32 and chunks == 1:
        dw = part[0].float()
    elif chunks == 1:
        dw = part[0]
    else:
        dw = col_sum(part.view(chunks, n * k)).view(n, k)
    if not want_bias:
        return dw
    return dw, (col_sum(partial) if partial is not None else col_sum(dpre))


SPLIT_GRAD_WORKGROUPS = 512  # two 64 KiB-LDS workgroups per CU x 256 CUs: the chunk count fills them once


def weight_grad_split_chunks(m: int, n: int, k: int):
    """``(chunks, chunk_rows)`` of :func:`weight_grad_split`: the M reduction is cut so that chunks x 128 x 128 tiles fill the
    chip, in chunks of at least 1024 rows (a multiple of the kernel's 32-row slab)."""
    tiles = ((n + 127) // 128) * ((k + 127) // 128)
    chunks = max(1, min(SPLIT_GRAD_WORKGROUPS // tiles if tiles <= SPLIT_GRAD_WORKGROUPS else 1, m // 1024))
    chunk_rows = max(32, round_up((m + chunks - 1) // chunks, 32))
    return max(1, (m + chunk_rows - 1) // chunk_rows), chunk_rows


def weight_grad_split(dpre: Tensor, x: Tensor, k: int, want_bias: bool = False, out: Optional[Tensor] = None):
    """``dW [N, k] = dpre^T @ x[:, :k]`` for f32 ``dpre [M, N]`` / ``x [M, >= k]`` with the split-bf16 product
    ``dpre_hi^T x_hi + (dpre_hi^T x_lo + dpre_lo^T x_hi)`` on the bf16 MFMA (``anemoi_weight_grad_split``; both operands are
    split inside the kernel and read as they lie).  Returns and ``out`` as the TN route of :func:`weight_grad`:
    ``want_bias`` gives ``(dW, db)`` with ``db = dpre.sum(0)`` in exact f32 (``col_sum``); ``out`` (optional, f32
    ``[N * k (+ N)]`` contiguous) receives ``dW`` and ``db`` behind it, the results are then views of it
    (``autograd.GradSink``).  N and k multiples of 4, 16-byte aligned operands with row pitches that are multiples of 4,
    else ``ValueError``.  ``M = 0`` gives zeros without a launch."""
    _dev(dpre, x, out)
    m, n = _rows(dpre).shape
    xr = _rows(x)
    if dpre.dtype != torch.float32 or xr.dtype != torch.float32:
        raise ValueError("weight_grad_split: both operands must be f32")
    if xr.shape[0] != m or xr.shape[1] < k or k <= 0 or n <= 0:
        raise ValueError(f"weight_grad_split: dpre {tuple(dpre.shape)} and x {tuple(x.shape)} do not give a [{n}, {k}] gradient")
    if n % 4 != 0 or k % 4 != 0:
        raise ValueError(f"weight_grad_split: N={n} and K={k} must be multiples of 4")
    width = n * k + (n if want_bias else 0)
    if out is not None and (out.dtype != torch.float32 or out.numel() != width or not out.is_contiguous()):
        raise ValueError(f"weight_grad_split: out must be a contiguous f32 vector of {width} elements")
    total = torch.empty(width, dtype=torch.float32, device=dpre.device) if out is None else out.view(width)
    lib = _lib.load()
    if m == 0:
        st = lib.anemoi_weight_grad_split(None, max(_ld(dpre), n), None, max(_ld(xr), k), total.data_ptr(), n * k, 0, n, k, 32,
                                          _stream())
        _lib.check(st, "anemoi_weight_grad_split")
        if want_bias:
            total[n * k:].zero_()
    else:
        chunks, chunk_rows = weight_grad_split_chunks(m, n, k)
        part = total[: n * k].view(1, n * k) if chunks == 1 else torch.empty((chunks, n * k), dtype=torch.float32,
                                                                             device=dpre.device)
        with _Timed("weight_grad_split", flops=2 * m * n * k, bytes=(m * (n + k) + chunks * n * k) * 4, m=m, n=n, k=k):
            st = lib.anemoi_weight_grad_split(dpre.data_ptr(), _ld(dpre), xr.data_ptr(), _ld(xr), part.data_ptr(), n * k, m, n,
                                              k, chunk_rows, _stream())
        _lib.check(st, "anemoi_weight_grad_split")
        if chunks > 1:
            col_sum(part, out=total[: n * k])
        if want_bias:
            col_sum(dpre, out=total[n * k:])
    dw = total[: n * k].view(n, k)
    return (dw, total[n * k:]) if want_bias else dw


# ---------------------------------------------------------------- the optimizer step (csrc/optim.hip, DESIGN.md section 7 "8f-10")
def multi_tensor_chunks(numels) -> int:
    """(tensor, chunk) pairs of a list of lengths: the workspace floats of :func:`multi_sumsq` (empty tensors have none)."""
    return sum((int(n) + _lib.OPT_CHUNK - 1) // _lib.OPT_CHUNK for n in numels)


def ptr_array(tensors):
    """The host array of device pointers the multi-tensor entry points take (a ``ctypes`` array; it may be kept and reused
    for as long as the tensors stay where they are)."""
    import ctypes

    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def numel_array(tensors):
    import ctypes

    return (ctypes.c_int64 * len(tensors))(*[t.numel() for t in tensors])


def _check_list(who: str, what: str, tensors, like=None) -> None:
    for i, t in enumerate(tensors):
        if not t.is_cuda:
            _dev(t)
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise NotImplementedError(f"{who}: {what}[{i}] must be a contiguous float32 tensor, got {t.dtype} "
                                      f"strides {t.stride()}")
        if like is not None and t.numel() != like[i].numel():
            raise ValueError(f"{who}: {what}[{i}] has {t.numel()} elements, the parameter {like[i].numel()}")


def _multi_args(n: int, numel, **fields):
    import ctypes

    a = _lib.MultiTensorArgs()
    a.struct_bytes, a.n_tensors = ctypes.sizeof(_lib.MultiTensorArgs), n
    a.numel = ctypes.cast(numel, ctypes.c_void_p)
    a._keep = [numel, *fields.values()]  # the host arrays live as long as the block
    for name, value in fields.items():
        setattr(a, name, ctypes.cast(value, ctypes.c_void_p) if isinstance(value, ctypes.Array) else value)
    return a


def multi_sumsq(grads, out: Optional[Tensor] = None, workspace: Optional[Tensor] = None) -> Tensor:
    """``sum over the list of g^2`` as an f32 device scalar: deterministic two-stage reduction without atomics, a function of
    the values and the ordered list of lengths alone (``anemoi_multi_sumsq``).  ``grads``: contiguous f32 tensors of any
    length and 4-byte alignment.  ``out`` (f32 ``[]`` or ``[1]``) and ``workspace`` (f32, at least
    :func:`multi_tensor_chunks` floats) are allocated when not given."""
    import ctypes

    grads = list(grads)
    _check_list("multi_sumsq", "grads", grads)
    if out is None:
        if not grads:
            raise ValueError("multi_sumsq: an empty list needs `out` (there is no device to allocate on)")
        out = torch.empty((), dtype=torch.float32, device=grads[0].device)
    n_ws = multi_tensor_chunks(t.numel() for t in grads)
    if workspace is None or workspace.numel() < n_ws:
        workspace = torch.empty(max(n_ws, 1), dtype=torch.float32, device=out.device)
    a = _multi_args(len(grads), numel_array(grads), grads=ptr_array(grads), workspace=workspace.data_ptr(),
                    workspace_floats=workspace.numel(), sumsq=out.data_ptr())
    with _Timed("multi_sumsq", bytes=4 * sum(t.numel() for t in grads)):
        st = _lib.load().anemoi_multi_sumsq(ctypes.byref(a), _stream())
    _lib.check(st, "anemoi_multi_sumsq")
    return out


def adamw_constants(consts: Tensor, steps=(), lrs=(), betas=(), weight_decays=(), *, sumsq: Optional[Tensor] = None,
                    max_norm: Optional[float] = None, skip_nonfinite: bool = False,
                    skipped: Optional[Tensor] = None) -> Tensor:
    """The scalars of one AdamW step (``anemoi_adamw_constants``), written to ``consts`` (f32 ``[1 + n_groups, 8]``: block 0 =
    norm, clip, finite, skip; block 1 + g = clip, 1 - lr wd, lr / bc1, sqrt(bc2), skip, lr, t) by one tiny kernel.  ``steps``:
    one f32 device counter per group, advanced in place; ``lrs``: floats or 0-dim f32 device tensors (read on the device);
    ``betas``: ``(beta1, beta2)`` per group.  No group: block 0 alone."""
    import ctypes

    n = len(steps)
    if not (len(lrs) == len(betas) == len(weight_decays) == n):
        raise ValueError("adamw_constants: steps, lrs, betas and weight_decays must have one entry per group")
    _dev(consts, sumsq, skipped, *steps)
    if consts.dtype != torch.float32 or not consts.is_contiguous() or consts.numel() < (1 + n) * _lib.OPT_CONSTS:
        raise ValueError(f"adamw_constants: consts must be contiguous float32 with {(1 + n) * _lib.OPT_CONSTS} elements")
    for i, lr in enumerate(lrs):
        if isinstance(lr, Tensor) and (not lr.is_cuda or lr.dtype != torch.float32 or lr.numel() != 1):
            raise ValueError(f"adamw_constants: lrs[{i}] must be a float or a one-element float32 device tensor")
    fa = ctypes.c_double * max(n, 1)
    c = _lib.AdamwConstantsArgs()
    c.struct_bytes, c.n_groups = ctypes.sizeof(_lib.AdamwConstantsArgs), n
    step_a, lr_dev_a = ptr_array(steps), (ctypes.c_void_p * max(n, 1))(*[lr.data_ptr() if isinstance(lr, Tensor) else None
                                                                        for lr in lrs])
    lr_a = fa(*[0.0 if isinstance(lr, Tensor) else float(lr) for lr in lrs])
    b1_a, b2_a = fa(*[float(b[0]) for b in betas]), fa(*[float(b[1]) for b in betas])
    wd_a = fa(*[float(w) for w in weight_decays])
    for name, arr in (("step", step_a), ("lr_dev", lr_dev_a), ("lr", lr_a), ("beta1", b1_a), ("beta2", b2_a),
                      ("weight_decay", wd_a)):
        setattr(c, name, ctypes.cast(arr, ctypes.c_void_p))
    c.sumsq, c.skipped, c.consts = _ptr(sumsq), _ptr(skipped), consts.data_ptr()
    c.max_norm, c.has_max_norm, c.skip_nonfinite = float(max_norm or 0.0), int(max_norm is not None), int(skip_nonfinite)
    st = _lib.load().anemoi_adamw_constants(ctypes.byref(c), _stream())
    _lib.check(st, "anemoi_adamw_constants")
    return consts


def multi_adamw(params, grads, exp_avg, exp_avg_sq, consts_block: Tensor, beta1: float, beta2: float, eps: float) -> None:
    """One AdamW update of the list in one pass (``anemoi_multi_adamw``): ``g' = clip g`` on load (``grads`` are not
    modified), ``m``, ``v`` and ``p`` updated in place with torch.optim.AdamW's arithmetic in correctly rounded f32.
    ``consts_block``: the group's 8 floats of :func:`adamw_constants`."""
    import ctypes

    params, grads, exp_avg, exp_avg_sq = list(params), list(grads), list(exp_avg), list(exp_avg_sq)
    if not (len(params) == len(grads) == len(exp_avg) == len(exp_avg_sq)):
        raise ValueError("multi_adamw: the four lists must have one tensor per parameter")
    _check_list("multi_adamw", "params", params)
    _check_list("multi_adamw", "grads", grads, params)
    _check_list("multi_adamw", "exp_avg", exp_avg, params)
    _check_list("multi_adamw", "exp_avg_sq", exp_avg_sq, params)
    _dev(consts_block)
    a = _multi_args(len(params), numel_array(params), params=ptr_array(params), grads=ptr_array(grads),
                    exp_avg=ptr_array(exp_avg), exp_avg_sq=ptr_array(exp_avg_sq),
                    consts=consts_block.data_ptr(), beta1=float(beta1), beta2=float(beta2), eps=float(eps))
    with _Timed("multi_adamw", bytes=28 * sum(t.numel() for t in params)):
        st = _lib.load().anemoi_multi_adamw(ctypes.byref(a), _stream())
    _lib.check(st, "anemoi_multi_adamw")


def multi_scale(grads, coef: Tensor) -> None:
    """``g <- coef * g`` in place over the list, ``coef`` a one-element f32 device tensor (``anemoi_multi_scale``)."""
    import ctypes

    grads = list(grads)
    _check_list("multi_scale", "grads", grads)
    _dev(coef)
    if coef.dtype != torch.float32 or coef.numel() != 1:
        raise ValueError("multi_scale: coef must be a one-element float32 device tensor")
    a = _multi_args(len(grads), numel_array(grads), grads=ptr_array(grads), coef=coef.data_ptr())
    with _Timed("multi_scale", bytes=8 * sum(t.numel() for t in grads)):
        st = _lib.load().anemoi_multi_scale(ctypes.byref(a), _stream())
    _lib.check(st, "anemoi_multi_scale")


# ---------------------------------------------------------------- weight averaging, device LR schedule (csrc/average.hip, DESIGN.md "8f-11")
def _scalar_f32(who: str, name: str, t: Optional[Tensor], numel: int = 1) -> None:
    if t is None:
        return
    _dev(t)
    if t.dtype != torch.float32 or t.numel() != numel or not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be a contiguous float32 device tensor of {numel} element(s)")


def average_constants(avg: Tensor, n_averaged: Tensor, *, kind: str = "ema", decay: float = 0.999, warmup: bool = False,
                      start_step: int = 0, every: int = 1, step: Optional[Tensor] = None,
                      skip: Optional[Tensor] = None) -> Tensor:
    """The scalars of one averaging update (``anemoi_average_constants``), written to ``avg`` (f32 ``[4]``: w, active, copy,
    n_after) by one tiny kernel.  ``n_averaged``: the f32 device counter, advanced in place when the update is active;
    ``step``: the optimizer's f32 device step counter (steps completed) that ``start_step`` / ``every`` gate on, or ``None``
    (every call counts); ``skip``: the optimizer's one-element skip flag, or ``None``."""
    import ctypes

    if kind not in ("ema", "swa"):
        raise ValueError(f"average_constants: kind must be 'ema' or 'swa', got {kind!r}")
    _scalar_f32("average_constants", "avg", avg, _lib.AVG_CONSTS)
    _scalar_f32("average_constants", "n_averaged", n_averaged)
    _scalar_f32("average_constants", "step", step)
    _scalar_f32("average_constants", "skip", skip)
    c = _lib.AverageConstantsArgs()
    c.struct_bytes = ctypes.sizeof(_lib.AverageConstantsArgs)
    c.n_averaged, c.step, c.skip, c.avg = n_averaged.data_ptr(), _ptr(step), _ptr(skip), avg.data_ptr()
    c.decay, c.start_step, c.every = float(decay), int(start_step), int(every)
    c.kind, c.use_warmup = _lib.AVERAGE_EMA if kind == "ema" else _lib.AVERAGE_SWA, int(bool(warmup))
    st = _lib.load().anemoi_average_constants(ctypes.byref(c), _stream())
    _lib.check(st, "anemoi_average_constants")
    return avg


def multi_average(params, shadow, avg: Tensor) -> None:
    """One averaging update of the list in one pass (``anemoi_multi_average``): under the block ``avg`` of
    :func:`average_constants`, ``shadow`` is left alone (inactive), becomes a bit copy of ``params`` (the first update) or
    ``s <- fmaf(p - s, w, s)``.  ``params`` are only read."""
    import ctypes

    params, shadow = list(params), list(shadow)
    if len(params) != len(shadow):
        raise ValueError("multi_average: the two lists must have one tensor per parameter")
    _check_list("multi_average", "params", params)
    _check_list("multi_average", "shadow", shadow, params)
    _scalar_f32("multi_average", "avg", avg, _lib.AVG_CONSTS)
    a = _lib.MultiAverageArgs()
    a.struct_bytes, a.n_tensors = ctypes.sizeof(_lib.MultiAverageArgs), len(params)
    keep = (numel_array(params), ptr_array(params), ptr_array(shadow))
    a.numel, a.params, a.shadow = (ctypes.cast(k, ctypes.c_void_p) for k in keep)
    a.avg = avg.data_ptr()
    with _Timed("multi_average", bytes=12 * sum(t.numel() for t in params)):
        st = _lib.load().anemoi_multi_average(ctypes.byref(a), _stream())
    _lib.check(st, "anemoi_multi_average")


def multi_swap(a_list, b_list) -> None:
    """``a[i] <-> b[i]`` over the two lists, exactly (``anemoi_multi_swap``).  The lists must not overlap."""
    import ctypes

    a_list, b_list = list(a_list), list(b_list)
    if len(a_list) != len(b_list):
        raise ValueError("multi_swap: the two lists must have one tensor per parameter")
    _check_list("multi_swap", "a", a_list)
    _check_list("multi_swap", "b", b_list, a_list)
    a = _lib.MultiSwapArgs()
    a.struct_bytes, a.n_tensors = ctypes.sizeof(_lib.MultiSwapArgs), len(a_list)
    keep = (numel_array(a_list), ptr_array(a_list), ptr_array(b_list))
    a.numel, a.a, a.b = (ctypes.cast(k, ctypes.c_void_p) for k in keep)
    with _Timed("multi_swap", bytes=16 * sum(t.numel() for t in a_list)):
        st = _lib.load().anemoi_multi_swap(ctypes.byref(a), _stream())
    _lib.check(st, "anemoi_multi_swap")


def lr_schedule(lrs, steps, bases, *, warmup_steps, total_steps, lr_min, warmup_start, warmup_prefix) -> None:
    """Linear warm-up and cosine decay evaluated on the device (``anemoi_lr_schedule``): ``lrs[g]`` (one-element f32 device
    tensors) is written from ``steps[g]`` (the group's f32 device step counter, steps completed).  Every other argument is a
    list with one entry per group; at most ``_lib.LR_MAX_GROUPS`` groups."""
    import ctypes

    lrs, steps = list(lrs), list(steps)
    n = len(lrs)
    per_group = (steps, bases, warmup_steps, total_steps, lr_min, warmup_start, warmup_prefix)
    if any(len(v) != n for v in per_group):
        raise ValueError("lr_schedule: every argument must have one entry per group")
    for i in range(n):
        _scalar_f32("lr_schedule", f"lrs[{i}]", lrs[i])
        _scalar_f32("lr_schedule", f"steps[{i}]", steps[i])
    fa, ia, ba = ctypes.c_double * max(n, 1), ctypes.c_int64 * max(n, 1), ctypes.c_int32 * max(n, 1)
    s = _lib.LrScheduleArgs()
    s.struct_bytes, s.n_groups = ctypes.sizeof(_lib.LrScheduleArgs), n
    keep = dict(step=ptr_array(steps), lr=ptr_array(lrs), base=fa(*[float(v) for v in bases]),
                lr_min=fa(*[float(v) for v in lr_min]), warmup_start=fa(*[float(v) for v in warmup_start]),
                warmup_steps=ia(*[int(v) for v in warmup_steps]), total_steps=ia(*[int(v) for v in total_steps]),
                warmup_prefix=ba(*[int(bool(v)) for v in warmup_prefix]))
    for name, arr in keep.items():
        setattr(s, name, ctypes.cast(arr, ctypes.c_void_p))
    st = _lib.load().anemoi_lr_schedule(ctypes.byref(s), _stream())
    _lib.check(st, "anemoi_lr_schedule")
