"""Torch restatement of the MXFP8 format of include/anemoi_amd.h ("MXFP8"), on the CPU.

OCP MX v1.0 with e4m3fn elements: one E8M0 scale per 32 consecutive K-elements of a row, ``e = floor(log2(amax)) - 8``
clamped to [-127, 127] and stored as ``e + 127``; elements ``v 2^-e`` rounded to nearest-even, saturated at +-448; an
all-zero block has scale byte 0; K is zero padded to a multiple of 128.
"""

import torch


def round_up(n, m):
    return (n + m - 1) // m * m


def block_exponent(amax):
    """e per block (int32 tensor) from the f32 block maxima: floor(log2(amax)) - 8 clamped; amax = 0 gives -127."""
    mant, ex = torch.frexp(amax.double())  # amax = mant 2^ex, mant in [0.5, 1): floor(log2 amax) = ex - 1
    e = (ex.to(torch.int32) - 1 - 8).clamp(-127, 127)
    return torch.where(amax == 0, torch.full_like(e, -127), e)


def quantize(x, kp=None):
    """MXFP8 of the rows of ``x`` ([M, K], any float dtype, taken as f32): (q uint8 [M, Kp], scales uint8 [M, Kp/32])."""
    x = x.detach().float().cpu()
    m, k = x.shape
    kp = round_up(k, 128) if kp is None else kp
    xp = torch.zeros((m, kp), dtype=torch.float32)
    xp[:, :k] = x
    blocks = xp.view(m, kp // 32, 32)
    e = block_exponent(blocks.abs().amax(-1))
    scaled = torch.ldexp(blocks, (-e).unsqueeze(-1).float())
    q = scaled.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8).view(m, kp)
    return q, (e + 127).to(torch.uint8)


def dequantize(q, scales, k=None):
    """f32 values of MXFP8 rows (``k``: the logical width to keep)."""
    q, scales = q.cpu(), scales.cpu()
    m, kp = q.shape
    v = q.view(torch.float8_e4m3fn).float().view(m, kp // 32, 32)
    v = torch.ldexp(v, (scales.to(torch.int32) - 127).unsqueeze(-1).float()).view(m, kp)
    return v if k is None else v[:, :k]


def e4m3_value(code):
    """f32 value of one e4m3fn byte."""
    return float(torch.tensor([code], dtype=torch.uint8).view(torch.float8_e4m3fn).float())
