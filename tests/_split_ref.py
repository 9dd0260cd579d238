"""Split-bf16 ("bf16x3") arithmetic restated in CPU torch from its definition (include/anemoi_amd.h, "Split-bf16"): the
yardstick of tests/test_split_cpu.py and tests/test_gpu_split*.py, not a copy of the kernel.

``hi = bf16(v)``, ``lo = bf16(v - hi)`` (round to nearest even, what ``Tensor.to(torch.bfloat16)`` does), and
``x w^T ~= x_hi w_hi^T + (x_hi w_lo^T + x_lo w_hi^T)`` with the products exact in f32 and f32 accumulation."""

import torch
import torch.nn.functional as F


def split(t):
    """``(hi, lo)`` as f32 tensors holding bf16 values."""
    t = t.float()
    hi = t.to(torch.bfloat16).float()
    lo = (t - hi).to(torch.bfloat16).float()
    return hi, lo


def linear_bf16x3(x, w, bias=None):
    xh, xl = split(x)
    wh, wl = split(w)
    y = xh @ wh.T + (xh @ wl.T + xl @ wh.T)
    return y if bias is None else y + bias.float()


class Bf16x3Linears(torch.overrides.TorchFunctionMode):
    """Every ``F.linear`` under this mode runs as :func:`linear_bf16x3` (the CPU oracle on split-bf16 Linears)."""

    def __torch_function__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        if func is F.linear:
            x, w = args[0], args[1]
            b = args[2] if len(args) > 2 else kwargs.get("bias")
            y = linear_bf16x3(x.reshape(-1, x.shape[-1]), w, b)
            return y.reshape(*x.shape[:-1], w.shape[0])
        return func(*args, **kwargs)
