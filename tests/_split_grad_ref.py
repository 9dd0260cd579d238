"""Split-bf16 ("bf16x3") weight gradient restated in CPU torch from its definition (include/anemoi_amd.h,
``anemoi_weight_grad_split``): the yardstick of tests/test_split_grad_cpu.py and tests/test_gpu_split_grad.py, not a copy of
the kernel.

Both operands are split (``hi = bf16(v)``, ``lo = bf16(v - hi)``, round to nearest even: ``_split_ref.split``) and
``dY^T x ~= dY_hi^T x_hi + (dY_hi^T x_lo + dY_lo^T x_hi)``; a product of two bf16 values is exact in f32, the sums are f32."""

from _split_ref import split


def weight_grad_bf16x3(dy, x):
    """``dW [N, K]`` of ``dy [M, N]``, ``x [M, K]`` (f32 CPU tensors)."""
    yh, yl = split(dy)
    xh, xl = split(x)
    return yh.T @ xh + (yh.T @ xl + yl.T @ xh)
