"""``ops.weight_grad_split`` (csrc/weight_grad_split.hip) on the MI355X (``-m gpu``): integer operands where the f64 product
is the only right answer, random operands against the CPU restatement of the arithmetic (tests/_split_grad_ref.py) on the
same data, bias gradient / strided operands / ``out`` buffers, and the contract at the edges."""

import functools

import pytest
import torch

from _split_grad_ref import weight_grad_bf16x3

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


def _ints(shape, bound, g):
    return torch.randint(-bound, bound + 1, shape, generator=g).float()


@pytest.mark.parametrize("m", [1, 63, 65, 4133])
@pytest.mark.parametrize("case", ["dy_needs_lo", "x_needs_lo", "both_bf16_exact"])
def test_integer_operands_give_the_exact_product(case, m):
    """|sums| <= 4133 * 300 * 3 < 2^24: every partial sum is exact in f32 in any order and over any chunking.  300 needs 9
    significand bits, so its ``lo`` is not zero: ``dy_needs_lo`` fails without ``dY_lo^T x_hi``, ``x_needs_lo`` without
    ``dY_hi^T x_lo``.  ``both_bf16_exact`` plants one 2^15 per operand, in different rows (2^15 * 120 + 4133 * 360 < 2^24).
    M = 4133 is cut into several chunks (asserted), the others are one ragged slab, 2 slabs - 1 row, 2 slabs + 1 row."""
    from anemoi_models_amd import ops

    g = torch.Generator().manual_seed(11 + m)
    n, k = 80, 96
    by, bx = {"dy_needs_lo": (300, 3), "x_needs_lo": (3, 300), "both_bf16_exact": (120, 3)}[case]
    dy, x = _ints((m, n), by, g), _ints((m, k), bx, g)
    if case != "both_bf16_exact" and m > 1:
        big = dy if case == "dy_needs_lo" else x
        assert not torch.equal(big.to(torch.bfloat16).float(), big)
    if case == "both_bf16_exact":
        dy[m // 2, 7] = 2.0 ** 15
        if m // 3 != m // 2:  # (never both in one row: their product alone would be 2^30)
            x[m // 3, 5] = -(2.0 ** 15)
    want = (dy.double().T @ x.double()).float()
    assert float(want.abs().max()) < 2 ** 24
    if m == 4133:
        assert ops.weight_grad_split_chunks(m, n, k)[0] > 1
    got = ops.weight_grad_split(dy.to(DEV), x.to(DEV), k)
    assert torch.equal(got.cpu(), want)


# (M, N, K): one ragged slab / odd tiles on both sides / N beyond one tile row, K = two tiles / several chunks, 8 x 8 tiles /
# the grid-sized reductions of the mappers: a narrow and a wide gradient
_SHAPES = [(1, 80, 32), (63, 144, 192), (129, 2240, 256), (4133, 1024, 1024), (40962, 80, 256), (40962, 1024, 192)]


@functools.lru_cache(maxsize=None)
def _case(m, n, k):
    """Operands and the three CPU results of one shape, computed once and shared by the tests below (read only)."""
    g = torch.Generator().manual_seed(m * 31 + n * 7 + k)
    dy = torch.randn(m, n, generator=g)
    x = torch.randn(m, k, generator=g)
    want = dy.double().T @ x.double()
    scale = want.abs().max()
    e_ref = float((weight_grad_bf16x3(dy, x).double() - want).abs().max() / scale)
    return dy, x, want, scale, e_ref, dy.double().sum(0), dy.double().abs().sum(0)


@pytest.mark.parametrize("m,n,k", _SHAPES)
def test_random_operands_against_the_cpu_restatement(m, n, k):
    """Error against the f64 product, normalised by max |ref|, at most 2 x the error of ``weight_grad_bf16x3`` on the same
    operands: kernel and restatement differ in f32 accumulation order only; a dropped correction product lands >= 100 x
    above."""
    from anemoi_models_amd import ops

    dy, x, want, scale, e_ref, _, _ = _case(m, n, k)
    got = ops.weight_grad_split(dy.to(DEV), x.to(DEV), k)
    e_got = float((got.cpu().double() - want).abs().max() / scale)
    print(f"M={m} N={n} K={k}: split kernel {e_got:.3e}, CPU restatement {e_ref:.3e}")
    assert got.shape == (n, k) and got.dtype == torch.float32
    assert e_got <= 2 * e_ref


@pytest.mark.parametrize("m,n,k", _SHAPES)
def test_bias_strided_operands_and_out_buffer(m, n, k):
    """The same shapes with the bias gradient, operands that are views of wider and longer buffers whose padding columns
    and rows behind M hold NaN, and an ``out`` slice with sentinels on both sides.  ``db`` is an exact-f32 column sum: any
    summation order of M f32 terms stays within (M - 1) * 2^-24 * sum |dy| of the true sum."""
    from anemoi_models_amd import ops

    dy, x, want, scale, e_ref, db_want, db_abs = _case(m, n, k)
    yb = torch.full((m + 37, n + 4), NAN, device=DEV)
    xb = torch.full((m + 37, k + 12), NAN, device=DEV)
    yb[:m, :n], xb[:m, :k] = dy.to(DEV), x.to(DEV)
    width = n * k + n
    buf = torch.full((width + 24,), -7.0, device=DEV)
    out = buf[8:8 + width]
    dw, db = ops.weight_grad_split(yb[:m, :n], xb[:m, :k + 4], k, want_bias=True, out=out)  # x may be wider than k
    assert dw.data_ptr() == out.data_ptr() and db.data_ptr() == out[n * k:].data_ptr()
    assert bool((buf[:8] == -7.0).all()) and bool((buf[8 + width:] == -7.0).all())
    e_got = float((dw.cpu().double() - want).abs().max() / scale)
    print(f"M={m} N={n} K={k} strided + bias: split kernel {e_got:.3e}, CPU restatement {e_ref:.3e}")
    assert e_got <= 2 * e_ref
    assert bool(((db.cpu().double() - db_want).abs() <= max(m - 1, 1) * 2.0 ** -24 * db_abs).all())
    plain = ops.weight_grad_split(dy.to(DEV), x.to(DEV), k)
    assert torch.equal(plain, dw)  # strides, padding and the out route change no bit


def test_run_to_run_bit_identity_and_one_nan():
    from anemoi_models_amd import ops

    g = torch.Generator().manual_seed(5)
    m, n, k = 4133, 144, 192
    dy = torch.randn(m, n, generator=g).to(DEV)
    x = torch.randn(m, k, generator=g).to(DEV)
    a, b = ops.weight_grad_split(dy, x, k), ops.weight_grad_split(dy, x, k)
    assert torch.equal(a, b) and not bool(torch.isnan(a).any())
    x2 = x.clone()
    x2[3000, 77] = NAN
    bad = torch.isnan(ops.weight_grad_split(dy, x2, k))
    assert bool(bad[:, 77].all()) and int(bad.sum()) == n
    dy2 = dy.clone()
    dy2[123, 131] = NAN
    bad = torch.isnan(ops.weight_grad_split(dy2, x, k))
    assert bool(bad[131].all()) and int(bad.sum()) == k


def test_empty_reduction_and_refusals():
    from anemoi_models_amd import ops

    dy = torch.randn(64, 80, device=DEV)
    x = torch.randn(64, 96, device=DEV)
    ops.PROFILE = []
    try:
        out = torch.full((80 * 96 + 80,), 3.0, device=DEV)
        dw, db = ops.weight_grad_split(dy[:0], x[:0], 96, want_bias=True, out=out)
        assert dw.shape == (80, 96) and db.shape == (80,) and ops.PROFILE == []  # no launch
        assert not bool(out.any())
    finally:
        ops.PROFILE = None
    with pytest.raises(ValueError):
        ops.weight_grad_split(dy[:, :78], x, 96)  # N off the multiple of 4
    with pytest.raises(ValueError):
        ops.weight_grad_split(dy, x, 94)  # K off the multiple of 4
    with pytest.raises(ValueError):
        ops.weight_grad_split(dy[:, 1:77], x, 96)  # 4-byte aligned operand
    with pytest.raises(ValueError):
        ops.weight_grad_split(torch.randn(64, 81, device=DEV)[:, :80], x, 96)  # row pitch off the multiple of 4
    with pytest.raises(ValueError):
        ops.weight_grad_split(dy.bfloat16(), x.bfloat16(), 96)
    with pytest.raises(ValueError):
        ops.weight_grad_split(dy, x, 96, out=torch.zeros(80 * 96 + 1, device=DEV))
