"""MXFP8 format (include/anemoi_amd.h, "MXFP8") on hand-made blocks, and the argument checks of anemoi_mx_quantize /
anemoi_linear_mx, without a GPU."""

import pytest
import torch

import _mx_ref as mx


def _row(*blocks):
    """One row of 32-element blocks; each block given as {position: value} (other elements zero)."""
    x = torch.zeros(1, 32 * len(blocks))
    for b, vals in enumerate(blocks):
        for i, v in vals.items():
            x[0, 32 * b + i] = v
    return x


def test_amax_a_power_of_two():
    q, s = mx.quantize(_row({0: 2.0, 5: -1.0, 9: 0.5}))
    assert int(s[0, 0]) == 127 - 7  # floor(log2 2) - 8 = -7
    assert int(q[0, 0]) == 0x78  # 2 * 2^7 = 256 = 1.0 x 2^8
    assert int(q[0, 5]) == 0xF0  # -128 = -(1.0 x 2^7)
    assert int(q[0, 9]) == 0x68  # 64
    assert mx.dequantize(q, s)[0, :10].tolist() == [2.0, 0, 0, 0, 0, -1.0, 0, 0, 0, 0.5]


def test_amax_just_below_one_saturates():
    v = float(torch.tensor(1.0).nextafter(torch.tensor(0.0)))  # 1 - 2^-24
    q, s = mx.quantize(_row({3: v, 4: -v}))
    assert int(s[0, 0]) == 127 - 9  # floor(log2 v) = -1
    assert int(q[0, 3]) == 0x7E and int(q[0, 4]) == 0xFE  # v 2^9 = 511.99997: saturates to +-448, never NaN


def test_scaled_max_in_448_512_saturates():
    q, s = mx.quantize(_row({0: 1.9, 1: 1.74, 2: 1.76}))  # 1.9 * 256 = 486.4; 1.76 * 256 = 450.56; 1.74 * 256 = 445.44
    assert int(s[0, 0]) == 127 - 8
    assert int(q[0, 0]) == 0x7E and int(q[0, 2]) == 0x7E
    assert int(q[0, 1]) == 0x7E  # 445.44 rounds to 448 (nearest of 416 / 448)
    assert mx.e4m3_value(0x7E) == 448.0


def test_all_zero_block():
    q, s = mx.quantize(_row({}, {0: 1.0}))
    assert int(s[0, 0]) == 0 and int(q[0, :32].abs().sum()) == 0
    assert int(s[0, 1]) == 127 - 8 and int(q[0, 32]) == 0x78  # e = -8: 1.0 2^8 = 256
    assert mx.dequantize(q, s)[0, 32] == 1.0


def test_e4m3_subnormals_and_ties():
    # amax 1.0 -> e = -8; 2^-17 -> 2^-9 (smallest subnormal, code 1); 3 2^-18 -> 1.5 2^-9 (tie -> even code 2);
    # 2^-18 -> 0.5 2^-9 (tie -> 0); 7.5 2^-9 2^-8 -> tie between codes 7 and 8 -> 8 (the smallest normal, 2^-6)
    q, s = mx.quantize(_row({0: 1.0, 1: 2.0 ** -17, 2: 3 * 2.0 ** -18, 3: 2.0 ** -18, 4: 7.5 * 2.0 ** -17}))
    assert int(s[0, 0]) == 127 - 8
    assert [int(c) for c in q[0, 1:5]] == [0x01, 0x02, 0x00, 0x08]
    # normal ties: 1.0625 -> 1.0 (even mantissa 0), 1.1875 -> 1.25 (even mantissa 2), scaled by 2^0 (amax 256 -> e = 0)
    q, s = mx.quantize(_row({0: 256.0, 1: 1.0625, 2: 1.1875}))
    assert int(s[0, 0]) == 127
    assert mx.e4m3_value(int(q[0, 1])) == 1.0 and mx.e4m3_value(int(q[0, 2])) == 1.25


def test_k_padding_and_clamped_exponents():
    x = torch.randn(3, 96)
    x[1, 40] = 2.0 ** 120  # e = 112
    x[2, :32] = 2.0 ** -140  # an f32 subnormal block: e clamps at -127
    q, s = mx.quantize(x)
    assert q.shape == (3, 128) and s.shape == (3, 4)
    assert int(q[:, 96:].abs().sum()) == 0 and s[:, 3].tolist() == [0, 0, 0]
    assert int(s[1, 1]) == 127 + 112
    assert int(s[2, 0]) == 0
    back = mx.dequantize(q, s, 96)
    rel = ((back - x).abs() / x.abs().clamp_min(1e-30))[x.abs() > x.abs().amax(1, keepdim=True) / 16]
    # 3 mantissa bits (half a step: 2^-4), but a block maximum in (448, 512) 2^e saturates: up to 64 / 512 = 2^-3
    assert float(rel.max()) <= 2.0 ** -3


def test_entry_points_refuse_bad_shapes_without_gpu():
    from anemoi_models_amd import _lib

    lib = _lib.load()
    P = 4096  # any 16-byte aligned non-null address: nothing is launched
    # anemoi_linear_mx(xq, ldxq, xs, ldxs, wq, ws, bias, res, ldr, out_mx, y, ldy, ys, ldys, M, N, K, act, stream)
    st = lib.anemoi_linear_mx(P, 256, P, 8, P, P, None, None, 0, 0, P, 64, None, 0, 7, 64, 200, 0, None)
    assert st == _lib.ANEMOI_ERR_UNSUPPORTED and b"multiple of 128" in lib.anemoi_last_error()
    st = lib.anemoi_linear_mx(P, 256, P, 8, P, P, None, None, 0, 0, P, 64, None, 0, 7, 24, 256, 0, None)
    assert st == _lib.ANEMOI_ERR_UNSUPPORTED and b"multiple of 16" in lib.anemoi_last_error()
    st = lib.anemoi_linear_mx(P, 256, P, 8, P, P, None, None, 0, 1, P, 128, P, 4, 7, 48, 256, 0, None)
    assert st == _lib.ANEMOI_ERR_UNSUPPORTED and b"multiple of 32" in lib.anemoi_last_error()
    st = lib.anemoi_linear_mx(P, 264, P, 8, P, P, None, None, 0, 0, P, 64, None, 0, 7, 64, 256, 0, None)
    assert st == _lib.ANEMOI_ERR_INVALID and b"ldxq" in lib.anemoi_last_error()
    st = lib.anemoi_linear_mx(P + 4, 256, P, 8, P, P, None, None, 0, 0, P, 64, None, 0, 7, 64, 256, 0, None)
    assert st == _lib.ANEMOI_ERR_INVALID and b"aligned" in lib.anemoi_last_error()
    st = lib.anemoi_linear_mx(P, 256, P, 8, P, P, None, None, 0, 0, None, 64, None, 0, 7, 64, 256, 0, None)
    assert st == _lib.ANEMOI_ERR_INVALID and b"null pointer" in lib.anemoi_last_error()
    # anemoi_mx_quantize(dtype, x, ldx, gamma, beta, eps, q, ldq, s, lds, rows, K, Kp, stream)
    st = lib.anemoi_mx_quantize(_lib.BF16, P, 96, None, None, 0.0, P, 96, P, 3, 5, 96, 96, None)
    assert st == _lib.ANEMOI_ERR_UNSUPPORTED and b"multiple of 128" in lib.anemoi_last_error()
    st = lib.anemoi_mx_quantize(_lib.BF16, P, 96, None, None, 0.0, P, 120, P, 4, 5, 96, 128, None)
    assert st == _lib.ANEMOI_ERR_INVALID and b"ldq" in lib.anemoi_last_error()
    st = lib.anemoi_mx_quantize(_lib.BF16, P, 96, P, None, 0.0, P, 128, P, 4, 5, 96, 128, None)
    assert st == _lib.ANEMOI_ERR_INVALID and b"gamma" in lib.anemoi_last_error()
    st = lib.anemoi_mx_quantize(_lib.F32, P, 8192, None, None, 0.0, P, 8192, P, 256, 5, 8192, 8192, None)
    assert st == _lib.ANEMOI_ERR_UNSUPPORTED and b"4096" in lib.anemoi_last_error()


def test_ops_wrappers_refuse_cpu_tensors():
    from anemoi_models_amd import ops

    with pytest.raises(RuntimeError, match="MI355X"):
        ops.mx_quantize(torch.zeros(4, 128, dtype=torch.bfloat16))
    xq = ops.MXTensor(torch.zeros(4, 128, dtype=torch.uint8), torch.zeros(4, 4, dtype=torch.uint8), 128)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.linear_mx(xq, xq)
