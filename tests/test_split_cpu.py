"""Split-bf16 ("bf16x3") arithmetic and its switch, without a GPU: the CPU restatement (tests/_split_ref.py) sits between
f32 and bf16 operands, ``hi + lo`` is exact for 16 significand bits, and ``ANEMOI_AMD_F32_LINEAR`` parses as documented."""

import pytest
import torch

from _split_ref import linear_bf16x3, split


def _rms_rel(got, want):
    return float(((got.double() - want).square().mean() / want.square().mean()).sqrt())


@pytest.mark.parametrize("k", [256, 1024, 4096])
def test_bf16x3_sits_between_f32_and_bf16_operands(k):
    g = torch.Generator().manual_seed(k)
    x = torch.randn(512, k, generator=g)
    w = (torch.rand(384, k, generator=g) * 2 - 1) / k ** 0.5
    want = x.double() @ w.double().T
    e_f32 = _rms_rel(x @ w.T, want)
    e_x3 = _rms_rel(linear_bf16x3(x, w), want)
    e_bf16 = _rms_rel(x.to(torch.bfloat16).float() @ w.to(torch.bfloat16).float().T, want)
    print(f"K={k}: rms relative error f32 {e_f32:.2e}, bf16x3 {e_x3:.2e}, bf16 operands {e_bf16:.2e}")
    assert 5 * e_f32 <= e_x3 and 5 * e_x3 <= e_bf16


def test_hi_plus_lo_is_exact_for_16_significand_bits():
    g = torch.Generator().manual_seed(3)
    m = torch.randint(-(1 << 16) + 1, 1 << 16, (4096,), generator=g).float()  # <= 16 significand bits
    e = torch.randint(-60, 60, (4096,), generator=g).float()
    v = m * torch.exp2(e)
    hi, lo = split(v)
    assert torch.equal(hi + lo, v)
    full = torch.randn(4096, generator=g)  # 24 bits: the remainder is below 2^-16 |v|
    hi, lo = split(full)
    assert float(((hi + lo) - full).abs().div(full.abs()).max()) <= 2.0 ** -16


def test_switch_parser(monkeypatch):
    from anemoi_models_amd import runtime

    monkeypatch.delenv("ANEMOI_AMD_F32_LINEAR", raising=False)
    assert runtime.f32_linear_split(torch.float32) is False
    monkeypatch.setenv("ANEMOI_AMD_F32_LINEAR", "exact")
    assert runtime.f32_linear_split(torch.float32) is False
    monkeypatch.setenv("ANEMOI_AMD_F32_LINEAR", "bf16x3")
    assert runtime.f32_linear_split(torch.float32) is True
    assert runtime.f32_linear_split(torch.bfloat16) is False
    monkeypatch.setenv("ANEMOI_AMD_F32_LINEAR", "tf32")
    with pytest.raises(ValueError, match="ANEMOI_AMD_F32_LINEAR"):
        runtime.f32_linear_split(torch.float32)


def test_argument_checks_before_any_launch():
    """K off the 32-multiple, null and misaligned planes are refused by the C entry points without touching a device."""
    from anemoi_models_amd import _lib

    lib = _lib.load()
    P = 1 << 20  # never dereferenced
    # anemoi_linear_split(x, ldx, w_hi, w_lo, bias, residual, ldr, y, ldy, M, N, K, act, stream)
    assert lib.anemoi_linear_split(P, 48, P, P, None, None, 0, P, 64, 7, 64, 48, 0, None) == _lib.ANEMOI_ERR_INVALID
    assert lib.anemoi_linear_split(P, 64, P, None, None, None, 0, P, 64, 7, 64, 64, 0, None) == _lib.ANEMOI_ERR_INVALID
    assert lib.anemoi_linear_split(P, 64, P + 2, P, None, None, 0, P, 64, 7, 64, 64, 0, None) == _lib.ANEMOI_ERR_INVALID
    assert lib.anemoi_linear_split(P, 64, P, P, None, None, 0, P, 64, 7, 64, 64, 9, None) == _lib.ANEMOI_ERR_INVALID
    assert lib.anemoi_linear_split(P, 64, P, P, None, None, 0, P, 64, 0, 64, 64, 0, None) == _lib.ANEMOI_OK  # M = 0: no launch
    # anemoi_split_weight(w, ldw, w_hi, w_lo, N, K, stream)
    assert lib.anemoi_split_weight(P, 48, P, P, 5, 48, None) == _lib.ANEMOI_ERR_INVALID
    assert lib.anemoi_split_weight(P, 64, P, P + 8, 5, 64, None) == _lib.ANEMOI_ERR_INVALID
    assert lib.anemoi_split_weight(P, 64, P, P, 0, 64, None) == _lib.ANEMOI_OK
