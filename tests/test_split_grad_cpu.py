"""Split-bf16 weight gradient and the training switch, without a GPU: the CPU restatement (tests/_split_grad_ref.py) sits
between the exact f32 product and bf16 operands, ``hi + lo`` is exact for 16 significand bits, ``ANEMOI_AMD_F32_TRAIN_LINEAR``
parses as documented and independently of the inference switch, the routing rules, and the C entry point's argument checks."""

import pytest
import torch

from _split_grad_ref import weight_grad_bf16x3
from _split_ref import split


def _max_rel(got, want):
    return float((got.double() - want).abs().max() / want.abs().max())


def test_bf16x3_weight_gradient_sits_between_f32_and_bf16_operands():
    g = torch.Generator().manual_seed(4096)
    dy = torch.randn(4096, 64, generator=g)
    x = torch.randn(4096, 64, generator=g)
    want = dy.double().T @ x.double()
    e_f32 = _max_rel(dy.T @ x, want)
    e_x3 = _max_rel(weight_grad_bf16x3(dy, x), want)
    e_bf16 = _max_rel(dy.to(torch.bfloat16).float().T @ x.to(torch.bfloat16).float(), want)
    print(f"M=4096 N=K=64: max relative error f32 {e_f32:.2e}, bf16x3 {e_x3:.2e}, bf16 operands {e_bf16:.2e}")
    assert e_f32 < e_x3 < e_bf16


def test_hi_plus_lo_is_exact_for_16_significand_bits():
    g = torch.Generator().manual_seed(8)
    m = torch.randint(-(1 << 16) + 1, 1 << 16, (4096,), generator=g).float()
    v = m * torch.exp2(torch.randint(-60, 60, (4096,), generator=g).float())
    hi, lo = split(v)
    assert torch.equal(hi + lo, v)
    ints = torch.randint(-(1 << 15), (1 << 15) + 1, (4096,), generator=g).float()  # the GPU exactness test's operands
    hi, lo = split(ints)
    assert torch.equal(hi + lo, ints)


def test_training_switch_parser_is_independent_of_the_inference_switch(monkeypatch):
    from anemoi_models_amd import runtime

    monkeypatch.delenv("ANEMOI_AMD_F32_LINEAR", raising=False)
    monkeypatch.delenv("ANEMOI_AMD_F32_TRAIN_LINEAR", raising=False)
    assert runtime.f32_train_linear_split(torch.float32) is False
    monkeypatch.setenv("ANEMOI_AMD_F32_TRAIN_LINEAR", "exact")
    assert runtime.f32_train_linear_split(torch.float32) is False
    monkeypatch.setenv("ANEMOI_AMD_F32_TRAIN_LINEAR", "bf16x3")
    assert runtime.f32_train_linear_split(torch.float32) is True
    assert runtime.f32_train_linear_split(torch.bfloat16) is False
    assert runtime.f32_linear_split(torch.float32) is False  # the inference switch has not moved
    monkeypatch.setenv("ANEMOI_AMD_F32_LINEAR", "bf16x3")
    monkeypatch.setenv("ANEMOI_AMD_F32_TRAIN_LINEAR", "exact")
    assert runtime.f32_linear_split(torch.float32) is True and runtime.f32_train_linear_split(torch.float32) is False
    monkeypatch.setenv("ANEMOI_AMD_F32_TRAIN_LINEAR", "tf32")
    with pytest.raises(ValueError, match="ANEMOI_AMD_F32_TRAIN_LINEAR"):
        runtime.f32_train_linear_split(torch.float32)
    assert runtime.f32_linear_split(torch.float32) is True  # garbage there does not reach the inference parser
    monkeypatch.setenv("ANEMOI_AMD_F32_LINEAR", "tf32")
    monkeypatch.setenv("ANEMOI_AMD_F32_TRAIN_LINEAR", "bf16x3")
    assert runtime.f32_train_linear_split(torch.float32) is True


def test_routing_rules_and_chunking():
    from anemoi_models_amd import ops, runtime

    assert runtime.split_grad_route(40962, 1024, 192) and runtime.split_grad_route(1, 4, 4)
    assert not runtime.split_grad_route(5248, 22, 128) and not runtime.split_grad_route(5248, 128, 30)
    assert runtime.train_split_route(5248, 22, 128) and not runtime.train_split_route(5248, 128, 16)
    for m, n, k in [(1, 80, 32), (63, 144, 192), (4133, 80, 96), (4133, 1024, 1024), (40962, 1024, 192), (542080, 1024, 192)]:
        chunks, rows = ops.weight_grad_split_chunks(m, n, k)
        assert rows % 32 == 0 and chunks * rows >= m > (chunks - 1) * rows
        assert chunks == 1 or (rows >= 1024 and chunks * ((n + 127) // 128) * ((k + 127) // 128) <= ops.SPLIT_GRAD_WORKGROUPS)
    assert ops.weight_grad_split_chunks(4133, 80, 96)[0] == 4


def test_argument_checks_before_any_launch():
    """Null pointers, N / K / pitches / pointers off their alignment, a pitch below the width, a bad chunk size and a short
    chunk stride are refused by the C entry point without touching a device."""
    from anemoi_models_amd import _lib

    lib = _lib.load()
    P = 1 << 20  # never dereferenced
    # anemoi_weight_grad_split(dy, ldy, x, ldx, partial, partial_stride, M, N, K, chunk_rows, stream)
    f = lib.anemoi_weight_grad_split
    bad = _lib.ANEMOI_ERR_INVALID
    assert f(None, 80, P, 96, P, 80 * 96, 64, 80, 96, 64, None) == bad
    assert f(P, 80, None, 96, P, 80 * 96, 64, 80, 96, 64, None) == bad
    assert f(P, 80, P, 96, None, 80 * 96, 64, 80, 96, 64, None) == bad
    assert f(P, 80, P, 96, None, 80 * 96, 0, 80, 96, 64, None) == bad  # M = 0 still needs somewhere to put the zeros
    assert f(P, 80, P, 96, P, 80 * 96, -1, 80, 96, 64, None) == bad
    assert f(P, 80, P, 96, P, 78 * 96, 64, 78, 96, 64, None) == bad and b"multiples of 4" in lib.anemoi_last_error()
    assert f(P, 80, P, 96, P, 80 * 94, 64, 80, 94, 64, None) == bad
    assert f(P, 76, P, 96, P, 80 * 96, 64, 80, 96, 64, None) == bad and b"leading dimension" in lib.anemoi_last_error()
    assert f(P, 80, P, 92, P, 80 * 96, 64, 80, 96, 64, None) == bad
    assert f(P, 82, P, 96, P, 80 * 96, 64, 80, 96, 64, None) == bad  # pitch off the multiple of 4
    assert f(P + 4, 80, P, 96, P, 80 * 96, 64, 80, 96, 64, None) == bad
    assert f(P, 80, P + 8, 96, P, 80 * 96, 64, 80, 96, 64, None) == bad
    assert f(P, 80, P, 96, P + 4, 80 * 96, 64, 80, 96, 64, None) == bad
    assert f(P, 80, P, 96, P, 80 * 96, 64, 80, 96, 48, None) == bad and b"chunk_rows" in lib.anemoi_last_error()
    assert f(P, 80, P, 96, P, 80 * 96, 64, 80, 96, 0, None) == bad
    assert f(P, 80, P, 96, P, 80 * 96 - 4, 64, 80, 96, 64, None) == bad and b"partial_stride" in lib.anemoi_last_error()
    assert f(P, 80, P, 96, P, 80 * 96 + 2, 64, 80, 96, 64, None) == bad


def test_op_refuses_cpu_tensors_and_bad_shapes():
    from anemoi_models_amd import ops

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.weight_grad_split(torch.zeros(8, 8), torch.zeros(8, 8), 8)
