"""``ops.split_weight`` / ``ops.linear_split`` (csrc/gemm_split.hip) on the MI355X (``-m gpu``): the planes against torch's
own casts bit for bit, integer operands where the f64 product is the only right answer, random operands against the CPU
restatement of the arithmetic (tests/_split_ref.py) on the same data, and the contract at the edges."""

import pytest
import torch

from _split_ref import linear_bf16x3

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _planes_by_torch(w):
    hi = w.to(torch.bfloat16)
    lo = (w - hi.float()).to(torch.bfloat16)
    return hi, lo


@pytest.mark.parametrize("n,k,ldw", [(7, 32, 32), (129, 256, 256), (80, 1024, 1056), (2240, 64, 64)])
def test_split_weight_planes_are_torchs_own_casts(n, k, ldw):
    from anemoi_models_amd import ops

    g = torch.Generator().manual_seed(n + k)
    buf = torch.randn(n, ldw, generator=g)
    buf[0, :8] = torch.tensor([0.0, -0.0, 1e-40, -3e-39, 2.0 ** -126, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -9, 65504.0])
    buf[-1, :4] = torch.tensor([1e-45, 9.1e-41, 2.0 ** -133, -(2.0 ** -140)])  # f32 subnormals (bf16 subnormals too)
    w = buf.to(DEV)[:, :k]
    hi, lo = ops.split_weight(w)
    want_hi, want_lo = _planes_by_torch(w)
    assert hi.dtype == lo.dtype == torch.bfloat16 and hi.is_contiguous() and lo.is_contiguous()
    assert torch.equal(hi.view(torch.int16), want_hi.view(torch.int16))
    assert torch.equal(lo.view(torch.int16), want_lo.view(torch.int16))


def _ints(shape, bound, g):
    return torch.randint(-bound, bound + 1, shape, generator=g).float()


@pytest.mark.parametrize("case", ["x_needs_lo", "w_needs_lo", "both_bf16_exact"])
def test_integer_operands_give_the_exact_product(case):
    """|sums| <= 1024 * 300 * 3 < 2^24: every partial sum is exact in f32 in any order.  300 needs 9 significand bits, so its
    ``lo`` is not zero: ``x_needs_lo`` fails without ``x_lo w_hi``, ``w_needs_lo`` without ``x_hi w_lo``."""
    from anemoi_models_amd import ops

    g = torch.Generator().manual_seed(11)
    m, n, k = 257, 208, 1024
    bx, bw = {"x_needs_lo": (300, 3), "w_needs_lo": (3, 300), "both_bf16_exact": (120, 3)}[case]
    x, w = _ints((m, k), bx, g), _ints((n, k), bw, g)
    if case != "both_bf16_exact":
        big = x if case == "x_needs_lo" else w
        assert not torch.equal(big.to(torch.bfloat16).float(), big)
    want = (x.double() @ w.double().T).float()
    got = ops.linear_split(x.to(DEV), ops.split_weight(w.to(DEV)))
    assert torch.equal(got.cpu(), want)


_ACTS = {"Identity": lambda t: t, "GELU": lambda t: 0.5 * t * (1 + torch.erf(t * 0.5 ** 0.5)),
         "SiLU": lambda t: t * torch.sigmoid(t), "ReLU": torch.relu}

# (M, N, K, act, bias, residual, strided)
_SHAPES = [
    (1, 80, 32, "Identity", True, False, False),
    (63, 2240, 256, "GELU", True, True, False),
    (129, 5 * 512 + 16, 1024, "SiLU", False, True, True),
    (129, 80, 4096, "ReLU", True, False, True),
    (40962, 80, 256, "Identity", True, False, False),
    (40962, 1024, 1024, "GELU", True, True, True),
    (1000, 512, 4096, "Identity", False, False, False),
    (63, 128, 32, "SiLU", True, True, True),
]


@pytest.mark.parametrize("m,n,k,act,with_bias,with_res,strided", _SHAPES)
def test_random_operands_against_the_cpu_restatement(m, n, k, act, with_bias, with_res, strided):
    """Error against the f64 product, normalised by max |ref|, at most 2 x the error of ``_split_ref.linear_bf16x3`` on the
    same operands: kernel and restatement differ in f32 accumulation order only (~3e-7 against the 4e-6 truncation term);
    a dropped correction product lands >= 100 x above."""
    from anemoi_models_amd import ops

    g = torch.Generator().manual_seed(m * 31 + n * 7 + k)
    x = torch.randn(m, k, generator=g)
    w = (torch.rand(n, k, generator=g) * 2 - 1) / k ** 0.5
    bias = torch.randn(n, generator=g) if with_bias else None
    res = torch.randn(m, n, generator=g) if with_res else None
    f = _ACTS[act]

    def finish(pre):  # the same torch activation on every pre-activation, in f64
        y = f(pre.double())  # (the bias is already inside `pre`)
        return y if res is None else y + res.double()

    pre64 = x.double() @ w.double().T + (0 if bias is None else bias.double())
    want = finish(pre64)
    ref = finish(linear_bf16x3(x, w, bias))
    xd = x.to(DEV)
    if strided:
        xd = torch.cat([xd, torch.full((m, 8), float("nan"), device=DEV)], dim=1)[:, :k]
        out = torch.full((m, n + 12), -7.0, device=DEV)[:, :n]
    else:
        out = None
    wd = w.to(DEV)
    kw = dict(act=act, residual=None if res is None else res.to(DEV))
    got = ops.linear_split(xd, ops.split_weight(wd), None if bias is None else bias.to(DEV), out=out, **kw)
    exact = ops.linear(x.to(DEV), wd, None if bias is None else bias.to(DEV), **kw)
    scale = want.abs().max()
    e_got = float((got.cpu().double() - want).abs().max() / scale)
    e_ref = float((ref.double() - want).abs().max() / scale)
    e_f32 = float((exact.cpu().double() - want).abs().max() / scale)
    print(f"M={m} N={n} K={k} {act}: split kernel {e_got:.3e}, CPU restatement {e_ref:.3e}, exact f32 kernel {e_f32:.3e}")
    if strided:
        assert got.data_ptr() == out.data_ptr() and bool((out._base[:, n:] == -7.0).all())
    assert e_got <= 2 * e_ref


def test_run_to_run_bit_identity_nan_row_empty_m_and_bad_k():
    from anemoi_models_amd import ops

    g = torch.Generator().manual_seed(5)
    x = torch.randn(300, 256, generator=g).to(DEV)
    w = torch.randn(144, 256, generator=g).to(DEV)
    planes = ops.split_weight(w)
    a, b = ops.linear_split(x, planes), ops.linear_split(x, planes)
    assert torch.equal(a, b)
    x[123, 77] = float("nan")
    y = ops.linear_split(x, planes)
    bad = torch.isnan(y).any(dim=1)
    assert bool(torch.isnan(y[123]).all()) and int(bad.sum()) == 1
    ops.PROFILE = []
    try:
        empty = ops.linear_split(x[:0], planes)
        assert empty.shape == (0, 144) and ops.PROFILE == []  # no launch
    finally:
        ops.PROFILE = None
    with pytest.raises(ValueError):
        ops.split_weight(torch.zeros(16, 48, device=DEV))
    with pytest.raises(ValueError):
        ops.linear_split(torch.zeros(4, 48, device=DEV),
                         ops.SplitWeight(torch.zeros(16, 48, dtype=torch.bfloat16, device=DEV),
                                         torch.zeros(16, 48, dtype=torch.bfloat16, device=DEV)))
