"""MXFP8 route on the MI355X (``-m gpu``): the quantiser bit for bit against the torch restatement of the format
(tests/_mx_ref.py), LayerNorm + quantise, ``linear_mx`` against an f64 product of the dequantised operands on every
epilogue, and the scaled MFMA's lane maps with exact integer data and an asymmetric B."""

import pytest
import torch

import _mx_ref as mx

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _wide_rows(m, k, dtype, seed):
    """Rows with a wide dynamic range: N(0, 1) times 2^u, u uniform in [-24, 24) per 8 elements (blocks mix magnitudes)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(m, k, generator=g)
    u = torch.randint(-24, 24, (m, (k + 7) // 8), generator=g).repeat_interleave(8, dim=1)[:, :k]
    x = torch.ldexp(x, u.float())
    x[:, ::97] = 0.0
    return x.to(dtype)


def _ordinal(codes):
    """e4m3 codes as signed magnitude ordinals: neighbouring representable values differ by one."""
    c = codes.to(torch.int32)
    return torch.where(c >= 128, -(c - 128), c)


def _count_rows(m):
    """Rows checked against the reference at height m: all up to 600, else the first 300, the last 300 and 300 random."""
    if m <= 600:
        return torch.arange(m)
    g = torch.Generator().manual_seed(m)
    return torch.cat([torch.arange(300), torch.arange(m - 300, m), torch.randint(300, m - 300, (300,), generator=g)])


@pytest.mark.parametrize("k", [96, 1024, 1280, 4096])
@pytest.mark.parametrize("m,dtype", [(1, torch.bfloat16), (7, torch.bfloat16), (257, torch.bfloat16),
                                     (40962, torch.bfloat16), (1, torch.float32), (7, torch.float32),
                                     (257, torch.float32), (5121, torch.float32)])
def test_quantize_bit_exact(m, k, dtype):
    from anemoi_models_amd import ops

    x = _wide_rows(m, k, dtype, seed=m * 7 + k)
    got = ops.mx_quantize(x.to(DEV))
    q, s = mx.quantize(x)
    assert got.k == k and got.q.shape == q.shape and got.scales.shape == s.shape
    torch.cuda.synchronize()
    bad_s = int((got.scales.cpu() != s).sum())
    bad_q = int((got.q.cpu() != q).sum())
    assert bad_s == 0 and bad_q == 0, f"{bad_s} scale bytes and {bad_q} element bytes differ"


def test_quantize_strided_rows():
    """Slices of wider device buffers: ldx = 1104 (ldx > K, 16-byte aligned rows: the vector loads) and ldx = 1093 at
    column offset 3 (misaligned rows: the element-wise loads)."""
    from anemoi_models_amd import ops

    for width, c0 in ((1104, 0), (1093, 3)):
        full = _wide_rows(33, width, torch.bfloat16, seed=width)
        view = full.to(DEV)[:, c0:c0 + 1024]
        assert view.stride(0) == width
        got = ops.mx_quantize(view)
        q, s = mx.quantize(full[:, c0:c0 + 1024])
        assert torch.equal(got.q.cpu(), q) and torch.equal(got.scales.cpu(), s)


@pytest.mark.parametrize("k", [96, 1024, 4096])
@pytest.mark.parametrize("m", [7, 5121])
def test_layer_norm_quantize(m, k):
    from anemoi_models_amd import ops

    g = torch.Generator().manual_seed(k + m)
    x = (torch.randn(m, k, generator=g) * 3 + 0.5).to(torch.bfloat16)
    w = torch.randn(k, generator=g) * 0.5 + 1
    b = torch.randn(k, generator=g) * 0.1
    got = ops.mx_quantize(x.to(DEV), ln=(w.to(DEV), b.to(DEV), 1e-5))
    ref = torch.nn.functional.layer_norm(x.float(), (k,), w, b, 1e-5)
    q, s = mx.quantize(ref)
    gq, gs = got.q.cpu(), got.scales.cpu()
    same = gs == s
    assert float(same.float().mean()) >= 0.999, f"scales equal on {float(same.float().mean()):.5f} of the blocks"
    d_ord = (_ordinal(gq) - _ordinal(q)).abs().view(m, -1, 32)
    assert int(d_ord[same].max()) <= 1, "an element is more than one e4m3 step from the f32 LayerNorm's"
    e = torch.maximum(gs, s).to(torch.int32) - 127
    step = torch.ldexp(torch.full(e.shape, 32.0), e.float()).unsqueeze(-1)  # one e4m3 step at the block maximum
    diff = (mx.dequantize(gq, gs) - mx.dequantize(q, s)).abs().view(m, -1, 32)
    assert bool((diff <= step).all())


def _quantized_pair(m, n, k, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(m, k, generator=g).to(torch.bfloat16)
    w = (torch.randn(n, k, generator=g) / k ** 0.5).to(torch.bfloat16)
    return x, w


EPILOGUES = [  # (bias, act, residual, out)
    (False, "Identity", False, "bf16"),
    (True, "GELU", False, "bf16"),
    (True, "Identity", True, "bf16"),
    (True, "GELU", True, "bf16"),
    (True, "GELU", False, "mx"),
    (False, "Identity", True, "mx"),
]


@pytest.mark.parametrize("k", [128, 1024, 4096])
@pytest.mark.parametrize("n", [16, 256, 1024, 4352])
@pytest.mark.parametrize("m", [1, 7, 255, 256, 257, 5121, 40962])
def test_linear_mx(m, n, k):
    from anemoi_models_amd import ops

    x, w = _quantized_pair(m, n, k, seed=m + 3 * n + 7 * k)
    xq = ops.mx_quantize(x.to(DEV))
    wq = ops.mx_quantize(w.to(DEV))
    rows = _count_rows(m)
    a = mx.dequantize(xq.q[rows.to(DEV)], xq.scales[rows.to(DEV)]).double().to(DEV)
    b = mx.dequantize(wq.q, wq.scales).double().to(DEV)
    prod = (a @ b.T).cpu()
    mag = (a.abs() @ b.abs().T).cpu()  # sum |a b| per output element
    gen = torch.Generator().manual_seed(n)
    bias = torch.randn(n, generator=gen) * 0.3
    res = (torch.randn(m, n, generator=gen)).to(torch.bfloat16)
    # accumulation bound per output: one scaled MFMA carries up to 1.6e-5 of the sum |a b| of its 128 products (measured,
    # profiles/r07_mxfp8.md); across MFMAs the C input is f32 and the errors do not add up (3.9e-6 at K = 1024)
    acc = 3e-5 if k == 128 else 1e-5
    for use_bias, act, use_res, out in EPILOGUES:
        if out == "mx" and n % 32:
            continue
        y = ops.linear_mx(xq, wq, bias.to(DEV) if use_bias else None, act=act,
                          residual=res.to(DEV) if use_res else None, out=out)
        pre = prod + (bias.double() if use_bias else 0.0)
        ref = torch.nn.functional.gelu(pre) if act == "GELU" else pre
        if use_res:
            ref = ref + res[rows].double()
        what = f"M={m} N={n} K={k} bias={use_bias} act={act} residual={use_res} out={out}"
        if out == "bf16":
            got = y[rows.to(DEV)].cpu().double()
            tol = acc * mag + 2.0 ** -8 * ref.abs() + 1e-6 * (1 + pre.abs())  # accumulation + bf16 rounding + GELU
            err = (got - ref).abs()
            assert bool((err <= tol).all()), f"{what}: worst |err| / tol = {float((err / tol).max()):.3g}"
        else:
            assert y.k == n and y.q.shape == (m, mx.round_up(n, 128)) and y.scales.shape == (m, mx.round_up(n, 128) // 32)
            gq, gs = y.q[rows.to(DEV)].cpu(), y.scales[rows.to(DEV)].cpu()
            q, s = mx.quantize(ref.float(), kp=mx.round_up(n, 128))
            assert int(gq[:, n:].count_nonzero()) == 0 and int(gs[:, n // 32:].count_nonzero()) == 0, what
            same = gs == s
            assert float(same.float().mean()) >= 0.99, f"{what}: scales equal on {float(same.float().mean()):.4f}"
            # one e4m3 step of the reference value at the scale the kernel chose (where its block maximum fell just below
            # a power of two that the reference's reached, the top of the block saturates: two steps there), plus the
            # accumulation bound of the bf16 route (an element much smaller than its sum of |a b| carries that absolute
            # error into its own e4m3 steps)
            e = (gs.to(torch.int32) - 127).repeat_interleave(32, dim=1)[:, :n].double()
            r = ref.abs() * torch.exp2(-e)
            step = torch.exp2(e + torch.floor(torch.log2(r.clamp_min(2.0 ** -6))) - 3)
            step = torch.where(r > 448, 2 * step, step)  # a block maximum in (448, 512) 2^e saturates to 448 2^e
            err = (mx.dequantize(gq, gs, n).double() - ref).abs()
            tol = step + (acc + 5e-6) * mag + 1e-6 * (1 + pre.abs())
            worst = int((err / tol).flatten().argmax())
            i, j = worst // n, worst % n
            assert bool((err <= tol).all()), (
                f"{what}: worst |err| / (one e4m3 step + tol) = {float((err / tol).max()):.3g} at [{i}, {j}]: "
                f"reference {float(ref[i, j]):.6g}, got {float(mx.dequantize(gq, gs, n)[i, j]):.6g} (code {int(gq[i, j]):#x}, "
                f"scale byte {int(gs[i, j // 32])}, reference scale byte {int(s[i, j // 32])})")


def test_linear_mx_exact_integers_asymmetric_b():
    """Small integers in e4m3 with per-block scales 2^0 .. 2^3 and an asymmetric B: every partial sum is an integer below
    2^24, so the f32 accumulation is exact and the bf16 result must equal the exact product rounded once."""
    from anemoi_models_amd import ops

    m, n, k = 300, 272, 1024
    g = torch.Generator().manual_seed(5)
    ia = torch.randint(-4, 5, (m, k), generator=g).float()
    ib = ((torch.arange(n)[:, None] * 3 + torch.arange(k)[None, :] * 5 + torch.arange(n)[:, None] ** 2 // 7) % 9 - 4).float()
    sa = torch.randint(127, 131, (m, k // 32), generator=g).to(torch.uint8)
    sb = torch.randint(127, 131, (n, k // 32), generator=g).to(torch.uint8)
    xq = ops.MXTensor(ia.to(torch.float8_e4m3fn).view(torch.uint8).to(DEV), sa.to(DEV), k)
    wq = ops.MXTensor(ib.to(torch.float8_e4m3fn).view(torch.uint8).to(DEV), sb.to(DEV), k)
    a = mx.dequantize(xq.q, xq.scales).double()
    b = mx.dequantize(wq.q, wq.scales).double()
    exact = a @ b.T
    assert float(exact.abs().max()) < 2 ** 24
    got = ops.linear_mx(xq, wq).cpu()
    want = exact.float().to(torch.bfloat16)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), \
        f"{int((got != want).sum())} of {got.numel()} outputs differ from the exact product"
    # the transposed roles (B as activations, the first 288 rows of A as the weight) catch a row <-> column swap of C/D
    got_t = ops.linear_mx(wq, ops.MXTensor(xq.q[:288], xq.scales[:288], k)).cpu()
    assert torch.equal(got_t.view(torch.int16), exact[:288].T.float().to(torch.bfloat16).view(torch.int16))


def test_linear_mx_refuses_mismatched_operands():
    from anemoi_models_amd import ops

    xq = ops.mx_quantize(torch.randn(8, 256, device=DEV, dtype=torch.bfloat16))
    wq = ops.mx_quantize(torch.randn(64, 384, device=DEV, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="K="):
        ops.linear_mx(xq, wq)
    with pytest.raises(NotImplementedError, match="multiple of 16"):
        ops.linear_mx(xq, ops.mx_quantize(torch.randn(24, 256, device=DEV, dtype=torch.bfloat16)))
    with pytest.raises(NotImplementedError, match="multiple of 32"):
        ops.linear_mx(xq, ops.mx_quantize(torch.randn(48, 256, device=DEV, dtype=torch.bfloat16)), out="mx")
