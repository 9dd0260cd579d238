"""``runtime.compose_decoder_fold`` on the CPU: the composed projection weight ``[W_p | W_t | W_p A_s | E]`` and bias
``b_p + W_p b_s + b_E`` against the unfolded mapper-block formula in f64 on random small layers, raw widths with padding
columns (and a constant-1 column that is not the first padding column) among them."""

import pytest
import torch

import _dec_fold_ref as R
from anemoi_models_amd import ops, runtime


def _layers(c, k_in, hup, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    return dict(proj_w=rnd(c, c) / c**0.5, proj_b=rnd(c), w_t=rnd(c, hup) / hup**0.5, self_w=rnd(c, c) / c**0.5, self_b=rnd(c),
                gamma=1.0 + 0.2 * rnd(c), beta=0.3 * rnd(c), emb_w=rnd(c, k_in) / k_in**0.5, emb_b=rnd(c)), g


def _unfolded(p, x, s, t, eps):
    """y = W_p (S + lin_self(LN(emb(x)))) + W_t t + b_p + emb(x), every step in f64."""
    h = x @ p["emb_w"].T + p["emb_b"]
    mean, var = h.mean(dim=1, keepdim=True), h.var(dim=1, unbiased=False, keepdim=True)
    rstd = (var + eps).rsqrt()
    x_r = ((h - mean) * rstd * p["gamma"] + p["beta"]) @ p["self_w"].T + p["self_b"]
    return (s + x_r) @ p["proj_w"].T + t @ p["w_t"].T + p["proj_b"] + h, rstd


@pytest.mark.parametrize("c,k_in,k_pad,one_col,hup", [(32, 37, 64, 37, 32), (64, 100, 128, 105, 64), (48, 63, 64, 63, 16),
                                                       (32, 20, 64, 63, 32)])
def test_composed_weight_and_bias_against_unfolded_formula(c, k_in, k_pad, one_col, hup):
    eps, n = 1e-5, 23
    p, g = _layers(c, k_in, hup, seed=c + k_in)
    x = torch.randn(n, k_in, generator=g, dtype=torch.float64)
    s, t = torch.randn(n, c, generator=g, dtype=torch.float64), torch.randn(n, hup, generator=g, dtype=torch.float64)
    want, rstd = _unfolded(p, x, s, t, eps)

    x_aug = torch.zeros(n, k_pad, dtype=torch.float64)
    x_aug[:, :k_in], x_aug[:, one_col] = x, 1.0
    w, b = runtime.compose_decoder_fold(p["proj_w"], p["proj_b"], p["w_t"], p["self_w"], p["self_b"], p["gamma"], p["beta"],
                                        p["emb_w"], p["emb_b"], k_pad, one_col, torch.float64)
    k = c + hup + 2 * k_pad
    assert w.dtype == torch.float64 and b.dtype == torch.float32 and tuple(b.shape) == (c,)
    assert tuple(w.shape) == (c, ops.round_up(k, ops.k_multiple(torch.float64))) and not w[:, k:].any()
    operand = torch.zeros(n, w.shape[1], dtype=torch.float64)
    operand[:, :k] = torch.cat([s, t, rstd * x_aug, x_aug], dim=1)
    got = operand @ w.T + b.double()
    # f64 products on both sides; the bias passes through f32 once (2^-24 relative to its own size)
    assert float((got - want).abs().max()) <= 1e-9 * float(want.abs().max()) + 2.0**-22 * float(b.abs().max())

    # the blocks: W_p and W_t untouched, E without its bias (it sits in the f32 bias), zero in every padding column but
    # the constant-1 column of the rstd block (the centred embedding bias, scaled by rstd with the row)
    assert torch.equal(w[:, :c], p["proj_w"]) and torch.equal(w[:, c:c + hup], p["w_t"])
    e_blk, a_blk = w[:, c + hup + k_pad:k], w[:, c + hup:c + hup + k_pad]
    assert torch.equal(e_blk[:, :k_in], p["emb_w"]) and not e_blk[:, k_in:].any()
    pad = [j for j in range(k_in, k_pad) if j != one_col]
    assert not a_blk[:, pad].any() and a_blk[:, one_col].abs().max() > 0

    # the kernel dtype: the same operator rounded ONCE, K padded to the bf16 slab
    wb, bb = runtime.compose_decoder_fold(p["proj_w"], p["proj_b"], p["w_t"], p["self_w"], p["self_b"], p["gamma"], p["beta"],
                                          p["emb_w"], p["emb_b"], k_pad, one_col, torch.bfloat16)
    assert wb.dtype == torch.bfloat16 and wb.shape[1] == ops.round_up(k, 64) and wb.is_contiguous()
    assert torch.equal(wb[:, :k], w[:, :k].to(torch.bfloat16)) and not wb[:, k:].any() and torch.equal(bb, b)


def test_layers_without_bias():
    c, k_in, k_pad, one_col, hup = 32, 30, 64, 30, 32
    p, g = _layers(c, k_in, hup, seed=5)
    p["proj_b"], p["self_b"], p["emb_b"] = None, None, None
    x = torch.randn(7, k_in, generator=g, dtype=torch.float64)
    s, t = torch.randn(7, c, generator=g, dtype=torch.float64), torch.randn(7, hup, generator=g, dtype=torch.float64)
    zero = torch.zeros(c, dtype=torch.float64)
    want, rstd = _unfolded({**p, "proj_b": zero, "self_b": zero, "emb_b": zero}, x, s, t, 1e-5)
    x_aug = torch.zeros(7, k_pad, dtype=torch.float64)
    x_aug[:, :k_in], x_aug[:, one_col] = x, 1.0
    w, b = runtime.compose_decoder_fold(p["proj_w"], None, p["w_t"], p["self_w"], None, p["gamma"], p["beta"], p["emb_w"], None,
                                        k_pad, one_col, torch.float64)
    got = torch.cat([s, t, rstd * x_aug, x_aug], dim=1) @ w[:, :c + hup + 2 * k_pad].T + b.double()
    assert float((got - want).abs().max()) <= 1e-9 * float(want.abs().max()) + 2.0**-22 * float(b.abs().max())


@pytest.mark.parametrize("ks,d,up", R.SHAPES)
def test_block_cases_keep_the_parent_error_away_from_zero(ks, d, up):
    """tests/test_gpu_dec_fold.py bounds the folded route's error by 1.5 x the parent route's on these cases: that ratio
    means something only while the parent's own error is a real rounding error.  Both routes restated in torch on bf16-rounded
    operands (``_dec_fold_ref.emulate_routes``): the parent's maximum error must be at least a quarter ulp of the largest
    output (bf16: 2^-9 relative per ulp, so 2^-11 |y|max) -- one of 65 x C outputs near the top binade rounded by more
    than half of the worst case."""
    parent, folded, ymax = R.emulate_routes(R.block_case(ks, d, up))
    print(f"Ks={ks} D={d} up={up}: emulated max error parent {parent:.3e}, folded {folded:.3e} (ratio {folded / parent:.2f}), "
          f"|y|max {ymax:.3f}")
    assert parent >= 2.0**-11 * ymax


def test_switch_and_grad_mode(monkeypatch):
    monkeypatch.delenv("ANEMOI_AMD_DEC_FOLD", raising=False)
    with torch.no_grad():
        assert runtime.dec_fold_enabled()
        monkeypatch.setenv("ANEMOI_AMD_DEC_FOLD", "0")
        assert not runtime.dec_fold_enabled()
        monkeypatch.setenv("ANEMOI_AMD_DEC_FOLD", "1")
        assert runtime.dec_fold_enabled()
    with torch.enable_grad():
        assert not runtime.dec_fold_enabled()


def test_route_conditions(monkeypatch):
    """``dec_fold_route``: bf16, one chunk, raw width 64 / 128 / 256, ``out | t`` whole K slabs; off under the switch, MXFP8,
    the unfolded edge kernel and the opt-in thin statistics site."""
    for name in ("ANEMOI_AMD_DEC_FOLD", "ANEMOI_AMD_THIN_STATS", "ANEMOI_AMD_MXFP8", "ANEMOI_AMD_EDGE_FOLD", "ANEMOI_AMD_LN_FOLD",
                 "ANEMOI_AMD_EMBED_FOLD"):
        monkeypatch.delenv(name, raising=False)
    blk = R.block_case(64, 32, 8)["blk"]
    bf16 = torch.bfloat16
    with torch.no_grad():
        assert blk.dec_fold_route(bf16, 64) and blk.dec_fold_route(bf16, 128) and blk.dec_fold_route(bf16, 256)
        assert not blk.dec_fold_route(bf16, 192) and not blk.dec_fold_route(torch.float32, 64)
        assert not blk.dec_fold_route(bf16, 64, num_chunks=2)
        for name, value in (("ANEMOI_AMD_DEC_FOLD", "0"), ("ANEMOI_AMD_THIN_STATS", "1"), ("ANEMOI_AMD_MXFP8", "1"),
                            ("ANEMOI_AMD_EDGE_FOLD", "0"), ("ANEMOI_AMD_EMBED_FOLD", "0")):
            monkeypatch.setenv(name, value)
            assert not blk.dec_fold_route(bf16, 64), name
            monkeypatch.delenv(name)
        assert blk.dec_fold_route(bf16, 64)
    with torch.enable_grad():
        assert not blk.dec_fold_route(bf16, 64)
