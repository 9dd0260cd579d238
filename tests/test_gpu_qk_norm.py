"""qk_norm on the HIP kernels (csrc/head_norm.hip): anemoi_head_norm / _backward per element and in aggregate against the f64
restatement of tests/_qk_norm_ref.py, their layouts (in place inside ``x_r | q | k | v`` and ``q | k | v``, guards, the scalar
route against the vector route), determinism and graph capture; then every module that takes the switch -- self attention, the
Transformer block, the GraphTransformer processor and mapper blocks, the mappers, one flat model per processor -- forward and
every gradient against the f64 restatement, and the launch trail of the Transformer block with and without the switch.

Worst used fraction of the per-element forward bound per case ``(rows, groups, H, D)``, as the first test prints it on an MI355X:

    f32   (1,1,1,4) 0.05  (37,2,3,4) 0.15  (33,2,2,5) 0.14  (130,1,5,12) 0.16  (257,2,16,32) 0.15  (200,2,16,64) 0.16
          (65,1,4,128) 0.14  (4100,2,16,64) 0.18
    bf16  (37,2,3,4) 1.00  (33,2,2,5) 1.00  (130,1,5,12) 1.00  (257,2,16,32) 1.00  (200,2,16,64) 1.00  (1027,2,16,64) 1.00
          (65,1,4,128) 1.00  (4100,2,16,64) 1.00  (the half-ulp of the bf16 result is nearly the whole bound: an element whose
          f32 value lies next to a rounding tie uses all of it)
"""

import pytest
import torch

import _qk_norm_ref as R
from test_gpu_mhsa import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = lambda v: R.name(v) if isinstance(v, torch.dtype) else str(v)  # noqa: E731


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from anemoi_models_amd import _lib

    _lib.load()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(_bits(a), _bits(b)))


# ------------------------------------------------------------------------------------------------ the kernels against f64
@pytest.mark.parametrize("dtype,rows,groups,h,d", R.CASES, ids=IDS)
def test_head_norm_forward_and_backward_vs_f64(dtype, rows, groups, h, d):
    from anemoi_models_amd import autograd, ops

    x, w, dy = R.inputs(dtype, rows, groups, h, d)
    want, dx_want, dw_want, stats_want = R.reference(dtype, rows, groups, h, d)
    _, bound = R.forward_bound(x, w, h, groups, dtype)
    xd, wd = x.to(DEV, dtype), w.to(DEV)
    y, stats = ops.head_norm(xd, wd, h, groups, with_stats=True)
    used = R.used_fraction(y.float(), want, bound)
    print(f"head_norm {R.name(dtype)} {(rows, groups, h, d)}: worst used fraction of the per-element bound {used:.2f}")
    assert used <= 1.0
    assert R.rel_err(y.float(), want) < R.FWD_TOL[dtype]
    # the statistics: (rstd, -mean rstd) within the f32 rounding of the kernel's sums (the K of the forward bound)
    k_u = R.bound_k(d) * R.U32
    rstd = stats_want[..., 0]
    xh = x.double().reshape(rows, groups * h, d)
    scale = rstd * (xh.abs().amax(-1) + xh.mean(-1).abs())
    got = stats.double().cpu()
    assert bool(((got[..., 0] - rstd).abs() <= k_u * rstd).all())
    assert bool(((got[..., 1] - stats_want[..., 1]).abs() <= k_u * scale).all())
    # gradients through the autograd node; its forward is the bits of ops.head_norm
    xl, wl = xd.clone().requires_grad_(), wd.clone().requires_grad_()
    y2 = autograd.head_norm(xl, wl, h, groups, R.EPS)
    assert _same_bits(y2.detach(), y)
    y2.backward(dy.to(DEV, dtype))
    ex, ew = R.rel_err(xl.grad.float(), dx_want), R.rel_err(wl.grad, dw_want)
    print(f"    aggregate: y {R.rel_err(y.float(), want):.2e}  dx {ex:.2e}  dw {ew:.2e}")
    assert xl.grad.dtype == dtype and wl.grad.dtype == torch.float32 and tuple(wl.grad.shape) == (groups, d)
    assert ex < R.GRAD_TOL[dtype] and ew < R.GRAD_TOL[dtype]


def test_head_norm_backward_takes_a_zero_weight():
    from anemoi_models_amd import ops

    rows, groups, h, d = 70, 2, 4, 16
    x, w, dy = R.inputs(torch.float32, rows, groups, h, d, seed=3)
    w[1, 3] = 0.0
    w[0] = 0.0
    xl, wl = x.double().requires_grad_(), w.double().requires_grad_()
    R.head_norm(xl, wl, h, groups).backward(dy.double())
    _, stats = ops.head_norm(x.to(DEV), w.to(DEV), h, groups, with_stats=True)
    dx, dw = ops.head_norm_backward(dy.to(DEV), x.to(DEV), stats, w.to(DEV), h, groups)
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dw).all())
    assert R.rel_err(dx, xl.grad) < R.GRAD_TOL[torch.float32] and R.rel_err(dw, wl.grad) < R.GRAD_TOL[torch.float32]
    assert float(dx[:, :h * d].abs().max()) == 0.0  # the group whose weight is zero passes no gradient to x


@pytest.mark.parametrize("dtype,rows,groups,h,d", [(torch.float32, 257, 2, 16, 32), (torch.bfloat16, 1027, 2, 16, 64),
                                                   (torch.float32, 33, 2, 2, 5), (torch.bfloat16, 65, 1, 4, 128)], ids=IDS)
def test_repeated_calls_give_the_same_bits(dtype, rows, groups, h, d):
    from anemoi_models_amd import ops

    x, w, dy = R.inputs(dtype, rows, groups, h, d)
    x, w, dy = x.to(DEV, dtype), w.to(DEV), dy.to(DEV, dtype)
    runs = []
    for _ in range(2):
        y, stats = ops.head_norm(x, w, h, groups, with_stats=True)
        dx, dw = ops.head_norm_backward(dy, x, stats, w, h, groups)
        runs.append((y, stats, dx, dw))
    for a, b in zip(*runs):
        assert _same_bits(a, b)


# ------------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=IDS)
@pytest.mark.parametrize("layout", ["x_r|q|k|v", "q|k|v"])
@pytest.mark.parametrize("rows,h,d,pad", [(37, 3, 8, 0), (130, 16, 64, 8), (33, 2, 5, 3)])
def test_in_place_inside_the_product_matrix_touches_nothing_else(dtype, layout, rows, h, d, pad):
    """``q | k`` as a column slice (offset ``C`` of pitch ``4C``, offset 0 of pitch ``3C``; ``pad`` more guard columns): in place
    the other columns and the guards keep their bits, out of place ``x`` keeps its bits, and both give the same bits."""
    from anemoi_models_amd import ops

    c = h * d
    col0, total = (c, 4 * c) if layout == "x_r|q|k|v" else (0, 3 * c)
    g = torch.Generator().manual_seed(rows + d)
    full = (2.0 * torch.randn(rows, total, generator=g) + 0.5).to(dtype)
    w = (1.0 + 0.2 * torch.randn(2, d, generator=g)).to(DEV)
    want, bound = R.forward_bound(full[:, col0:col0 + 2 * c].float(), w.cpu(), h, 2, dtype)
    src = Guarded(rows, total, dtype, pad=pad, data=full.to(DEV))
    before = src.raw.clone()
    # out of place, into a guarded result of the same layout
    dst = Guarded(rows, total, dtype, pad=pad)
    y = ops.head_norm(src.view[:, col0:col0 + 2 * c], w, h, 2, out=dst.view[:, col0:col0 + 2 * c])
    assert torch.equal(src.raw, before), "the out-of-place call changed x"
    dst.assert_clean("head_norm out of place")
    rest = torch.ones(total, dtype=torch.bool, device=DEV)
    rest[col0:col0 + 2 * c] = False
    assert bool((_bits(dst.view[:, rest]) == dst.pattern).all()), "columns outside q | k of the result were written"
    assert R.used_fraction(y.float(), want, bound) <= 1.0
    # in place
    out = ops.head_norm(src.view[:, col0:col0 + 2 * c], w, h, 2, out=src.view[:, col0:col0 + 2 * c])
    assert out.data_ptr() == src.view[:, col0:col0 + 2 * c].data_ptr()
    assert _same_bits(out.contiguous(), y.contiguous())
    assert bool(torch.equal(_bits(src.view[:, rest]), _bits(full.to(DEV)[:, rest]))), "x_r / v columns changed"
    flat = src.raw.view(dtype)
    assert bool(torch.isnan(flat[src.outside]).all()) and bool(torch.equal(src.raw[src.outside], before[src.outside]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=IDS)
@pytest.mark.parametrize("rows,groups,h,d", [(37, 2, 3, 4), (130, 1, 5, 12), (200, 2, 16, 64), (65, 1, 4, 128), (50, 2, 4, 96)])
def test_scalar_route_equals_the_vector_route(dtype, rows, groups, h, d):
    """The same values at an odd column offset (no 16-byte alignment: the scalar route) and contiguous (the vector route where
    ``D`` fills 16-byte words): the same bits forward and backward -- every sum is the same balanced tree on both routes."""
    from anemoi_models_amd import ops

    x, w, dy = R.inputs(dtype, rows, groups, h, d, seed=1)
    width = groups * h * d
    x, w, dy = x.to(DEV, dtype), w.to(DEV), dy.to(DEV, dtype)
    y, stats = ops.head_norm(x, w, h, groups, with_stats=True)
    dx, dw = ops.head_norm_backward(dy, x, stats, w, h, groups)
    wide_x = torch.full((rows, width + 5), float("nan"), dtype=dtype, device=DEV)
    wide_dy, wide_y, wide_dx = wide_x.clone(), wide_x.clone(), wide_x.clone()
    wide_x[:, 1:1 + width], wide_dy[:, 3:3 + width] = x, dy
    assert wide_x[:, 1:].data_ptr() % 16 != 0
    y_s, stats_s = ops.head_norm(wide_x[:, 1:1 + width], w, h, groups, out=wide_y[:, 1:1 + width], with_stats=True)
    dx_s, dw_s = ops.head_norm_backward(wide_dy[:, 3:3 + width], wide_x[:, 1:1 + width], stats_s, w, h, groups,
                                        out=wide_dx[:, 3:3 + width])
    assert _same_bits(y_s.contiguous(), y) and _same_bits(stats_s, stats)
    assert _same_bits(dx_s.contiguous(), dx) and _same_bits(dw_s, dw)
    for wide, lo in ((wide_y, 1), (wide_dx, 3)):  # nothing outside the addressed columns was written
        assert bool(torch.isnan(wide[:, :lo]).all()) and bool(torch.isnan(wide[:, lo + width:]).all())


def test_forward_and_backward_captured_in_a_graph_replay_to_the_eager_bits():
    from anemoi_models_amd import ops

    dtype, rows, groups, h, d = torch.bfloat16, 1027, 2, 16, 64
    x, w, dy = R.inputs(dtype, rows, groups, h, d)
    x, w, dy = x.to(DEV, dtype), w.to(DEV), dy.to(DEV, dtype)
    y, stats = ops.head_norm(x, w, h, groups, with_stats=True)
    dx, dw = ops.head_norm_backward(dy, x, stats, w, h, groups)
    xs, dys = torch.zeros_like(x), torch.zeros_like(dy)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # one stream, no parallel branches
        ops.head_norm_backward(dys, xs, ops.head_norm(xs, w, h, groups, with_stats=True)[1], w, h, groups)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gy, gstats = ops.head_norm(xs, w, h, groups, with_stats=True)
        gdx, gdw = ops.head_norm_backward(dys, xs, gstats, w, h, groups)
    xs.copy_(x)
    dys.copy_(dy)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in ((gy, y), (gstats, stats), (gdx, dx), (gdw, dw)):
        assert _same_bits(a, b)


# ------------------------------------------------------------------------------------------------ modules
ATT_FWD = {torch.float32: 2e-5, torch.bfloat16: 2e-2}  # tests/test_gpu_training.py: test_mhsa_backward_vs_torch_autograd
ATT_GRAD = {torch.float32: 1e-4, torch.bfloat16: 3e-2}
GT_TOL = {torch.float32: 2e-3, torch.bfloat16: 8e-2}  # its GraphTransformer block tests


def _mode(monkeypatch, dtype):
    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "fp32" if dtype == torch.float32 else "bf16")


def _randomise_norms(module, seed=0):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in module.named_parameters():
            if "q_norm" in n or "k_norm" in n:
                p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))


def _ref_sd(module, prefix="m"):
    return {f"{prefix}.{k}": (v.detach().double().requires_grad_() if v.is_floating_point() else v.detach())
            for k, v in module.state_dict(keep_vars=True).items()}


def _compare_param_grads(module, rsd, tol, prefix="m"):
    """Every gradient of the restatement against the module's, relative to its own size or 2 % of the largest."""
    wanted = {k: v.grad for k, v in rsd.items() if isinstance(v, torch.Tensor) and v.is_floating_point() and v.grad is not None}
    scale_all = max(float(g.abs().max()) for g in wanted.values())
    seen = []
    for k, p in module.named_parameters():
        want = wanted.get(f"{prefix}.{k}")
        if want is None or float(want.abs().max()) == 0.0:
            continue
        assert p.grad is not None, k
        err = float((p.grad.double().cpu() - want).abs().max())
        assert err <= tol * max(float(want.abs().max()), 0.02 * scale_all), (k, err, float(want.abs().max()))
        seen.append(k)
    return seen


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=IDS)
@pytest.mark.parametrize("b,s,h,d,window", [(2, 70, 4, 32, None), (1, 130, 2, 64, None), (1, 50, 16, 4, None), (1, 130, 2, 64, 20)])
def test_self_attention_module_with_qk_norm(dtype, b, s, h, d, window, monkeypatch):
    from anemoi_models_amd.layers.attention import MultiHeadSelfAttention

    _mode(monkeypatch, dtype)
    if window is not None:
        monkeypatch.setenv("ANEMOI_AMD_FLASH_WINDOW", "1")
    c = h * d
    torch.manual_seed(s + d)
    att = MultiHeadSelfAttention(h, c, window_size=window, qk_norm=True)
    _randomise_norms(att)
    g = torch.Generator().manual_seed(s)
    x0 = torch.randn(b * s, c, generator=g).to(dtype).float()
    dy = torch.randn(b * s, c, generator=g).to(dtype).float()
    rsd = _ref_sd(att)
    xr = x0.double().requires_grad_()
    want = R.mhsa(rsd, "m", xr, b, h, window)
    want.backward(dy.double())
    att = att.to(DEV)
    x = x0.to(DEV).requires_grad_()
    y = att(x, None, b)
    assert y.requires_grad and R.rel_err(y, want) < ATT_FWD[dtype]
    y.backward(dy.to(DEV, y.dtype))
    assert R.rel_err(x.grad, xr.grad) < ATT_GRAD[dtype]
    seen = _compare_param_grads(att, rsd, ATT_GRAD[dtype])
    assert {"q_norm.weight", "k_norm.weight", "lin_qkv.weight", "projection.weight"} <= set(seen)
    with torch.no_grad():
        y_inf = att.eval()(x0.to(DEV), None, b)
    assert R.rel_err(y_inf, want) < ATT_FWD[dtype]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=IDS)
def test_transformer_block_with_qk_norm(dtype, monkeypatch):
    from anemoi_models_amd.layers.block import TransformerProcessorBlock

    _mode(monkeypatch, dtype)
    rows, c, h = 130, 128, 4
    torch.manual_seed(11)
    blk = TransformerProcessorBlock(c, 2 * c, h, "GELU", window_size=None, qk_norm=True)
    _randomise_norms(blk)
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(rows, c, generator=g).to(dtype).float()
    dy = torch.randn(rows, c, generator=g).to(dtype).float()
    rsd = _ref_sd(blk)
    xr = x0.double().requires_grad_()
    want = R.transformer_block(rsd, "m", xr, 1, h)
    want.backward(dy.double())
    blk = blk.to(DEV)
    x = x0.to(DEV).requires_grad_()
    y = blk(x, None, 1)
    assert R.rel_err(y, want) < ATT_FWD[dtype]
    y.backward(dy.to(DEV, y.dtype))
    assert R.rel_err(x.grad, xr.grad) < ATT_GRAD[dtype]
    assert {"attention.q_norm.weight", "attention.k_norm.weight"} <= set(_compare_param_grads(blk, rsd, ATT_GRAD[dtype]))
    with torch.no_grad():
        y_inf = blk.eval()(x0.to(DEV), None, 1)
    assert R.rel_err(y_inf, want) < ATT_FWD[dtype]
    assert R.rel_err(y_inf, y.detach()) < ATT_FWD[dtype]  # inference against the training-route forward


def test_unit_norms_on_standardised_heads_reproduce_the_plain_attention(monkeypatch):
    """The wiring: the module with the switch and unit norm weights equals the plain attention kernel handed q and k whose heads
    torch standardised beforehand -- the norm sits on q and k, between ``lin_qkv`` and the attention, and on nothing else."""
    from anemoi_models_amd import ops
    from anemoi_models_amd.layers.attention import MultiHeadSelfAttention

    _mode(monkeypatch, torch.float32)
    rows, c, h = 130, 128, 4
    torch.manual_seed(2)
    plain, normed = MultiHeadSelfAttention(h, c).to(DEV).eval(), MultiHeadSelfAttention(h, c, qk_norm=True).to(DEV).eval()
    normed.load_state_dict(plain.state_dict(), strict=False)
    x = torch.randn(rows, c, device=DEV)
    with torch.no_grad():
        got = normed(x, None, 1)
        qkv = x @ plain.lin_qkv.weight.T
        qk = torch.nn.functional.layer_norm(qkv[:, :2 * c].reshape(rows, 2 * h, c // h), (c // h,)).reshape(rows, 2 * c)
        pre = torch.cat([qk, qkv[:, 2 * c:]], dim=1).contiguous()  # q, k pre-standardised: what the plain attention is handed
        want = ops.mhsa(pre, 1, h) @ plain.projection.weight.T + plain.projection.bias
    assert R.rel_err(got, want) < ATT_FWD[torch.float32]


def test_block_with_unit_norms_equals_the_plain_block_on_standardised_heads(monkeypatch):
    """The block's own call site: a ``TransformerProcessorBlock(qk_norm=True)`` with unit norm weights equals the plain block run
    op by op with the q and k heads of its ``lin_qkv`` product standardised by torch in the norm's place."""
    from anemoi_models_amd.layers.block import TransformerProcessorBlock

    _mode(monkeypatch, torch.float32)
    rows, c, h = 130, 128, 4
    torch.manual_seed(4)
    kw = dict(num_channels=c, hidden_dim=2 * c, num_heads=h, activation="GELU", window_size=None)
    plain, normed = TransformerProcessorBlock(**kw).to(DEV).eval(), TransformerProcessorBlock(**kw, qk_norm=True).to(DEV).eval()
    normed.load_state_dict(plain.state_dict(), strict=False)
    plain.block_abi = False  # op by op: the route that passes the product through the attention's norm hook

    def standardise_(qkv):
        qk = torch.nn.functional.layer_norm(qkv[:, :2 * c].float().reshape(rows, 2 * h, c // h), (c // h,))
        qkv[:, :2 * c] = qk.reshape(rows, 2 * c).to(qkv.dtype)
        return qkv

    plain.attention.norm_qk_ = standardise_
    x = torch.randn(rows, c, device=DEV)
    with torch.no_grad():
        got, want = normed(x, None, 1), plain(x, None, 1)
    assert R.rel_err(got, want) < ATT_FWD[torch.float32]


def _graph(n_src, n_dst, e, edge_dim, seed):
    g = torch.Generator().manual_seed(seed)
    ei = torch.stack([torch.randint(0, n_src, (e,), generator=g), torch.randint(0, n_dst - 1, (e,), generator=g)])
    return ei, torch.randn(e, edge_dim, generator=g)


GT_SHAPES = [(torch.float32, 64, 16, 3), (torch.bfloat16, 128, 16, 11), (torch.float32, 96, 8, 11)]


@pytest.mark.parametrize("edges", [300, 0])
@pytest.mark.parametrize("dtype,c,h,edge_dim", GT_SHAPES, ids=IDS)
def test_graph_transformer_processor_block_with_qk_norm(dtype, c, h, edge_dim, edges, monkeypatch):
    from anemoi_models_amd.layers.block import GraphTransformerProcessorBlock

    _mode(monkeypatch, dtype)
    tol, n = GT_TOL[dtype], 70
    torch.manual_seed(c + h)
    blk = GraphTransformerProcessorBlock(c, 2 * c, c, edge_dim=edge_dim, num_heads=h, qk_norm=True)
    _randomise_norms(blk)
    ei, ea0 = _graph(n, n, edges, edge_dim, c)
    x0 = torch.randn(n, c, generator=torch.Generator().manual_seed(edge_dim))
    rsd = _ref_sd(blk)
    xr, ear = x0.double().requires_grad_(), ea0.double().requires_grad_()
    want = R.gt_processor_block(rsd, "m", xr, ear, ei, h)
    want.sum().backward()
    blk = blk.to(DEV)
    x, ea = x0.to(DEV).requires_grad_(), ea0.to(DEV).requires_grad_()
    y, _ = blk(x, ea, ei.to(DEV), None, 1)
    assert R.rel_err(y, want) < tol
    y.float().sum().backward()
    assert R.rel_err(x.grad, xr.grad) < tol
    seen = _compare_param_grads(blk, rsd, tol)
    if edges:
        assert R.rel_err(ea.grad, ear.grad) < tol
        assert {"q_norm.weight", "k_norm.weight", "lin_query.weight", "lin_key.weight", "lin_edge.weight"} <= set(seen)
    with torch.no_grad():
        y_inf, _ = blk.eval()(x0.to(DEV), ea0.to(DEV), ei.to(DEV), None, 1)
    assert R.rel_err(y_inf, want) < tol


@pytest.mark.parametrize("dtype,c,h,edge_dim", GT_SHAPES, ids=IDS)
def test_graph_transformer_mapper_block_with_qk_norm(dtype, c, h, edge_dim, monkeypatch):
    from anemoi_models_amd.layers.block import GraphTransformerMapperBlock

    _mode(monkeypatch, dtype)
    tol, n_src, n_dst = GT_TOL[dtype], 45, 70
    torch.manual_seed(c + h + 1)
    blk = GraphTransformerMapperBlock(c, 2 * c, c, edge_dim=edge_dim, num_heads=h, qk_norm=True)
    _randomise_norms(blk)
    ei, ea0 = _graph(n_src, n_dst, 300, edge_dim, c + 1)
    g = torch.Generator().manual_seed(edge_dim + 1)
    xs0, xd0 = torch.randn(n_src, c, generator=g), torch.randn(n_dst, c, generator=g)
    rsd = _ref_sd(blk)
    xsr, xdr, ear = xs0.double().requires_grad_(), xd0.double().requires_grad_(), ea0.double().requires_grad_()
    want = R.gt_mapper_block(rsd, "m", xsr, xdr, ear, ei, h)
    want.sum().backward()
    blk = blk.to(DEV)
    xs, xd, ea = xs0.to(DEV).requires_grad_(), xd0.to(DEV).requires_grad_(), ea0.to(DEV).requires_grad_()
    (_, y), _ = blk((xs, xd), ea, ei.to(DEV), None, 1, size=(n_src, n_dst))
    assert R.rel_err(y, want) < tol
    y.float().sum().backward()
    assert R.rel_err(xs.grad, xsr.grad) < tol and R.rel_err(xd.grad, xdr.grad) < tol and R.rel_err(ea.grad, ear.grad) < tol
    assert {"q_norm.weight", "k_norm.weight"} <= set(_compare_param_grads(blk, rsd, tol))
    with torch.no_grad():
        (_, y_inf), _ = blk.eval()((xs0.to(DEV), xd0.to(DEV)), ea0.to(DEV), ei.to(DEV), None, 1, size=(n_src, n_dst))
    assert R.rel_err(y_inf, want) < tol


@pytest.mark.parametrize("which", ["forward", "backward"])
def test_mappers_with_qk_norm_on_folded_embeddings(graph_o32, which, monkeypatch):
    """bf16, few input features (``2 (in + 1) <= hidden``): the mappers hand the block ``EmbeddedRows`` -- the embedding folded
    into the block's first products -- and the block takes the unfolded route."""
    from anemoi_models_amd.layers.mapper import GraphTransformerBackwardMapper, GraphTransformerForwardMapper

    _mode(monkeypatch, torch.bfloat16)
    tol, hidden, heads = GT_TOL[torch.bfloat16], 128, 16
    n_grid, n_mesh = graph_o32["data"].num_nodes, graph_o32["hidden"].num_nodes
    attrs = ["edge_length", "edge_dirs"]
    torch.manual_seed(3)
    g = torch.Generator().manual_seed(4)
    if which == "forward":
        sub = graph_o32[("data", "to", "hidden")]
        m = GraphTransformerForwardMapper(in_channels_src=20, in_channels_dst=6, hidden_dim=hidden, trainable_size=4,
                                          num_heads=heads, sub_graph=sub, sub_graph_edge_attributes=attrs,
                                          src_grid_size=n_grid, dst_grid_size=n_mesh, qk_norm=True)
        xs0, xd0 = torch.randn(n_grid, 20, generator=g), torch.randn(n_mesh, 6, generator=g)
        ref_fn = R.forward_mapper
    else:
        sub = graph_o32[("hidden", "to", "data")]
        m = GraphTransformerBackwardMapper(in_channels_src=hidden, in_channels_dst=20, hidden_dim=hidden, out_channels_dst=7,
                                           trainable_size=4, num_heads=heads, sub_graph=sub, sub_graph_edge_attributes=attrs,
                                           src_grid_size=n_mesh, dst_grid_size=n_grid, qk_norm=True)
        xs0, xd0 = torch.randn(n_mesh, hidden, generator=g), torch.randn(n_grid, 20, generator=g)
        ref_fn = R.backward_mapper
    _randomise_norms(m)
    with torch.no_grad():
        m.trainable.trainable.normal_(0.0, 0.1)
    assert m.proc.qk_norm and m.proc.fold_width(torch.bfloat16) is None
    attr = torch.cat([sub[a] for a in attrs], dim=1).double()
    rsd = _ref_sd(m)
    xsr, xdr = xs0.double().requires_grad_(), xd0.double().requires_grad_()
    want = ref_fn(rsd, "m", xsr, xdr, attr, sub.edge_index, heads)
    want.sum().backward()
    m = m.to(DEV)
    with torch.no_grad():
        out = m.eval()((xs0.to(DEV), xd0.to(DEV)), 1, None)
    y_inf = out[1] if which == "forward" else out
    assert R.rel_err(y_inf, want) < tol
    xs, xd = xs0.to(DEV).requires_grad_(), xd0.to(DEV).requires_grad_()
    out = m.train()((xs, xd), 1, None)
    y = out[1] if which == "forward" else out
    assert R.rel_err(y, want) < tol
    y.float().sum().backward()
    assert R.rel_err(xd.grad, xdr.grad) < tol and R.rel_err(xs.grad, xsr.grad) < tol
    assert {"proc.q_norm.weight", "proc.k_norm.weight"} <= set(_compare_param_grads(m, rsd, tol))


@pytest.mark.parametrize("processor", ["GraphTransformer", "Transformer"])
def test_flat_model_with_qk_norm_everywhere(graph_o32, processor):
    """qk_norm in encoder, processor and decoder: inference and one training step against the f64 restatement, at the bounds of
    the whole-model tests without it (1e-4 on the output, 5e-3 on the gradients: tests/test_gpu_training.py, f32)."""
    from test_oracle_golden import graph_tensors
    from test_qk_norm_cpu import _model

    torch.manual_seed(21)
    model = _model(graph_o32, processor, channels=64, layers=4)
    _randomise_norms(model)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("trainable"):
                p.normal_(0.0, 0.1)
    for mod in model.modules():
        if hasattr(mod, "dropout_p"):
            mod.dropout_p = 0.0
    n_grid = graph_o32["data"].num_nodes
    n_var = (model.encoder.emb_nodes_src.in_features - model.node_attributes.attr_ndims["data"]) // 2
    g = torch.Generator().manual_seed(6)
    x0 = torch.randn(1, 2, 1, n_grid, n_var, generator=g)
    graph = {k: (v.double() if v.is_floating_point() else v) for k, v in graph_tensors(graph_o32).items()}
    rsd = _ref_sd(model)
    kw = dict(num_heads=16, num_layers=4, num_chunks=2, prognostic_in=list(range(10)), prognostic_out=list(range(10)))
    want = R.flat_model({k[2:]: v for k, v in rsd.items()}, graph, x0.double(), processor=processor, **kw)
    dy = torch.randn(want.shape, generator=g)
    want.backward(dy.double())
    model = model.to(DEV)
    with torch.no_grad():
        y_inf = model.eval()(x0.to(DEV))
    assert y_inf.shape == want.shape and R.rel_err(y_inf, want) < 1e-4
    y = model.train()(x0.to(DEV))
    assert y.requires_grad and R.rel_err(y, want) < 1e-4
    y.backward(dy.to(DEV))
    seen = _compare_param_grads(model, rsd, 5e-3)
    att = "attention." if processor == "Transformer" else ""
    assert {"encoder.proc.q_norm.weight", "decoder.proc.k_norm.weight", f"processor.proc.1.blocks.1.{att}q_norm.weight"} <= set(seen)


# ------------------------------------------------------------------------------------------------ the launch trail
def _entry_points(t):
    return [n.split(":")[0] for n in t.names()]


def test_trail_lists_head_norm_between_the_qkv_product_and_the_attention(monkeypatch):
    from anemoi_models_amd import trail
    from anemoi_models_amd.layers.block import TransformerProcessorBlock

    _mode(monkeypatch, torch.bfloat16)
    torch.manual_seed(1)
    kw = dict(num_channels=128, hidden_dim=256, num_heads=4, activation="GELU", window_size=None)
    normed = TransformerProcessorBlock(**kw, qk_norm=True).to(DEV).eval()
    today, off = TransformerProcessorBlock(**kw).to(DEV).eval(), TransformerProcessorBlock(**kw, qk_norm=False).to(DEV).eval()
    off.load_state_dict(today.state_dict())
    x = torch.randn(130, 128, device=DEV)
    with torch.no_grad():
        with trail.record() as t_on:
            normed(x, None, 1)
        names = _entry_points(t_on)
        i = names.index("anemoi_mhsa")
        assert names.count("anemoi_head_norm") == 1 and names[i - 1] == "anemoi_head_norm"
        assert names[i - 2].startswith("anemoi_linear")  # the q | k | v product
        # the default: the block without the switch has the trail of the block built without the argument, and no norm
        with trail.record() as t_today:
            y_today = today(x, None, 1)
        with trail.record() as t_off:
            y_off = off(x, None, 1)
        # pinned: the launch list the plain block had before the switch existed
        assert t_off.names() == ["anemoi_layer_norm:out", "anemoi_linear:out", "anemoi_mhsa:out", "anemoi_linear:out",
                                 "anemoi_layer_norm:out", "anemoi_linear:out", "anemoi_linear:out"]
        assert t_off.names() == t_today.names() and "anemoi_head_norm" not in _entry_points(t_off)
        assert [e.digest for e in t_off.entries] == [e.digest for e in t_today.entries] and _same_bits(y_off, y_today)
        # op by op (what the switch makes the block run): the same list with the one entry of the norm taken out
        today.block_abi = False
        with trail.record() as t_ops:
            today(x, None, 1)
        assert [n for n in t_on.names() if not n.startswith("anemoi_head_norm")] == t_ops.names()
        assert len(t_on.names()) == len(t_ops.names()) + 1
