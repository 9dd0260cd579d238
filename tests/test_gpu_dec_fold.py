"""The decoder fold on the GPU, kernel and block level.

Kernels: the folded edge kernels without ``x_r`` (plain on a graph with in-degrees 0 / 1 / 3 / 104 among 65 destinations;
runs and groups on a uniform in-degree-3 graph of 65 destinations -- the only graphs those two take) against the same
kernels with the operand, and ``anemoi_raw_row_tail`` against torch, everything bit for bit inside guarded buffers.

Block: ``y`` (projection + residual, in front of the node MLP) of ``GraphTransformerMapperBlock`` on raw destination rows,
route on and off, per element against the f64 restatement of tests/_dec_fold_ref.py.  Measured on an MI355X (maximum
error against f64, parent route / folded route): see profiles/r12_dec_fold.md."""

import pytest
import torch

import _dec_fold_ref as R
from _raw_rows_ref import degree_graph
from test_gpu_linear import BF16, Guarded

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("kernel", ["plain", "runs", "groups3"])
@pytest.mark.parametrize("ks,d,up", R.SHAPES)
def test_edge_kernels_without_x_r_and_the_raw_row_tail(kernel, ks, d, up):
    from anemoi_models_amd import ops

    h, c = R.HEADS, R.HEADS * d
    gen = torch.Generator().manual_seed(ks + up)
    n_src, n_dst = 301, 65
    if kernel == "plain":
        deg = R.degrees(gen, n_dst)
        assert {0, 1, 3, 104} <= set(deg)
        rowptr, col, _ = degree_graph(deg, n_src, ks)
        lists = None
    else:
        rowptr, col, runs, groups = R.uniform3_lists(n_dst, n_src, gen)
        lists = runs if kernel == "runs" else groups
    e = int(rowptr[-1])
    rnd = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    dev = lambda t: t.to(DEV).contiguous()  # noqa: E731
    q, k, v = dev(rnd(n_dst, c).bfloat16()), dev((0.5 * rnd(n_src, c)).bfloat16()), dev(rnd(n_src, c).bfloat16())
    u = dev((0.3 * rnd(n_dst, h * up)).bfloat16())
    attr = rnd(e, up)
    attr[:, up - 1] = 1.0
    attr, rowptr, col = dev(attr), dev(rowptr), dev(col)
    x_r = dev(rnd(n_dst, c).bfloat16())
    x = dev(rnd(n_dst, ks).bfloat16())
    stats = dev(torch.stack([0.5 + torch.rand(n_dst, generator=gen), rnd(n_dst)], dim=1))
    lists = None if lists is None else tuple(dev(t) for t in lists)
    width, k_att = c + h * up, c + h * up + 2 * ks

    def edge(x_r_arg, out, lse):
        return ops.gt_edge_attention_folded(q, k, v, x_r_arg, u, attr, rowptr, col, h, up, out=out, lse=lse, runs=lists)

    def folded_operand():
        g = Guarded(n_dst, k_att, BF16, pad=8)
        lse = torch.full((n_dst, h), float("nan"), device=DEV)
        edge(None, g.view, lse)
        g.assert_clean("edge kernel without x_r")
        assert bool((_bits(g.view[:, width:]) == g.pattern).all()), "the edge kernel wrote behind out | t"
        out_t = g.view[:, :width].clone()
        ops.raw_row_tail(x, stats, g.view[:, width:])
        g.assert_clean("raw-row tail")
        assert _same_bits(g.view[:, :width], out_t), "the tail kernel wrote into out | t"
        return g, lse

    g, lse = folded_operand()
    # the parent kernel: t and lse do not depend on x_r; with an all-zero x_r its out is sum alpha v itself
    lse_p, lse_z = torch.empty(n_dst, h, device=DEV), torch.empty(n_dst, h, device=DEV)
    parent = edge(x_r, torch.zeros(n_dst, width, dtype=BF16, device=DEV), lse_p)
    zero = edge(torch.zeros_like(x_r), torch.zeros(n_dst, width, dtype=BF16, device=DEV), lse_z)
    assert _same_bits(g.view[:, c:width], parent[:, c:]) and _same_bits(lse, lse_p) and _same_bits(lse, lse_z)
    assert _same_bits(g.view[:, :c], zero[:, :c])
    assert not _same_bits(parent[:, :c], zero[:, :c]), "x_r does not reach the parent's out: the comparison shows nothing"
    # the two raw blocks, as torch computes them on the same inputs: one f32 product, one rounding
    assert _same_bits(g.view[:, width:width + ks], (stats[:, :1] * x.float()).to(BF16))
    assert _same_bits(g.view[:, width + ks:], x)
    # a second pair of launches: the same bits everywhere
    g2, lse2 = folded_operand()
    assert torch.equal(g.raw, g2.raw) and _same_bits(lse, lse2)


@pytest.fixture(scope="module")
def measured():
    rows = []
    yield rows
    for row in rows:
        print("[decoder fold, block y vs f64] Ks=%d D=%d up=%d: parent max err %.3e, folded %.3e, ratio %.2f" % row)


@pytest.mark.parametrize("ks,d,up", R.SHAPES)
def test_block_y_against_f64_both_routes(monkeypatch, measured, ks, d, up):
    """``y`` per element against f64 on the same bf16 inputs and f32 parameters; the folded route's maximum error within
    1.5 x the parent route's on the same case (the rule of tests/test_gpu_raw_rows.py, there at 2 x)."""
    from anemoi_models_amd import runtime
    from anemoi_models_amd.layers.block import EmbeddedRows
    from anemoi_models_amd.layers.mlp import linear_native

    case = R.block_case(ks, d, up)
    want = R.reference(case)[0]
    blk, emb = case["blk"].to(DEV), case["emb"].to(DEV)
    blk.block_abi = False  # op by op: y is what _node_mlp receives
    monkeypatch.setattr(blk, "_node_mlp", lambda y, *a, **kw: y)
    x_aug, x_src = case["x_aug"].to(DEV), case["x_src"].to(DEV)
    eps = blk.layer_norm2.eps
    packed = runtime.PackedWeights()

    def run(flag):
        monkeypatch.setenv("ANEMOI_AMD_DEC_FOLD", flag)
        with torch.no_grad():
            fold = blk.dec_fold_route(BF16, ks)
            assert fold == (flag == "1")
            plan, ea = blk._edge_inputs(case["edge_attr"].to(DEV), case["edge_index"].to(DEV), case["n_src"], case["n_dst"], BF16)
            hd = None if fold else linear_native(packed, "emb_nodes_dst", emb, x_aug, stats_eps=eps)
            rows = EmbeddedRows(x_aug, case["one_col"], emb, hd, packed, "emb_nodes_dst")
            _, y = blk.native(x_src, rows, ea, plan, 1)
        torch.cuda.synchronize()
        return y

    y_off, y_on, y_on2 = run("0"), run("1"), run("1")
    assert torch.equal(y_on, y_on2) and not torch.equal(y_on, y_off)
    err = lambda y: float((y.double().cpu() - want).abs().max())  # noqa: E731
    e_off, e_on = err(y_off), err(y_on)
    measured.append((ks, d, up, e_off, e_on, e_on / e_off))
    print(f"Ks={ks} D={d} up={up}: max |y - f64| parent {e_off:.3e}, folded {e_on:.3e}, |y|max {float(want.abs().max()):.3f}")
    assert e_off <= 2.0**-6 * float(want.abs().max())  # the parent itself is a bf16 route, not something else
    assert e_on <= 1.5 * e_off
