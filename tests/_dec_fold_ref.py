"""Cases and f64 restatements for the decoder fold: the mapper block's projection with ``x_r`` and
the embedded destination rows folded in.  Shared by tests/test_dec_fold_cpu.py (the cases keep the parent route's own
error away from zero) and tests/test_gpu_dec_fold.py (kernels and block against these references)."""

import torch
from torch import nn

from _raw_rows_ref import degree_graph, segment_softmax

SHAPES = [(256, 64, 4), (128, 64, 4), (64, 32, 8)]  # (K_s, D, up), 16 heads
HEADS = 16
DEGREES = [0, 1, 104, 16, 17, 3, 0, 32, 15, 1, 64, 9]


def degrees(gen, n=65):
    return DEGREES + [int(v) for v in torch.randint(0, 40, (n - len(DEGREES),), generator=gen)]


def uniform3_lists(n_dst, n_src, gen):
    """A uniform in-degree-3 graph whose destinations share source triples, consecutively (runs) and apart (groups), with
    the lists of ``runtime._runs3`` / ``runtime._groups3`` built by their rules (which decline graphs this small):
    ``(rowptr, col, (run_ptr, run_perm), (grp_ptr, grp_perm, grp_dst))``."""
    base = (torch.arange(n_dst) // 2) % 7  # pairs of neighbours share a triple; every triple comes back ~9 times
    tri = torch.stack([base, base + 7, base + 20], 1)
    assert int(tri.max()) < n_src
    order = torch.stack([torch.randperm(3, generator=gen) for _ in range(n_dst)])
    src = torch.gather(tri, 1, order)
    rowptr = torch.arange(0, 3 * n_dst + 1, 3, dtype=torch.int32)
    srt, pos = torch.sort(src, dim=1, stable=True)
    perm = pos[:, 0] | (pos[:, 1] << 2) | (pos[:, 2] << 4)
    idx = torch.arange(n_dst)

    def cut(start, cap):
        first = torch.cummax(torch.where(start, idx, torch.zeros_like(idx)), 0).values
        return torch.nonzero(start | (((idx - first) % cap) == 0)).flatten()

    start = torch.ones(n_dst, dtype=torch.bool)
    start[1:] = (srt[1:] != srt[:-1]).any(dim=1)
    begin = cut(start, 2)
    run_ptr = torch.cat([begin, torch.tensor([n_dst])])
    lens = run_ptr[1:] - run_ptr[:-1]
    packed = perm[begin].clone()
    two = lens > 1
    packed[two] |= perm[(begin + 1)[two]] << 6
    key = (srt[:, 0] * n_src + srt[:, 1]) * n_src + srt[:, 2]
    by_key = torch.argsort(key, stable=True)
    sk = key[by_key]
    gstart = torch.ones(n_dst, dtype=torch.bool)
    gstart[1:] = sk[1:] != sk[:-1]
    gbegin = cut(gstart, 8)
    grp_ptr = torch.cat([gbegin, torch.tensor([n_dst])])
    assert int((grp_ptr[1:] - grp_ptr[:-1]).max()) == 8 and int(lens.max()) == 2
    i32 = lambda t: t.to(torch.int32).contiguous()  # noqa: E731
    return rowptr, i32(src.reshape(-1)), (i32(run_ptr), i32(packed)), (i32(grp_ptr), i32(perm[by_key]), i32(by_key))


def block_case(ks, d, up, seed=None):
    """One mapper block on raw destination rows: the block and the destination embedding (f32 parameters, LayerNorms away
    from the identity), bf16 inputs, a graph with in-degrees 0 / 1 / 3 / 104 among its 65 destinations."""
    from anemoi_models_amd.layers.block import GraphTransformerMapperBlock

    seed = ks + up if seed is None else seed
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    c, k_in, edge_dim = HEADS * d, ks - 9, up - 1
    blk = GraphTransformerMapperBlock(c, 2 * c, c, edge_dim=edge_dim, num_heads=HEADS).eval()
    emb = nn.Linear(k_in, c)
    with torch.no_grad():
        for ln in (blk.layer_norm1, blk.layer_norm2):
            ln.weight.add_(0.2 * torch.randn(c, generator=gen))
            ln.bias.add_(0.2 * torch.randn(c, generator=gen))
    deg = degrees(gen)
    n_src, n_dst = 301, len(deg)
    _, _, edge_index = degree_graph(deg, n_src, seed)
    x = torch.zeros(n_dst, ks)
    x[:, :k_in], x[:, k_in] = torch.randn(n_dst, k_in, generator=gen), 1.0
    return dict(blk=blk, emb=emb, c=c, d=d, up=up, ks=ks, k_in=k_in, one_col=k_in, n_src=n_src, n_dst=n_dst, degrees=deg,
                edge_index=edge_index, x_aug=x.bfloat16(), x_src=torch.randn(n_src, c, generator=gen).bfloat16(),
                edge_attr=torch.randn(edge_index.shape[1], edge_dim, generator=gen))


def reference(case):
    """The block's ``y = projection(conv + lin_self(LN2 h)) + h``, ``h = emb(x)``, in f64 on the case's inputs and f32
    parameters -- with the pieces the two routes round on the way: ``(y, h, x_r, S = sum alpha v, t = sum alpha [a | 1],
    rstd of LN2)``."""
    blk, emb = case["blk"], case["emb"]
    sd = {k: v.detach().double() for k, v in blk.state_dict().items()}
    lin = lambda p, t: t @ sd[p + ".weight"].T + sd[p + ".bias"]  # noqa: E731
    h_, d, n_src, n_dst = HEADS, case["d"], case["n_src"], case["n_dst"]
    x = case["x_aug"].double()[:, :case["k_in"]]
    h = x @ emb.weight.detach().double().T + emb.bias.detach().double()

    def ln(p, t):
        mean, var = t.mean(1, keepdim=True), t.var(1, unbiased=False, keepdim=True)
        rstd = (var + 1e-5).rsqrt()
        return (t - mean) * rstd * sd[p + ".weight"] + sd[p + ".bias"], rstd

    hd, rstd = ln("layer_norm2", h)
    hs, _ = ln("layer_norm1", case["x_src"].double())
    x_r = lin("lin_self", hd)
    q = lin("lin_query", hd).view(n_dst, h_, d)
    k, v = lin("lin_key", hs).view(n_src, h_, d), lin("lin_value", hs).view(n_src, h_, d)
    attr = case["edge_attr"].double()
    e = lin("lin_edge", attr).view(-1, h_, d)
    src, dst = case["edge_index"][0], case["edge_index"][1]
    score = (q.index_select(0, dst) * (k.index_select(0, src) + e)).sum(-1) / d**0.5
    alpha = segment_softmax(score, dst, n_dst)
    s = torch.zeros(n_dst, h_, d, dtype=torch.float64).index_add_(0, dst, alpha[:, :, None] * v.index_select(0, src))
    a1 = torch.cat([attr, torch.ones(attr.shape[0], 1, dtype=torch.float64),
                    torch.zeros(attr.shape[0], case["up"] - attr.shape[1] - 1, dtype=torch.float64)], 1)
    t = torch.zeros(n_dst, h_, case["up"], dtype=torch.float64).index_add_(0, dst, alpha[:, :, None] * a1[:, None, :])
    conv = s + torch.zeros_like(s).index_add_(0, dst, alpha[:, :, None] * e)
    y = lin("projection", conv.reshape(n_dst, -1) + x_r) + h
    return y, h, x_r, s.reshape(n_dst, -1), t.reshape(n_dst, -1), rstd


def emulate_routes(case):
    """Both routes restated in torch on bf16-rounded operands (products in f64: only the roundings the routes make to
    bf16 are modelled).  Parent: ``bf16(proj(bf16(S + bf16 x_r)) + W_t bf16 t + b + bf16 h)`` with bf16 ``[W_p | W_t]``;
    folded: ``bf16(W [bf16 S | bf16 t | bf16(rstd x) | x] + b)`` with the composed bf16 weight.  Returns the maximum
    errors against the f64 reference ``(parent, folded, max |y|)``."""
    from anemoi_models_amd import runtime

    blk, emb, up = case["blk"], case["emb"], case["up"]
    y, h, x_r, s, t, rstd = reference(case)
    r = lambda z: z.to(torch.bfloat16).double()  # noqa: E731
    w_t = blk._projection_fold(up).double()
    wp, bp = blk.projection.weight.detach().double(), blk.projection.bias.detach().double()
    parent = r(r(s + r(x_r)) @ r(wp).T + r(t) @ r(w_t).T + bp + r(h))
    ln = blk.layer_norm2
    w, b = runtime.compose_decoder_fold(blk.projection.weight, blk.projection.bias, w_t, blk.lin_self.weight, blk.lin_self.bias,
                                        ln.weight, ln.bias, emb.weight, emb.bias, case["ks"], case["one_col"], torch.bfloat16)
    xa = case["x_aug"].double()
    operand = torch.cat([r(s), r(t), r(rstd * xa), xa], dim=1)
    folded = r(operand @ w.double()[:, :operand.shape[1]].T + b.double())
    return float((parent - y).abs().max()), float((folded - y).abs().max()), float(y.abs().max())
