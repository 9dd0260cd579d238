"""The algebra of the raw-row encoder attention against the oracle's mapper-block attention, in
f64 on the CPU: k and v are linear in the raw source row, so ``A_k`` moves to the query and ``A_v`` behind the
aggregation.  Pins the formulas -- the rstd / mean terms of the LayerNorm fold, the bias terms, the lin_edge terms and
the empty-segment case -- independently of any kernel."""

import torch

from _raw_rows_ref import degree_graph, fold_source_side, kernel_reference, raw_row_attention
from oracle import reference_path as ref


def _problem(seed, degrees, n_src=37, k_in=11, c=32, h=4, edge_dim=3):
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)  # noqa: E731
    d = c // h
    rowptr, col, edge_index = degree_graph(degrees, n_src, seed)
    n_dst, e = len(degrees), edge_index.shape[1]
    p = dict(x=rnd(n_src, k_in), emb_w=rnd(c, k_in) / k_in**0.5, emb_b=rnd(c), gamma=1 + 0.2 * rnd(c), beta=0.3 * rnd(c),
             w_k=rnd(c, c) / c**0.5, b_k=rnd(c), w_v=rnd(c, c) / c**0.5, b_v=rnd(c), q=rnd(n_dst, h, d),
             e=rnd(e, h, d) if e else torch.zeros((0, h, d), dtype=torch.float64))
    return p, edge_index, n_dst, h, d


def _oracle(p, edge_index, n_dst, h, d):
    hs = p["x"] @ p["emb_w"].T + p["emb_b"]
    xs = torch.nn.functional.layer_norm(hs, (hs.shape[1],), p["gamma"], p["beta"], 1e-5)
    k = (xs @ p["w_k"].T + p["b_k"]).view(-1, h, d)
    v = (xs @ p["w_v"].T + p["b_v"]).view(-1, h, d)
    return ref.gt_conv(p["q"], k, v, p["e"], edge_index, n_dst), hs


def test_raw_row_attention_equals_the_oracle_in_f64():
    degrees = [0, 1, 3, 70, 0, 16, 17, 1, 104, 5]  # isolated destinations, in-degree 1, in-degree > 64
    p, edge_index, n_dst, h, d = _problem(3, degrees)
    want, hs = _oracle(p, edge_index, n_dst, h, d)
    mean = hs.mean(dim=1)
    rstd = (hs.var(dim=1, unbiased=False) + 1e-5).rsqrt()
    x_aug = torch.cat([p["x"], torch.ones(p["x"].shape[0], 1, dtype=torch.float64)], dim=1)
    ak, sk, bk = fold_source_side(p["w_k"], p["b_k"], p["gamma"], p["beta"], p["emb_w"], p["emb_b"])
    av, sv, bv = fold_source_side(p["w_v"], p["b_v"], p["gamma"], p["beta"], p["emb_w"], p["emb_b"])
    ks = x_aug.shape[1]
    got = raw_row_attention(p["q"], x_aug, rstd, mean, ak.view(h, d, ks), sk.view(h, d), bk.view(h, d), av.view(h, d, ks),
                            sv.view(h, d), bv.view(h, d), p["e"], edge_index, n_dst)
    err = float((got - want).abs().max() / want.abs().max())
    print(f"raw-row attention vs oracle.gt_conv in f64: max rel err {err:.3e}")
    assert err < 1e-12
    assert torch.equal(got[0], torch.zeros_like(got[0])) and torch.equal(got[4], torch.zeros_like(got[4]))  # isolated


def test_kernel_form_centred_embedding_no_mean_term_no_score_bias():
    """The form the kernel implements: the embedding is centred over the channels (``runtime.fold_embedded_layer_norm``), so
    the mean term vanishes; ``q . b_k`` is constant over a destination's in-edges and drops out of the softmax; ``b_v``
    rides on column ``sum_col`` of g; lin_edge enters through u and t.  Same oracle, f64."""
    from anemoi_models_amd import runtime

    degrees = [2, 0, 1, 33, 104, 7]
    p, edge_index, n_dst, h, d = _problem(5, degrees)
    c, k_in = h * d, p["x"].shape[1]
    w_e, b_e = torch.randn(c, 3, dtype=torch.float64), torch.randn(c, dtype=torch.float64)
    attr = torch.randn(edge_index.shape[1], 3, dtype=torch.float64)
    p["e"] = (attr @ w_e.T + b_e).view(-1, h, d)
    want, hs = _oracle(p, edge_index, n_dst, h, d)
    rstd = (hs.var(dim=1, unbiased=False) + 1e-5).rsqrt()
    ks, one_col, sum_col, up = 16, k_in, 15, 4
    f, b, zero = runtime.fold_embedded_layer_norm(torch.cat([p["w_k"], p["w_v"]]), torch.cat([p["b_k"], p["b_v"]]),
                                                  p["gamma"], p["beta"], p["emb_w"], p["emb_b"], ks, one_col, torch.float64)
    assert not zero.any()
    x_aug = torch.zeros(p["x"].shape[0], ks, dtype=torch.float64)
    x_aug[:, :k_in], x_aug[:, one_col] = p["x"], 1.0
    a_k, a_v = f[:c].view(h, d, ks), f[c:].view(h, d, ks).clone()
    a_v[:, :, sum_col] = b[c:].double().view(h, d)
    qt = torch.einsum("hdk,nhd->nhk", a_k, p["q"])
    we = torch.zeros(h, d, up, dtype=torch.float64)  # W_e' = [W_e | b_e]
    we[:, :, :3], we[:, :, 3] = w_e.view(h, d, 3), b_e.view(h, d)
    u = torch.einsum("hda,nhd->nha", we, p["q"])
    attr1 = torch.cat([attr, torch.ones(attr.shape[0], 1, dtype=torch.float64)], dim=1)
    rowptr, col, _ = degree_graph(degrees, p["x"].shape[0], 5)
    g, t = kernel_reference(qt, x_aug, rstd, u, attr1, rowptr, col, d, sum_col)
    got = torch.einsum("hdk,nhk->nhd", a_v, g) + torch.einsum("hda,nha->nhd", we, t)
    err = float((got - want).abs().max() / want.abs().max())
    print(f"kernel form (centred embedding, b_v on sum_col, u / t) vs oracle.gt_conv in f64: max rel err {err:.3e}")
    assert err < 1e-6  # (b' of the fold is returned in f32: its rounding is the floor here)
    assert torch.equal(got[1], torch.zeros_like(got[1]))
