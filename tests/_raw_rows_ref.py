"""Plain-torch restatement of the raw-row encoder attention: the edge phase of a mapper block
whose source rows are given as the raw features ``x_j`` they are embedded from, with k and v moved to the destination
side.  Shared by the CPU test that pins the algebra against ``oracle.reference_path`` and by the GPU kernel tests."""

import torch


def segment_softmax(s, dst, n_dst):
    """PyG softmax over the in-edges of every destination: ``exp(s - max) / (sum exp(s - max) + 1e-16)``; s is [E, H]."""
    mx = torch.full((n_dst, s.shape[1]), float("-inf"), dtype=s.dtype)
    mx = mx.scatter_reduce(0, dst[:, None].expand_as(s), s, "amax", include_self=True)
    ex = (s - mx.index_select(0, dst)).exp()
    den = torch.zeros((n_dst, s.shape[1]), dtype=s.dtype).index_add_(0, dst, ex)
    return ex / (den.index_select(0, dst) + 1e-16)


def fold_source_side(w, b, gamma, beta, emb_w, emb_b):
    """``Linear(LayerNorm(emb(x)))`` as the issue writes it: ``rstd (A x_aug) - rstd mean s + b'`` with
    ``x_aug = [x | 1]``.  Returns ``(A [N, K + 1], s [N], b' [N])``."""
    wg = w * gamma[None, :]
    a = torch.cat([wg @ emb_w, (wg @ emb_b)[:, None]], dim=1)
    return a, wg.sum(dim=1), w @ beta + b


def raw_row_attention(q, x_aug, rstd, mean, a_k, s_k, b_k, a_v, s_v, b_v, e, edge_index, n_dst):
    """``sum_j alpha_ij (v_j + e_ij)`` per destination and head without ever forming k or v.

    q [n_dst, H, D]; x_aug [n_src, Ks]; rstd, mean [n_src]; a_* [H, D, Ks], s_* / b_* [H, D]; e [E, H, D] (lin_edge);
    edge_index [2, E] (row 0 = source).  The score uses ``qt = A_k^T q`` and two scalars per (destination, head); the
    value side aggregates ``rstd x`` and ``rstd mean`` and applies ``A_v``, ``s_v``, ``b_v`` once per destination."""
    src, dst = edge_index[0], edge_index[1]
    d = q.shape[-1]
    qt = torch.einsum("hdk,nhd->nhk", a_k, q)  # [n_dst, H, Ks]
    qs = torch.einsum("hd,nhd->nh", s_k, q)
    qb = torch.einsum("hd,nhd->nh", b_k, q)
    xj, rj, mj = x_aug.index_select(0, src), rstd.index_select(0, src), mean.index_select(0, src)
    score = (rj[:, None] * torch.einsum("ehk,ek->eh", qt.index_select(0, dst), xj)
             - (rj * mj)[:, None] * qs.index_select(0, dst) + qb.index_select(0, dst)
             + (q.index_select(0, dst) * e).sum(-1)) / d**0.5
    alpha = segment_softmax(score, dst, n_dst)  # [E, H]
    h = q.shape[1]
    g = torch.zeros((n_dst, h, x_aug.shape[1]), dtype=q.dtype).index_add_(0, dst, alpha[:, :, None] * (rj[:, None] * xj)[:, None, :])
    gm = torch.zeros((n_dst, h), dtype=q.dtype).index_add_(0, dst, alpha * (rj * mj)[:, None])
    asum = torch.zeros((n_dst, h), dtype=q.dtype).index_add_(0, dst, alpha)
    out = torch.einsum("hdk,nhk->nhd", a_v, g) - s_v[None] * gm[:, :, None] + b_v[None] * asum[:, :, None]
    return out + torch.zeros_like(out).index_add_(0, dst, alpha[:, :, None] * e)


def kernel_reference(qt, x, rstd, u, attr, rowptr, col, head_dim, sum_col):
    """What ``anemoi_gt_edge_attention_raw`` computes, in the dtype of its (already rounded) inputs promoted by the
    caller: ``(g [n_dst, H, Ks], t [n_dst, H, up])``.  qt [n_dst, H, Ks], x [n_src, Ks], u [n_dst, H, up], attr [E, up]
    in CSR order."""
    n_dst = rowptr.shape[0] - 1
    dst = torch.repeat_interleave(torch.arange(n_dst), (rowptr[1:] - rowptr[:-1]).long())
    src = col.long()
    xj, rj = x.index_select(0, src), rstd.index_select(0, src)
    score = (rj[:, None] * torch.einsum("ehk,ek->eh", qt.index_select(0, dst), xj)
             + torch.einsum("eha,ea->eh", u.index_select(0, dst), attr)) / head_dim**0.5
    alpha = segment_softmax(score, dst, n_dst)
    h = qt.shape[1]
    g = torch.zeros((n_dst, h, x.shape[1]), dtype=qt.dtype).index_add_(0, dst, alpha[:, :, None] * (rj[:, None] * xj)[:, None, :])
    t = torch.zeros((n_dst, h, attr.shape[1]), dtype=qt.dtype).index_add_(0, dst, alpha[:, :, None] * attr[:, None, :])
    if sum_col >= 0:
        g[:, :, sum_col] = torch.zeros((n_dst, h), dtype=qt.dtype).index_add_(0, dst, alpha)
    return g, t


def degree_graph(degrees, n_src, seed):
    """CSR (rowptr int32, col int32) and edge_index int64 [2, E] of a bipartite graph with the given in-degrees."""
    gen = torch.Generator().manual_seed(seed)
    deg = torch.tensor(degrees, dtype=torch.int64)
    rowptr = torch.zeros(len(degrees) + 1, dtype=torch.int64)
    rowptr[1:] = deg.cumsum(0)
    col = torch.randint(0, n_src, (int(rowptr[-1]),), generator=gen)
    dst = torch.repeat_interleave(torch.arange(len(degrees)), deg)
    return rowptr.int(), col.int(), torch.stack([col, dst])
