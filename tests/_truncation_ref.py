"""f64 restatement of the truncated residual connection (``csrc/truncation.hip``, ``layers/truncation.py``) for the tests: dense
matrices or ``torch.sparse`` on the CPU, gradients from torch autograd.  Shares no code with the package."""

import numpy as np
import torch

U = 2.0 ** -24  # unit roundoff of f32


def random_csr(rng, n_out, n_in, lengths, val_scale=1.0):
    """``(indptr int64, idx int32, val f32)`` with row ``i`` of length ``lengths[i]``; column indices ascending within a row
    (repeats allowed where a row is longer than the matrix is wide)."""
    indptr = np.zeros(n_out + 1, dtype=np.int64)
    np.cumsum(lengths, out=indptr[1:])
    idx = np.concatenate([np.sort(rng.choice(n_in, size=n, replace=n > n_in)) for n in lengths] + [np.zeros(0, dtype=np.int64)])
    val = (rng.standard_normal(idx.size) * val_scale).astype(np.float32)
    return torch.from_numpy(indptr), torch.from_numpy(idx.astype(np.int32)), torch.from_numpy(val)


def row_lengths(rng, n_out, choices=(0, 1, 3, 63, 64, 65, 200)):
    """One of each choice at least, the rest drawn from them, shuffled."""
    n = np.concatenate([np.asarray(choices), rng.choice(choices, size=n_out - len(choices), p=_weights(choices))])
    rng.shuffle(n)
    return n.astype(np.int64)


def _weights(choices):  # short rows are the common case of an interpolation matrix; keep the long ones rare
    w = np.asarray([4.0 if c <= 3 else 1.0 for c in choices])
    return w / w.sum()


def dense(indptr, idx, val, n_cols):
    """f64 dense matrix of a CSR (repeated entries add)."""
    n_rows = indptr.numel() - 1
    rows = torch.repeat_interleave(torch.arange(n_rows), indptr[1:] - indptr[:-1])
    m = torch.zeros(n_rows, n_cols, dtype=torch.float64)
    m.index_put_((rows, idx.long()), val.double(), accumulate=True)
    return m


def lengths_of(indptr):
    return (indptr[1:] - indptr[:-1]).double()


def project(m, x):
    """``m [n_out, n_in] @ x [..., n_in, P]`` in f64."""
    return torch.matmul(m, x.double())


def project_with_bound(csr, n_cols, x, y0=None, prior_err=None):
    """``(want, bound)`` of one launch on f64 input ``x [..., n_in, P]``: want = A x (+ y0); bound = 1.01 (L_i + 4) 2^-24 (sum_k
    |val_k| |x_k| + |y0|), the forward error of an L-term f32 FMA recursion plus one rounding each for the affine map and the
    accumulate.  ``prior_err`` (a bound on the error already in x, chained launches) is carried through |A|."""
    m = dense(*csr, n_cols)
    want = project(m, x)
    mag = project(m.abs(), x.abs())
    if y0 is not None:
        want = want + y0.double()
        mag = mag + y0.double().abs()
    bound = 1.01 * (lengths_of(csr[0])[:, None] + 4) * U * mag
    if prior_err is not None:
        bound = bound + 1.01 * project(m.abs(), prior_err)
    return want, bound


def project_with_bound_sparse(csr, x, y0=None):
    """:func:`project_with_bound` without the dense matrix (many output rows): the same want and the same bound, summed
    entry by entry in f64."""
    indptr, idx, val = csr
    n_out = indptr.numel() - 1
    rows = torch.repeat_interleave(torch.arange(n_out), indptr[1:] - indptr[:-1])
    terms = val.double()[:, None] * x.double()[..., idx.long(), :]
    shape = tuple(x.shape[:-2]) + (n_out, x.shape[-1])
    want = torch.zeros(shape, dtype=torch.float64).index_add_(-2, rows, terms)
    mag = torch.zeros(shape, dtype=torch.float64).index_add_(-2, rows, terms.abs())
    if y0 is not None:
        want = want + y0.double()
        mag = mag + y0.double().abs()
    return want, 1.01 * (lengths_of(indptr)[:, None] + 4) * U * mag


def truncated_residual(out, x, mats, out_idx, in_idx):
    """``y = out`` with ``y[..., out_idx] += A_up (A_down x[:, -1, ..., in_idx])`` in f64; ``mats``: dense f64 stages in the order
    they are applied.  Differentiable with respect to ``out`` and ``x``."""
    skip = x[:, -1].double().index_select(-1, in_idx)
    for m in mats:
        skip = torch.matmul(m, skip)
    res = torch.zeros_like(out, dtype=torch.float64).index_add(-1, out_idx, skip)
    return out.double() + res


def upstream_style(out, x, sparse_mats, out_idx, in_idx):
    """The composition of current anemoi-models: per batch entry, every variable through ``torch.sparse.mm``, then the
    prognostic columns selected.  ``x [B, T, E, G, V_in]``, ``out [B, E, G, V_out]``, ``sparse_mats`` f64 sparse stages."""
    b, _, e, g, v = x.shape
    last = x[:, -1].double().reshape(b * e, g, v)
    rows = []
    for i in range(b * e):
        s = last[i]
        for m in sparse_mats:
            s = torch.sparse.mm(m, s)
        rows.append(s)
    skip = torch.stack(rows).reshape(b, e, g, v)
    y = out.double().clone()
    y[..., out_idx] += skip[..., in_idx]
    return y
