"""Restatements for ``qk_norm`` (csrc/head_norm.hip and the modules that call it), sharing no code with the package.

The operation.  For a row ``r``, a head ``h`` of size ``D`` and ``x`` the query or the key of that row and head::

    mean = (1/D) sum_d x_d      var = (1/D) sum_d (x_d - mean)^2      rstd = 1 / sqrt(var + eps)      y_d = (x_d - mean) rstd w_d

``w [D]`` is shared by all heads and rows, queries use ``q_norm.weight`` and keys ``k_norm.weight``, there is no bias, and the
values, the self term and the projected edge features are untouched.  :func:`head_norm` is that in torch (f64 when handed
f64; gradients come from autograd on it); :func:`mhsa`, :func:`transformer_block`, :func:`gt_processor_block`,
:func:`gt_mapper_block` and :func:`flat_model` are the modules with the norm, from a ``state_dict`` of f64 tensors.

The per-element forward bound (:func:`forward_bound`)::

    |got - want| <= half_ulp(want) + K s,      s = 2^-24 |w_d| (|xhat_d| + rstd max_j |x_j|)

``half_ulp(want)`` is the half-ulp of the storage dtype at ``want``, the one rounding of the result: ``2^(e - 9)`` for bf16 (8
significant bits) and ``2^(e - 25)`` for f32 with ``2^e <= |want| < 2^(e + 1)`` -- between ``2^-9 |want|`` and ``2^-8 |want|`` for
bf16, between ``2^-25 |want|`` and ``2^-24 |want|`` for f32.  (A flat ``2^-9 |want|`` is not a bound of a correctly rounded bf16
result: just above a power of two the rounding alone is twice that, and a plain f32 evaluation rounded to bf16 then shows 1.99
of it.  The exact half-ulp is what the words ask for and is never looser than ``2^-8 |want|`` / ``2^-24 |want|``.)  ``K`` counts
the roundings of the kernel's f32 arithmetic in units of ``u = 2^-24``, with ``L = ceil(log2 D)`` the depth of its sums (every
sum over a head is one balanced tree over the head zero-padded to a power of two)::

    mean      the tree: L u sum|x_j| / D <= L u max|x|;  1 / D rounded and the product rounded: 2 u |mean| <= 2 u max|x|
              -> |d mean| <= (L + 2) u max_j |x_j|, which reaches y_d as  |w_d| rstd (L + 2) u max_j |x_j|
    centring  c_d = x_d - mean, one rounding: u |c_d|, which reaches y_d as  u |w_d| |xhat_d|
    variance  c_d^2 carries 2 u from c_d (the common shift d mean moves the variance in second order only: sum c_d = 0) and
              1 u of its own; the tree of positive terms L u; 1 / D and the product 2 u; + eps 1 u:  (L + 6) u relative
    rsqrt     halves that, and the hardware's own error is at most one ulp = 2 u:  ((L + 6) / 2 + 2) u relative to rstd
    products  c_d rstd and (.) w_d: 2 u

    -> |dy_d| <= u |w_d| ( |xhat_d| (1 + (L + 6) / 2 + 2 + 2)  +  rstd max|x| (L + 2) )  <=  K s,
       K = max((L + 6) / 2 + 5, L + 2) = L / 2 + 8  for every L <= 12

so ``K`` is 9 at ``D = 4`` and 11.5 at ``D = 128``: it grows with the depth of the tree, not with ``D``.  A plain torch f32
evaluation (:func:`emulate`) uses up to 2.1 of the unit ``s`` at the shapes of the tests; the aggregate bounds are the
project's LayerNorm bounds (tests/test_gpu_cond_ln.py).
"""

import math

import torch

EPS = 1e-5
U32 = 2.0 ** -24
SIGNIFICANT_BITS = {torch.float32: 24, torch.bfloat16: 8}
FWD_TOL = {torch.float32: 1e-5, torch.bfloat16: 1e-2}
GRAD_TOL = {torch.float32: 1e-4, torch.bfloat16: 3e-2}

F32_CASES = [(1, 1, 1, 4), (37, 2, 3, 4), (33, 2, 2, 5), (130, 1, 5, 12), (257, 2, 16, 32), (200, 2, 16, 64), (65, 1, 4, 128),
             (4100, 2, 16, 64)]
BF16_CASES = [(37, 2, 3, 4), (33, 2, 2, 5), (130, 1, 5, 12), (257, 2, 16, 32), (200, 2, 16, 64), (1027, 2, 16, 64), (65, 1, 4, 128),
              (4100, 2, 16, 64)]
CASES = [(torch.float32, *c) for c in F32_CASES] + [(torch.bfloat16, *c) for c in BF16_CASES]


def name(dtype) -> str:
    return "f32" if dtype == torch.float32 else "bf16"


def rel_err(got, want) -> float:
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def inputs(dtype, rows, groups, h, d, seed=0):
    """``(x, w, dy)``: ``x = 2 randn + 0.5`` and ``dy = randn`` rounded to ``dtype`` and held in f32 (the reference sees what the
    kernel sees), ``w = 1 + 0.2 randn`` f32 ``[groups, d]``."""
    g = torch.Generator().manual_seed(7919 * seed + 131 * rows + 17 * groups + 5 * h + d)
    x = (2.0 * torch.randn(rows, groups * h * d, generator=g) + 0.5).to(dtype).float()
    w = 1.0 + 0.2 * torch.randn(groups, d, generator=g)
    dy = torch.randn(rows, groups * h * d, generator=g).to(dtype).float()
    return x, w, dy


def head_norm(x, w, num_heads: int, groups: int = 1, eps: float = EPS):
    """The norm of every head of ``x [rows, groups * H * D]`` with ``w [groups, D]``, in ``x``'s dtype."""
    rows = x.shape[0]
    xh = x.reshape(rows, groups, num_heads, -1)
    mean = xh.mean(dim=-1, keepdim=True)
    var = ((xh - mean) ** 2).mean(dim=-1, keepdim=True)
    y = (xh - mean) / torch.sqrt(var + eps) * w.reshape(1, groups, 1, -1)
    return y.reshape(rows, -1)


def stats(x, num_heads: int, groups: int = 1, eps: float = EPS):
    """``[rows, groups * H, 2] = (rstd, -mean rstd)``."""
    xh = x.reshape(x.shape[0], groups * num_heads, -1)
    mean = xh.mean(dim=-1)
    rstd = 1.0 / torch.sqrt(((xh - mean[..., None]) ** 2).mean(dim=-1) + eps)
    return torch.stack([rstd, -mean * rstd], dim=-1)


_REF = {}


def reference(dtype, rows, groups, h, d):
    """``(y, dx, dw, stats)`` in f64 for the case's :func:`inputs`, computed once."""
    key = (dtype, rows, groups, h, d)
    if key not in _REF:
        x, w, dy = inputs(dtype, rows, groups, h, d)
        xl, wl = x.double().requires_grad_(), w.double().requires_grad_()
        y = head_norm(xl, wl, h, groups)
        y.backward(dy.double())
        _REF[key] = (y.detach(), xl.grad, wl.grad, stats(x.double(), h, groups))
    return _REF[key]


def bound_k(d: int) -> float:
    return math.ceil(math.log2(d)) / 2.0 + 8.0 if d > 1 else 8.0


def half_ulp(want, dtype):
    """Half a unit in the last place of ``dtype`` at every element of ``want`` (f64): ``2^(e - bits - 1)`` for
    ``2^e <= |want| < 2^(e + 1)``, 0 at 0."""
    _, e = torch.frexp(want.abs())  # |want| = m 2^e with m in [0.5, 1)
    return torch.where(want == 0, torch.zeros_like(want), torch.ldexp(torch.ones_like(want), e - 1 - SIGNIFICANT_BITS[dtype]))


def forward_bound(x, w, num_heads: int, groups: int, dtype, eps: float = EPS):
    """``(want, bound)`` per element in f64 for ``x`` (f32 values of ``dtype``) and ``w``."""
    x, w = x.double(), w.double()
    rows = x.shape[0]
    d = x.shape[1] // (groups * num_heads)
    want = head_norm(x, w, num_heads, groups, eps)
    xh = x.reshape(rows, groups, num_heads, d)
    mean = xh.mean(dim=-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((xh - mean) ** 2).mean(dim=-1, keepdim=True) + eps)
    xhat = (xh - mean) * rstd
    s = U32 * w.reshape(1, groups, 1, d).abs() * (xhat.abs() + rstd * xh.abs().amax(dim=-1, keepdim=True))
    return want, half_ulp(want, dtype) + bound_k(d) * s.reshape(rows, -1)


def used_fraction(got, want, bound) -> float:
    """The worst ``|got - want| / bound`` (``inf`` for a non-finite result)."""
    got = got.detach().double().cpu()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - want).abs() / bound).max())


FAULTS_FORWARD = ("var_d_minus_1", "no_eps", "rms", "offset_one", "k_with_q_weight")
FAULTS_BACKWARD = ("dw_both_groups", "dw_row_dropped", "dx_without_projection")


def emulate(x, w, num_heads: int, groups: int = 1, eps: float = EPS, fault=None, dtype=torch.float32):
    """A plain torch f32 evaluation of the forward, the result rounded to ``dtype`` -- the calibration of the bound -- and, with
    ``fault``, one of the mistakes a kernel of this kind can make."""
    x, w = x.float(), w.float()
    rows = x.shape[0]
    d = x.shape[1] // (groups * num_heads)
    if fault == "offset_one":  # statistics taken across a head boundary
        flat = torch.roll(x, -1, dims=1).reshape(rows, groups, num_heads, d)
    else:
        flat = x.reshape(rows, groups, num_heads, d)
    mean = flat.mean(dim=-1, keepdim=True)
    if fault == "rms":
        mean = torch.zeros_like(mean)
    c = flat - mean
    var = (c * c).sum(dim=-1, keepdim=True) / (d - 1 if fault == "var_d_minus_1" else d)
    rstd = torch.rsqrt(var + (0.0 if fault == "no_eps" else eps))
    wv = w.reshape(1, groups, 1, d)
    if fault == "k_with_q_weight":
        wv = wv[:, :1].expand(1, groups, 1, d)
    y = (x.reshape(rows, groups, num_heads, d) - mean) * rstd * wv
    return y.reshape(rows, -1).to(dtype).float()


def emulate_backward(x, w, dy, num_heads: int, groups: int = 1, eps: float = EPS, fault=None, dtype=torch.float32):
    """``(dx, dw)`` the same way: ``g = dy w``, ``dx = rstd (g - mean g - xhat mean(g xhat))``, ``dw = sum dy xhat``."""
    x, w, dy = x.float(), w.float(), dy.float()
    rows = x.shape[0]
    d = x.shape[1] // (groups * num_heads)
    xh = x.reshape(rows, groups, num_heads, d)
    mean = xh.mean(dim=-1, keepdim=True)
    rstd = torch.rsqrt(((xh - mean) ** 2).mean(dim=-1, keepdim=True) + eps)
    xhat = (xh - mean) * rstd
    dyh = dy.reshape(rows, groups, num_heads, d)
    g = dyh * w.reshape(1, groups, 1, d)
    proj = 0.0 if fault == "dx_without_projection" else xhat * (g * xhat).mean(dim=-1, keepdim=True)
    dx = rstd * (g - g.mean(dim=-1, keepdim=True) - proj)
    terms = dyh * xhat
    if fault == "dw_row_dropped":
        terms = terms[:-1] if rows > 1 else terms * 0.0
    dw = terms.sum(dim=(0, 2))
    if fault == "dw_both_groups":
        dw = dw.sum(dim=0, keepdim=True).expand(groups, d)
    return dx.reshape(rows, -1).to(dtype).float(), dw


# ------------------------------------------------------------------------------------------------ modules, f64
def _lin(sd, p, x):
    y = x @ sd[p + ".weight"].T
    return y + sd[p + ".bias"] if p + ".bias" in sd else y


def _ln(sd, p, x, eps=1e-5):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), sd[p + ".weight"], sd[p + ".bias"], eps)


def _act(name):
    return {"GELU": torch.nn.functional.gelu, "SiLU": torch.nn.functional.silu, "ReLU": torch.relu}[name]


def _qk(sd, p, q, k, num_heads):
    """q and k ``[n, H * D]`` normalised where the block ``p`` carries the norms."""
    if p + ".q_norm.weight" not in sd:
        return q, k
    return (head_norm(q, sd[p + ".q_norm.weight"][None], num_heads), head_norm(k, sd[p + ".k_norm.weight"][None], num_heads))


def mhsa(sd, p, x, batch_size: int, num_heads: int, window=None):
    """``MultiHeadSelfAttention``: scores ``qhat . khat / sqrt D``; ``window``: key j visible from query i iff ``|i - j| <= w``."""
    c = x.shape[1]
    d = c // num_heads
    q, k, v = _lin(sd, p + ".lin_qkv", x).chunk(3, -1)
    q, k = _qk(sd, p, q, k, num_heads)
    s_len = x.shape[0] // batch_size
    q, k, v = (t.reshape(batch_size, s_len, num_heads, d).permute(0, 2, 1, 3) for t in (q, k, v))
    sc = q @ k.transpose(-1, -2) / math.sqrt(d)
    if window is not None:
        i = torch.arange(s_len)
        sc = sc.masked_fill((i[:, None] - i[None, :]).abs() > window, float("-inf"))
    out = (torch.softmax(sc, dim=-1) @ v).permute(0, 2, 1, 3).reshape(batch_size * s_len, c)
    return _lin(sd, p + ".projection", out)


def transformer_block(sd, p, x, batch_size: int, num_heads: int, act="GELU", window=None):
    x = x + mhsa(sd, p + ".attention", _ln(sd, p + ".layer_norm1", x), batch_size, num_heads, window)
    return x + _lin(sd, p + ".mlp.2", _act(act)(_lin(sd, p + ".mlp.0", _ln(sd, p + ".layer_norm2", x))))


def _conv(q, k, v, e, edge_index, n_dst: int, num_heads: int):
    """Scores ``qhat . (khat + e) / sqrt D`` per edge and head, softmax over the edges of a destination, values ``v + e``."""
    src, dst = edge_index[0], edge_index[1]
    d = q.shape[1] // num_heads
    qh, kh, vh, eh = (t.reshape(t.shape[0], num_heads, d) for t in (q, k, v, e))
    kj = kh[src] + eh
    alpha = (qh[dst] * kj).sum(-1) / math.sqrt(d)
    top = torch.full((n_dst, num_heads), float("-inf"), dtype=alpha.dtype).scatter_reduce(
        0, dst[:, None].expand_as(alpha), alpha, "amax", include_self=True)
    ex = torch.exp(alpha - top[dst])
    den = torch.zeros((n_dst, num_heads), dtype=alpha.dtype).index_add(0, dst, ex)
    msg = (vh[src] + eh) * (ex / den[dst])[..., None]
    return torch.zeros((n_dst, num_heads, d), dtype=alpha.dtype).index_add(0, dst, msg).reshape(n_dst, num_heads * d)


def _gt_tail(sd, p, out, x_r, x_skip, act):
    y = _lin(sd, p + ".projection", out + x_r) + x_skip
    h = _act(act)(_lin(sd, p + ".node_dst_mlp.1", _ln(sd, p + ".node_dst_mlp.0", y)))
    return _lin(sd, p + ".node_dst_mlp.3", h) + y


def gt_processor_block(sd, p, x, edge_attr, edge_index, num_heads: int, act="GELU"):
    xh = _ln(sd, p + ".layer_norm1", x)
    q, k = _qk(sd, p, _lin(sd, p + ".lin_query", xh), _lin(sd, p + ".lin_key", xh), num_heads)
    out = _conv(q, k, _lin(sd, p + ".lin_value", xh), _lin(sd, p + ".lin_edge", edge_attr), edge_index, x.shape[0], num_heads)
    return _gt_tail(sd, p, out, _lin(sd, p + ".lin_self", xh), x, act)


def gt_mapper_block(sd, p, x_src, x_dst, edge_attr, edge_index, num_heads: int, act="GELU"):
    xs, xd = _ln(sd, p + ".layer_norm1", x_src), _ln(sd, p + ".layer_norm2", x_dst)
    q, k = _qk(sd, p, _lin(sd, p + ".lin_query", xd), _lin(sd, p + ".lin_key", xs), num_heads)
    out = _conv(q, k, _lin(sd, p + ".lin_value", xs), _lin(sd, p + ".lin_edge", edge_attr), edge_index, x_dst.shape[0], num_heads)
    return _gt_tail(sd, p, out, _lin(sd, p + ".lin_self", xd), x_dst, act)


def _edges(sd, p, attr):
    tr = sd.get(p + ".trainable.trainable")
    return attr if tr is None else torch.cat([attr, tr], dim=1)


def forward_mapper(sd, p, x_src, x_dst, attr, edge_index, num_heads: int):
    return gt_mapper_block(sd, p + ".proc", _lin(sd, p + ".emb_nodes_src", x_src), _lin(sd, p + ".emb_nodes_dst", x_dst),
                           _edges(sd, p, attr), edge_index, num_heads)


def backward_mapper(sd, p, x_src, x_dst, attr, edge_index, num_heads: int):
    out = gt_mapper_block(sd, p + ".proc", x_src, _lin(sd, p + ".emb_nodes_dst", x_dst), _edges(sd, p, attr), edge_index, num_heads)
    return _lin(sd, p + ".node_data_extractor.1", _ln(sd, p + ".node_data_extractor.0", out))


def flat_model(sd, graph, x, *, num_heads: int, num_layers: int, num_chunks: int, prognostic_in, prognostic_out, processor: str):
    """The flat encoder-processor-decoder model (batch 1, ensemble 1) on GraphTransformer mappers with a GraphTransformer or a
    Transformer processor; ``graph``: ``{enc,proc,dec}_edge_index`` / ``_edge_attr``."""
    b, t, ens, g, v = x.shape
    assert b == 1 and ens == 1

    def attrs(name):
        tr = sd.get(f"node_attributes.trainable_tensors.{name}.trainable")
        return sd[f"node_attributes.latlons_{name}"] if tr is None else torch.cat([sd[f"node_attributes.latlons_{name}"], tr], 1)

    x_data = torch.cat([x.permute(0, 2, 3, 1, 4).reshape(g, t * v), attrs("data")], dim=1)
    x_latent = forward_mapper(sd, "encoder", x_data, attrs("hidden"), graph["enc_edge_attr"], graph["enc_edge_index"], num_heads)
    h = x_latent
    for ci in range(num_chunks):
        for bi in range(num_layers // num_chunks):
            p = f"processor.proc.{ci}.blocks.{bi}"
            if processor == "Transformer":
                h = transformer_block(sd, p, h, 1, num_heads)
            else:
                h = gt_processor_block(sd, p, h, _edges(sd, "processor", graph["proc_edge_attr"]), graph["proc_edge_index"],
                                       num_heads)
    out = backward_mapper(sd, "decoder", h + x_latent, x_data, graph["dec_edge_attr"], graph["dec_edge_index"], num_heads)
    y = out.reshape(1, 1, g, -1).clone()
    y[..., list(prognostic_out)] = y[..., list(prognostic_out)] + x[:, -1, :, :, list(prognostic_in)]
    return y
