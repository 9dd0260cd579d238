"""Per-layer blocks mirroring reference layers/block.py, executed by the gfx950 kernels.

Class names, constructor kwargs, sub-module names (``state_dict`` keys) and forward signatures follow the
reference; the forward bodies are launch sequences over ``libanemoi_amd.so``:

GraphTransformerProcessorBlock (reference layers/block.py:602-635), per call
    LayerNorm -> ONE GEMM for lin_self|lin_query|lin_key|lin_value -> fused edge attention (+ x_r)
    -> projection GEMM (+ x skip in the epilogue) -> LayerNorm -> GEMM+GELU -> GEMM (+ residual).
GraphTransformerMapperBlock (reference layers/block.py:479-550)
    same with separate source / destination node sets (k|v from the sources, self|q from the destinations).
"""

from __future__ import annotations

import os
from abc import ABC
from abc import abstractmethod
from typing import NamedTuple
from typing import Optional

import torch
from torch import Tensor
from torch import nn

from .. import ops
from .. import runtime
from .. import training
from ..runtime import EdgePlan
from .conv import GraphConv
from .conv import GraphTransformerConv
from .mlp import MLP
from .mlp import NativeSequential
from .mlp import activation_class
from .mlp import fused_activation_name
from .mlp import linear_native
from .normalization import ConditionalLayerNorm


def inference_num_chunks() -> int:
    """``ANEMOI_INFERENCE_NUM_CHUNKS`` (reference layers/block.py:38-39), read at call time."""
    return int(os.environ.get("ANEMOI_INFERENCE_NUM_CHUNKS", "1"))


def _group_size(group) -> int:
    return 1 if group is None else group.size()


def _as_compute(x: Tensor, dtype: torch.dtype) -> Tensor:
    x = x if x.dtype == dtype else x.to(dtype)
    return x if (x.dim() == 2 and x.stride(1) == 1) else x.contiguous()



def folded_edge_phase(q: Tensor, k: Tensor, v: Tensor, x_r: Optional[Tensor], u: Tensor, edge_attr_csr: Tensor, plan,
                      num_heads: int, up: int, ld_out: Optional[int] = None, out: Optional[Tensor] = None) -> Tensor:
    """The folded edge phase (``anemoi_gt_edge_attention_folded``: one fused gather -> score -> segment softmax -> weighted
    sum -> ``+ x_r`` pass over the destination-sorted CSR).  ``out``: the caller's buffer (only ``out | t`` is written)."""
    lists = runtime.edge_lists(plan, q.dtype, q.shape[-1], num_heads, up)
    return ops.gt_edge_attention_folded(q, k, v, x_r, u, edge_attr_csr, plan.rowptr, plan.col, num_heads, up, out=out,
                                        ld_out=ld_out, **lists._asdict())


class EmbeddedRows:
    """Node rows ``h = emb(x)`` handed to a mapper block as the raw features they are embedded from.

    ``x_aug = [x | 1 | 0-pad]`` (the constant-1 column ``one_col`` sits in the K padding and carries the embedding's bias),
    ``emb`` the mapper's ``nn.Linear``.  The block's ``LayerNorm -> Linear`` on these rows then runs as ONE narrow GEMM
    on ``x_aug`` (``runtime.fold_embedded_layer_norm``) instead of a K = C GEMM on ``h``.  ``h`` itself is present only
    when something else needs it (the destination rows: residual of the projection); for source rows that only feed
    k | v it is never formed, and the LayerNorm's row statistics come from a [rows, 256] side product
    (``runtime.embedding_stats_operator``)."""

    def __init__(self, x_aug: Tensor, one_col: int, emb: nn.Linear, h: Optional[Tensor], packed, tag: str) -> None:
        self.x_aug, self.one_col, self.emb, self.h, self._packed, self._tag = x_aug, one_col, emb, h, packed, tag

    @property
    def dtype(self) -> torch.dtype:
        return self.x_aug.dtype

    @property
    def device(self) -> torch.device:
        return self.x_aug.device

    @property
    def shape(self):
        return (self.x_aug.shape[0], self.emb.out_features)

    def stats(self, eps: float) -> Tensor:
        """``{rstd, -mean rstd}`` per row of ``LayerNorm(h)`` (only ``rstd`` is used by the folded product)."""
        if self.h is not None:
            return ops.row_stats(self.h, eps)  # carried by the embedding GEMM's epilogue
        kp = self.x_aug.shape[1]
        t = self._packed.get((self._tag, "embstats", self.dtype, kp, self.one_col), [self.emb.weight, self.emb.bias],
                             lambda: runtime.embedding_stats_operator(self.emb.weight, self.emb.bias, kp, self.one_col,
                                                                      self.dtype))
        # nothing but these statistics is read of T x_aug: the thin kernel can keep the product in registers and store only
        # them.  Measured slower than the persistent kernel + finalize at config 3 (0.189 against 0.132 ms: four waves share a
        # row block and meet at two barriers per block, profiles/r11_thin_hoist.md), so this site is opt-in:
        # ANEMOI_AMD_THIN_STATS=1 (under ANEMOI_AMD_THIN).
        thin = ops.thin_enabled() and runtime.thin_stats_enabled()
        st = ops.linear_thin(self.x_aug, t, stats_eps=eps) if thin else None
        return st if st is not None else ops.row_stats(runtime.linear(self.x_aug, t, None, stats_eps=eps), eps)


class Rows(NamedTuple):
    """What the route decision (``GraphTransformerMapperBlock.route``) knows of one node set before anything is launched.
    ``kind``: ``"tensor"`` (plain rows), ``"embedded"`` (``EmbeddedRows`` with ``h``) or ``"raw"`` (``EmbeddedRows`` that come,
    or -- when a mapper asks before it embeds -- could come, without ``h``).  The other fields describe ``EmbeddedRows``:
    raw width, constant-1 column, the embedding's ``in_features``."""

    kind: str = "tensor"
    k_pad: int = 0
    one_col: int = 0
    in_features: int = 0
    on_gpu: bool = False

    @classmethod
    def of(cls, x) -> "Rows":
        if not isinstance(x, EmbeddedRows):
            return cls("tensor", on_gpu=x.is_cuda)
        return cls("embedded" if x.h is not None else "raw", x.x_aug.shape[1], x.one_col, x.emb.in_features, x.x_aug.is_cuda)


class Route(NamedTuple):
    """Result of ``GraphTransformerMapperBlock.route`` (DESIGN.md section 4.2 has the table of routes)."""

    name: str  # "dec_fold" | "raw_sources" | "folded" | "unfolded"
    up: Optional[int]  # per-head width of the lin_edge fold (``fold_width``), None on the unfolded route
    mx: bool  # the destination nodes' MLP on MXFP8
    chunked: bool  # node MLPs in row chunks; no LayerNorm statistics on the projection's epilogue
    block_tail: bool  # ``anemoi_gt_block_tail`` may run edge phase, projection and node MLP (``_block_tail`` can still refuse)
    src_h: bool  # the route reads the embedded source rows ``h``
    dst_h: bool  # ... the embedded destination rows


class BaseBlock(nn.Module, ABC):
    """Base class for network blocks."""

    @abstractmethod
    def forward(self, x, edge_attr, edge_index, shapes, batch_size, size=None, model_comm_group=None): ...


# =============================================================================================
# Graph transformer blocks
# =============================================================================================
class GraphTransformerBaseBlock(BaseBlock, ABC):
    """Parameters of one graph-transformer layer (reference layers/block.py:289-364)."""

    def __init__(
        self,
        in_channels: int,
        hidden_dim: int,
        out_channels: int,
        edge_dim: int,
        num_heads: int = 16,
        bias: bool = True,
        activation: str = "GELU",
        num_chunks: int = 1,
        update_src_nodes: bool = False,
        qk_norm: bool = False,
        **kwargs,
    ) -> None:
        super().__init__(**kwargs)
        self.update_src_nodes = update_src_nodes
        self.qk_norm = qk_norm
        self.out_channels_conv = out_channels // num_heads
        self.num_heads = num_heads
        self.num_chunks = num_chunks
        self.activation = activation
        self.edge_dim = edge_dim
        width = num_heads * self.out_channels_conv

        self.lin_key = nn.Linear(in_channels, width)
        self.lin_query = nn.Linear(in_channels, width)
        self.lin_value = nn.Linear(in_channels, width)
        self.lin_self = nn.Linear(in_channels, width, bias=bias)
        self.lin_edge = nn.Linear(edge_dim, width)
        self.conv = GraphTransformerConv(out_channels=self.out_channels_conv)
        self.projection = nn.Linear(out_channels, out_channels)
        if qk_norm:  # bias-free LayerNorms over the head dimension of the queries and keys (current anemoi-models)
            self.q_norm = nn.LayerNorm(self.out_channels_conv, bias=False)
            self.k_norm = nn.LayerNorm(self.out_channels_conv, bias=False)

        act = activation_class(activation)
        self.node_dst_mlp = nn.Sequential(
            nn.LayerNorm(out_channels), nn.Linear(out_channels, hidden_dim), act(), nn.Linear(hidden_dim, out_channels)
        )
        self.layer_norm1 = nn.LayerNorm(in_channels)
        if self.update_src_nodes:
            self.node_src_mlp = nn.Sequential(
                nn.LayerNorm(out_channels), nn.Linear(out_channels, hidden_dim), act(),
                nn.Linear(hidden_dim, out_channels),
            )
        self._packed = runtime.PackedWeights()
        self._plans = runtime.PlanCache()
        self._mlps: dict = {}  # "dst" / "src" -> NativeSequential (``_native_mlp``)

    # ---- the reference's head / sequence re-sharding helpers (layers/block.py:366-414) -----------------
    def shard_qkve_heads(self, query: Tensor, key: Tensor, value: Tensor, edges: Tensor, shapes: tuple, batch_size: int,
                         model_comm_group=None):
        """``(batch grid) (heads vars) -> (batch grid) heads vars`` for q, k, v and the projected edge features; with a
        model group, the reference's exchange (layers/block.py:366-399): every tensor goes through ``shard_heads`` -- all
        nodes / edges of the group, this rank's heads -- with ``shapes = (source, destination, edge)`` shard shapes.  (The
        model root does not use it: it partitions by mesh node, ``distributed/partition.py``.)"""
        h, d = self.num_heads, self.out_channels_conv
        if _group_size(model_comm_group) <= 1:
            return tuple(t.reshape(t.shape[0], h, d) for t in (query, key, value, edges))
        from ..distributed.transformer import shard_heads

        assert batch_size == 1, "Only batch size of 1 is supported when model is sharded across GPUs"
        shapes_src, shapes_dst, shapes_edges = shapes
        out = []
        for t, shp in ((query, shapes_dst), (key, shapes_src), (value, shapes_src), (edges, shapes_edges)):
            t = t.reshape(1, t.shape[0], h, d).permute(0, 2, 1, 3)  # batch heads grid vars
            t = shard_heads(t, shapes=shp, mgroup=model_comm_group)
            out.append(t[0].permute(1, 0, 2).contiguous())  # grid heads vars
        return tuple(out)

    def shard_output_seq(self, out: Tensor, shapes: tuple, batch_size: int, model_comm_group=None) -> Tensor:
        """``(batch grid) heads vars -> (batch grid) (heads vars)`` (reference layers/block.py:401-414); with a model
        group the destination rows come back through ``shard_sequence`` (all heads, this rank's rows)."""
        if _group_size(model_comm_group) <= 1:
            return out.reshape(out.shape[0], -1)
        from ..distributed.transformer import shard_sequence

        t = out.permute(1, 0, 2).unsqueeze(0)  # batch heads grid vars
        t = shard_sequence(t, shapes=shapes[1], mgroup=model_comm_group)
        return t[0].permute(1, 0, 2).reshape(t.shape[2], -1).contiguous()

    # ---- packed parameters -------------------------------------------------------------------
    def _cat_linear(self, tag: str, layers, dtype):
        w = self._packed.get((tag, "w", dtype), [l.weight for l in layers],
                             lambda: runtime.pack_weight([l.weight for l in layers], dtype))
        b = self._packed.get((tag, "b"), [l.bias for l in layers],
                             lambda: runtime.pack_bias([l.bias for l in layers], [l.out_features for l in layers],
                                                       layers[0].weight.device))
        return w, b

    # ---- LayerNorm -> Linear pairs: row statistics + anemoi_linear_ln (the normalised activation is never stored)
    @staticmethod
    def _ln_begin(ln: nn.LayerNorm, x: Tensor):
        """Handle of ``LayerNorm(x)`` for ``_ln_product``: ``(x, stats, ln)`` when folding, else ``(LN(x), None, None)``."""
        if isinstance(x, EmbeddedRows):
            return x, x.stats(ln.eps), ln
        if runtime.ln_fold_enabled(x.dtype):
            return x, ops.row_stats(x, ln.eps), ln
        return ops.layer_norm(x, runtime.f32c(ln.weight), runtime.f32c(ln.bias), ln.eps), None, None

    def _ln_product(self, handle, tag: str, layers, up: Optional[int] = None, **kw) -> Tensor:
        """``Linear(LayerNorm(x))`` for the packed ``[layers..., W_u]`` (``up`` None: the layers alone), every product in
        front of the edge phase: ``k | v``, ``x_r | q | u``, ``q | u``, the processor's ``x_r | q | k | v | u``, the unfolded
        ``x_r | q`` -- cached under ``tag`` as the plain packed weight, its LayerNorm fold or its embedding + LayerNorm fold."""
        xin, stats, ln = handle
        if up is None:
            plain, rows = (lambda: self._cat_linear(tag, layers, xin.dtype)), (lambda: self._cat_rows(layers))
            params = [l.weight for l in layers] + [l.bias for l in layers]
        else:
            plain, rows = (lambda: self._folded_in(tag, layers, xin.dtype, up)), (lambda: self._folded_rows(layers, up))
            params = self._fold_params(layers)
        if isinstance(xin, EmbeddedRows):
            # embedding -> LayerNorm -> Linear as one product on the raw features (K = padded feature count, not C)
            xa = xin.x_aug
            wf, bf, zero = self._packed.get(
                (tag, "embfold", xa.dtype, xa.shape[1], xin.one_col, xin._tag),
                list(params) + [ln.weight, ln.bias, xin.emb.weight, xin.emb.bias],
                lambda: runtime.fold_embedded_layer_norm(*rows(), ln.weight, ln.bias, xin.emb.weight, xin.emb.bias,
                                                         xa.shape[1], xin.one_col, xa.dtype))
            return runtime.linear(xa, wf, bf, ln=(stats, zero), **kw)
        if stats is None:
            w, b = plain()
            return runtime.linear(xin, w, b, **kw)
        wf, bf, cs = self._packed.get(
            (tag, "lnfold", xin.dtype), list(params) + [ln.weight, ln.bias],
            lambda: runtime.fold_layer_norm(*rows(), ln.weight, ln.bias, xin.dtype))
        return runtime.linear(xin, wf, bf, ln=(stats, cs), **kw)

    def _cat_rows(self, layers):
        """f32 ``(cat of weights, cat of biases)`` of a list of Linear layers (input of the LayerNorm fold)."""
        w = torch.cat([l.weight.detach().float() for l in layers], dim=0)
        b = runtime.pack_bias([l.bias for l in layers], [l.out_features for l in layers], w.device)
        return w, b

    def _folded_rows(self, lead_layers, up: int):
        """As ``_cat_rows`` with the ``W_u`` rows of the lin_edge fold appended (q/k/v side of the lin_edge fold, ``_folded_in``)."""
        w, b = self._cat_rows(lead_layers)
        wu, bu = self._query_fold(up)
        return torch.cat([w, wu], dim=0), torch.cat([b, bu], dim=0)

    def _edge_params(self):
        return runtime.f32c(self.lin_edge.weight), runtime.f32c(self.lin_edge.bias)

    # ---- lin_edge folded into the neighbouring GEMMs (see include/anemoi_amd.h: anemoi_gt_edge_attention_folded)
    def fold_width(self, dtype) -> Optional[int]:
        """Per-head width ``up`` of the folded edge representation (``edge_dim`` attributes + the constant 1,
        rounded up to 4), or ``None`` when this shape has to use the unfolded kernel.  ``qk_norm`` has no fold: ``u = q W_e`` comes
        out of the GEMM that forms ``q``, and the queries of the scores are normalised after that GEMM.  This one switch takes the
        block off every route built on the fold (``route``: "unfolded"; no block-level entry point, decoder fold, raw source rows)."""
        if self.qk_norm or not runtime.edge_fold_enabled():
            return None
        vec = 16 // dtype.itemsize  # (asked several times per forward, by ``route`` among others: no tensor for it)
        d, h = self.out_channels_conv, self.num_heads
        if d % vec != 0 or (d // vec) not in (1, 2, 4, 8, 16):
            return None
        up = ops.round_up(self.edge_dim + 1, 4)
        if up > 16 or (h * up) % vec != 0 or self.lin_self.in_features % vec != 0:
            return None
        return up

    def edge_layout(self, dtype):
        """(row width, index of the constant-1 column or -1) of the CSR edge-attribute matrix this block consumes."""
        up = self.fold_width(dtype)
        return (ops.round_up(self.edge_dim, 4), -1) if up is None else (up, self.edge_dim)

    def _edge_fold(self, up: int) -> Tensor:
        """``W_e' = [W_e | b_e | 0]`` as ``[H, D, up]`` in f32."""
        h, d = self.num_heads, self.out_channels_conv
        we = torch.zeros((h * d, up), dtype=torch.float32, device=self.lin_edge.weight.device)
        we[:, : self.edge_dim] = self.lin_edge.weight.detach().float()
        we[:, self.edge_dim] = self.lin_edge.bias.detach().float()
        return we.view(h, d, up)

    def _query_fold(self, up: int):
        """Rows / bias that make the q GEMM also emit ``u[n, h, a] = sum_{c in h} W_e'[c, a] q[n, c]``."""
        h, d = self.num_heads, self.out_channels_conv
        weh = self._edge_fold(up)
        wq = self.lin_query.weight.detach().float().view(h, d, -1)
        wu = torch.einsum("hda,hdc->hac", weh, wq).reshape(h * up, -1)
        bu = torch.einsum("hda,hd->ha", weh, self.lin_query.bias.detach().float().view(h, d)).reshape(h * up)
        return wu, bu

    def _projection_fold(self, up: int) -> Tensor:
        """Columns that make ``projection`` absorb ``W_e' t``: ``W_t[o, (h, a)] = sum_{c in h} W_p[o, c] W_e'[c, a]``."""
        h, d = self.num_heads, self.out_channels_conv
        wp = self.projection.weight.detach().float()
        return torch.einsum("ohd,hda->oha", wp.view(wp.shape[0], h, d), self._edge_fold(up)).reshape(wp.shape[0],
                                                                                                       h * up)

    def _folded_in(self, tag: str, lead_layers, dtype, up: int):
        """Packed ``[lead_layers..., W_u]`` weight + bias (q/k/v side of the lin_edge fold)."""
        edge_q = [self.lin_edge.weight, self.lin_edge.bias, self.lin_query.weight, self.lin_query.bias]
        w_in = self._packed.get((tag, "w", dtype, up), [l.weight for l in lead_layers] + edge_q,
                                lambda: runtime.pack_weight([l.weight for l in lead_layers] + [self._query_fold(up)[0]],
                                                            dtype))
        b_in = self._packed.get((tag, "b", up), [l.bias for l in lead_layers] + edge_q,
                                lambda: torch.cat([runtime.pack_bias([l.bias for l in lead_layers],
                                                                     [l.out_features for l in lead_layers],
                                                                     self.lin_edge.weight.device),
                                                   self._query_fold(up)[1]]).contiguous())
        return w_in, b_in

    def _folded_out(self, dtype, up: int):
        """Packed ``[W_p | W_t]`` weight + bias (projection side of the lin_edge fold)."""
        edge_p = [self.lin_edge.weight, self.lin_edge.bias, self.projection.weight]
        w_out = self._packed.get(("projf", "w", dtype, up), edge_p,
                                 lambda: runtime.pack_weight_cols([self.projection.weight.detach().float(),
                                                                   self._projection_fold(up)], dtype))
        return w_out, runtime.f32c(self.projection.bias)

    def _fold_params(self, lead_layers):
        return ([l.weight for l in lead_layers] + [l.bias for l in lead_layers]
                + [self.lin_edge.weight, self.lin_edge.bias, self.lin_query.weight, self.lin_query.bias])

    def _mlp_ln_eps(self, which: str, dtype) -> Optional[float]:
        """Epsilon of the LayerNorm that opens the node MLP when its statistics can ride on the producing GEMM."""
        mlp = self.node_dst_mlp if which == "dst" else self.node_src_mlp
        first = mlp[0] if isinstance(mlp, nn.Sequential) else None
        return first.eps if isinstance(first, nn.LayerNorm) and runtime.ln_fold_enabled(dtype) else None

    def _next_ln_eps(self, dtype) -> Optional[float]:
        """Processor blocks are stacked: the output enters the next block's ``layer_norm1`` (same construction)."""
        ln1 = getattr(self, "layer_norm1", None)
        return ln1.eps if isinstance(ln1, nn.LayerNorm) and runtime.ln_fold_enabled(dtype) else None

    def block_abi_operands(self, dtype: torch.dtype, lead_layers, tag: str):
        """Packed operands of this block for the block-level C entry points (``anemoi_gt_block_tail`` /
        ``anemoi_gt_processor_block_forward``) -- the very tensors the op-by-op route caches and passes --, or ``None`` when
        the block cannot take that route (f32, LayerNorm fold off, unfolded edge kernel, another node MLP shape).
        ``lead_layers`` / ``tag``: the Linear layers whose rows open the LayerNorm-folded input product (processor block:
        lin_self, lin_query, lin_key, lin_value under "sqkvu")."""
        up = self.fold_width(dtype)
        if up is None or not runtime.ln_fold_enabled(dtype):
            return None
        mlp = self._native_mlp("dst").folded_pair(dtype)
        if mlp is None:
            return None
        ln = self.layer_norm1
        w_in, b_in, cs_in = self._packed.get(
            (tag, "lnfold", dtype), list(self._fold_params(lead_layers)) + [ln.weight, ln.bias],
            lambda: runtime.fold_layer_norm(*self._folded_rows(lead_layers, up), ln.weight, ln.bias, dtype))
        w_proj, b_proj = self._folded_out(dtype, up)
        eps_mlp, act, w1, b1, cs1, w2, b2 = mlp
        return dict(up=up, w_in=w_in, b_in=b_in, cs_in=cs_in, w_proj=w_proj, b_proj=b_proj, eps_mlp=eps_mlp, act=act, w_fc1=w1,
                    b_fc1=b1, cs_fc1=cs1, w_fc2=w2, b_fc2=b2, eps_ln1=ln.eps)

    def _block_tail(self, q: Tensor, k: Tensor, v: Tensor, x_r: Tensor, u: Tensor, edge_attr_csr: Tensor, plan, res: Tensor,
                    up: int, out_stats_eps: Optional[float]) -> Optional[Tensor]:
        """Edge phase -> projection (+ ``res``) -> node MLP (+ skip) as ONE call of ``anemoi_gt_block_tail`` (the launches
        and packed weights of ``folded_edge_phase`` + ``ops.linear`` + ``_node_mlp``; bit-identical), or ``None`` when this
        block / call has to go op by op (f32, LayerNorm fold off, another MLP shape, bench.py's per-kernel timing pass)."""
        import ctypes

        from .. import _lib

        dtype = q.dtype
        if (ops.PROFILE is not None or dtype != torch.bfloat16 or not q.is_cuda or plan.num_edges == 0 or q.shape[0] == 0
                or not self.block_abi or self._mlp_ln_eps("dst", dtype) is None):
            return None
        mlp = self._native_mlp("dst").folded_pair(dtype)
        if mlp is None or not (res.dim() == 2 and res.stride(1) == 1):
            return None
        eps_mlp, act, w1, b1, cs1, w2, b2 = mlp
        wp, bp = self._folded_out(dtype, up)
        n, c, h = q.shape[0], q.shape[1], self.num_heads
        dev = q.device
        att = self._att_buffer(n, wp.shape[1], c + h * up, dtype, dev)
        y, hid, out = (torch.empty((n, w), dtype=dtype, device=dev) for w in (c, w1.shape[0], c))
        stats = torch.empty((2 if out_stats_eps is not None else 1, n, 2), dtype=torch.float32, device=dev)
        ws = torch.empty((n * max(c // 128, 1), 2), dtype=torch.float32, device=dev)
        a = _lib.GtBlockArgs()
        a.struct_bytes, a.n_dst, a.dtype = ctypes.sizeof(_lib.GtBlockArgs), n, ops.dtype_code(dtype)
        a.C, a.H, a.up, a.hidden, a.act, a.k_proj = c, h, up, w1.shape[0], _lib.ACT_CODES[act], wp.shape[1]
        a.eps_mlp, a.eps_out = eps_mlp, (out_stats_eps if out_stats_eps is not None else 0.0)
        a.q, a.k, a.v, a.x_r, a.u = q.data_ptr(), k.data_ptr(), v.data_ptr(), x_r.data_ptr(), u.data_ptr()
        a.ldq, a.ldkv, a.ldr, a.ldu = ops._ld(q), ops._ld(k), ops._ld(x_r), ops._ld(u)
        a.edge_attr, a.rowptr, a.col = edge_attr_csr.data_ptr(), plan.rowptr.data_ptr(), plan.col.data_ptr()
        runtime.set_edge_list_args(a, runtime.edge_lists(plan, dtype, c, h, up), k.shape[0], edge_attr_csr.shape[0])
        a.att, a.ld_att = att.data_ptr(), wp.shape[1]
        a.w_proj, a.b_proj = wp.data_ptr(), ops._ptr(bp)
        a.res, a.ld_res, a.y, a.y_stats = res.data_ptr(), ops._ld(res), y.data_ptr(), stats[0].data_ptr()
        a.w_fc1, a.b_fc1, a.cs_fc1, a.h = w1.data_ptr(), ops._ptr(b1), cs1.data_ptr(), hid.data_ptr()
        a.w_fc2, a.b_fc2, a.out = w2.data_ptr(), ops._ptr(b2), out.data_ptr()
        a.out_stats = stats[1].data_ptr() if out_stats_eps is not None else None
        a.stats_ws, a.stats_ws_bytes = ws.data_ptr(), ws.numel() * 4
        _lib.check(_lib.load().anemoi_gt_block_tail(ctypes.byref(a), ops._stream()), "anemoi_gt_block_tail")
        if out_stats_eps is not None:
            ops._carry_stats(out, out_stats_eps, stats[1])
        return out

    block_abi = True  # False: op by op (tests compare the two routes)

    def _norm_qk_(self, q: Optional[Tensor], k: Optional[Tensor], qk: Optional[Tensor] = None) -> None:
        """``qk_norm`` in place on the ``q`` and ``k`` column slices of the products in front of the edge phase -- ``qk``: the
        ``q | k`` columns where ``k`` follows ``q`` in one matrix (the processor block's ``x_r | q | k | v``), ONE ``groups = 2``
        launch; else one launch each for ``q`` (destination rows) and ``k`` (source rows).  A no-op without the switch."""
        if not self.qk_norm:
            return
        h = self.num_heads
        params = [self.q_norm.weight, self.k_norm.weight]
        w = self._packed.get(("qk_norm", "w"), params, lambda: torch.stack([p.detach().float() for p in params]).contiguous())
        if qk is not None:
            ops.head_norm(qk, w, h, 2, self.q_norm.eps, out=qk)
            return
        ops.head_norm(q, w[0], h, 1, self.q_norm.eps, out=q)
        ops.head_norm(k, w[1], h, 1, self.k_norm.eps, out=k)

    def _norm_qk_grad(self, q: Tensor, k: Tensor):
        """The same with gradients, on separate ``q`` and ``k`` (the head-sharded protocol: before the rows -> heads exchange)."""
        if not self.qk_norm:
            return q, k
        from .. import autograd

        return (autograd.head_norm(q, self.q_norm.weight, self.num_heads, 1, self.q_norm.eps),
                autograd.head_norm(k, self.k_norm.weight, self.num_heads, 1, self.k_norm.eps))

    def _qk_norm_refuse(self, dtype, halo) -> None:
        """The routes ``qk_norm`` does not have, refused before anything is launched."""
        if not self.qk_norm:
            return
        if halo is not None:
            raise NotImplementedError("qk_norm: node-partitioned GraphTransformer blocks need the folded edge kernel, which "
                                      "has no qk_norm")
        if runtime.mxfp8_enabled(dtype):
            raise NotImplementedError("qk_norm: ANEMOI_AMD_MXFP8=1 runs the GraphTransformer blocks on the folded edge kernel, "
                                      "which has no qk_norm")

    @staticmethod
    def _att_buffer(n: int, ld: int, written: int, dtype, device) -> Tensor:
        """The projection's operand ``[n, ld]``: the edge phase writes the first ``written`` columns, the K padding behind
        them is zeroed here."""
        att = torch.empty((n, ld), dtype=dtype, device=device)
        if ld > written:
            att[:, written:].zero_()
        return att

    def _attention(self, q: Tensor, k: Tensor, v: Tensor, x_r: Tensor, u: Optional[Tensor], edge_attr_csr: Tensor, plan,
                   up: Optional[int]):
        """Edge phase of the folded (``up``) or unfolded route -> ``(attention buffer, projection weight, bias)``: ``out + x_r``
        for the plain projection, ``out + x_r | t | 0-pad`` for ``[W_p | W_t]`` (the lin_edge part via ``W_t``)."""
        if up is None:
            wp, bp = self._cat_linear("proj", [self.projection], q.dtype)
            we, be = self._edge_params()
            return self.conv.fused(q, k, v, x_r, edge_attr_csr, self.edge_dim, we, be, plan, self.num_heads), wp, bp
        wp, bp = self._folded_out(q.dtype, up)
        return folded_edge_phase(q, k, v, x_r, u, edge_attr_csr, plan, self.num_heads, up, ld_out=wp.shape[1]), wp, bp

    def _project(self, att: Tensor, w: Tensor, b: Optional[Tensor], res: Optional[Tensor], chunked: bool = False) -> Tensor:
        """The projection product (+ ``res``) of every route.  The statistics of the MLP's LayerNorm ride on its epilogue
        unless the MLP runs in row chunks (those of the LayerNorm that reads the new nodes next ride on the MLP's last
        Linear, ``_node_mlp``).  The caller drops ``att`` before it goes on to the node MLP."""
        return runtime.linear(att, w, b, residual=res, stats_eps=None if chunked else self._mlp_ln_eps("dst", att.dtype))

    def _native_mlp(self, which: str) -> NativeSequential:
        """``node_dst_mlp`` / ``node_src_mlp`` on the kernels, built on first use."""
        if which not in self._mlps:
            self._mlps[which] = NativeSequential(self.node_dst_mlp if which == "dst" else self.node_src_mlp)
        return self._mlps[which]

    def _node_mlp(self, y: Tensor, which: str, num_chunks: int, out_stats_eps: Optional[float] = None) -> Tensor:
        """``mlp(y) + y`` with mlp = LayerNorm, Linear, act, Linear; optionally in row chunks (bounded hidden buffer)."""
        run = self._native_mlp(which)
        if num_chunks <= 1:
            return run(y, residual=y, out_stats_eps=out_stats_eps)
        return torch.cat([run(c, residual=c) for c in y.tensor_split(num_chunks, dim=0) if c.shape[0] > 0], dim=0)

    # ---- MXFP8 route (runtime.mxfp8_enabled): op by op, weights quantised once per version
    def _mx_check(self, width: int, halo) -> None:
        if halo is not None:
            raise NotImplementedError("ANEMOI_AMD_MXFP8=1: the node-partitioned forward has no MXFP8 route")
        if width % 128 != 0:
            raise NotImplementedError(f"ANEMOI_AMD_MXFP8=1 needs block widths that are a multiple of 128, got {width}")

    def _mx_node_mlp(self, y: Tensor, which: str, num_chunks: int = 1) -> Tensor:
        """``mlp(y) + y`` for mlp = LayerNorm, Linear + act, Linear: LayerNorm + quantise in one pass, fc1 with an MXFP8
        output, fc2 with the residual."""
        seq = self.node_dst_mlp if which == "dst" else self.node_src_mlp
        mods = list(seq)
        if (len(mods) != 4 or not isinstance(mods[0], nn.LayerNorm) or not isinstance(mods[1], nn.Linear)
                or not isinstance(mods[3], nn.Linear) or fused_activation_name(mods[2]) is None):
            raise NotImplementedError("ANEMOI_AMD_MXFP8=1 covers node MLPs of the form LayerNorm, Linear, act, Linear")
        ln, fc1, fc2 = mods[0], mods[1], mods[3]
        self._mx_check(fc1.in_features, None)
        w1 = runtime.mx_weight(self._packed, ("mlp", which, 1), [fc1.weight, fc1.bias], lambda: (fc1.weight, fc1.bias))
        w2 = runtime.mx_weight(self._packed, ("mlp", which, 2), [fc2.weight, fc2.bias], lambda: (fc2.weight, fc2.bias))
        ln_args = (runtime.f32c(ln.weight), runtime.f32c(ln.bias), ln.eps)
        act = fused_activation_name(mods[2])

        def run(rows: Tensor) -> Tensor:
            h = ops.linear_mx(ops.mx_quantize(rows, ln=ln_args), w1[0], w1[1], act=act, out="mx")
            return ops.linear_mx(h, w2[0], w2[1], residual=rows)

        if num_chunks <= 1:
            return run(y)
        return torch.cat([run(c) for c in y.tensor_split(num_chunks, dim=0) if c.shape[0] > 0], dim=0)

    def _check_channels(self, dtype) -> None:
        mult = ops.k_multiple(dtype)
        width = self.num_heads * self.out_channels_conv
        if width % mult != 0:
            raise NotImplementedError(
                f"hidden width {width} must be a multiple of {mult} for {dtype} on the MI355X path"
            )

    def _edge_inputs(self, edge_attr: Tensor, edge_index: Tensor, n_src: int, n_dst: int, dtype):
        if edge_attr.shape[1] != self.edge_dim:
            raise ValueError(f"edge_attr has {edge_attr.shape[1]} features, lin_edge expects {self.edge_dim}")
        if edge_attr.shape[0] != edge_index.shape[1]:
            raise ValueError(f"edge_attr has {edge_attr.shape[0]} rows for {edge_index.shape[1]} edges")
        plan = self._plans.get(edge_index, n_src, n_dst)
        return plan, ops.edge_attr_csr(edge_attr, None, plan.perm, *self.edge_layout(dtype))

    @abstractmethod
    def forward(self, x, edge_attr, edge_index, shapes, batch_size, model_comm_group=None, size=None): ...


class GraphTransformerProcessorBlock(GraphTransformerBaseBlock):
    """Graph transformer layer on one node set (reference layers/block.py:553-635)."""

    def native(self, x: Tensor, edge_attr_csr: Tensor, plan: EdgePlan, halo=None) -> Tensor:
        """x ``[N, C]`` in the compute dtype, edge attributes already in CSR order.  Returns the new nodes.

        With ``halo`` (node-partitioned run) ``x`` holds this rank's rows only; the k|v rows of the halo sources are
        fetched from their owners by one all-to-all-v and appended behind the own rows (the plan's source index space).
        """
        dtype = x.dtype
        self._check_channels(dtype)
        self._qk_norm_refuse(dtype, halo)
        if runtime.mxfp8_enabled(dtype):
            return self._native_mx(x, edge_attr_csr, plan, halo)
        c = self.num_heads * self.out_channels_conv
        xh = self._ln_begin(self.layer_norm1, x)
        up = self.fold_width(dtype)
        if halo is not None:
            if up is None:
                raise NotImplementedError("node-partitioned blocks need the folded edge kernel")
            n_own = x.shape[0]
            kv = torch.empty((n_own + halo.n_recv, 2 * c), dtype=dtype, device=x.device)
            self._ln_product(xh, "kv", [self.lin_key, self.lin_value], out=kv[:n_own])
            pending = halo.start(kv, n_own)  # xGMI transfer of the halo k|v rows ...
            sq = self._ln_product(xh, "squ", [self.lin_self, self.lin_query], up)  # ... overlapped with the x_r | q | u GEMM
            halo.finish(pending)
            k, v, u = kv[:, :c], kv[:, c:], sq[:, 2 * c:]
        else:
            # [N, 4C (+ H*up)] = x_r | q | k | v (| u)
            sq = self._ln_product(xh, "sqkvu" if up is not None else "sqkv",
                                  [self.lin_self, self.lin_query, self.lin_key, self.lin_value], up)
            k, v, u = sq[:, 2 * c:3 * c], sq[:, 3 * c:4 * c], sq[:, 4 * c:]
            self._norm_qk_(None, None, sq[:, c:3 * c])
        q, x_r, next_eps = sq[:, c:2 * c], sq[:, :c], self._next_ln_eps(dtype)
        done = None if up is None else self._block_tail(q, k, v, x_r, u, edge_attr_csr, plan, x, up, next_eps)
        if done is not None:
            return done
        att, wp, bp = self._attention(q, k, v, x_r, u, edge_attr_csr, plan, up)
        y = self._project(att, wp, bp, x)  # projection(out + x_r) + x
        del att
        return self._node_mlp(y, "dst", 1, out_stats_eps=next_eps)

    # ANEMOI_AMD_MXFP8=1 runs the x_r | q | k | v | u product on MXFP8 only when this is set; off by default, it costs the
    # most accuracy of the covered products (profiles/r07_mxfp8.md section 5); off, the product keeps the bf16 LayerNorm fold
    mx_sqkvu = False

    def _native_mx(self, x: Tensor, edge_attr_csr: Tensor, plan: EdgePlan, halo=None) -> Tensor:
        """The block with its four products on MXFP8: LayerNorm + quantise -> x_r | q | k | v | u; the folded edge phase
        (bf16); quantise -> projection of [out | t] + x; the node MLP (``_mx_node_mlp``)."""
        c = self.num_heads * self.out_channels_conv
        self._mx_check(x.shape[1], halo)
        self._mx_check(c, None)
        up = self.fold_width(x.dtype)
        if up is None:
            raise NotImplementedError("ANEMOI_AMD_MXFP8=1 needs the folded edge kernel (head size / edge width)")
        all4 = [self.lin_self, self.lin_query, self.lin_key, self.lin_value]
        w_in = (runtime.mx_weight(self._packed, ("sqkvu", up), self._fold_params(all4), lambda: self._folded_rows(all4, up))
                if self.mx_sqkvu else None)
        w_out = runtime.mx_weight(
            self._packed, ("projf", up), [self.lin_edge.weight, self.lin_edge.bias, self.projection.weight,
                                          self.projection.bias],
            lambda: (torch.cat([self.projection.weight.detach().float(), self._projection_fold(up)], dim=1),
                     self.projection.bias))
        ln = self.layer_norm1
        if self.mx_sqkvu:
            xq = ops.mx_quantize(x, ln=(runtime.f32c(ln.weight), runtime.f32c(ln.bias), ln.eps))
            sq = ops.linear_mx(xq, w_in[0], w_in[1])  # [N, 4C + H*up] = x_r | q | k | v | u
        else:
            sq = self._ln_product(self._ln_begin(ln, x), "sqkvu", all4, up)
        width = c + self.num_heads * up
        att = self._att_buffer(x.shape[0], ops.round_up(width, ops.k_multiple(x.dtype)), width, x.dtype, x.device)
        folded_edge_phase(sq[:, c:2 * c], sq[:, 2 * c:3 * c], sq[:, 3 * c:4 * c], sq[:, :c], sq[:, 4 * c:], edge_attr_csr, plan,
                          self.num_heads, up, out=att)
        y = ops.linear_mx(ops.mx_quantize(att[:, :c + self.num_heads * up]), w_out[0], w_out[1], residual=x)
        return self._mx_node_mlp(y, "dst")

    def _sharded(self, x: Tensor, edge_attr: Tensor, edge_index: Tensor, shapes: tuple, batch_size: int, model_comm_group,
                 size=None) -> Tensor:
        """The reference's module-level protocol across a model group (layers/block.py:602-635 with ``shard_qkve_heads`` /
        ``shard_output_seq``): ``x`` and ``edge_attr`` are this rank's row / edge shards, ``edge_index`` the whole edge
        list.  Everything is row-local except the conv, which runs on all nodes and edges for this rank's heads
        (``GraphTransformerConv.forward`` = ``anemoi_gt_conv``).  One code path on the autograd nodes (they run their
        forward kernels under ``no_grad`` as well); the model root partitions by mesh node instead and is the fast route."""
        from .. import autograd

        dtype = runtime.compute_dtype(x)
        x = _as_compute(x, dtype)
        ln = self.layer_norm1
        h = autograd.layer_norm(x, ln.weight, ln.bias, ln.eps)
        x_r, q, k, v = (autograd.linear(h, lin.weight, lin.bias) for lin in (self.lin_self, self.lin_query, self.lin_key,
                                                                              self.lin_value))
        q, k = self._norm_qk_grad(q, k)
        e = autograd.linear(_as_compute(edge_attr, dtype), self.lin_edge.weight, self.lin_edge.bias)
        q, k, v, e = self.shard_qkve_heads(q, k, v, e, shapes, batch_size, model_comm_group)
        out = self.conv(q, k, v, e, edge_index, size=size)
        out = self.shard_output_seq(out, shapes, batch_size, model_comm_group)
        out = autograd.linear(out + x_r, self.projection.weight, self.projection.bias, "Identity", x)
        return training.sequential(self.node_dst_mlp, out, residual=out)

    def forward(
        self,
        x: Tensor,
        edge_attr: Tensor,
        edge_index: Tensor,
        shapes: tuple,
        batch_size: int,
        model_comm_group=None,
        size=None,
    ):
        if _group_size(model_comm_group) > 1:
            assert batch_size == 1, "Only batch size of 1 is supported when model is sharded across GPUs"
            return self._sharded(x, edge_attr, edge_index, shapes, batch_size, model_comm_group, size), edge_attr
        if training.wants_grad(self, x, edge_attr):
            return training.gt_processor_block(self, x, edge_attr, edge_index, size)
        dtype = runtime.compute_dtype(x)
        n = x.shape[0]
        if size is not None and tuple(size) != (n, n):
            raise ValueError(f"Encountered tensor with size {n} in dimension 0, but expected size {tuple(size)}")
        plan, ea = self._edge_inputs(edge_attr, edge_index, n, n, dtype)
        return self.native(_as_compute(x, dtype), ea, plan), edge_attr


class GraphTransformerMapperBlock(GraphTransformerBaseBlock):
    """Graph transformer layer between two node sets (reference layers/block.py:429-550)."""

    def __init__(
        self,
        in_channels: int,
        hidden_dim: int,
        out_channels: int,
        edge_dim: int,
        num_heads: int = 16,
        bias: bool = True,
        activation: str = "GELU",
        num_chunks: int = 1,
        update_src_nodes: bool = False,
        **kwargs,
    ) -> None:
        super().__init__(
            in_channels=in_channels, hidden_dim=hidden_dim, out_channels=out_channels, edge_dim=edge_dim,
            num_heads=num_heads, bias=bias, activation=activation, num_chunks=num_chunks,
            update_src_nodes=update_src_nodes, **kwargs,
        )
        self.layer_norm2 = nn.LayerNorm(in_channels)

    mx_node_mlp = True  # ANEMOI_AMD_MXFP8=1 runs node_dst_mlp on MXFP8 (the decoder's mapper turns it off)

    # ---- the route: decided here and nowhere else (DESIGN.md section 4.2 has the table of routes)
    def route(self, dtype, src: Rows, dst: Rows, num_chunks: int = 1, halo: bool = False) -> Route:
        """Which launch sequence ``native`` runs for these rows, from what is known before anything is launched; the switches
        are read now.  In precedence order: ``dec_fold`` (raw destination rows ride in the projection product),
        ``raw_sources`` (attention over raw source rows, no ``k | v``), ``folded`` (``lin_edge`` folded into the neighbouring
        products), ``unfolded``.  ``native`` takes its route from here; the mappers ask with rows of kind ``"raw"`` before
        they embed and form ``h`` only where ``src_h`` / ``dst_h`` say the route reads it."""
        mxfp8 = runtime.mxfp8_enabled(dtype)
        mx = mxfp8 and self.mx_node_mlp  # the destination nodes' MLP on MXFP8
        if mx:
            fc1 = self.node_dst_mlp[1]
            self._mx_check(fc1.in_features if isinstance(fc1, nn.Linear) else 0, True if halo else None)
        up = self.fold_width(dtype)
        h, d = self.num_heads, self.out_channels_conv
        plain = dtype == torch.bfloat16 and num_chunks <= 1 and not halo and not self.update_src_nodes and up is not None
        if (plain and dst.kind == "raw" and src.kind == "tensor" and dst.on_gpu and runtime.dec_fold_enabled()
                and not mxfp8 and runtime.embed_fold_enabled(dtype) and dst.k_pad in (64, 128, 256)
                # the rows' statistics come from the side product of ``EmbeddedRows.stats``, which the opt-in thin statistics
                # site would move to the slower kernel on every grid row (and a launch-list test pins the decoder's list
                # under it); ``out | t`` a whole number of K slabs: the raw blocks start right behind them
                and not runtime.thin_stats_enabled() and (h * (d + up)) % ops.k_multiple(dtype) == 0):
            name = "dec_fold"
        elif (plain and src.kind == "raw" and not mx and src.on_gpu and runtime.edge_raw_enabled() and h == 16
              and src.k_pad in (64, 128, 256) and self._sum_col(src.k_pad, src.one_col) >= src.in_features):
            name = "raw_sources"
        elif up is not None:
            name = "folded"
        elif halo:
            raise NotImplementedError("node-partitioned blocks need the folded edge kernel")
        else:
            name = "unfolded"
        return Route(name, up, mx, num_chunks > 1,
                     block_tail=name == "folded" and num_chunks <= 1 and not self.update_src_nodes and not mx,
                     src_h=self.update_src_nodes, dst_h=name != "dec_fold")

    def dec_fold_route(self, dtype, k_pad: int, num_chunks: int = 1) -> bool:
        """``route`` for plain source rows and raw destination rows of ``k_pad`` columns on the GPU: is it ``dec_fold``?"""
        return self.route(dtype, Rows(), Rows("raw", k_pad, on_gpu=True), num_chunks).name == "dec_fold"

    def native(self, x_src, x_dst, edge_attr_csr: Tensor, plan: EdgePlan, num_chunks: int = 1, halo=None,
               out_stats_eps: Optional[float] = None):
        """``(source rows, new destination rows)``.  The first element: the updated source rows under ``update_src_nodes``,
        else the embedded source rows as they came (``h`` of ``EmbeddedRows``, or the plain tensor) -- ``None`` where the rows
        came without ``h``.  ``out_stats_eps``: epsilon of the LayerNorm the new destination nodes enter next (its
        statistics then come out of the node MLP's last GEMM).  ``halo``: node-partitioned run -- ``x_src`` holds this rank's
        source rows, the k|v rows of the other sources of the plan are appended by one all-to-all-v.

        Four stages, each selected by ``route``: source side, destination product, edge phase into the attention buffer,
        tail.  Large intermediates are dropped before the next stage allocates."""
        dtype = x_dst.dtype
        self._check_channels(dtype)
        self._qk_norm_refuse(dtype, halo)
        src, dst = Rows.of(x_src), Rows.of(x_dst)
        r = self.route(dtype, src, dst, num_chunks, halo is not None)
        # the hand-over: a mapper that asked ``route`` formed every ``h`` the route reads; other callers may not have
        if r.src_h and src.kind == "raw":
            raise ValueError("update_src_nodes needs the embedded source rows")
        if r.dst_h and dst.kind == "raw":
            raise ValueError("destination rows without their embedding need the decoder fold (dec_fold_route)")
        c, h, up = self.num_heads * self.out_channels_conv, self.num_heads, r.up
        # EmbeddedRows (mappers): the rows arrive as the raw features they are embedded from
        h_src = x_src.h if isinstance(x_src, EmbeddedRows) else x_src
        h_dst = x_dst.h if isinstance(x_dst, EmbeddedRows) else x_dst

        # 1. source side: k | v from the LayerNorm-folded product (into the halo buffer, then the all-to-all), or nothing
        xs = self._ln_begin(self.layer_norm1, x_src)
        kv = pending = None
        if r.name == "raw_sources":
            src_stats = xs[1]
        elif halo is None:
            kv = self._ln_product(xs, "kv", [self.lin_key, self.lin_value])  # [N_src, 2C] = k | v
        else:
            n_own = x_src.shape[0]
            kv = torch.empty((n_own + halo.n_recv, 2 * c), dtype=dtype, device=x_src.device)
            self._ln_product(xs, "kv", [self.lin_key, self.lin_value], out=kv[:n_own])
            pending = halo.start(kv, n_own)  # overlapped with the destination-side LayerNorm + GEMM below
        del xs

        # 2. destination product: x_r | q | u, q | u (decoder fold), x_r | q (unfolded); x_r | q | u and qt on raw sources
        qt = None
        if r.name == "raw_sources":
            raw = self._raw_source_weights(x_src, dtype)
            sq, qt = self._raw_dst_side(x_src, x_dst, h_dst, up, raw[0])
        else:
            xd = self._ln_begin(self.layer_norm2, x_dst)
            dst_stats = xd[1]
            if r.name == "dec_fold":
                sq = self._ln_product(xd, "qu", [self.lin_query], up)  # [N_dst, C + H*up] = q | u (no x_r rows)
            else:  # [N_dst, 2C (+ H*up)] = x_r | q (| u)
                sq = self._ln_product(xd, "sq" if up is None else "squ", [self.lin_self, self.lin_query], up)
            del xd
        if pending is not None:
            halo.finish(pending)

        # 3. edge phase into the attention buffer, the projection's operand
        res = h_dst
        if r.name == "dec_fold":
            # rstd x | x written behind out | t: ONE projection product over [out | t | rstd x | x] carries W_p x_r and the
            # residual emb(x) -- neither is ever formed
            xa, res = x_dst.x_aug, None
            wp, bp = self._dec_fold_weights(x_dst, dtype, up)
            width, k_att = c + h * up, c + h * up + 2 * xa.shape[1]
            att = self._att_buffer(xa.shape[0], wp.shape[1], k_att, dtype, xa.device)
            folded_edge_phase(sq[:, :c], kv[:, :c], kv[:, c:], None, sq[:, c:], edge_attr_csr, plan, h, up, out=att)
            ops.raw_row_tail(xa, dst_stats, att[:, width:k_att])
        elif r.name == "raw_sources":
            # the raw-row edge kernel, then g -> sum alpha v (one launch over the heads) + x_r
            w_qt, w_g, sum_col = raw
            wp, bp = self._folded_out(dtype, up)
            att = self._att_buffer(sq.shape[0], wp.shape[1], c + h * up, dtype, sq.device)
            g = ops.gt_edge_attention_raw(qt, x_src.x_aug, src_stats, sq[:, 2 * c:2 * c + h * up], edge_attr_csr, plan.rowptr,
                                          plan.col, h, self.out_channels_conv, up, sum_col, att[:, c:c + h * up])
            del qt
            if w_g.dim() == 3:
                ops.linear_heads(g, w_g, out=att[:, :c], residual=sq[:, :c])
            else:
                runtime.linear(g, w_g, residual=sq[:, :c], out=att[:, :c])
            del g
        else:
            q, k, v, x_r, u = sq[:, c:2 * c], kv[:, :c], kv[:, c:], sq[:, :c], sq[:, 2 * c:]
            done = self._block_tail(q, k, v, x_r, u, edge_attr_csr, plan, res, up, out_stats_eps) if r.block_tail else None
            if done is not None:
                return h_src, done
            self._norm_qk_(q, k)
            att, wp, bp = self._attention(q, k, v, x_r, u, edge_attr_csr, plan, up)
            del q, k, v, x_r, u
        del sq, kv

        # 4. tail: projection (+ residual) and the node MLPs
        y = self._project(att, wp, bp, res, r.chunked)
        del att
        if r.mx:
            new_dst = self._mx_node_mlp(y, "dst", num_chunks)
        else:
            new_dst = self._node_mlp(y, "dst", num_chunks, out_stats_eps=out_stats_eps)
        return (self._node_mlp(h_src, "src", num_chunks) if self.update_src_nodes else h_src), new_dst

    # ---- sources given as raw rows: k | v are never formed ("raw-row encoder")
    @staticmethod
    def _sum_col(ks: int, one_col: int) -> int:
        """The last column of the raw rows that is not the constant-1 column; the route needs it inside the K padding."""
        return ks - 1 if one_col != ks - 1 else ks - 2

    def _raw_source_weights(self, x_src: EmbeddedRows, dtype):
        """``(W_qt [H, Ks, D], W_g [H, D, Ks], sum_col)`` of the ``raw_sources`` route (``route`` says when it is taken).

        With ``F = [F_k; F_v]`` and ``b' = [b_k; b_v]`` the embedding- and LayerNorm-folded k | v operator of
        ``runtime.fold_embedded_layer_norm`` (``k_j = rstd_j F_k x_j + b_k``): ``W_qt[h] = F_k[h]^T`` carries a query to
        the raw space, ``W_g[h] = F_v[h]`` brings the aggregate back, with ``b_v[h]`` in column ``sum_col`` -- a zero
        column of the raw rows where the edge kernel leaves ``sum_j alpha_ij``.  They depend on parameters only."""
        h, d, ks = self.num_heads, self.out_channels_conv, x_src.x_aug.shape[1]
        sum_col = self._sum_col(ks, x_src.one_col)
        kv_layers = [self.lin_key, self.lin_value]
        ln, emb = self.layer_norm1, x_src.emb

        def build():
            f, b, _ = runtime.fold_embedded_layer_norm(*self._cat_rows(kv_layers), ln.weight, ln.bias, emb.weight,
                                                       emb.bias, ks, x_src.one_col, torch.float32)
            c = h * d
            w_qt = f[:c].view(h, d, ks).transpose(1, 2)
            w_g = f[c:].view(h, d, ks).clone()
            w_g[:, :, sum_col] = b[c:].view(h, d)
            if d % ops.k_multiple(dtype) != 0:
                # heads narrower than a K slab: the same two products as block-diagonal weights of ONE plain Linear each
                # ([H*Ks, C] and [C, H*Ks]; small models only -- the zeros cost H x the multiply-adds)
                w_qt, w_g = torch.block_diag(*w_qt), torch.block_diag(*w_g)
            return w_qt.to(dtype).contiguous(), w_g.to(dtype).contiguous(), sum_col

        return self._packed.get(("kv", "rawrows", dtype, ks, x_src.one_col, x_src._tag),
                                [l.weight for l in kv_layers] + [l.bias for l in kv_layers]
                                + [ln.weight, ln.bias, emb.weight, emb.bias], build)

    def _raw_dst_side(self, x_src: EmbeddedRows, x_dst, h_dst: Tensor, up: int, w_qt: Tensor):
        """``(x_r | q | u, qt)`` of the ``raw_sources`` route: the destination product and ``q -> qt`` (one launch over the
        heads).  For hoisted destination rows (the encoder's mesh rows on the inference path) both depend on parameters only
        and are kept -- both are read, never written, downstream.  Sources: the rows' own, this block's destination-side
        parameters, and the source-side ones that form A_k in ``w_qt``."""
        dtype, c = x_dst.dtype, self.num_heads * self.out_channels_conv
        sq_layers = [self.lin_self, self.lin_query]

        def dst_side():
            sq = self._ln_product(self._ln_begin(self.layer_norm2, x_dst), "squ", sq_layers, up)  # x_r | q | u
            return sq, (ops.linear_heads(sq[:, c:2 * c], w_qt) if w_qt.dim() == 3 else runtime.linear(sq[:, c:2 * c], w_qt))

        sources = runtime.static_sources(x_dst) if runtime.enc_hoist_enabled() else None
        if sources is None:
            return dst_side()
        ln1, ln2, emb = self.layer_norm1, self.layer_norm2, x_src.emb
        sources = (sources + [h_dst, ln2.weight, ln2.bias] + self._fold_params(sq_layers)
                   + [self.lin_key.weight, self.lin_key.bias, self.lin_value.weight, self.lin_value.bias, ln1.weight,
                      ln1.bias, emb.weight, emb.bias])
        return runtime.hoisted(self._packed, ("squ|qt", dtype, tuple(h_dst.shape), up, x_src.x_aug.shape[1], x_src.one_col),
                               sources, dst_side)

    # ---- destinations given as raw rows: x_r and the embedded rows ride in the projection product
    def _dec_fold_weights(self, x_dst: EmbeddedRows, dtype, up: int):
        """Packed ``[W_p | W_t | W_p A_s | E]`` + f32 bias of ``runtime.compose_decoder_fold``, rebuilt when any parameter that
        enters changes (pointer, in-place version, device)."""
        ln, emb, ks = self.layer_norm2, x_dst.emb, x_dst.x_aug.shape[1]
        params = [self.projection.weight, self.projection.bias, self.lin_edge.weight, self.lin_edge.bias, self.lin_self.weight,
                  self.lin_self.bias, ln.weight, ln.bias, emb.weight, emb.bias]
        return self._packed.get(
            ("projf", "decfold", dtype, up, ks, x_dst.one_col, x_dst._tag), params,
            lambda: runtime.compose_decoder_fold(self.projection.weight, self.projection.bias, self._projection_fold(up),
                                                 self.lin_self.weight, self.lin_self.bias, ln.weight, ln.bias, emb.weight,
                                                 emb.bias, ks, x_dst.one_col, dtype))

    def _sharded(self, x, edge_attr: Tensor, edge_index: Tensor, shapes: tuple, batch_size: int, model_comm_group, size=None):
        """The reference's module-level protocol across a model group (layers/block.py:479-550): row shards of the source
        and destination nodes, an edge shard of the attributes, the whole edge index; heads exchanged around the conv
        (see ``GraphTransformerProcessorBlock._sharded``)."""
        from .. import autograd

        x_src, x_dst = x
        dtype = runtime.compute_dtype(x_dst)
        x_src, x_dst = _as_compute(x_src, dtype), _as_compute(x_dst, dtype)
        ln1, ln2 = self.layer_norm1, self.layer_norm2
        hs = autograd.layer_norm(x_src, ln1.weight, ln1.bias, ln1.eps)
        hd = autograd.layer_norm(x_dst, ln2.weight, ln2.bias, ln2.eps)
        x_r = autograd.linear(hd, self.lin_self.weight, self.lin_self.bias)
        q = autograd.linear(hd, self.lin_query.weight, self.lin_query.bias)
        k = autograd.linear(hs, self.lin_key.weight, self.lin_key.bias)
        v = autograd.linear(hs, self.lin_value.weight, self.lin_value.bias)
        q, k = self._norm_qk_grad(q, k)
        e = autograd.linear(_as_compute(edge_attr, dtype), self.lin_edge.weight, self.lin_edge.bias)
        q, k, v, e = self.shard_qkve_heads(q, k, v, e, shapes, batch_size, model_comm_group)
        out = self.conv(q, k, v, e, edge_index, size=size)
        out = self.shard_output_seq(out, shapes, batch_size, model_comm_group)
        out = autograd.linear(out + x_r, self.projection.weight, self.projection.bias, "Identity", x_dst)
        # update_src_nodes: row-local on whatever source rows this rank holds (reference layers/block.py:540-546)
        new_src = training.sequential(self.node_src_mlp, x_src, residual=x_src) if self.update_src_nodes else x_src
        return new_src, training.sequential(self.node_dst_mlp, out, residual=out)

    def forward(
        self,
        x,
        edge_attr: Tensor,
        edge_index: Tensor,
        shapes: tuple,
        batch_size: int,
        model_comm_group=None,
        size=None,
    ):
        if _group_size(model_comm_group) > 1:
            assert batch_size == 1, "Only batch size of 1 is supported when model is sharded across GPUs"
            return self._sharded(x, edge_attr, edge_index, shapes, batch_size, model_comm_group, size), edge_attr
        if training.wants_grad(self, x[0], x[1], edge_attr):
            return training.gt_mapper_block(self, x, edge_attr, edge_index, size)
        x_src, x_dst = x
        dtype = runtime.compute_dtype(x_dst)
        n_src, n_dst = x_src.shape[0], x_dst.shape[0]
        if size is not None and tuple(size) != (n_src, n_dst):
            raise ValueError(f"Encountered tensors with sizes {(n_src, n_dst)}, but expected size {tuple(size)}")
        plan, ea = self._edge_inputs(edge_attr, edge_index, n_src, n_dst, dtype)
        num_chunks = self.num_chunks if self.training else inference_num_chunks()
        new_src, new_dst = self.native(_as_compute(x_src, dtype), _as_compute(x_dst, dtype), ea, plan, num_chunks)
        return (new_src if self.update_src_nodes else x[0], new_dst), edge_attr


# =============================================================================================
# GNN (edge-MLP message passing) blocks -- parameters mirror reference layers/block.py:108-286
# =============================================================================================
class GraphConvBaseBlock(BaseBlock, ABC):
    def __init__(
        self,
        in_channels: int,
        out_channels: int,
        mlp_extra_layers: int = 0,
        activation: str = "SiLU",
        update_src_nodes: bool = True,
        num_chunks: int = 1,
        **kwargs,
    ) -> None:
        super().__init__(**kwargs)
        self.update_src_nodes = update_src_nodes
        self.num_chunks = num_chunks
        self.node_mlp = MLP(2 * in_channels, out_channels, out_channels, n_extra_layers=mlp_extra_layers,
                            activation=activation)
        self.conv = GraphConv(in_channels=in_channels, out_channels=out_channels, mlp_extra_layers=mlp_extra_layers,
                              activation=activation)
        self._packed = runtime.PackedWeights()
        self._plans = runtime.PlanCache()

    @abstractmethod
    def forward(self, x, edge_attr: Tensor, edge_index: Tensor, shapes: tuple, model_comm_group=None, size=None):
        """``(new nodes, new edge state)`` -- reference layers/block.py:157-167."""

    @staticmethod
    def _check_width(width: int, dtype) -> None:
        """The node / edge width splits the first edge-MLP Linear into column blocks that are GEMM operands of their own
        (K = width): it has to be a whole number of the GEMM's K slabs, as the graph-transformer blocks' hidden width."""
        mult = ops.k_multiple(dtype)
        if width % mult != 0:
            raise NotImplementedError(f"hidden width {width} must be a multiple of {mult} for {dtype} on the MI355X path")


class GraphConvProcessorBlock(GraphConvBaseBlock):
    """Edge-MLP message passing on one node set (reference layers/block.py:170-223, layers/conv.py:27-76)."""

    def native(self, x: Tensor, e_csr: Tensor, plan: EdgePlan, halo=None):
        """x ``[N, C]``, edge state ``[E, C]`` in CSR (destination-sorted) order -> (new nodes, new edge state).

        ``halo`` (node-partitioned run): ``x`` holds this rank's rows; the ``W1b x`` rows of halo sources are fetched
        from their owners by one all-to-all-v (C values per halo node) while the edge-side GEMM runs."""
        dtype = x.dtype
        c = x.shape[1]
        self._check_width(c, dtype)
        edge_mlp, node_mlp = self.conv.edge_mlp.native(), self.node_mlp.native()
        lin1 = edge_mlp.steps[0][1]
        act1 = edge_mlp.steps[0][2]
        if lin1.in_features != 3 * c or e_csr.shape[1] != c:
            raise ValueError(f"GNN block expects node / edge width {lin1.in_features // 3}, got {c} / {e_csr.shape[1]}")
        if e_csr.shape[0] == 0 and halo is None:  # an edge set without edges: empty new state, zero sums, nothing launched on it
            xcat = torch.zeros((x.shape[0], 2 * c), dtype=dtype, device=x.device)
            xcat[:, :c].copy_(x)
            return node_mlp(xcat, residual=x), e_csr
        # W1 [x_i | x_j | e] = (W1a x)_i + (W1b x)_j + W1c e : node part as ONE [N, 2C] GEMM, edge part as [E, C] GEMM
        w_nodes = self._packed.get(("w1_nodes", dtype), [lin1.weight],
                                   lambda: runtime.pack_weight([lin1.weight[:, :c], lin1.weight[:, c:2 * c]], dtype))
        w_edges = self._packed.get(("w1_edges", dtype), [lin1.weight],
                                   lambda: runtime.pack_weight([lin1.weight[:, 2 * c:]], dtype))
        b1 = None if lin1.bias is None else runtime.f32c(lin1.bias)
        if halo is None:
            p = runtime.linear(x, w_nodes, None)  # [N, 2C] = W1a x | W1b x
            p_dst, p_src = p[:, :c], p[:, c:]
            t = runtime.linear(e_csr, w_edges, b1)
        else:
            n_own = x.shape[0]
            p_src = torch.empty((n_own + halo.n_recv, c), dtype=dtype, device=x.device)
            runtime.linear(x, w_nodes[c:], None, out=p_src[:n_own])  # W1b x of the own rows, halo rows appended below
            pending = halo.start(p_src, n_own)
            p_dst = runtime.linear(x, w_nodes[:c], None)
            t = runtime.linear(e_csr, w_edges, b1)
            halo.finish(pending)
            p = None
        h = ops.gather_add_act(t, p_dst, p_src, plan.dst, plan.col, act=act1, out=t)
        e_new = edge_mlp(h, residual=e_csr, start=1)  # remaining Linear/act pairs, LayerNorm, "+ e"
        del h, t, p, p_dst, p_src
        xcat = ops.segment_sum(e_new, plan.rowptr, cat_with=x)  # [x | scatter-sum over destinations]: the node MLP's input
        return node_mlp(xcat, residual=x), e_new

    def _sharded(self, x, edge_attr, edge_index, shapes, model_comm_group, size=None):
        """The reference's module-level protocol across a model group (layers/block.py:193-223): ``x`` is this rank's row
        shard, ``edge_attr`` / ``edge_index`` its 1-hop edge shard (global node ids).  ``sync_tensor`` gathers the nodes,
        the conv updates the local edges and sums them over ALL destinations, ``shard_tensor`` keeps this rank's rows."""
        from ..distributed.graph import shard_tensor, sync_tensor

        dtype = runtime.compute_dtype(x)
        x = _as_compute(x, dtype)
        x_in = sync_tensor(x, 0, shapes[1], model_comm_group)
        out, edges_new = self.conv(x_in, _as_compute(edge_attr, dtype), edge_index, size=size)
        out = shard_tensor(out, 0, shapes[1], model_comm_group, gather_in_backward=False)
        return training.mlp(self.node_mlp, torch.cat([x, out], dim=1), residual=x), edges_new

    def forward(self, x, edge_attr, edge_index, shapes, model_comm_group=None, size=None):
        if _group_size(model_comm_group) > 1:
            return self._sharded(x, edge_attr, edge_index, shapes, model_comm_group, size)
        if training.wants_grad(self, x, edge_attr):
            return training.gnn_processor_block(self, x, edge_attr, edge_index, size)
        dtype = runtime.compute_dtype(x)
        n = x.shape[0]
        plan = self._plans.get(edge_index, n, n)
        perm = plan.perm.long()
        e_csr = _as_compute(edge_attr, dtype).index_select(0, perm)
        x_new, e_new = self.native(_as_compute(x, dtype), e_csr, plan)
        edges_new = torch.empty_like(e_new)
        edges_new[perm] = e_new  # back to the caller's edge order
        return x_new, edges_new


class GraphConvMapperBlock(GraphConvBaseBlock):
    """Edge-MLP message passing between two node sets (reference layers/block.py:226-286)."""

    def native(self, x_src: Tensor, x_dst: Tensor, e_csr: Tensor, plan: EdgePlan, halo=None):
        """``halo`` (node-partitioned run, backward mapper): ``x_src`` holds this rank's source rows only; the ``W1b x``
        rows of the halo sources arrive from their owners by one all-to-all-v (C values per row) while the destination
        and edge GEMMs run."""
        dtype = x_dst.dtype
        c = x_dst.shape[1]
        self._check_width(c, dtype)
        edge_mlp, node_mlp = self.conv.edge_mlp.native(), self.node_mlp.native()
        lin1, act1 = edge_mlp.steps[0][1], edge_mlp.steps[0][2]
        if e_csr.shape[0] == 0 and halo is None:  # (see GraphConvProcessorBlock.native)
            def lone(x, second):  # node_mlp(cat[x, second]) + x
                xcat = torch.zeros((x.shape[0], 2 * c), dtype=dtype, device=x.device)
                xcat[:, :c].copy_(x)
                if second is not None:
                    xcat[:, c:].copy_(second)
                return node_mlp(xcat, residual=x)

            return (lone(x_src, x_src) if self.update_src_nodes else x_src, lone(x_dst, None)), e_csr
        w_dst = self._packed.get(("w1_dst", dtype), [lin1.weight], lambda: runtime.pack_weight([lin1.weight[:, :c]], dtype))
        w_src = self._packed.get(("w1_src", dtype), [lin1.weight],
                                 lambda: runtime.pack_weight([lin1.weight[:, c:2 * c]], dtype))
        w_edges = self._packed.get(("w1_edges", dtype), [lin1.weight],
                                   lambda: runtime.pack_weight([lin1.weight[:, 2 * c:]], dtype))
        if halo is None:
            p_src = runtime.linear(x_src, w_src, None)
            pending = None
        else:
            n_own = x_src.shape[0]
            p_src = torch.empty((n_own + halo.n_recv, c), dtype=dtype, device=x_dst.device)
            runtime.linear(x_src, w_src, None, out=p_src[:n_own])
            pending = halo.start(p_src, n_own)
        p_dst = runtime.linear(x_dst, w_dst, None)
        t = runtime.linear(e_csr, w_edges, None if lin1.bias is None else runtime.f32c(lin1.bias))
        if pending is not None:
            halo.finish(pending)
        h = ops.gather_add_act(t, p_dst, p_src, plan.dst, plan.col, act=act1, out=t)
        e_new = edge_mlp(h, residual=e_csr, start=1)
        del h, t, p_dst, p_src

        def update(x, agg):  # node_mlp(cat[x, agg]) + x
            if agg is not None:
                return node_mlp(ops.segment_sum(agg, plan.rowptr, cat_with=x), residual=x)
            xcat = torch.empty((x.shape[0], 2 * c), dtype=dtype, device=x.device)
            xcat[:, :c].copy_(x)
            xcat[:, c:].copy_(x)
            return node_mlp(xcat, residual=x)

        new_dst = update(x_dst, e_new)
        new_src = update(x_src, None) if self.update_src_nodes else x_src  # reference block.py:282
        return (new_src, new_dst), e_new

    def _sharded(self, x, edge_attr, edge_index, shapes, model_comm_group, size=None):
        """Reference layers/block.py:249-286 across a model group: both node sets gathered (``sync_tensor``), the conv on
        the local 1-hop edges, this rank's destination rows kept; the source update is row-local."""
        from ..distributed.graph import shard_tensor, sync_tensor

        dtype = runtime.compute_dtype(x[1])
        x_src, x_dst = _as_compute(x[0], dtype), _as_compute(x[1], dtype)
        x_in = (sync_tensor(x_src, 0, shapes[0], model_comm_group), sync_tensor(x_dst, 0, shapes[1], model_comm_group))
        out, edges_new = self.conv(x_in, _as_compute(edge_attr, dtype), edge_index, size=size)
        out = shard_tensor(out, 0, shapes[1], model_comm_group, gather_in_backward=False)
        new_dst = training.mlp(self.node_mlp, torch.cat([x_dst, out], dim=1), residual=x_dst)
        new_src = x_src if not self.update_src_nodes else training.mlp(self.node_mlp, torch.cat([x_src, x_src], dim=1),
                                                                      residual=x_src)
        return (new_src, new_dst), edges_new

    def forward(self, x, edge_attr, edge_index, shapes, model_comm_group=None, size=None):
        if _group_size(model_comm_group) > 1:
            return self._sharded(x, edge_attr, edge_index, shapes, model_comm_group, size)
        if training.wants_grad(self, x[0], x[1], edge_attr):
            return training.gnn_mapper_block(self, x, edge_attr, edge_index, size)
        x_src, x_dst = x
        dtype = runtime.compute_dtype(x_dst)
        n_src, n_dst = x_src.shape[0], x_dst.shape[0]
        if size is not None and tuple(size) != (n_src, n_dst):
            raise ValueError(f"Encountered tensors with sizes {(n_src, n_dst)}, but expected size {tuple(size)}")
        plan = self._plans.get(edge_index, n_src, n_dst)
        perm = plan.perm.long()
        e_csr = _as_compute(edge_attr, dtype).index_select(0, perm)
        nodes, e_new = self.native(_as_compute(x_src, dtype), _as_compute(x_dst, dtype), e_csr, plan)
        edges_new = torch.empty_like(e_new)
        edges_new[perm] = e_new
        return nodes, edges_new


# =============================================================================================
# Transformer block (mesh-node multi-head self attention) -- reference layers/block.py:61-105
# =============================================================================================
class TransformerProcessorBlock(BaseBlock):
    def __init__(self, num_channels: int, hidden_dim: int, num_heads: int, activation: str, window_size: int,
                 dropout_p: float = 0.0, cond_dim: Optional[int] = None, qk_norm: bool = False):
        super().__init__()
        from .attention import MultiHeadSelfAttention

        act = activation_class(activation)
        self.cond_dim = cond_dim
        # cond_dim: both LayerNorms are conditional on a per-row embedding of width cond_dim (the ensemble model's noise)
        norm = (lambda: nn.LayerNorm(num_channels)) if cond_dim is None else (
            lambda: ConditionalLayerNorm(num_channels, cond_dim))
        self.layer_norm1 = norm()
        self.attention = MultiHeadSelfAttention(num_heads=num_heads, embed_dim=num_channels, window_size=window_size,
                                                bias=False, is_causal=False, dropout_p=dropout_p, qk_norm=qk_norm)
        self.mlp = nn.Sequential(nn.Linear(num_channels, hidden_dim), act(), nn.Linear(hidden_dim, num_channels))
        self.layer_norm2 = norm()

        self._mlp: Optional[NativeSequential] = None

    def _check_cond(self, cond: Optional[Tensor], sharded: bool) -> None:
        if (cond is None) != (self.cond_dim is None):
            raise ValueError("TransformerProcessorBlock: `cond` goes with cond_dim (a block built with cond_dim needs it, "
                             "a block built without takes none)")
        if cond is not None and sharded:
            raise NotImplementedError("TransformerProcessorBlock: conditional LayerNorms are not implemented across a model "
                                      "communication group")

    def native(self, x: Tensor, batch_size: int, head_exchange=None, cond: Optional[Tensor] = None) -> Tensor:
        """Pre-LN attention residual + pre-LN MLP residual (reference layers/block.py:99-105).

        ``head_exchange`` (node-partitioned run): q|k|v of the own rows go through an all-to-all so that this rank holds
        ALL rows of its share of the heads, attention runs on those heads, and a second all-to-all brings the own rows
        of all heads back.  ``cond`` ``[rows, cond_dim]`` f32: the condition of the two conditional LayerNorms."""
        self._check_cond(cond, head_exchange is not None)
        ln1, ln2 = self.layer_norm1, self.layer_norm2
        att = self.attention
        if cond is not None:  # op by op: the block-level entry point knows the plain LayerNorm only
            h = ln1.native(x, cond)
            qkv = att.norm_qk_(linear_native(att._packed, "lin_qkv", att.lin_qkv, h))
            drop_p, drop_seed, drop_dev = att.dropout()
            a = ops.mhsa(qkv, batch_size, att.num_heads, att.attention_window(), dropout_p=drop_p, dropout_seed=drop_seed,
                         seed_dev=drop_dev)
            x = linear_native(att._packed, "projection", att.projection, a, residual=x)
            if self._mlp is None:
                self._mlp = NativeSequential(self.mlp)
            return self._mlp(ln2.native(x, cond), residual=x)
        if head_exchange is None:
            done = self._block_abi(x, batch_size)
            if done is not None:
                return done
        h = ops.layer_norm(x, runtime.f32c(ln1.weight), runtime.f32c(ln1.bias), ln1.eps)
        # qk_norm is row- and head-local: on the own rows' q | k, in front of the rows -> heads exchange
        qkv = att.norm_qk_(linear_native(att._packed, "lin_qkv", att.lin_qkv, h))
        # attention dropout (training mode, reference layers/attention.py:90) across a model group: ONE seed -- rank 0's draw,
        # broadcast -- and the GLOBAL head index in the mask's hash, so the ranks together drop exactly what the unsharded
        # attention drops with that seed (every rank sees the whole sequence of its heads in the unsharded row order)
        drop_p, drop_seed, drop_dev = att.dropout(None if head_exchange is None else head_exchange.group)
        if head_exchange is not None:
            window = att.attention_window()
            qkv_heads = head_exchange.rows_to_heads(qkv, att.num_heads)  # [S, 3 * C_local], internal row order
            if window >= 0:  # the window slides over the EXTERNAL node order
                qkv_heads = qkv_heads.index_select(0, head_exchange.to_external)
            a_heads = ops.mhsa(qkv_heads, batch_size, head_exchange.local_heads(att.num_heads), window, dropout_p=drop_p,
                               dropout_seed=drop_seed, head_offset=head_exchange._head_bounds(att.num_heads)[head_exchange.rank],
                               heads_total=att.num_heads, seed_dev=drop_dev)
            if window >= 0:
                a_heads = a_heads.index_select(0, head_exchange.to_internal)
            a = head_exchange.heads_to_rows(a_heads, att.num_heads)  # [n_own, C]
        else:
            a = ops.mhsa(qkv, batch_size, att.num_heads, att.attention_window(), dropout_p=drop_p, dropout_seed=drop_seed,
                         seed_dev=drop_dev)
        x = linear_native(att._packed, "projection", att.projection, a, residual=x)  # x + attention(...)
        if self._mlp is None:
            self._mlp = NativeSequential(self.mlp)
        h = ops.layer_norm(x, runtime.f32c(ln2.weight), runtime.f32c(ln2.bias), ln2.eps)
        return self._mlp(h, residual=x)

    block_abi = True  # False: op by op (tests compare the two routes)

    def _block_abi(self, x: Tensor, batch_size: int) -> Optional[Tensor]:
        """The whole block as ONE call of ``anemoi_transformer_block_forward`` (the launches and packed weights of the
        op-by-op route below; bit-identical), f32 or bf16 -- or ``None`` when this call has to go op by op (bench.py's
        per-kernel timing pass, channel widths that need K padding, an MLP of another shape)."""
        import ctypes

        from .. import _lib

        if self.cond_dim is not None or self.attention.qk_norm:  # (the C entry point knows neither: op by op)
            return None
        dtype, att = x.dtype, self.attention
        c, rows = x.shape[1], x.shape[0]
        mult = ops.k_multiple(dtype)
        if (not self.block_abi or ops.PROFILE is not None or not x.is_cuda or rows == 0 or x.stride(1) != 1
                or c != att.embed_dim or c % mult != 0 or rows % batch_size != 0):
            return None
        if runtime.f32_linear_split(dtype):  # the C entry point calls anemoi_linear itself: the split route runs op by op
            return None
        if self._mlp is None:
            self._mlp = NativeSequential(self.mlp)
        steps = self._mlp.steps
        if [k for k, _, _ in steps] != ["linear", "linear"] or steps[0][2] not in _lib.ACT_CODES or steps[1][2] != "Identity":
            return None
        fc1, fc2 = steps[0][1], steps[1][1]
        hidden = fc1.out_features
        if hidden % mult != 0 or fc1.in_features != c or fc2.out_features != c:
            return None

        def packed(cache, tag, lin):
            w = cache.get((tag, "w", dtype), [lin.weight], lambda: runtime.pack_weight([lin.weight], dtype))
            return w, (None if lin.bias is None else runtime.f32c(lin.bias))

        w_qkv, b_qkv = packed(att._packed, "lin_qkv", att.lin_qkv)
        w_proj, b_proj = packed(att._packed, "projection", att.projection)
        w1 = self._mlp.cache.get(("w", 0, dtype), [fc1.weight], lambda: runtime.pack_weight([fc1.weight], dtype))
        w2 = self._mlp.cache.get(("w", 1, dtype), [fc2.weight], lambda: runtime.pack_weight([fc2.weight], dtype))
        b1 = None if fc1.bias is None else runtime.f32c(fc1.bias)
        b2 = None if fc2.bias is None else runtime.f32c(fc2.bias)
        ln1, ln2 = self.layer_norm1, self.layer_norm2
        p, seed, seed_dev = att.dropout()
        new = lambda *shape: torch.empty(shape, dtype=dtype, device=x.device)  # noqa: E731
        h_ln, qkv, a_out, y, hid, out = new(rows, c), new(rows, 3 * c), new(rows, c), new(rows, c), new(rows, hidden), new(rows, c)
        lib = _lib.load()
        s_len, heads = rows // batch_size, att.num_heads
        ws_bytes = lib.anemoi_mhsa_workspace_bytes(ops.dtype_code(dtype), batch_size, s_len, heads, c // heads)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device) if ws_bytes > 0 else None
        keep = [runtime.f32c(t) for t in (ln1.weight, ln1.bias, ln2.weight, ln2.bias)]
        a = _lib.TfmBlockArgs()
        a.struct_bytes, a.rows, a.dtype = ctypes.sizeof(_lib.TfmBlockArgs), rows, ops.dtype_code(dtype)
        a.B, a.S, a.C, a.H, a.hidden, a.act = batch_size, s_len, c, heads, hidden, _lib.ACT_CODES[steps[0][2]]
        a.window, a.eps1, a.eps2 = att.attention_window(), ln1.eps, ln2.eps
        a.dropout_p, a.dropout_seed, a.dropout_seed_dev = float(p), int(seed) & 0xFFFFFFFF, ops._seed_dev_ptr(seed_dev, x)
        a.dropout_h0, a.dropout_h_total = 0, 0
        a.x, a.ldx = x.data_ptr(), ops._ld(x)
        a.ln1_w, a.ln1_b, a.ln2_w, a.ln2_b = (t.data_ptr() for t in keep)
        a.w_qkv, a.b_qkv, a.w_proj, a.b_proj = w_qkv.data_ptr(), ops._ptr(b_qkv), w_proj.data_ptr(), ops._ptr(b_proj)
        a.w_fc1, a.b_fc1, a.w_fc2, a.b_fc2 = w1.data_ptr(), ops._ptr(b1), w2.data_ptr(), ops._ptr(b2)
        a.h_ln, a.qkv, a.att, a.y, a.h = h_ln.data_ptr(), qkv.data_ptr(), a_out.data_ptr(), y.data_ptr(), hid.data_ptr()
        a.mhsa_ws, a.out = ops._ptr(ws), out.data_ptr()
        _lib.check(lib.anemoi_transformer_block_forward(ctypes.byref(a), ops._stream()), "anemoi_transformer_block_forward")
        return out

    def _sharded(self, x: Tensor, shapes: list, batch_size: int, model_comm_group) -> Tensor:
        """Sequence-sharded call as in the reference (layers/block.py:99-105 with a model group): everything but the
        attention is row-local; the attention module reshards rows <-> heads around its kernel."""
        from .. import autograd

        grad = training.wants_grad(self, x)
        dtype = runtime.compute_dtype(x)
        x = _as_compute(x, dtype)
        ln1, ln2 = self.layer_norm1, self.layer_norm2
        if grad:
            h = autograd.layer_norm(x, ln1.weight, ln1.bias, ln1.eps)
            x = x + self.attention(h, shapes, batch_size, model_comm_group)
            h = autograd.layer_norm(x, ln2.weight, ln2.bias, ln2.eps)
            return training.sequential(self.mlp, h, residual=x)
        h = ops.layer_norm(x, runtime.f32c(ln1.weight), runtime.f32c(ln1.bias), ln1.eps)
        x = ops.add(x, self.attention(h, shapes, batch_size, model_comm_group))
        if self._mlp is None:
            self._mlp = NativeSequential(self.mlp)
        h = ops.layer_norm(x, runtime.f32c(ln2.weight), runtime.f32c(ln2.bias), ln2.eps)
        return self._mlp(h, residual=x)

    def forward(self, x: Tensor, shapes: list, batch_size: int, model_comm_group=None, cond: Optional[Tensor] = None) -> Tensor:
        self._check_cond(cond, _group_size(model_comm_group) > 1)
        if _group_size(model_comm_group) > 1:
            return self._sharded(x, shapes, batch_size, model_comm_group)
        if training.wants_grad(self, x, cond):
            return training.transformer_block(self, x, batch_size, cond)
        dtype = runtime.compute_dtype(x)
        return self.native(_as_compute(x, dtype), batch_size, cond=cond)
