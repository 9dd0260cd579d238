"""Times qk_norm (anemoi_head_norm / _backward) at config 3's shapes against the byte floor, the plain LayerNorm and the route
composed from existing operations, and one Transformer block and one GraphTransformer processor block with and without it.

    python tools/head_norm_bench.py [--iters 50] [--out profiles/qk_norm.md]

Kernels, bf16 and f32: rows = 40 962, groups = 2 (the mesh: q | k inside one product) and rows = 542 080, groups = 1 (the grid: a
mapper's q or k), H = 16, D = 64.  Next to each time: the byte floor 2 rows groups H D sizeof over the HBM peak (8.0 TB/s spec,
6.29 TB/s measured by a float4 copy), ``ops.layer_norm`` on [40 962, 1024] of the same dtype (the run's own baseline), and the
composed route, per tensor: slice copy -> ``ops.layer_norm`` on the [rows H, D] view with its weight -> copy back.

Blocks at config 3's size (40 962 mesh nodes, 1024 channels, 16 heads; the GraphTransformer block on the ico-6 multi-scale mesh
edges, 12 edge attributes), bf16 inference, in one process, alternating: without qk_norm, without qk_norm and the lin_edge fold
switched off (ANEMOI_AMD_EDGE_FOLD=0: what leaving the folded route costs on its own), with qk_norm.

Every figure is the median of ``--iters`` calls, each between its own pair of device events, after warm-up; the spread is the
10th .. 90th percentile.  The variants of a table are timed in alternating rounds.
"""

from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda"
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12  # bytes / s


def timed_alternating(fns: dict, iters: int, rounds: int = 5) -> dict:
    """``{name: (median ms, p10 ms, p90 ms)}``: every function warmed up, then ``rounds`` rounds over all of them in turn."""
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    per_round = max(1, iters // rounds)
    for _ in range(rounds):
        for name, fn in fns.items():
            for _ in range(per_round):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ms[name].append(a.elapsed_time(b))
    out = {}
    for name, v in ms.items():
        v = sorted(v)
        out[name] = (v[len(v) // 2], v[len(v) // 10], v[(9 * len(v)) // 10])
    return out


def _fmt(t) -> str:
    return f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"


def kernel_table(iters: int) -> list:
    from anemoi_models_amd import autograd, ops

    lines = ["| dtype | rows | groups | floor ms at 8.0 / 6.29 TB/s | fused fwd ms | share of the copy rate | LayerNorm [40962, 1024] ms | "
             "composed fwd ms | fused fwd+bwd ms | composed fwd+bwd ms |", "|---|---|---|---|---|---|---|---|---|---|"]
    h, d = 16, 64
    for dtype in (torch.bfloat16, torch.float32):
        g = torch.Generator().manual_seed(0)
        ln_x = torch.randn(40962, 1024, generator=g).to(DEV, dtype)
        ones, zeros = torch.ones(1024, device=DEV), torch.zeros(1024, device=DEV)
        for rows, groups in ((40962, 2), (542080, 1)):
            c = h * d
            total = 3 * c if groups == 2 else 2 * c  # q | k | v of lin_qkv; x_r | q of a mapper's destination product
            col0 = 0 if groups == 2 else c
            width = groups * c
            full = torch.randn(rows, total, generator=g).to(DEV, dtype)
            dy = torch.randn(rows, total, generator=g).to(DEV, dtype)
            w = (1.0 + 0.2 * torch.randn(groups, d, generator=g)).to(DEV)
            d_zeros = torch.zeros(d, device=DEV)
            w_g = [w[i].contiguous() for i in range(groups)]
            view = full[:, col0:col0 + width]
            floor = 2 * rows * width * full.element_size()

            def fused():
                ops.head_norm(view, w, h, groups, out=view)

            def composed():  # per tensor: slice copy -> LayerNorm over the [rows H, D] view with its weight -> copy back
                for i in range(groups):
                    part = view[:, i * c:(i + 1) * c]
                    t = ops.layer_norm(part.contiguous().view(rows * h, d), w_g[i], d_zeros)
                    part.copy_(t.view(rows, c))

            leaf = full.clone().requires_grad_()
            w_leaf = w.clone().requires_grad_()

            def fused_both():
                leaf.grad = w_leaf.grad = None
                autograd.head_norm(leaf, w_leaf, h, groups, 1e-5, col0, width).backward(dy)

            def composed_both():
                leaf.grad = w_leaf.grad = None
                parts = [leaf[:, :col0]]
                for i in range(groups):
                    t = autograd.layer_norm(leaf[:, col0 + i * c:col0 + (i + 1) * c].reshape(rows * h, d), w_leaf[i], d_zeros)
                    parts.append(t.view(rows, c))
                torch.cat(parts + [leaf[:, col0 + width:]], dim=1).backward(dy)

            with torch.no_grad():
                fwd = timed_alternating({"fused": fused, "composed": composed,
                                         "ln": lambda: ops.layer_norm(ln_x, ones, zeros)}, iters)
            both = timed_alternating({"fused": fused_both, "composed": composed_both}, max(10, iters // 2))
            lines.append(f"| {str(dtype)[6:]} | {rows} | {groups} | {floor / HBM_SPEC * 1e3:.3f} / {floor / HBM_COPY * 1e3:.3f} | "
                         f"{_fmt(fwd['fused'])} | {floor / HBM_COPY * 1e3 / fwd['fused'][0]:.2f} | {_fmt(fwd['ln'])} | "
                         f"{_fmt(fwd['composed'])} | {_fmt(both['fused'])} | {_fmt(both['composed'])} |")
            print(lines[-1], flush=True)
            del full, dy, leaf
    return lines


def _mesh_edges(refinement: int = 6):
    from anemoi_models_amd.graphs.synthetic import icosphere, multiscale_mesh_edges

    xyz, levels = icosphere(refinement)
    return xyz.shape[0], torch.from_numpy(multiscale_mesh_edges(levels)).long()


def block_table(iters: int) -> list:
    from anemoi_models_amd.layers.block import GraphTransformerProcessorBlock, TransformerProcessorBlock

    os.environ["ANEMOI_AMD_DTYPE"] = "bf16"
    c, h = 1024, 16
    n, ei = _mesh_edges()
    torch.manual_seed(0)
    x = torch.randn(n, c, device=DEV)
    lines = ["| block | variant | forward ms | against the plain block |", "|---|---|---|---|"]
    with torch.no_grad():
        kw = dict(num_channels=c, hidden_dim=4 * c, num_heads=h, activation="GELU", window_size=None)
        tfm = {"plain": TransformerProcessorBlock(**kw).to(DEV).eval(), "qk_norm": TransformerProcessorBlock(**kw, qk_norm=True).to(DEV).eval()}
        tfm["plain, op by op"] = TransformerProcessorBlock(**kw).to(DEV).eval()
        tfm["plain, op by op"].block_abi = False
        t = timed_alternating({k: (lambda b=b: b(x, None, 1)) for k, b in tfm.items()}, iters)
        for k in tfm:
            lines.append(f"| Transformer | {k} | {_fmt(t[k])} | {t[k][0] / t['plain'][0]:.3f} |")
            print(lines[-1], flush=True)
        del tfm
        edge_dim = 12
        ea = torch.randn(ei.shape[1], edge_dim, device=DEV)
        eid = ei.to(DEV)
        kw = dict(in_channels=c, hidden_dim=4 * c, out_channels=c, edge_dim=edge_dim, num_heads=h)
        plain = GraphTransformerProcessorBlock(**kw).to(DEV).eval()
        normed = GraphTransformerProcessorBlock(**kw, qk_norm=True).to(DEV).eval()

        def unfolded():  # the plain block with the lin_edge fold switched off: the route qk_norm takes, without the norm
            os.environ["ANEMOI_AMD_EDGE_FOLD"] = "0"
            try:
                plain(x, ea, eid, None, 1)
            finally:
                os.environ.pop("ANEMOI_AMD_EDGE_FOLD", None)

        t = timed_alternating({"plain": lambda: plain(x, ea, eid, None, 1), "plain, fold off": unfolded,
                               "qk_norm": lambda: normed(x, ea, eid, None, 1)}, iters)
        for k in t:
            lines.append(f"| GraphTransformer ({ei.shape[1]} edges) | {k} | {_fmt(t[k])} | {t[k][0] / t['plain'][0]:.3f} |")
            print(lines[-1], flush=True)
        lines += ["", f"Leaving the folded route costs {t['plain, fold off'][0] - t['plain'][0]:.3f} ms per block, the norm itself "
                      f"{t['qk_norm'][0] - t['plain, fold off'][0]:.3f} ms."]
    os.environ.pop("ANEMOI_AMD_DTYPE", None)
    return lines


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None, help="also write the tables to this file (markdown)")
    ap.add_argument("--skip-blocks", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_norm_bench: needs an MI355X (a CPU timing says nothing about the kernels)")
    lines = ["# qk_norm: anemoi_head_norm at config 3's shapes", "",
             f"`python tools/head_norm_bench.py --iters {args.iters}`: median ms (10th .. 90th percentile) of calls timed one by one "
             "between device events, the variants of a row in alternating rounds.", "",
             "## Kernels: H = 16, D = 64, in place on the q | k columns (forward), out of place through autograd (forward + backward)",
             ""] + kernel_table(args.iters)
    if not args.skip_blocks:
        lines += ["", "## Blocks: 40 962 nodes, 1024 channels, 16 heads, bf16 inference", ""] + block_table(args.iters)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
