"""Times the fused conditional LayerNorm (anemoi_cond_layer_norm / _backward) against the route composed from a Linear, a
LayerNorm and element-wise passes, and against the plain LayerNorm, and a whole training step of a small ensemble model on the
fused against the composed route.

    python tools/cond_ln_bench.py [--iters 30] [--out profiles/ens_noise.md]

Shapes: rows = 40 962 x {1, 4} (the O96 mesh, one and four members), C = 1024, K in {4, 16, 32}, bf16 and f32.  Bytes over time
are printed next to the byte floor rows C 2 sizeof(T) + rows K 4 (x read, y written, cond read).
"""

from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda"


def timed(fn, iters: int) -> float:
    """Median milliseconds of ``fn`` over ``iters`` launches, each between its own pair of events, after 5 warm-up calls."""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2]


def kernel_table(iters: int) -> list:
    from anemoi_models_amd import autograd, ops

    lines = ["| dtype | rows | K | LN fwd ms | fused fwd ms | GB/s of floor | x LN | composed fwd ms | LN bwd ms | fused bwd ms "
             "| composed fwd+bwd ms | fused fwd+bwd ms |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    c = 1024
    for dtype in (torch.bfloat16, torch.float32):
        for rows in (40962, 4 * 40962):
            g = torch.Generator().manual_seed(0)
            x = torch.randn(rows, c, generator=g).to(DEV, dtype)
            dy = torch.randn(rows, c, generator=g).to(DEV, dtype)
            ones, zeros = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
            ln_f = timed(lambda: ops.layer_norm(x, ones, zeros), iters)
            _, st = ops.layer_norm_with_stats(x, ones, zeros)
            ln_b = timed(lambda: ops.layer_norm_backward(x, st, ones, dy), iters)
            for k in (4, 16, 32):
                cond = torch.randn(rows, k, generator=g).to(DEV)
                ws, wb = (torch.randn(c, k, generator=g).to(DEV) / k**0.5 for _ in range(2))
                bs, bb = (0.1 * torch.randn(c, generator=g).to(DEV) for _ in range(2))
                floor = rows * c * 2 * x.element_size() + rows * k * 4
                f_f = timed(lambda: ops.cond_layer_norm(x, cond, ws, bs, wb, bb), iters)
                _, stats = ops.cond_layer_norm(x, cond, ws, bs, wb, bb, with_stats=True)
                f_b = timed(lambda: ops.cond_layer_norm_backward(dy, x, stats, cond, ws, bs, wb), iters)
                with torch.no_grad():
                    c_f = timed(lambda: autograd.cond_layer_norm_composed(x, cond, ws, bs, wb, bb), iters)
                leaves = [t.clone().requires_grad_() for t in (x, cond, ws, bs, wb, bb)]

                def both(fn):
                    for t in leaves:
                        t.grad = None
                    fn(*leaves).backward(dy)

                c_fb = timed(lambda: both(autograd.cond_layer_norm_composed), iters)
                f_fb = timed(lambda: both(autograd.cond_layer_norm), iters)
                lines.append(f"| {str(dtype)[6:]} | {rows} | {k} | {ln_f:.3f} | {f_f:.3f} | {floor / f_f / 1e6:.0f} | "
                             f"{f_f / ln_f:.2f} | {c_f:.3f} | {ln_b:.3f} | {f_b:.3f} | {c_fb:.3f} | {f_fb:.3f} |")
                print(lines[-1], flush=True)
    return lines


def step_table(iters: int) -> list:
    """One training step (forward, almost-fair CRPS, backward) of a 3-member ensemble model on the O32 test graph."""
    from anemoi_models_amd import AlmostFairKernelCRPS
    from anemoi_models_amd.graphs.synthetic import build_graph
    from anemoi_models_amd.models import AnemoiEnsModelEncProcDec
    from anemoi_models_amd.utils.indices import SimpleDataIndices
    from anemoi_models_amd.utils.presets import model_config

    graph = build_graph("o32_ico2")
    idx = SimpleDataIndices(n_prognostic=10, n_forcing=2, n_diagnostic=1)
    lines = ["| dtype | channels | K | route | step ms |", "|---|---|---|---|---|"]
    for dtype_name in ("bf16", "fp32"):
        os.environ["ANEMOI_AMD_DTYPE"] = dtype_name
        for k in (4, 16):
            torch.manual_seed(0)
            noise = {"noise_std": 1.0, "noise_channels_dim": k, "noise_mlp_hidden_dim": 32}
            model = AnemoiEnsModelEncProcDec(model_config=model_config("Transformer", 256, 4, noise_injector=noise),
                                             data_indices=idx, graph_data=graph).to(DEV).train()
            n = graph["data"].num_nodes
            x = torch.randn(1, 2, 3, n, idx.num_input, device=DEV)
            target = torch.randn(1, n, model.num_output_channels, device=DEV)
            loss_fn = AlmostFairKernelCRPS(torch.ones(n), alpha=0.95).to(DEV)

            def step():
                for p in model.parameters():
                    p.grad = None
                loss_fn(model(x), target).backward()

            for route in ("fused", "composed"):
                os.environ["ANEMOI_AMD_COND_LN"] = route
                lines.append(f"| {dtype_name} | 256 | {k} | {route} | {timed(step, iters):.3f} |")
                print(lines[-1], flush=True)
            os.environ.pop("ANEMOI_AMD_COND_LN", None)
    os.environ.pop("ANEMOI_AMD_DTYPE", None)
    return lines


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None, help="also write the two tables to this file (markdown)")
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    lines = ["## Kernels: C = 1024", ""] + kernel_table(args.iters)
    if not args.skip_step:
        lines += ["", "## Training step: 3 members, O32 grid, Transformer processor (4 layers), almost-fair CRPS", ""]
        lines += step_table(max(5, args.iters // 3))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
