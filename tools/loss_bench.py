#!/usr/bin/env python
"""Timings of the loss family (csrc/losses.hip) at the benchmark's own grids, next to the scalar ``weighted_mse`` kernel and the
torch composition of the same loss measured in the same process.

    python tools/loss_bench.py [--vars 80] [--iters 20] [--out profiles/loss_family_bench.md]

Sizes: config 3's grid (N320, 542 080 nodes) and config 2's (O96, 40 320 nodes) x the model's output width, 1 and 4 rollout
steps.  Every line is the median of ``--iters`` device-event timings after 3 warm-up calls; GB/s is the bytes the algorithm
needs (forward: both operands read once, backward: both read and dpred written) over that time.  Needs an MI355X: there is no
CPU path to time."""

from __future__ import annotations

import argparse
import os
import statistics
import sys
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GRIDS = (("cfg3 N320", 542080), ("cfg2 O96", 40320))
KINDS = ("mse", "mae", "huber", "logcosh")


def timed(fn, iters):
    for _ in range(3):
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
    return statistics.median(ms)


def torch_pointwise(kind, d, delta=1.0):
    if kind == "mse":
        return d * d
    a = d.abs()
    if kind == "mae":
        return a
    if kind == "huber":
        return torch.where(a <= delta, 0.5 * d * d, delta * (a - 0.5 * delta))
    return a + torch.log1p(torch.exp(-2.0 * a)) - 0.6931471805599453


def torch_loss(kind, pred, target, w, s, squash):
    """The torch composition a user of the package writes today: [steps, B, Ens, G, V] -> a scalar or [steps, V]."""
    out = (torch_pointwise(kind, pred - target) * w[:, None] * s).sum(-2).mean((1, 2))
    return out.mean() if squash else out


def normalizer(n_out, n_forcing, dev):
    from anemoi_models_amd.preprocessing.normalizer import InputNormalizer
    from anemoi_models_amd.utils.indices import SimpleDataIndices

    n = n_out + n_forcing
    rng = np.random.default_rng(0)
    stats = {"minimum": np.zeros(n), "maximum": np.ones(n), "mean": rng.normal(size=n) * 50.0,
             "stdev": rng.uniform(0.5, 20.0, size=n)}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return InputNormalizer({"default": "mean-std"}, SimpleDataIndices(n_out, n_forcing, 0), stats).to(dev)


def trainer_metrics(norm, pred, target, w):
    """The trainer's torch form of the validation metrics: de-normalise both operands, then one reduction per variable."""
    pp, tp = norm.inverse_transform(pred, in_place=False), norm.inverse_transform(target, in_place=False)
    out = []
    for v in range(pred.shape[-1]):
        out.append((((pp[..., v] - tp[..., v]) ** 2) * w).sum(-1).mean((1, 2)))
    return torch.stack(out, -1)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--vars", type=int, default=80, help="output variables of the model (bench.py: 80 prognostic)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("loss_bench: no GPU -- these are device timings, there is nothing to measure on the CPU")
    from anemoi_models_amd import ValidationMetrics, ops

    dev, v = "cuda", args.vars
    lines = ["| grid x steps | what | kind | forward ms | forward GB/s | backward ms | backward GB/s |", "|---|---|---|---|---|---|---|"]

    def row(size, what, kind, n_elem, fwd, bwd):
        gb = lambda nbytes, ms: "-" if ms is None else f"{nbytes / ms / 1e6:.0f}"  # noqa: E731
        f = lambda ms: "-" if ms is None else f"{ms:.3f}"  # noqa: E731
        lines.append(f"| {size} | {what} | {kind} | {f(fwd)} | {gb(8 * n_elem, fwd)} | {f(bwd)} | {gb(12 * n_elem, bwd)} |")
        print(lines[-1], flush=True)

    print("\n".join(lines), flush=True)
    for grid_name, g in GRIDS:
        for steps in (1, 4):
            size = f"{grid_name} x {steps}"
            gen = torch.Generator(device=dev).manual_seed(steps)
            pred = torch.randn((steps, 1, 1, g, v), device=dev, generator=gen)
            target = torch.randn((steps, 1, 1, g, v), device=dev, generator=gen)
            w = torch.rand(g, device=dev, generator=gen) + 0.1
            w = w / w.sum()
            s = torch.rand(v, device=dev, generator=gen) + 0.5
            p2, t2, n = pred.view(-1, v), target.view(-1, v), pred.numel()
            one = torch.ones((), device=dev)
            row(size, "weighted_mse (scalar kernel)", "mse", n, timed(lambda: ops.weighted_mse(p2, t2, w, s, None, 1.0 / steps), args.iters),
                timed(lambda: ops.weighted_mse_backward(p2, t2, w, s, None, 1.0 / steps, one), args.iters))
            for kind in KINDS:
                for what, groups in (("weighted_error squashed", 1), ("weighted_error per variable", steps)):
                    up = torch.full((groups, v), 1.0 / v, device=dev)
                    kw = dict(col_w=s, n_groups=groups, scale=groups / steps)
                    if groups == 1:
                        fwd = timed(lambda: ops.weighted_error(p2, t2, w, kind, **kw).mean(), args.iters)
                    else:
                        fwd = timed(lambda: ops.weighted_error(p2, t2, w, kind, **kw), args.iters)
                    bwd = timed(lambda: ops.weighted_error_backward(p2, t2, w, kind, upstream=up, **kw), args.iters)
                    row(size, what, kind, n, fwd, bwd)
                for what, squash in (("torch composition squashed", True), ("torch composition per variable", False)):
                    pg = pred.detach().requires_grad_()
                    with torch.no_grad():
                        fwd = timed(lambda: torch_loss(kind, pg, target, w, s, squash), max(args.iters // 2, 3))
                    out = torch_loss(kind, pg, target, w, s, squash)
                    go = torch.ones_like(out)
                    bwd = timed(lambda: torch.autograd.grad(out, pg, go, retain_graph=True), max(args.iters // 2, 3))
                    row(size, what, kind, n, fwd, bwd)
                    del out, pg
            norm = normalizer(v, 10, dev)
            vm = ValidationMetrics(w, norm, kinds=("mse",)).to(dev)
            row(size, "ValidationMetrics (one launch pair)", "mse", n, timed(lambda: vm(pred, target), args.iters), None)
            with torch.no_grad():
                row(size, "trainer's torch metrics (de-normalise, V reductions)", "mse", n,
                    timed(lambda: trainer_metrics(norm, pred, target, w), 3), None)
            a, b = vm(pred, target)["mse"], trainer_metrics(norm, pred, target, w)
            print(f"  ValidationMetrics vs the torch form at {size}: largest relative difference "
                  f"{float(((a - b).abs() / b.abs()).max()):.2e}", flush=True)
            del pred, target, p2, t2
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
