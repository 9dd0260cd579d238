#!/usr/bin/env python
"""Timings of the ensemble scores (csrc/ensemble.hip) at config 3's output size, next to the explicit torch route measured in
the same process, and against the byte floor.

    python tools/ensemble_loss_bench.py [--vars 80] [--members 2,4,8,16] [--iters 15] [--out table.md]

``--out`` writes the raw table only; the written profile, which quotes that table and says what it shows, is
``profiles/ensemble_loss.md``.

Size: config 3's grid (N320, 542 080 nodes) x the model's output width, B = 1, one step, E members.  The two routes alternate
call by call in one process; every figure is the median of ``--iters`` device-event timings after 3 warm-up calls.  Byte floor:
forward ``(E + 1) * 4`` bytes per point and variable (every member and the target read once), backward ``(2 E + 1) * 4`` (read
again, E gradients written), over the float4-copy rate measured on this chip (launch trail: 6.29 TB/s).  The
explicit route is the almost-fair CRPS in its per-pair form with torch autograd: for E <= 4 the broadcast ``[E, E, G, V]``
tensor, above that a loop over the pairs (the broadcast form needs E^2 x 173 MB per temporary).  Needs an MI355X: there is no CPU
path to time."""

from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GRID = 542080  # config 3, N320
HBM_COPY_GBS = 6290.0  # the measured float4-copy rate, GB/s


def interleaved(fns, iters):
    """Median ms of each callable, the callables taking turns (what drifts -- clocks, a neighbour on the host -- hits all)."""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(iters):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    return [statistics.median(m) for m in ms]


def torch_afcrps(pred, target, w, s, alpha, broadcast):
    """[1, E, G, V], [1, G, V] -> [V]: 1 / (2 E (E - 1)) sum_{j != k} (|x_j - y| + |x_k - y| - (1 - eps) |x_j - x_k|), node
    and variable weights, summed over the grid."""
    e = pred.shape[1]
    eps = (1.0 - alpha) / e
    ay = (pred - target.unsqueeze(1)).abs()
    if broadcast:
        pair = ay.unsqueeze(1) + ay.unsqueeze(2) - (1.0 - eps) * (pred.unsqueeze(1) - pred.unsqueeze(2)).abs()
        off = 1.0 - torch.eye(e, device=pred.device).reshape(1, e, e, 1, 1)
        point = (pair * off).sum((1, 2)) / (2.0 * e * (e - 1))
    else:
        point = None
        for j in range(e):
            for k in range(j + 1, e):
                term = ay[:, j] + ay[:, k] - (1.0 - eps) * (pred[:, j] - pred[:, k]).abs()
                point = term if point is None else point + term
        point = point / (e * (e - 1))  # each unordered pair stands for (j, k) and (k, j)
    return (point * w[:, None] * s).sum((0, 1))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--vars", type=int, default=80, help="output variables of the model (bench.py: 80 prognostic)")
    ap.add_argument("--members", default="2,4,8,16")
    ap.add_argument("--grid", type=int, default=GRID)
    ap.add_argument("--alpha", type=float, default=0.95)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_loss_bench: no GPU -- these are device timings, there is nothing to measure on the CPU")
    from anemoi_models_amd import ops

    dev, v, g = "cuda", args.vars, args.grid
    lines = ["| E | what | forward ms | forward GB/s | x byte floor | backward ms | backward GB/s | x byte floor |",
             "|---|---|---|---|---|---|---|---|"]

    def row(e, what, fwd, bwd):
        fb, bb = (e + 1) * 4 * g * v, (2 * e + 1) * 4 * g * v
        cell = lambda nbytes, ms: f"{ms:.3f} | {nbytes / ms / 1e6:.0f} | {ms / (nbytes / HBM_COPY_GBS / 1e6):.2f}"  # noqa: E731
        lines.append(f"| {e} | {what} | {cell(fb, fwd)} | {cell(bb, bwd)} |")
        print(lines[-1], flush=True)

    print("\n".join(lines), flush=True)
    for e in [int(m) for m in args.members.split(",")]:
        gen = torch.Generator(device=dev).manual_seed(e)
        target = torch.randn((1, g, v), device=dev, generator=gen)
        pred = target.unsqueeze(1) + 0.7 * torch.randn((1, e, g, v), device=dev, generator=gen)
        w = torch.rand(g, device=dev, generator=gen) + 0.1
        w = w / w.sum()
        s = torch.rand(v, device=dev, generator=gen) + 0.5
        up = torch.full((1, v), 1.0 / v, device=dev)
        p2, t2 = pred.view(-1, v), target.view(-1, v)
        kw = dict(n_members=e, alpha=args.alpha, col_w=s)
        routes = [("broadcast [E, E, G, V]", True)] if e <= 4 else []
        routes.append(("pair loop", False))
        for name, broadcast in routes:
            pg = pred.detach().requires_grad_()

            def torch_fwd():
                with torch.no_grad():
                    return torch_afcrps(pg, target, w, s, args.alpha, broadcast)

            out = torch_afcrps(pg, target, w, s, args.alpha, broadcast)
            go = up[0].clone()
            kf, tf = interleaved([lambda: ops.ensemble_score(p2, t2, w, "afcrps", **kw), torch_fwd], args.iters)
            kb, tb = interleaved([lambda: ops.ensemble_score_backward(p2, t2, w, "afcrps", upstream=up, **kw),
                                  lambda: torch.autograd.grad(out, pg, go, retain_graph=True)], args.iters)
            row(e, "anemoi_ensemble_score afcrps", kf, kb)
            row(e, f"torch, {name}", tf, tb)
            got = ops.ensemble_score(p2, t2, w, "afcrps", **kw)[0]
            (tg,) = torch.autograd.grad(out, pg, go, retain_graph=True)
            kg = ops.ensemble_score_backward(p2, t2, w, "afcrps", upstream=up, **kw).view_as(tg)
            print(f"  E={e} kernel vs torch ({name}): value, largest relative difference "
                  f"{float(((got - out.detach()).abs() / out.detach().abs()).max()):.2e}; gradient, of max |dpred| "
                  f"{float((kg - tg).abs().max() / tg.abs().max()):.2e}", flush=True)
            del out, pg, tg, kg
            torch.cuda.empty_cache()
        others = interleaved([lambda: ops.ensemble_score(p2, t2, w, "mean_se", **kw),
                              lambda: ops.ensemble_score(p2, t2, w, "variance", **kw)], args.iters)
        for kind, ms in zip(("mean_se", "variance"), others):
            fb = (e + 1) * 4 * g * v
            lines.append(f"| {e} | anemoi_ensemble_score {kind} | {ms:.3f} | {fb / ms / 1e6:.0f} | "
                         f"{ms / (fb / HBM_COPY_GBS / 1e6):.2f} | - | - | - |")
            print(lines[-1], flush=True)
        del pred, target, p2, t2
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
