#!/usr/bin/env python
"""Rollout training step (n forward steps chained by the state advance, weighted loss over the stack, one backward) of the flat
GraphTransformer model in bf16 at a bench workload, eager and as one HIP graph (runtime.GraphedTrainStep):
   python tools/rollout_train_bench.py [cfg2|cfg3] [--steps 1,2,3,4] [--pairs 5] [--no-graph] [--out FILE]
Two sides, alternated step by step in this one process (medians over ``--pairs`` pairs):
   A  training.RolloutModel + WeightedMSELoss: autograd.advance_input, the one-pass I/O kernels kept from step 2 on
      (anemoi_assemble_nodes / anemoi_finalize_output and their input gradients), the loss and its gradient on their kernels;
   B  what the package could express before: the same loop on plain ``model(x)`` (the generic torch input route once the input
      requires a gradient, as under ANEMOI_AMD_ROLLOUT_FUSED=0), the advance as roll + index writes, the loss as torch ops.
Reported per n: ms per step of both sides, the seam cost t(n) - n t(1), the peak memory of an eager step, and -- for the
``accumulate`` question -- what ONE add pass over the state gradient costs (autograd runs two per seam on side A: the state
feeds the input assembly, the prognostic residual and the next advance)."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("workload", nargs="?", default="cfg3")
ap.add_argument("--steps", default="1,2,3,4")
ap.add_argument("--pairs", type=int, default=5)
ap.add_argument("--no-graph", action="store_true")
ap.add_argument("--out", default=None, help="append the report lines to this file too")
args = ap.parse_args()
os.environ.setdefault("ANEMOI_AMD_DTYPE", "bf16")

from anemoi_models_amd import WeightedMSELoss  # noqa: E402
from anemoi_models_amd.runtime import GraphedTrainStep  # noqa: E402
from anemoi_models_amd.training import RolloutModel  # noqa: E402
from anemoi_models_amd.utils.indices import advance_colmap  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("rollout_train_bench: needs an MI355X (nothing is measured without one)")
dev = torch.device("cuda", 0)
model, graph, x, idx = bench.build(args.workload, dev)
model.train()
g, v_out = graph["data"].num_nodes, idx.num_output
gen = torch.Generator().manual_seed(3)
node_w = (torch.rand(g, generator=gen) + 0.1).to(dev)
var_w = (torch.rand(v_out, generator=gen) + 0.5).to(dev)
loss_a = WeightedMSELoss(node_w, var_w).to(dev)
w_hat = loss_a.node_weights
colmap = advance_colmap(idx).tolist()
pin = torch.tensor([v for v, m in enumerate(colmap) if m >= 0], device=dev)
pout = torch.tensor([m for m in colmap if m >= 0], device=dev)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def loss_b(y, t):  # the same formula as torch ops
    return (w_hat[:, None] * var_w[None, :] * (y - t) ** 2).sum() / (y.shape[0] * y.shape[1] * y.shape[2] * y.shape[-1])


class TorchRollout(torch.nn.Module):
    def __init__(self, n):
        super().__init__()
        self.model, self.n = model, n

    def forward(self, x):
        outs = []
        for s in range(self.n):
            y = self.model(x)
            outs.append(y)
            if s + 1 < self.n:
                nxt = x.roll(-1, dims=1)
                nxt[:, -1] = x[:, -1]
                nxt[:, -1, :, :, pin] = y[..., pout].to(x.dtype)
                x = nxt
        return torch.stack(outs)


def zero():
    for p in model.parameters():
        p.grad = None


def eager(mod, loss_fn, targets):
    def step():
        zero()
        loss = loss_fn(mod(x), targets)
        loss.backward()
        return float(loss.detach())  # (synchronises)
    return step


def alternate(step_a, step_b, pairs):
    ta, tb, la, lb = [], [], 0.0, 0.0
    for _ in range(2):  # plans, allocator and code objects of both sides
        step_a(), step_b()
    for _ in range(pairs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        la = step_a()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        lb = step_b()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        ta.append((t1 - t0) * 1e3)
        tb.append((t2 - t1) * 1e3)
    return statistics.median(ta), statistics.median(tb), (min(ta), max(ta)), (min(tb), max(tb)), la, lb


def peak(step):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() / 2**30


say(f"# rollout training, {args.workload} bf16 on {torch.cuda.get_device_name(0)}: grid {g}, {idx.num_input} input / {v_out} "
    f"output variables; medians of {args.pairs} alternated pairs (min .. max in brackets)")
res = {}
for n in [int(s) for s in args.steps.split(",")]:
    targets = torch.randn((n, 1, 1, g, v_out), generator=torch.Generator().manual_seed(n)).to(dev)
    mod_a, mod_b = RolloutModel(model, idx, n), TorchRollout(n)
    sa, sb = eager(mod_a, loss_a, targets), eager(mod_b, loss_b, targets)
    a, b, ra, rb, la, lb = alternate(sa, sb, args.pairs)
    pa, pb = peak(sa), peak(sb)
    res[n] = {"eager": (a, b)}
    say(f"n_steps={n} eager : A {a:8.1f} ms [{ra[0]:.1f} .. {ra[1]:.1f}]  B {b:8.1f} ms [{rb[0]:.1f} .. {rb[1]:.1f}]  B/A x{b / a:.3f}  "
        f"peak memory A {pa:.1f} GiB  B {pb:.1f} GiB  loss A {la:.6f}  B {lb:.6f}")
    if not args.no_graph:
        zero()
        ga = GraphedTrainStep(mod_a, loss_a, x, targets)
        zero()
        gb = GraphedTrainStep(mod_b, loss_b, x, targets)
        a, b, ra, rb, la, lb = alternate(lambda: float(ga(x, targets)), lambda: float(gb(x, targets)), args.pairs)
        res[n]["graph"] = (a, b)
        say(f"n_steps={n} graph : A {a:8.1f} ms [{ra[0]:.1f} .. {ra[1]:.1f}]  B {b:8.1f} ms [{rb[0]:.1f} .. {rb[1]:.1f}]  B/A x{b / a:.3f}  "
            f"loss A {la:.6f}  B {lb:.6f}")
        del ga, gb
        zero()
        torch.cuda.empty_cache()
if 1 in res:
    for kind in ("eager", "graph"):
        for n in sorted(res):
            if n > 1 and kind in res[n] and kind in res[1]:
                (a, b), (a1, b1) = res[n][kind], res[1][kind]
                say(f"seam cost {kind} n_steps={n}: t(n) - n t(1) = A {a - n * a1:+.1f} ms  B {b - n * b1:+.1f} ms "
                    f"(per seam A {(a - n * a1) / (n - 1):+.2f}  B {(b - n * b1) / (n - 1):+.2f})")
# the accumulate question: one add pass over a state-gradient sized tensor
d1, d2 = torch.randn_like(x), torch.randn_like(x)
for _ in range(3):
    d1.add_(d2)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(50):
    d1.add_(d2)
torch.cuda.synchronize()
say(f"one add pass over the state gradient {tuple(x.shape)} f32: {(time.perf_counter() - t0) / 50 * 1e3:.3f} ms "
    f"(an accumulate flag on the three dx producers would save two of them per seam)")
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
