"""Times the bounding stage of a training step: the module route (a gather, an activation and an index_put per module, torch's
index accumulation per module in the backward) against the fused pair anemoi_bound_output_train / anemoi_bound_output_backward.

    python tools/bounding_bench.py [--iters 30] [--rounds 5] [--steps 5] [--no-step] [--out profiles/bounding_train.md]

* the stage alone, forward + backward, on config 3's output shape (542 080 rows, 80 columns, f32): the three-module list of the
  repo's tests (ReLU, hardtanh, fraction) and its leaky twin, A (module route) and B (fused pair) alternated ``--rounds`` times,
  each figure the median of ``--iters`` event-timed calls after warm-up, with the spread (min .. max) of those calls;
* the pair's time against its byte count -- g read and dx written once, the tape written once and read once, y read and
  written where the forward touches it -- and against the 8 TB/s HBM peak of an MI355X;
* one whole config-3 training step (bench.py's model with the three-module list attached) with ANEMOI_AMD_TRAIN_FUSED_BOUND=0 and 1,
  alternated step by step, medians of ``--steps`` pairs.
"""

from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda"
HBM_PEAK = 8.0e12
ROWS, V_OUT = 542080, 80
A = "anemoi_models_amd.layers.bounding."
HARD = [
    {"_target_": A + "ReluBounding", "variables": ["prog_0", "prog_5"]},
    {"_target_": A + "HardtanhBounding", "variables": ["prog_1", "prog_0"], "min_val": -0.5, "max_val": 0.75},
    {"_target_": A + "FractionBounding", "variables": ["prog_3", "prog_2"], "min_val": 0.0, "max_val": 1.0, "total_var": "prog_4"},
]
LEAKY = [dict(b, _target_=b["_target_"].replace("bounding.", "bounding.Leaky")) for b in HARD]


def timed(fn, iters: int):
    """``(median, min, max)`` milliseconds of ``fn`` over ``iters`` calls, each between its own pair of events, after 5 warm-up
    calls."""
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
    return statistics.median(ms), min(ms), max(ms)


def modules_of(configs):
    from anemoi_models_amd.utils.config import instantiate

    n2i = {f"prog_{i}": i for i in range(V_OUT)}
    return [instantiate(c, name_to_index=n2i) for c in configs]


def plan_of(modules):
    from anemoi_models_amd.layers.bounding import bounding_slopes, compile_boundings

    ops, slopes = compile_boundings(modules), bounding_slopes(modules)
    slopes = [0.0] * len(ops) if slopes is None else slopes
    t = lambda i, dt: torch.tensor([o[i] for o in ops], dtype=dt, device=DEV)  # noqa: E731
    lists = (t(0, torch.int32), t(1, torch.float32), t(2, torch.float32), t(3, torch.int32))
    return lists, torch.tensor(slopes, dtype=torch.float32, device=DEV), len(ops) + sum(o[3] >= 0 for o in ops), ops


def stage(name: str, configs, iters: int, rounds: int) -> list:
    from anemoi_models_amd import autograd, ops

    modules = modules_of(configs)
    lists, slope, n_tape, op_list = plan_of(modules)
    gen = torch.Generator().manual_seed(0)
    base = torch.randn(ROWS, V_OUT, generator=gen).to(DEV)
    dy = torch.randn(ROWS, V_OUT, generator=gen).to(DEV)
    leaf = base.clone().requires_grad_()

    def module_route():
        leaf.grad = None
        y = leaf.clone()  # (the fresh output of the residual: both routes pay this copy)
        for m in modules:
            y = m(y)
        y.backward(dy)

    def fused_pair():
        leaf.grad = None
        autograd.bound_output(leaf.clone(), lists, slope, n_tape).backward(dy)

    lines = [f"### {name}: {len(modules)} modules, {len(op_list)} ops, {n_tape} tape entries per row", "",
             "| round | module route ms (min .. max) | fused pair ms (min .. max) | ratio |", "|---|---|---|---|"]
    verdict = True
    for r in range(rounds):
        a, b = timed(module_route, iters), timed(fused_pair, iters)
        verdict &= b[0] <= a[0]
        lines.append(f"| {r + 1} | {a[0]:.3f} ({a[1]:.3f} .. {a[2]:.3f}) | {b[0]:.3f} ({b[1]:.3f} .. {b[2]:.3f}) | x{a[0] / b[0]:.2f} |")
        print(lines[-1], flush=True)
    lines += ["", f"Fused pair's median at or below the module route's in every round: {'yes' if verdict else 'NO'}.", ""]

    # the two launches alone against their bytes: every operand once
    touched = len({o[0] for o in op_list} | {o[3] for o in op_list if o[3] >= 0})
    y = base.clone()
    tape = ops.bound_output_train(y, *lists, slope, n_tape)
    fwd = timed(lambda: ops.bound_output_train(y, *lists, slope, n_tape), iters)
    bwd = timed(lambda: ops.bound_output_backward(dy, tape, *lists, slope), iters)
    # forward: the touched columns of y in 64-byte sectors read and written (a row of 320 bytes is 5 sectors: counted whole when
    # the columns spread over all of them) and the tape written; backward: g read, dx written, the tape read
    f_bytes = ROWS * (2 * min(touched * 64, V_OUT * 4) + n_tape * 4)
    b_bytes = ROWS * (2 * V_OUT * 4 + n_tape * 4)
    lines += ["| launch | ms (min .. max) | bytes MB | GB/s | of HBM peak |", "|---|---|---|---|---|"]
    for what, t, nbytes in (("anemoi_bound_output_train", fwd, f_bytes), ("anemoi_bound_output_backward", bwd, b_bytes)):
        rate = nbytes / t[0] / 1e6
        lines.append(f"| {what} | {t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f}) | {nbytes / 1e6:.1f} | {rate:.0f} | {100 * rate * 1e9 / HBM_PEAK:.1f} % |")
        print(lines[-1], flush=True)
    lines.append("")
    return lines, verdict


def whole_step(steps: int) -> list:
    import time

    import bench

    os.environ.setdefault("ANEMOI_AMD_DTYPE", "bf16")
    model, graph, x, _ = bench.build("cfg3", torch.device("cuda", 0))
    model.boundings = torch.nn.ModuleList(modules_of(HARD))
    model.train()
    target = torch.zeros((1, 1, graph["data"].num_nodes, V_OUT), device=DEV)

    def step():
        loss = ((model(x) - target) ** 2).mean()
        loss.backward()
        for p in model.parameters():
            p.grad = None
        return float(loss.detach())  # (synchronises)

    times, losses = {"0": [], "1": []}, {}
    for mode in times:  # plans and allocator warm-up of both routes
        os.environ["ANEMOI_AMD_TRAIN_FUSED_BOUND"] = mode
        step(), step()
    for _ in range(steps):
        for mode in times:
            os.environ["ANEMOI_AMD_TRAIN_FUSED_BOUND"] = mode
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            losses[mode] = step()
            times[mode].append((time.perf_counter() - t0) * 1e3)
    os.environ.pop("ANEMOI_AMD_TRAIN_FUSED_BOUND")
    a, b = statistics.median(times["0"]), statistics.median(times["1"])
    line = (f"Config-3 training step ({os.environ['ANEMOI_AMD_DTYPE']}, three-module list): module route {a:.1f} ms "
            f"({min(times['0']):.1f} .. {max(times['0']):.1f}), fused pair {b:.1f} ms ({min(times['1']):.1f} .. {max(times['1']):.1f}); "
            f"medians of {steps} alternated steps; loss {losses['0']:.6f} / {losses['1']:.6f}")
    print(line, flush=True)
    return ["### Whole step", "", line, ""]


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5, help="A/B alternations of the stage-alone comparison")
    ap.add_argument("--steps", type=int, default=5, help="alternated pairs of whole training steps")
    ap.add_argument("--no-step", action="store_true", help="skip the whole config-3 training step")
    ap.add_argument("--out", default=None, help="also write the tables to this file (markdown)")
    args = ap.parse_args()
    lines = [f"## Bounding stage of a training step: {ROWS} rows, V_out = {V_OUT}, f32", ""]
    ok = True
    for name, configs in (("three-module list (ReLU, hardtanh, fraction)", HARD), ("leaky twin", LEAKY)):
        more, verdict = stage(name, configs, args.iters, args.rounds)
        lines += more
        ok &= verdict
    lines += [f"Acceptance for the default being on (both lists, every round): {'met' if ok else 'NOT met'}.", ""]
    if not args.no_step:
        lines += whole_step(args.steps)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
