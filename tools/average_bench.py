#!/usr/bin/env python
"""Weight averaging and the device LR schedule measured on the MI355X (DESIGN section 7 "8f-11"):

  * the EMA update of ``optim.WeightAverager`` over the parameter list of a bench model (real shapes, random values), eager
    and replayed from a HIP graph, against its byte floor of 12 B per parameter (8 read, 4 written) at the float4-copy rate
    and against ``torch._foreach_lerp_`` on the same list;
  * ``WeightAverager.swap()`` against 16 B per parameter;
  * the launch cost of the two one-wave kernels (``anemoi_average_constants``, ``anemoi_lr_schedule``);
  * one whole ``runtime.GraphedTrainStep`` with ``FusedAdamW`` alone and with averager + schedule attached.

   python tools/average_bench.py [--list cfg3] [--steps cfg2,cfg3] [--rounds 20] [--step-rounds 10]

A run without a GPU fails: there is nothing to measure."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from anemoi_models_amd import _lib  # noqa: E402
from anemoi_models_amd import ops  # noqa: E402
from anemoi_models_amd import optim  # noqa: E402
from tools.optim_bench import COPY_RATE, HYPER, count_launches, timed  # noqa: E402


def _graph_of(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph


def _row(name, r, floor):
    launches = count_launches(r["fn"])
    ratio = f"{statistics.median(r['replay']) / floor:.2f} x" if floor else ""
    print(f"| {name} | {statistics.median(r['eager']):.3f} / {min(r['eager']):.3f} | {statistics.median(r['host']):.3f} | "
          f"{statistics.median(r['replay']):.3f} / {min(r['replay']):.3f} | {launches if launches is not None else 'not measured'} | "
          f"{ratio} |", flush=True)


def list_bench(workload, rounds):
    dev = torch.device("cuda", 0)
    model, _, _, _ = bench.build(workload, dev)
    shapes = [tuple(p.shape) for p in model.parameters() if p.requires_grad]
    del model
    torch.cuda.empty_cache()
    n = sum(int(torch.Size(s).numel()) for s in shapes)
    gen = torch.Generator(device=dev).manual_seed(0)
    params = [torch.randn(s, device=dev, generator=gen) for s in shapes]
    av = optim.WeightAverager(params, kind="ema", decay=0.999)
    av.update()  # the copy; every timed update is the lerp form
    theirs = [p.clone() for p in params]
    small = optim.FusedAdamW([torch.nn.Parameter(torch.zeros(8, device=dev))], **HYPER)
    sched = optim.DeviceLRSchedule(small, warmup_steps=10, total_steps=100)
    sched.detach()
    routes = {
        "WeightAverager.update (EMA)": (av.update, 12),
        "torch._foreach_lerp_": (lambda: torch._foreach_lerp_(theirs, params, 1e-3), 12),
        "WeightAverager.swap": (av.swap, 16),
        "anemoi_average_constants alone": (lambda: ops.average_constants(av._avg, av.n_averaged, decay=0.999), 0),
        "anemoi_lr_schedule alone (1 group)": (sched._launch, 0),
    }
    runs = {name: dict(fn=fn, graph=_graph_of(fn), eager=[], host=[], replay=[]) for name, (fn, _) in routes.items()}
    print(f"{workload}: {len(shapes)} parameter tensors, {n / 1e6:.1f} M parameters; byte floor of the update "
          f"{12 * n / COPY_RATE * 1e3:.3f} ms (12 B / parameter), of the swap {16 * n / COPY_RATE * 1e3:.3f} ms (16 B), at "
          f"{COPY_RATE / 1e12:.2f} TB/s; OPT_CHUNK {_lib.OPT_CHUNK}, OPT_MAX_TENSORS {_lib.OPT_MAX_TENSORS}", flush=True)
    for _ in range(rounds):  # alternated: one round = every route once, eager then replayed
        for r in runs.values():
            r["host"].append(timed(r["fn"], sync=False))
            r["eager"].append(timed(r["fn"]))
            r["replay"].append(timed(r["graph"].replay))
    print("| route | eager ms (median / min) | eager host enqueue ms | graph replay ms (median / min) | launches | "
          "replay / byte floor |", flush=True)
    print("|---|---|---|---|---|---|", flush=True)
    for name, r in runs.items():
        _row(name, r, routes[name][1] * n / COPY_RATE * 1e3)


def step_bench(workload, rounds):
    from anemoi_models_amd.runtime import GraphedTrainStep

    dev = torch.device("cuda", 0)
    steps, graph = {}, None
    loss_fn = lambda y, t: ((y - t) ** 2).mean()  # noqa: E731
    for name in ("fusedadamw", "fusedadamw + averager + schedule"):
        model, graph, x, _ = bench.build(workload, dev, graph=graph)
        model.train()
        target = torch.zeros((1, 1, graph["data"].num_nodes, 80), device=dev)
        opt = optim.FusedAdamW([p for p in model.parameters() if p.requires_grad], max_grad_norm=1.0, **HYPER)
        if "averager" in name:
            optim.DeviceLRSchedule(opt, warmup_steps=10, total_steps=1000)
            optim.WeightAverager(opt, kind="ema", decay=0.999)
        steps[name] = (GraphedTrainStep(model, loss_fn, x, target, optimizer=opt, warmup=2), x, target, [])
        print(f"  {workload} {name}: captured ({torch.cuda.memory_allocated() / 2**30:.1f} GiB allocated)", flush=True)
    for _ in range(rounds):
        for g, x, target, times in steps.values():
            times.append(timed(lambda: g(x, target)))
    base = statistics.median(steps["fusedadamw"][3])
    print(f"| {workload}: whole GraphedTrainStep | ms (median / min) | over the step with FusedAdamW alone |", flush=True)
    print("|---|---|---|", flush=True)
    for name, (_, _, _, times) in steps.items():
        print(f"| {name} | {statistics.median(times):.2f} / {min(times):.2f} | +{statistics.median(times) - base:.2f} ms |", flush=True)
    steps.clear()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--list", default="cfg3", help="workload whose parameter list is averaged alone ('' to skip)")
    ap.add_argument("--steps", default="cfg2,cfg3", help="workloads for the whole captured training step ('' to skip)")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--step-rounds", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("average_bench: no GPU -- nothing can be measured here")
    os.environ.setdefault("ANEMOI_AMD_DTYPE", "bf16")
    if args.list:
        list_bench(args.list, args.rounds)
    for workload in [w for w in args.steps.split(",") if w]:
        step_bench(workload, args.step_rounds)


if __name__ == "__main__":
    main()
