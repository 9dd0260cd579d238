#!/usr/bin/env python
"""The optimizer step measured on the MI355X: gradient clipping by global norm + AdamW over the parameter list of a bench
model (real shapes, random gradients), three routes alternated in one process, eager and inside a captured HIP graph:

  (a) torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW(foreach=True, capturable=True)
  (b) the same with fused=True
  (c) anemoi_models_amd.optim.FusedAdamW(max_grad_norm=...)

and one whole ``runtime.GraphedTrainStep`` (forward, loss, backward, optimizer) with each of the three and with none.

   python tools/optim_bench.py [--list cfg3] [--steps cfg2,cfg3] [--rounds 20] [--step-rounds 10]

Per route: median and minimum time, kernel launches (torch.profiler, one eager step) and the ratio to the byte floor --
(28 + 4) B per parameter with the norm (16 read and 12 written by the update, 4 read by the norm), 28 without, at the
float4-copy rate of 6.29 TB/s.  A run without a GPU fails: there is nothing to measure."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from anemoi_models_amd import _lib  # noqa: E402
from anemoi_models_amd import optim  # noqa: E402

COPY_RATE = 6.29e12  # B/s, float4 copy
HYPER = dict(lr=1e-4, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1)
MAX_NORM = 1.0


def make_route(name, params):
    """(step function, optimizer) of route `name` over `params`."""
    if name == "fusedadamw":
        opt = optim.FusedAdamW(params, max_grad_norm=MAX_NORM, **HYPER)
        return opt.step, opt
    if name == "fusedadamw-noclip":
        opt = optim.FusedAdamW(params, **HYPER)
        return opt.step, opt
    if name == "none":
        return (lambda: None), None
    opt = torch.optim.AdamW(params, capturable=True, **(dict(fused=True) if name == "torch-fused" else dict(foreach=True)), **HYPER)

    def step():
        torch.nn.utils.clip_grad_norm_(params, MAX_NORM, foreach=True)
        opt.step()

    return step, opt


class _ClippedTorch:
    """clip_grad_norm_ + a torch optimizer behind one ``step()``, for GraphedTrainStep's ``optimizer=``."""

    def __init__(self, params, opt):
        self.params, self.opt = params, opt

    def step(self):
        torch.nn.utils.clip_grad_norm_(self.params, MAX_NORM, foreach=True)
        self.opt.step()


def timed(fn, sync=True):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    if sync:
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def count_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile

        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
                   and "memset" not in e.name.lower())
    except Exception as e:  # the profiler is an aid; the timings stand without it
        print(f"  (launch count not measured: {type(e).__name__}: {e})", flush=True)
        return None


def list_bench(workload, rounds):
    dev = torch.device("cuda", 0)
    model, _, _, _ = bench.build(workload, dev)
    shapes = [tuple(p.shape) for p in model.parameters() if p.requires_grad]
    del model
    torch.cuda.empty_cache()
    n = sum(int(torch.Size(s).numel()) for s in shapes)
    gen = torch.Generator(device=dev).manual_seed(0)
    routes = {}
    for name in ("torch-foreach", "torch-fused", "fusedadamw", "fusedadamw-noclip"):
        params = [torch.nn.Parameter(torch.randn(s, device=dev, generator=gen)) for s in shapes]
        for p in params:
            p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-2
        step, opt = make_route(name, params)
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step()
        routes[name] = dict(step=step, graph=graph, opt=opt, params=params, eager=[], host=[], replay=[])
    floor = {name: (28 if name.endswith("noclip") else 32) * n / COPY_RATE * 1e3 for name in routes}
    print(f"{workload}: {len(shapes)} parameter tensors, {n / 1e6:.1f} M parameters, {4 * n / 2**30:.2f} GiB of gradients; "
          f"byte floor {floor['fusedadamw']:.3f} ms with the norm (32 B / parameter), {floor['fusedadamw-noclip']:.3f} ms "
          f"without (28 B), at {COPY_RATE / 1e12:.2f} TB/s; OPT_CHUNK {_lib.OPT_CHUNK}, OPT_MAX_TENSORS {_lib.OPT_MAX_TENSORS}",
          flush=True)
    for _ in range(rounds):  # alternated: one round = every route once, eager then replayed
        for r in routes.values():
            r["host"].append(timed(r["step"], sync=False))
            r["eager"].append(timed(r["step"]))
            r["replay"].append(timed(r["graph"].replay))
    print("| route | eager ms (median / min) | eager host enqueue ms | graph replay ms (median / min) | launches | "
          "replay / byte floor |", flush=True)
    print("|---|---|---|---|---|---|", flush=True)
    for name, r in routes.items():
        launches = count_launches(r["step"])
        print(f"| {name} | {statistics.median(r['eager']):.3f} / {min(r['eager']):.3f} | {statistics.median(r['host']):.3f} | "
              f"{statistics.median(r['replay']):.3f} / {min(r['replay']):.3f} | {launches if launches is not None else 'not measured'} | "
              f"{statistics.median(r['replay']) / floor[name]:.2f} x |", flush=True)


def step_bench(workload, rounds):
    from anemoi_models_amd.runtime import GraphedTrainStep

    dev = torch.device("cuda", 0)
    steps, graph = {}, None
    loss_fn = lambda y, t: ((y - t) ** 2).mean()  # noqa: E731
    for name in ("none", "torch-foreach", "torch-fused", "fusedadamw"):
        model, graph, x, _ = bench.build(workload, dev, graph=graph)
        model.train()
        target = torch.zeros((1, 1, graph["data"].num_nodes, 80), device=dev)
        params = [p for p in model.parameters() if p.requires_grad]
        _, opt = make_route(name, params)
        if name.startswith("torch"):
            opt = _ClippedTorch(params, opt)
        steps[name] = (GraphedTrainStep(model, loss_fn, x, target, optimizer=opt, warmup=2), x, target, [])
        print(f"  {workload} {name}: captured ({torch.cuda.memory_allocated() / 2**30:.1f} GiB allocated)", flush=True)
    for _ in range(rounds):
        for g, x, target, times in steps.values():
            times.append(timed(lambda: g(x, target)))
    base = statistics.median(steps["none"][3])
    print(f"| {workload}: whole GraphedTrainStep | ms (median / min) | over forward + backward alone |", flush=True)
    print("|---|---|---|", flush=True)
    for name, (_, _, _, times) in steps.items():
        print(f"| {name} | {statistics.median(times):.2f} / {min(times):.2f} | +{statistics.median(times) - base:.2f} ms |", flush=True)
    steps.clear()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--list", default="cfg3", help="workload whose parameter list is stepped alone ('' to skip)")
    ap.add_argument("--steps", default="cfg2,cfg3", help="workloads for the whole captured training step ('' to skip)")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--step-rounds", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench: no GPU -- nothing can be measured here")
    os.environ.setdefault("ANEMOI_AMD_DTYPE", "bf16")
    if args.list:
        list_bench(args.list, args.rounds)
    for workload in [w for w in args.steps.split(",") if w]:
        step_bench(workload, args.step_rounds)


if __name__ == "__main__":
    main()
