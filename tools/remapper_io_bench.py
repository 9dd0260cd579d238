"""Time ``AnemoiModelInterface.predict_step`` with a remapper next to the ``InputNormalizer`` in ``config.data.processors``: the
generic route (normaliser and remapper as ATen passes around the forward) against the fused one (both inside
``anemoi_assemble_nodes_remapped`` / ``anemoi_residual_remapped`` / ``anemoi_unmap_output``).

    python tools/remapper_io_bench.py [--workload cfg3] [--pairs 5] [--warmup 3]      # predict_step and the kernels alone
    python tools/remapper_io_bench.py --trace                                          # a few fused calls, for a kernel trace

Workload: the grid and the variable counts (80 prognostic, 10 forcing) of ``bench.py``'s config, bf16 forward, batch 1, two time
steps.  A fused chain holds ONE remapper, so the two cos_sin and the three mono columns are two chains:

    multi   [InputNormalizer, Remapper {cos_sin: prog_7, forc_1}]          (V_raw 90 -> V_int 92, output 81 -> 80)
    mono    [Remapper {log1p: prog_2, sqrt: forc_0, boxcox: prog_8}, InputNormalizer]
    floor   [InputNormalizer]                                               (the normaliser-only fused route)

After a first (always generic) call and ``--warmup`` calls per setting, ``--pairs`` pairs of calls are timed between device
events (``end.synchronize()``), ALTERNATING ``ANEMOI_AMD_FUSE_NORMALIZER=0`` and ``=1``; every pair is listed.  Then the three
kernels and the plain ``anemoi_assemble_nodes`` run alone at the same shape (median of 20 launches between events; the
per-kernel times of the profile come from a separate ``rocprofv3 --kernel-trace --stats`` run of ``--trace``), with the bytes
each must move, counted from the shapes, and that over the time as a share of the 8.0 TB/s HBM peak (the bound that applies
to all four: a few flops per byte).  One JSON line per chain."""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

HBM_PEAK = 8.0e12  # bytes / s, MI355X specification
PRE = "anemoi.models.preprocessing."
NORMALIZER = ("normalizer", PRE + "normalizer.InputNormalizer", {"default": "mean-std", "none": ["prog_7", "forc_1"]})
MULTI = {"prog_7": ["cos_p7", "sin_p7"], "forc_1": ["cos_f1", "sin_f1"]}
CHAINS = {
    "multi": ([NORMALIZER, ("remapper", PRE + "remapper.Remapper", {"default": "none", "cos_sin": MULTI})], MULTI),
    "mono": ([("remapper", PRE + "remapper.Remapper", {"default": "none", "log1p": ["prog_2"], "sqrt": ["forc_0"],
                                                       "boxcox": ["prog_8"]}), NORMALIZER], None),
    "floor": ([NORMALIZER], None),
}


def kernel_bytes(grid: int, t: int, v_raw: int, v_int: int, v_int_out: int, v_out: int, n_res: int, ld_bytes: int) -> dict:
    """Bytes each kernel must read + write (f32 state [1, t, grid, v_raw], bf16 rows of ``ld_bytes``, f32 outputs)."""
    return {"assemble_remapped": 4 * t * grid * v_raw + grid * ld_bytes, "assemble_plain": 4 * t * grid * v_raw + grid * ld_bytes,
            "residual_remapped": 2 * 4 * grid * v_int_out + 4 * grid * n_res, "unmap_output": 4 * grid * (v_int_out + v_out)}


def build(workload: str, chain: str):
    import torch

    import bench
    from anemoi_models_amd.graphs.synthetic import build_graph
    from anemoi_models_amd.interface import AnemoiModelInterface
    from anemoi_models_amd.utils.indices import SimpleDataIndices
    from anemoi_models_amd.utils.presets import model_config

    dev = torch.device("cuda:0")
    graph_name, channels, layers, heads, what = bench.WORKLOADS[workload]
    graph = build_graph(graph_name)
    processors, remapped = CHAINS[chain]
    idx = SimpleDataIndices(n_prognostic=80, n_forcing=10, n_diagnostic=0, remapped=remapped)
    cfg = model_config("GraphTransformer", channels, layers, heads)
    cfg["data"] = {"forcing": [f"forc_{i}" for i in range(10)], "diagnostic": [],
                   "processors": {name: {"_target_": target, "config": config} for name, target, config in processors}}
    cfg["model"]["model"] = {"_target_": "anemoi.models.models.encoder_processor_decoder.AnemoiModelEncProcDec"}
    cfg = type(cfg)(cfg)
    gen = torch.Generator().manual_seed(11)
    mean = (torch.randn(90, generator=gen) * 3.0).numpy()
    stdev = (0.5 + torch.rand(90, generator=gen) * 2.0).numpy()
    stats = {"mean": mean, "stdev": stdev, "minimum": mean - 3.0 * stdev, "maximum": mean + 3.5 * stdev}
    torch.manual_seed(1234)
    with torch.device(dev):
        iface = AnemoiModelInterface(config=cfg, graph_data=graph.to(dev), statistics=stats, data_indices=idx, metadata={})
    iface = iface.to(dev).eval()
    grid = graph["data"].num_nodes
    batch = torch.randn((1, 2, grid, 90), generator=torch.Generator().manual_seed(7)) * torch.from_numpy(stdev).float() + \
        torch.from_numpy(mean).float()
    for c in (7, 81):  # the directions
        batch[..., c] = torch.rand((1, 2, grid), generator=gen) * 360.0
    for c in (2, 80, 8):  # the mono columns
        batch[..., c] = batch[..., c].abs()
    return iface, batch.to(dev), grid, what


def timed(fn):
    import torch

    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end), out


def kernels_alone(iface, batch, grid: int) -> dict:
    """Median time of each kernel alone at the workload's shape, the bytes it must move and its share of the HBM peak."""
    import torch

    from anemoi_models_amd import ops

    route = iface._fused_route(batch)
    remap = route[0].remap
    x = batch[:, 0:2, None].contiguous()
    ll = torch.randn((grid, 4), device=batch.device)
    tr = torch.randn((grid, 9), device=batch.device)
    ld = -(-(2 * remap.v_int + 13) // 64) * 64
    y = torch.randn((1, 1, grid, remap.v_int_out), device=batch.device)
    plain_affine = (route[0][0], route[0][1])
    calls = {"assemble_remapped": lambda: ops.assemble_nodes(x, ll, tr, 1, torch.bfloat16, ld_out=ld, remap=remap),
             "assemble_plain": lambda: ops.assemble_nodes(x, ll, tr, 1, torch.bfloat16, ld_out=ld, in_affine=plain_affine),
             "residual_remapped": lambda: ops.residual_remapped(y, x, remap),
             "unmap_output": lambda: ops.unmap_output(y, remap)}
    need = kernel_bytes(grid, 2, remap.v_raw, remap.v_int, remap.v_int_out, remap.v_out,
                        sum(r >= 0 for r in remap.h_res.tolist()), 2 * ld)
    out = {}
    for name, fn in calls.items():
        for _ in range(3):
            fn()
        ms = statistics.median(timed(fn)[0] for _ in range(20))
        out[name] = {"median_ms": round(ms, 4), "bytes": need[name], "TB_per_s": round(need[name] / ms / 1e9, 3),
                     "share_of_hbm_peak": round(need[name] / (ms * 1e-3) / HBM_PEAK, 3)}
    return out


def run(workload: str, chain: str, pairs: int, warmup: int) -> dict:
    import torch

    iface, batch, grid, what = build(workload, chain)
    timed(lambda: iface.predict_step(batch))  # always generic: the reference's one-off check of the first batch
    settings = ("1",) if chain == "floor" else ("0", "1")
    times, routes, last = {s: [] for s in settings}, {}, {}
    for i in range(warmup + pairs):
        for setting in settings:
            os.environ["ANEMOI_AMD_FUSE_NORMALIZER"] = setting
            routes[setting] = "generic" if iface._fused_route(batch) is None else "fused"
            ms, last[setting] = timed(lambda: iface.predict_step(batch))
            if i >= warmup:
                times[setting].append(round(ms, 3))
    os.environ["ANEMOI_AMD_FUSE_NORMALIZER"] = "1"
    out = {"workload": workload, "what": what, "chain": chain, "grid": grid, "dtype": os.environ["ANEMOI_AMD_DTYPE"],
           "fused_ms": times["1"], "fused_route": routes["1"], "fused_median_ms": statistics.median(times["1"])}
    if chain != "floor":
        out.update({"generic_ms": times["0"], "generic_route": routes["0"], "generic_median_ms": statistics.median(times["0"]),
                    "fused_faster_in_every_pair": all(f < g for f, g in zip(times["1"], times["0"])),
                    "max_rel_diff_between_routes": float((last["0"].float() - last["1"].float()).abs().max() /
                                                         last["0"].float().abs().max()),
                    "kernels_alone": kernels_alone(iface, batch, grid)})
    return out


def trace(workload: str, calls: int = 5) -> None:
    """A few fused calls of both chains and nothing else: the program of a kernel-trace run."""
    import torch

    for chain in ("multi", "mono"):
        iface, batch, _, _ = build(workload, chain)
        for _ in range(1 + calls):
            iface.predict_step(batch)
        torch.cuda.synchronize()
        print(json.dumps({"chain": chain, "fused_calls": calls}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="cfg3", choices=["cfg1", "cfg2", "cfg3"])
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace", action="store_true", help="run a few fused calls only (under rocprofv3 --kernel-trace --stats)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ["ANEMOI_AMD_DTYPE"] = "bf16"
    if args.trace:
        trace(args.workload)
        return
    for chain in ("multi", "mono", "floor"):
        print(json.dumps(run(args.workload, chain, args.pairs, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
