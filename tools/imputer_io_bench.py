"""Time ``AnemoiModelInterface.predict_step`` with a NaN imputer in ``config.data.processors``: the generic route (imputer and
normaliser as ATen passes around the forward) against the fused one (both inside the forward's first and last kernel).

    python tools/imputer_io_bench.py --workload cfg2 cfg3 [--calls 20] [--warmup 3] [--root DIR]

Only the public interface is used, so the same file times another checkout of the package (``--root``: the directory that
holds ``anemoi_models_amd`` and ``bench.py``), e.g. the parent commit, where both settings take the generic route.  Workload:
the processor chain ``[InputImputer {mean: [prog_2], minimum: [forc_1]}, InputNormalizer]`` on the grid and the variable counts
(80 prognostic, 10 forcing) of ``bench.py``'s config 2 / 3, bf16 forward, batch 1, two time steps; 30 % of the grid is NaN in
both imputed variables.  After a first (always generic) call and ``--warmup`` calls per setting, ``--calls`` calls per setting
are timed between device events, ALTERNATING ``ANEMOI_AMD_FUSE_NORMALIZER=0`` and ``=1`` so that clock and thermal drift hit
both alike.  One JSON line per workload: median / min / max / inter-quartile range per setting in ms, the route each setting
took, and the bytes the pre- / post-processing of each route moves, counted from the shapes (``traffic()``)."""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys


def traffic(grid: int, t: int, v_in: int, v_out: int, n_imputed_in: int, n_imputed_out: int, ld_bytes: int) -> dict:
    """Bytes read + written outside the forward's own layers, per call (f32 state ``S`` = [1, t, grid, v_in], f32 prediction
    ``P`` = [1, 1, grid, v_out], ``c`` = one column of either over the whole tensor).

    generic: imputer.transform(in_place=False) = clone (2 S) + gather of the imputed columns, ``where``, index-put (4 reads / 3
    writes of c per imputed column, plus the map); normaliser.transform(in_place=False) = clone, ``* mul``, ``+ add``, copy
    back (8 S); the same two on the prediction in reverse (8 P, then 2 P + 7 c per restored column); then what the fused route
    does too: anemoi_assemble_nodes reads S and writes the bf16 rows, anemoi_finalize_output reads and writes P and reads the
    prognostic columns of the last time slice."""
    s, p = 4 * t * grid * v_in, 4 * grid * v_out
    c_in, c_out = 4 * t * grid, 4 * grid
    kernels = s + grid * ld_bytes + 2 * p + 4 * grid * min(v_in, v_out)
    maps = grid * (n_imputed_in + n_imputed_out)
    generic = 2 * s + 7 * c_in * n_imputed_in + 8 * s + 8 * p + 2 * p + 7 * c_out * n_imputed_out + maps
    return {"kernels_both_routes_bytes": kernels, "generic_extra_bytes": generic, "fused_extra_bytes": maps}


def run(workload: str, calls: int, warmup: int) -> dict:
    import torch

    import bench
    from anemoi_models_amd.graphs.synthetic import build_graph
    from anemoi_models_amd.interface import AnemoiModelInterface
    from anemoi_models_amd.utils.indices import SimpleDataIndices
    from anemoi_models_amd.utils.presets import model_config

    dev = torch.device("cuda:0")
    graph_name, channels, layers, heads, what = bench.WORKLOADS[workload]
    graph = build_graph(graph_name)
    idx = SimpleDataIndices(n_prognostic=80, n_forcing=10, n_diagnostic=0)
    cfg = model_config("GraphTransformer", channels, layers, heads)
    pre = "anemoi.models.preprocessing."
    cfg["data"] = {"forcing": [f"forc_{i}" for i in range(10)], "diagnostic": [],
                   "processors": {"imputer": {"_target_": pre + "imputer.InputImputer",
                                              "config": {"default": "none", "mean": ["prog_2"], "minimum": ["forc_1"]}},
                                  "normalizer": {"_target_": pre + "normalizer.InputNormalizer",
                                                 "config": {"default": "mean-std"}}}}
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
    holes = torch.rand(grid, generator=gen) < 0.3
    batch[:, :, holes, 2] = float("nan")
    batch[:, :, holes, 81] = float("nan")
    batch = batch.to(dev)

    def route() -> str:
        query = getattr(iface, "_fused_route", None) or iface._normalizer_affines
        return "generic" if query(batch) is None else "fused"

    def call():
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        y = iface.predict_step(batch)
        end.record()
        end.synchronize()
        return start.elapsed_time(end), y

    _, first = call()  # always generic: fixes the imputer's NaN map
    times, routes, last = {"0": [], "1": []}, {}, {}
    for i in range(warmup + calls):
        for setting in ("0", "1"):
            os.environ["ANEMOI_AMD_FUSE_NORMALIZER"] = setting
            routes[setting] = route()
            ms, last[setting] = call()
            if i >= warmup:
                times[setting].append(ms)
    same_nans = bool(torch.equal(torch.isnan(last["0"]), torch.isnan(last["1"])))
    diff = float((torch.nan_to_num(last["0"].float()) - torch.nan_to_num(last["1"].float())).abs().max() /
                 torch.nan_to_num(last["0"].float()).abs().max())

    def summary(ts):
        q = statistics.quantiles(ts, n=4)
        return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3),
                "iqr_ms": round(q[2] - q[0], 3)}

    ld_bytes = 2 * (-(-(2 * 90 + 4 + 8 + 1) // 64) * 64)  # a bf16 row of the assembled input: state, sin / cos, trainable, 1, pad
    return {"workload": workload, "what": what, "grid": grid, "calls": calls, "dtype": os.environ["ANEMOI_AMD_DTYPE"],
            "setting_0": dict(summary(times["0"]), route=routes["0"]), "setting_1": dict(summary(times["1"]), route=routes["1"]),
            "nan_maps_equal": same_nans, "nan_in_prediction": int(torch.isnan(last["1"]).sum()),
            "max_rel_diff_between_settings": diff, "traffic": traffic(grid, 2, 90, 80, 2, 1, ld_bytes)}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", nargs="+", default=["cfg2", "cfg3"], choices=["cfg1", "cfg2", "cfg3"])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="checkout whose anemoi_models_amd is timed (default: the one this file is in)")
    args = ap.parse_args()
    if args.calls < 20:
        ap.error("at least 20 timed calls per setting")
    sys.path.insert(0, os.path.abspath(args.root))
    os.environ["ANEMOI_AMD_DTYPE"] = "bf16"
    for w in args.workload:
        print(json.dumps(dict(run(w, args.calls, args.warmup), root=os.path.abspath(args.root))), flush=True)


if __name__ == "__main__":
    main()
