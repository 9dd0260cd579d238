#!/usr/bin/env python
"""Split-bf16 Linear (``ops.linear_split``) against the exact f32 ``ops.linear``, on the GPU; not part
of the product.

    python tools/split_bench.py [--cfg CFG]       the f32 Linear shapes of one profiled f32 forward of bench.build(CFG)
                                                  (default config 3), each distinct (M, N, K, act, bias, residual) once:
                                                  both kernels alternated, median of 21 event-timed launches after warm-up,
                                                  TFLOP/s f32-equivalent and the fraction of the 833 TFLOP/s ceiling
    python tools/split_bench.py MxNxK ...         the same at the given shapes (bias, no activation, no residual)
    python tools/split_bench.py --model CFG [N]   bench.build(CFG) f32 forward with ANEMOI_AMD_F32_LINEAR exact / bf16x3,
                                                  alternated N times in one process (median ms each) and the error of the
                                                  split route against the exact one
"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from anemoi_models_amd import ops  # noqa: E402

CEILING = 2500.0 / 3  # TFLOP/s f32-equivalent: the bf16 MFMA peak over three products


def _once(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    return s, e


def alternated(fns, reps=21, warm=3):
    """Median ms of each callable, the callables taking turns (so drift and clocks hit all of them alike)."""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ev = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            ev[i].append(_once(fn))
    torch.cuda.synchronize()
    return [statistics.median(s.elapsed_time(e) for s, e in evs) for evs in ev]


def profiled_shapes(cfg: str):
    """Distinct ``ops.linear`` calls of one f32 forward, with their counts: {(m, n, k, act, bias, residual): count}."""
    import bench

    m, _graph, x, _idx = bench.build(cfg, torch.device("cuda"))
    os.environ["ANEMOI_AMD_DTYPE"] = "fp32"
    os.environ.pop("ANEMOI_AMD_F32_LINEAR", None)
    seen = {}
    real = ops.linear

    def spy(xx, w, bias=None, *, act="Identity", residual=None, n_out=None, **kw):
        key = (xx.shape[0], w.shape[0] if n_out is None else n_out, w.shape[1], act, bias is not None, residual is not None)
        seen[key] = seen.get(key, 0) + 1
        return real(xx, w, bias, act=act, residual=residual, n_out=n_out, **kw)

    ops.linear = spy
    try:
        with torch.no_grad():
            m(x)
    finally:
        ops.linear = real
    del m, x
    torch.cuda.empty_cache()
    return seen


def kernels(shapes):
    dev = "cuda"
    print(f"{'M':>7s} {'N':>5s} {'K':>5s} act      bias res  calls | exact f32 ms  TF/s | bf16x3 ms   TF/s  of {CEILING:.0f} | speed")
    total = [0.0, 0.0]
    for (m, n, k, act, has_b, has_r), count in sorted(shapes.items(), key=lambda kv: -kv[0][0] * kv[0][1] * kv[0][2] * kv[1]):
        x = torch.randn(m, k, device=dev)
        w = torch.randn(n, k, device=dev) / k ** 0.5
        b = torch.randn(n, device=dev) if has_b else None
        r = torch.randn(m, n, device=dev) if has_r else None
        planes = ops.split_weight(w)
        y0, y1 = torch.empty(m, n, device=dev), torch.empty(m, n, device=dev)
        t_exact, t_split = alternated([lambda: ops.linear(x, w, b, act=act, residual=r, out=y0),
                                       lambda: ops.linear_split(x, planes, b, act=act, residual=r, out=y1)])
        tf = 2 * m * n * k / 1e9
        total[0] += count * t_exact
        total[1] += count * t_split
        print(f"{m:7d} {n:5d} {k:5d} {act:8s} {has_b!s:5s}{has_r!s:5s}{count:5d} | {t_exact:9.3f} {tf / t_exact:8.1f} | "
              f"{t_split:9.3f} {tf / t_split:7.1f} {tf / t_split / CEILING:6.2f} | {t_exact / t_split:5.2f}x", flush=True)
        del x, w, r, planes, y0, y1
        torch.cuda.empty_cache()
    print(f"sum over the forward's Linears: exact f32 {total[0]:.2f} ms, bf16x3 {total[1]:.2f} ms")


def model(cfg: str, reps: int):
    import bench

    m, _graph, x, _idx = bench.build(cfg, torch.device("cuda"))
    print(f"{cfg}: {bench.WORKLOADS[cfg][4]}; Linear FLOP per forward {bench.reference_linear_flops(m) / 1e12:.2f} T")
    os.environ["ANEMOI_AMD_DTYPE"] = "fp32"
    modes = ("exact", "bf16x3")
    times, outs = {k: [] for k in modes}, {}
    with torch.no_grad():
        for mode in modes:  # warm-up: plans, packed weights, planes
            os.environ["ANEMOI_AMD_F32_LINEAR"] = mode
            for _ in range(2):
                outs[mode] = m(x).float()
        torch.cuda.synchronize()
        for _ in range(reps):
            for mode in modes:
                os.environ["ANEMOI_AMD_F32_LINEAR"] = mode
                s, e = _once(lambda: m(x))
                torch.cuda.synchronize()
                times[mode].append(s.elapsed_time(e))
    os.environ.pop("ANEMOI_AMD_F32_LINEAR", None)
    want, got = outs["exact"].cpu(), outs["bf16x3"].cpu()
    err = float((got - want).abs().max() / want.abs().max())
    pv = (got - want).abs().flatten(0, -2).max(0).values / want.abs().flatten(0, -2).max(0).values.clamp_min(1e-30)
    for mode in modes:
        print(f"  f32 {mode:7s} median {statistics.median(times[mode]):8.3f} ms  (runs {', '.join(f'{t:.1f}' for t in times[mode])})")
    print(f"  bf16x3 against exact: {statistics.median(times['exact']) / statistics.median(times['bf16x3']):.2f} x faster, "
          f"max-rel {err:.3e}, per-variable max {float(pv.max()):.3e}")


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "--model":
        model(args[1], int(args[2]) if len(args) > 2 else 5)
    elif args and args[0] != "--cfg":
        kernels({tuple(int(v) for v in a.split("x")) + ("Identity", True, False): 1 for a in args})
    else:
        kernels(profiled_shapes(args[1] if args else "cfg3"))
