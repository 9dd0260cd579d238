#!/usr/bin/env python
"""MXFP8 Linear (``ops.linear_mx``) against the bf16 ``ops.linear``, on the GPU; not part of the product.

    python tools/mx_bench.py [MxNxK ...]          at the shapes of the GraphTransformer Linears of config 3 (default), plus
                                                  ``ops.mx_quantize`` of the activations
    python tools/mx_bench.py --budget [MxN]       K sweep 128 ... 4096 at one M x N: the per-tile cost split into the K loop
                                                  (slope per 128-byte slab) and the fixed part (intercept: epilogue, prologue)
    python tools/mx_bench.py --model CFG [N]      bench.build(CFG) forward with ANEMOI_AMD_MXFP8 off / on, alternated N times
                                                  in one process (median ms each), max-rel and per-variable error of both
                                                  against the exact-f32 route of the same model
"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from anemoi_models_amd import ops  # noqa: E402

SHAPES = [(40962, 4288, 1024), (40962, 1024, 1216), (40962, 4096, 1024), (40962, 1024, 4096), (542080, 4096, 1024),
          (542080, 1024, 4096)]


def timed(fn, it=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(it):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / it


def kernels():
    dev = "cuda"
    for m, n, k in SHAPES:
        x = torch.randn(m, k, device=dev).bfloat16()
        w = (torch.randn(n, k, device=dev) / k ** 0.5).bfloat16()
        b = torch.randn(n, device=dev)
        r = torch.randn(m, n, device=dev).bfloat16()
        xq, wq = ops.mx_quantize(x), ops.mx_quantize(w)
        tf = 2 * m * n * k / 1e9
        for act, res in (("Identity", None), ("GELU", None), ("Identity", r)):
            bf = timed(lambda: ops.linear(x, w, b, act=act, residual=res))  # both legs allocate their output
            mxb = timed(lambda: ops.linear_mx(xq, wq, b, act=act, residual=res))
            line = (f"M={m:6d} N={n:5d} K={k:5d} act={act:8s} res={res is not None!s:5s}  bf16 {bf:8.3f} ms "
                    f"{tf / bf:7.1f} TF/s   mx {mxb:8.3f} ms {tf / mxb:7.1f} TF/s   mx/bf16 speed {bf / mxb:5.2f}x")
            if act == "GELU" and n % 32 == 0:
                mxo = timed(lambda: ops.linear_mx(xq, wq, b, act=act, out="mx"))
                line += f"   (mx out {mxo:8.3f} ms)"
            print(line, flush=True)
        q = timed(lambda: ops.mx_quantize(x))
        print(f"M={m:6d} K={k:5d} mx_quantize {q:8.3f} ms  {m * k * 2 * (1 + 33 / 64) / q / 1e6:7.1f} GB/s", flush=True)
        del x, w, r, xq, wq
        torch.cuda.empty_cache()


def budget(m: int, n: int):
    """Least-squares line of linear_mx time over K: per-slab cost of the K loop and the fixed part, per block tile."""
    dev = "cuda"
    ks = [128, 256, 512, 1024, 2048, 4096]
    tiles = -(-m // 128) * -(-n // 128)
    ms = []
    for k in ks:
        xq = ops.mx_quantize(torch.randn(m, k, device=dev).bfloat16())
        wq = ops.mx_quantize((torch.randn(n, k, device=dev) / k ** 0.5).bfloat16())
        ms.append(timed(lambda: ops.linear_mx(xq, wq)))
        print(f"M={m} N={n} K={k:5d}: {ms[-1]:8.4f} ms", flush=True)
    slabs = [k / 128 for k in ks]
    mean_s, mean_t = statistics.mean(slabs), statistics.mean(ms)
    slope = sum((s - mean_s) * (t - mean_t) for s, t in zip(slabs, ms)) / sum((s - mean_s) ** 2 for s in slabs)
    icpt = mean_t - slope * mean_s
    print(f"{tiles} tiles of 128 x 128 on 256 CUs: K loop {slope * 1e3:.2f} us per 128-byte slab, fixed part "
          f"{icpt * 1e3:.2f} us; at K = 1024 the K loop is {8 * slope / (8 * slope + icpt):.0%} of the time")


def model(cfg: str, reps: int):
    import bench

    dev = torch.device("cuda")
    m, _graph, x, _idx = bench.build(cfg, dev)
    print(f"{cfg}: {bench.WORKLOADS[cfg][4]}; Linear FLOP per forward {bench.reference_linear_flops(m) / 1e12:.2f} T")
    with torch.no_grad():
        os.environ["ANEMOI_AMD_DTYPE"] = "fp32"
        want = m(x).float().cpu()
        os.environ["ANEMOI_AMD_DTYPE"] = "bf16"
        times, outs = {"0": [], "1": []}, {}
        for rep in range(reps):
            for sw in ("0", "1"):
                os.environ["ANEMOI_AMD_MXFP8"] = sw
                times[sw].append(timed(lambda: m(x), it=5, warm=2 if rep == 0 else 1))
                outs[sw] = m(x).float().cpu()
    os.environ.pop("ANEMOI_AMD_MXFP8", None)
    for sw, name in (("0", "bf16"), ("1", "bf16 + MXFP8")):
        got = outs[sw]
        err = float((got - want).abs().max() / want.abs().max())
        pv = (got - want).abs().flatten(0, -2).max(0).values / want.abs().flatten(0, -2).max(0).values.clamp_min(1e-30)
        print(f"  {name:13s} median {statistics.median(times[sw]):8.3f} ms  (runs {', '.join(f'{t:.2f}' for t in times[sw])})"
              f"  max-rel vs f32 {err:.3e}  per-variable max {float(pv.max()):.3e} median {float(pv.median()):.3e}")
    print(f"  MXFP8 on / off speed: {statistics.median(times['0']) / statistics.median(times['1']):.3f} x")
    # the covered sets, widest first, narrowed in the order decoder MLP, x_r | q | k | v | u product
    from anemoi_models_amd.layers.block import GraphTransformerMapperBlock, GraphTransformerProcessorBlock

    maps = [b for b in m.modules() if isinstance(b, GraphTransformerMapperBlock)]
    procs = [b for b in m.modules() if isinstance(b, GraphTransformerProcessorBlock)]
    dec = maps[-1]
    os.environ["ANEMOI_AMD_MXFP8"] = "1"
    for name, dec_mlp, sqkvu in (("all covered", True, True), ("without the decoder MLP", False, True),
                                 ("default: also without x_r|q|k|v|u", False, False)):
        dec.mx_node_mlp = dec_mlp
        for b in procs:
            b.mx_sqkvu = sqkvu
        with torch.no_grad():
            ms = timed(lambda: m(x), it=5, warm=2)
            got = m(x).float().cpu()
        err = float((got - want).abs().max() / want.abs().max())
        pv = (got - want).abs().flatten(0, -2).max(0).values / want.abs().flatten(0, -2).max(0).values.clamp_min(1e-30)
        print(f"  set {name:36s} {ms:8.3f} ms  max-rel vs f32 {err:.3e}  per-variable max {float(pv.max()):.3e}")
    dec.mx_node_mlp = False
    for b in procs:
        del b.mx_sqkvu
    os.environ.pop("ANEMOI_AMD_MXFP8", None)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--model":
        model(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 5)
    elif len(sys.argv) > 1 and sys.argv[1] == "--budget":
        mm, nn = (int(v) for v in (sys.argv[2] if len(sys.argv) > 2 else "40962x4096").split("x"))
        budget(mm, nn)
    else:
        if len(sys.argv) > 1:
            SHAPES[:] = [tuple(int(v) for v in a.split("x")) for a in sys.argv[1:]]
        kernels()
