#!/usr/bin/env python
"""Weight-gradient GEMM dW = dpre^T x at the config-3 shapes: the TN kernel (no transposed copies) against the older
route (chunked transposes + batched NT GEMM), same operands.   python tools/dw_bench.py
``--split``: f32 operands, ``ops.weight_grad_split`` (split-bf16 on the bf16 MFMA) against the exact f32 route of
``ops.weight_grad`` (chunked transposes + the 128 x 128 f32 kernel), alternated in one process, medians of 7."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from anemoi_models_amd import ops  # noqa: E402

dev = torch.device("cuda", 0)


def timed(fn, iters=10):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def split_mode():
    import statistics

    def once(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    # the dW shapes of an f32 config-3 training step (mapper embeddings and blocks, processor blocks, node MLPs)
    shapes3 = [(542080, 1024, 128), (542080, 1024, 1024), (542080, 2240, 1024), (542080, 4096, 1024), (542080, 1024, 4096),
               (542080, 96, 1024), (40962, 1024, 32), (40962, 1024, 1024), (40962, 4288, 1024), (40962, 1024, 1216),
               (40962, 5312, 1024), (40962, 4096, 1024), (40962, 1024, 4096), (5248, 128, 128), (5248, 512, 128)]
    for m, n, k in shapes3:
        torch.manual_seed(0)
        dpre, x = torch.randn(m, n, device=dev), torch.randn(m, k, device=dev)
        routes = {"exact": lambda: ops.weight_grad(dpre, x, k, want_bias=True),
                  "split": lambda: ops.weight_grad_split(dpre, x, k, want_bias=True)}
        for fn in routes.values():
            fn(), fn()
        t = {name: [] for name in routes}
        for _ in range(7):
            for name, fn in routes.items():
                t[name].append(once(fn))
        te, ts = statistics.median(t["exact"]), statistics.median(t["split"])
        err = float((routes["split"]()[0] - routes["exact"]()[0]).abs().max() / routes["exact"]()[0].abs().max())
        fl = 2.0 * m * n * k / 1e9
        print(f"dW [{n} x {k}] over {m} rows (f32, incl. bias sums): exact {te:.3f} ms ({fl / te:.0f} TFLOP/s)   "
              f"bf16x3 {ts:.3f} ms ({fl / ts:.0f} TFLOP/s f32-equivalent, {fl / ts / 833:.2f} of 833)   "
              f"x{te / ts:.2f}   max |diff| / max = {err:.1e}", flush=True)
        del dpre, x, routes


if "--split" in sys.argv:
    split_mode()
    sys.exit(0)

shapes = [(40962, 4096, 1024), (40962, 1024, 4096), (40962, 4288, 1024), (40962, 1024, 1216), (542080, 1024, 256),
          (542080, 4096, 1024), (40962, 1024, 192), (5121, 4096, 1024)]
for m, n, k in shapes:
    torch.manual_seed(0)
    dpre = torch.randn(m, n, device=dev).bfloat16()
    x = torch.randn(m, k, device=dev).bfloat16()
    res = {}
    for name, tr in (("tn", False), ("transposes", True)):
        res[name] = (timed(lambda: ops.weight_grad(dpre, x, k, want_bias=True, transposed_route=tr)),
                     ops.weight_grad(dpre, x, k, transposed_route=tr))
    want = dpre[:8192].double().t() @ x[:8192].double() if m <= 8192 else None
    err = float((res["tn"][1] - res["transposes"][1]).abs().max() / res["transposes"][1].abs().max())
    fl = 2.0 * m * n * k / 1e9
    print(f"dW [{n} x {k}] over {m} rows: TN {res['tn'][0]:.3f} ms ({fl / res['tn'][0]:.0f} TFLOP/s incl. bias sums)   "
          f"transposes + NT {res['transposes'][0]:.3f} ms ({fl / res['transposes'][0]:.0f})   max |diff| / max = {err:.1e}")
    del dpre, x, res
