#!/usr/bin/env python
"""Repeat one forward (or training step) of a preset model under the launch trail and name the first launch that differs.

    python tools/trail_diff.py [--cfg 1|2|3] [--dtype bf16|fp32] [--repeats N] [--train] [--out DIR]

The model is built once (bench.py's preset), warmed up, and a reference trail is recorded (anemoi_models_amd/trail.py: one
digest per output buffer of every kernel-library call).  Each of the N repeats records its own trail of the same work; for a
repeat that differs, the first differing launch is printed -- index, name, shape, both digests, both absmax -- and both trails
are saved as JSON under --out.  Exit status 0 whether or not a difference is found; the first step that raises ends the run
(nothing more is started on the GPU after it) with status 1.

tools/micro/forward_repeat.py compares the final output only; this names the kernel.
"""

import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def describe(e) -> str:
    return "(no record)" if e is None else (f"{e.name} [{e.rows} x {e.cols}] {e.dtype} digest {e.digest:016x} "
                                            f"absmax {e.absmax:.6g} nonfinite {e.nonfinite}")


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cfg", type=int, default=1, choices=[1, 2, 3])
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--train", action="store_true", help="one forward + backward per step instead of an inference forward")
    ap.add_argument("--processor", default="GraphTransformer", choices=["GraphTransformer", "GNN", "Transformer"])
    ap.add_argument("--capacity", type=int, default=65536)
    ap.add_argument("--out", default="trail_diff_out", help="directory for the trails of differing repeats")
    args = ap.parse_args()
    os.environ["ANEMOI_AMD_DTYPE"] = args.dtype

    import bench
    from anemoi_models_amd import trail

    if not torch.cuda.is_available():
        print("trail_diff: no GPU (the launch trail records kernels on the device)", file=sys.stderr)
        return 1
    dev = torch.device("cuda", 0)
    model, _, x, _ = bench.build(f"cfg{args.cfg}", dev, args.processor)
    dy = None
    if args.train:
        model.train()

    def step():
        nonlocal dy
        if not args.train:
            with torch.no_grad():
                return model(x)
        for p in model.parameters():
            p.grad = None
        y = model(x)
        if dy is None:
            dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(2)).to(y.device, y.dtype)
        y.backward(dy)
        return y.detach()

    def recorded():
        with trail.record(capacity=args.capacity) as t:
            y = step()
        return y, t

    try:
        step()  # warm-up: weight packing, edge plans
        t0 = time.perf_counter()
        y_ref, ref = recorded()
        torch.cuda.synchronize()
        print(f"cfg{args.cfg} {args.processor} {args.dtype} {'training step' if args.train else 'forward'}: reference trail of "
              f"{len(ref.entries)} records ({ref.dropped} dropped) in {time.perf_counter() - t0:.3f} s; "
              f"first non-finite: {describe(ref.first_nonfinite()) if ref.first_nonfinite() else 'none'}", flush=True)
        differing = 0
        for it in range(args.repeats):
            y, t = recorded()
            diff = trail.first_difference(ref, t)
            if diff is None:
                if not torch.equal(y, y_ref):
                    print(f"repeat {it}: all {len(t.entries)} records equal but the output differs: an op outside the "
                          "kernel library (trail.mark it)", flush=True)
                continue
            differing += 1
            i, ea, eb = diff
            print(f"repeat {it}: first difference at launch {i} of {len(ref.entries)}\n  reference: {describe(ea)}\n"
                  f"  repeat   : {describe(eb)}", flush=True)
            os.makedirs(args.out, exist_ok=True)
            ref.save(os.path.join(args.out, "reference.json"))
            t.save(os.path.join(args.out, f"repeat_{it:04d}.json"))
        print(f"{differing} of {args.repeats} repeats differ from the reference trail"
              + (f"; trails saved under {args.out}/" if differing else ""), flush=True)
    except Exception as exc:  # noqa: BLE001 -- whatever failed, nothing more is started on the GPU
        print(f"trail_diff: step failed, stopping: {type(exc).__name__}: {exc}", file=sys.stderr, flush=True)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
