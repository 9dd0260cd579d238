#!/usr/bin/env python
"""Repeat one forward (or training step) of a model under the launch trail and name the first launch that differs.

    python tools/trail_diff.py [--cfg 1|2|3 | --model GRAPH:CHANNELS:LAYERS] [--dtype bf16|fp32] [--set NAME=VALUE ...]
                               [--op-by-op] [--repeats N] [--train] [--out DIR] [--save DIR | --against DIR] [--no-output]

The model is built once (bench.py's preset, or ``--model o32_ico2:256:2``: the small model of the GPU tests), warmed up, and a
reference trail is recorded (anemoi_models_amd/trail.py: one digest per output buffer of every kernel-library call) -- of the
SECOND step after fresh caches, so what a route builds once and keeps is not in it.  Each of the N repeats records its own
trail of the same work; for a repeat that differs, the first differing launch is printed -- index, name, shape, both digests,
both absmax -- and both trails are saved as JSON under --out.

Two trees (a change against its parent commit): ``--save DIR`` in one tree writes the reference trail and the output tensor
under DIR, ``--against DIR`` in the other compares its own reference trail and output with them instead of with repeats and
prints one line, ``IDENTICAL`` or ``DIFFERENT`` with the first differing launch.  ``--set`` sets a switch in the environment
before the package is imported; ``--op-by-op`` turns the blocks' block-level entry points off (``block_abi = False``).

Exit status 0 whether or not a difference is found; the first step that raises ends the run (nothing more is started on the
GPU after it) with status 1.

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


def small_model(spec: str, dev):
    """``GRAPH:CHANNELS:LAYERS`` -> the GraphTransformer model the GPU tests build on a synthetic graph (16 heads, 10 prognostic,
    2 forcing and 1 diagnostic variable, seeds as there) and its input."""
    from anemoi_models_amd.graphs.synthetic import build_graph
    from anemoi_models_amd.models import AnemoiModelEncProcDec
    from anemoi_models_amd.utils.indices import SimpleDataIndices
    from anemoi_models_amd.utils.presets import model_config

    graph_name, channels, layers = spec.split(":")
    graph = build_graph(graph_name)
    idx = SimpleDataIndices(n_prognostic=10, n_forcing=2, n_diagnostic=1)
    torch.manual_seed(1234)
    model = AnemoiModelEncProcDec(model_config=model_config("GraphTransformer", int(channels), int(layers), 16), data_indices=idx,
                                  graph_data=graph)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("trainable"):
                p.normal_(0.0, 0.1)
    x = torch.randn(1, 2, 1, graph["data"].num_nodes, idx.num_input, generator=torch.Generator().manual_seed(7))
    return model.eval().to(dev), x.to(dev)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cfg", type=int, default=1, choices=[1, 2, 3])
    ap.add_argument("--model", default=None, metavar="GRAPH:CHANNELS:LAYERS", help="a small model instead of a preset")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--set", action="append", default=[], metavar="NAME=VALUE", help="environment switch (repeatable)")
    ap.add_argument("--op-by-op", action="store_true", help="GraphTransformer blocks without their block-level entry points")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--train", action="store_true", help="one forward + backward per step instead of an inference forward")
    ap.add_argument("--processor", default="GraphTransformer", choices=["GraphTransformer", "GNN", "Transformer"])
    ap.add_argument("--capacity", type=int, default=65536)
    ap.add_argument("--out", default="trail_diff_out", help="directory for the trails of differing repeats")
    ap.add_argument("--save", default=None, metavar="DIR", help="write the reference trail and the output tensor under DIR")
    ap.add_argument("--against", default=None, metavar="DIR", help="compare with what --save wrote, instead of with repeats")
    ap.add_argument("--no-output", action="store_true", help="--save / --against: the trail only, not the output tensor")
    args = ap.parse_args()
    os.environ["ANEMOI_AMD_DTYPE"] = args.dtype
    for item in args.set:
        name, _, value = item.partition("=")
        os.environ[name] = value

    import bench
    from anemoi_models_amd import trail

    if not torch.cuda.is_available():
        print("trail_diff: no GPU (the launch trail records kernels on the device)", file=sys.stderr)
        return 1
    dev = torch.device("cuda", 0)
    if args.op_by_op:
        from anemoi_models_amd.layers.block import GraphTransformerBaseBlock

        GraphTransformerBaseBlock.block_abi = False
    label = args.model or f"cfg{args.cfg}"
    if args.model:
        model, x = small_model(args.model, dev)
    else:
        model, _, x, _ = bench.build(label, dev, args.processor)
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
        step()  # warm-up: weight packing, edge plans, hoisted operands
        t0 = time.perf_counter()
        y_ref, ref = recorded()
        torch.cuda.synchronize()
        what = " ".join([label, args.processor, args.dtype] + args.set + (["op-by-op"] if args.op_by_op else []))
        print(f"{what} {'training step' if args.train else 'forward'}: reference trail of "
              f"{len(ref.entries)} records ({ref.dropped} dropped) in {time.perf_counter() - t0:.3f} s; "
              f"first non-finite: {describe(ref.first_nonfinite()) if ref.first_nonfinite() else 'none'}", flush=True)
        if args.save:
            os.makedirs(args.save, exist_ok=True)
            ref.save(os.path.join(args.save, "reference.json"))
            if not args.no_output:
                torch.save(y_ref.cpu(), os.path.join(args.save, "output.pt"))
            print(f"saved under {args.save}/", flush=True)
        if args.against:
            other = trail.load(os.path.join(args.against, "reference.json"))
            diff = trail.first_difference(other, ref)
            same_out = args.no_output or torch.equal(torch.load(os.path.join(args.against, "output.pt")), y_ref.cpu())
            if diff is None and same_out and other.dropped == ref.dropped == 0:
                print(f"IDENTICAL {what}: {len(ref.entries)} records" + ("" if args.no_output else ", outputs torch.equal"),
                      flush=True)
            elif diff is None:
                print(f"DIFFERENT {what}: all {len(ref.entries)} records equal, outputs equal: {same_out}, dropped "
                      f"{other.dropped} / {ref.dropped}", flush=True)
            else:
                i, ea, eb = diff
                print(f"DIFFERENT {what}: first difference at launch {i} ({len(other.entries)} records saved, {len(ref.entries)} "
                      f"here)\n  saved: {describe(ea)}\n  here : {describe(eb)}", flush=True)
                os.makedirs(args.out, exist_ok=True)
                ref.save(os.path.join(args.out, "here.json"))
        if args.save or args.against:
            return 0
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
