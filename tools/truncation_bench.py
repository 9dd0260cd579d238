"""Times the truncated residual connection on anemoi_csr_project (the fused route) against the route composed from torch ops as
current anemoi-models does it (index_select, two torch.sparse.mm, a full-width add), forward and forward + backward.

    python tools/truncation_bench.py [--iters 30] [--out profiles/truncation.md]

Shapes: config 3's grid (G = 542 080, V_in = 90, V_out = 80, 80 prognostic columns, T = 2, one batch entry, one member) and an
O96-sized coarse grid (G_c = 40 320).  The matrices are synthetic, from a seeded numpy generator, with index locality: up has 4
entries per row around i G_c / G, down ceil(G / G_c) = 14 around i G / G_c; a second set has 16 and 56.  Bytes over time are
printed next to the byte floor of each launch (every operand once: the gathered columns, the output -- twice where it is
accumulated into -- and the CSR arrays) and against the 8 TB/s HBM peak of an MI355X.
"""

from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda"
HBM_PEAK = 8.0e12
G, G_C, V_IN, V_OUT, N_PROG, T = 542080, 40320, 90, 80, 80, 2


def timed(fn, iters: int) -> float:
    """Median milliseconds of ``fn`` over ``iters`` calls, each between its own pair of events, after 5 warm-up calls."""
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
    return sorted(ms)[len(ms) // 2]


def local_matrix(rng, n_out: int, n_in: int, per_row: int):
    """``(indptr, indices, values, shape)``: ``per_row`` distinct columns per row inside a window around ``i n_in / n_out``,
    positive weights that sum to 1 (an interpolation stencil)."""
    centre = (np.arange(n_out, dtype=np.int64) * n_in) // n_out
    window = 4 * per_row
    off = np.argsort(rng.random((n_out, window)), axis=1)[:, :per_row] - window // 2
    cols = np.sort(np.clip(centre[:, None] + off, 0, n_in - 1), axis=1)
    w = rng.random((n_out, per_row)).astype(np.float32) + 0.1
    w /= w.sum(axis=1, keepdims=True)
    indptr = np.arange(n_out + 1, dtype=np.int64) * per_row
    return torch.from_numpy(indptr), torch.from_numpy(cols.reshape(-1)), torch.from_numpy(w.reshape(-1)), (n_out, n_in)


def composed(out, x, mats, o_idx, i_idx):
    """The torch route of ``training._finish`` with truncation (what upstream composes)."""
    y = out.float().reshape(1, 1, G, -1).clone()
    skip = x[:, -1].index_select(-1, i_idx)
    flat = skip.reshape(1, G, -1)
    for m in mats:
        flat = torch.stack([torch.sparse.mm(m, flat[i]) for i in range(flat.shape[0])])
    res = torch.zeros_like(y)
    res[..., o_idx] = flat.reshape(skip.shape)
    return y + res


def table(iters: int, up_per_row: int) -> list:
    from anemoi_models_amd import autograd, ops
    from anemoi_models_amd.layers.truncation import TruncationPlan

    rng = np.random.default_rng(up_per_row)
    down_per_row = -(-G // G_C) * (up_per_row // 4)
    plan = TruncationPlan({"down": local_matrix(rng, G_C, G, down_per_row), "up": local_matrix(rng, G, G_C, up_per_row)})
    dev = plan.on(DEV)
    (down, up), (down_t, up_t) = dev.stages, dev.stages_t
    mats = plan.sparse(DEV)
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(1, T, 1, G, V_IN, generator=gen).to(DEV)
    out = torch.randn(G, V_OUT, generator=gen).to(DEV)
    dy = torch.randn(1, 1, G, V_OUT, generator=gen).to(DEV)
    i_idx = torch.arange(N_PROG, dtype=torch.int32, device=DEV)
    o_idx = torch.arange(N_PROG, dtype=torch.int32, device=DEV)
    i_long, o_long = i_idx.long(), o_idx.long()
    mid = torch.empty(1, 1, G_C, N_PROG, device=DEV)
    y = out.view(1, 1, G, V_OUT).clone()
    dmid = torch.empty(1, 1, G_C, N_PROG, device=DEV)
    dx = torch.zeros(1, T, 1, G, V_IN, device=DEV)

    def csr_bytes(m):
        return m.indptr.numel() * 8 + m.idx.numel() * 8

    lines = [f"### up: {up_per_row} entries per row, down: {down_per_row} (nnz {up.idx.numel()} / {down.idx.numel()})", "",
             "| launch | ms | byte floor MB | GB/s of floor | of HBM peak |", "|---|---|---|---|---|"]
    launches = [
        ("down  x[:, -1] -> mid (store)", lambda: ops.csr_project(x[:, -1], mid, down.indptr, down.idx, down.val, i_idx, None),
         (G + G_C) * N_PROG * 4 + csr_bytes(down)),
        ("up    mid -> y (accumulate)", lambda: ops.csr_project(mid, y, up.indptr, up.idx, up.val, None, o_idx, accumulate=True),
         (G_C + 2 * G) * N_PROG * 4 + csr_bytes(up)),
        ("up^T  dy -> dmid (store)", lambda: ops.csr_project(dy, dmid, up_t.indptr, up_t.idx, up_t.val, o_idx, None),
         (G + G_C) * N_PROG * 4 + csr_bytes(up_t)),
        ("down^T dmid -> dx[:, -1] (store)",
         lambda: ops.csr_project(dmid, dx[:, -1], down_t.indptr, down_t.idx, down_t.val, None, i_idx),
         (G_C + G) * N_PROG * 4 + csr_bytes(down_t)),
    ]
    for name, fn, floor in launches:
        ms = timed(fn, iters)
        rate = floor / ms / 1e6
        lines.append(f"| {name} | {ms:.3f} | {floor / 1e6:.1f} | {rate:.0f} | {100 * rate * 1e9 / HBM_PEAK:.1f} % |")
        print(lines[-1], flush=True)

    with torch.no_grad():
        f_f = timed(lambda: autograd.truncated_residual(out, x, plan, o_idx, i_idx, (1, 1, G, V_OUT)), iters)
        c_f = timed(lambda: composed(out, x, mats, o_long, i_long), iters)
    leaves = [out.clone().requires_grad_(), x.clone().requires_grad_()]

    def both(fn):
        for t in leaves:
            t.grad = None
        fn(*leaves).backward(dy)

    f_fb = timed(lambda: both(lambda o, xx: autograd.truncated_residual(o, xx, plan, o_idx, i_idx, (1, 1, G, V_OUT))), iters)
    c_fb = timed(lambda: both(lambda o, xx: composed(o, xx, mats, o_long, i_long)), iters)
    lines += ["", "| route | forward ms | forward + backward ms |", "|---|---|---|",
              f"| fused (copy of out + 2 launches; backward: zero-fill of dx + 2 launches) | {f_f:.3f} | {f_fb:.3f} |",
              f"| composed torch (index_select, 2 torch.sparse.mm, full-width add) | {c_f:.3f} | {c_fb:.3f} |", ""]
    print("\n".join(lines[-4:]), flush=True)
    return lines


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None, help="also write the tables to this file (markdown)")
    args = ap.parse_args()
    lines = [f"## Truncated residual: G = {G}, G_c = {G_C}, V_in = {V_IN}, V_out = {V_OUT}, {N_PROG} prognostic columns, f32", ""]
    for per_row in (4, 16):
        lines += table(args.iters, per_row)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
