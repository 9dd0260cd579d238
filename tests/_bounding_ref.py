"""Reference side of the bounding family (layers/bounding.py; csrc/elementwise.hip LEAKY, csrc/bounding.hip): the 11-op chain
every test uses, sequential restatements of the op list with slopes (forward with its tape, reverse walk), and the f64
contracts with per-element bounds of the forward and the backward.

Pure torch on the CPU.  Used by tests/test_bounding_family_cpu.py (the restatements equal the module route and torch autograd)
and tests/test_gpu_bounding_family.py (the kernels against ``(want, bound)``, in the style of tests/_remap_ref.py).

The contract is the MODULE CHAIN in f64 on the operands as stored: the f32 inputs widened, thresholds rounded to f32 (the
values the device lists hold).  Bounds, with u = 2^-24 per rounded f32 operation relative to its result:

  one op  f(v) = lo + s (v - lo) | v | hi + s (v - hi).  f is continuous and piecewise linear with slopes in {1, s}, s <= 1: an
    input known to within Ev gives f to within Ev on either side of a threshold -- the forward needs no exclusions.  A branch
    that computes (v not safely inside [lo, hi], s != 0) rounds at most three times -- the difference, the product, the sum --
    on the magnitudes it combines: 3 u (|bound| + s (|v - bound| + Ev) + |f| + Ev).  s = 0 and the inside select copy bits.
  the multiplier  y = f ym:  |f| Em + |ym| Ef + Ef Em + u |y|.
  the slope: the modules hold 0.01, the device list its f32 neighbour: |0.01 - f32(0.01)| (|v - bound| + Ev) on such a branch.
  the reference's own error: 8 * 2^-53 of the magnitudes of every op (relu(v - t) + t in f64 is not v to the bit).

Backward (reverse walk, go = gradient at column c on entry): the derivative is 1 strictly inside (lo, hi) and s elsewhere --
discontinuous AT a threshold, so a row whose reference input of any op lies within a guard of one of that op's finite
thresholds is left out (``guarded_rows``); on the others both sides take the same branch and
  gc = go d:        d Ego + (d not in {0, 1}: u |gc|)
  dx[c] = gc ym:    |ym| Egc + |gc| Em + Egc Em + u |gc ym|           (with a multiplier)
  dx[m] += go f:    the term to |f| Ego + |go| Ef + Ego Ef + u |go f|, the sum one more rounding u |dx[m]|.
"""

from __future__ import annotations

import math

import numpy as np
import torch

from anemoi_models_amd.layers import bounding as B

U = 2.0 ** -24
U64 = 8.0 * 2.0 ** -53
F64 = torch.float64
GUARD = 1e-5
SLOPE_GAP = abs(B.LEAKY_SLOPE - float(np.float32(B.LEAKY_SLOPE)))
ROWS = (1, 257, 1000)  # a single thread, one past a workgroup, a grid-stride tail
WIDTHS = (3, 7, 19)


def f32(v: float) -> float:
    return float(np.float32(v))


STATISTICS = {"mean": np.array([0.5, -1.0, 2.0]), "stdev": np.array([2.0, 1.5, 0.5]),
              "minimum": np.array([-4.0, -6.0, 0.0]), "maximum": np.array([6.0, 4.0, 3.0])}


def names(v_out: int):
    """The three bounded variables a, b, c of a ``v_out``-wide output: its first, middle and last column."""
    n2i = {f"v{i}": i for i in range(v_out)}
    return n2i, "v0", f"v{v_out // 2}", f"v{v_out - 1}"


def chain(v_out: int):
    """Nine modules, 11 ops: every class; one fraction whose total is among its own variables (7), one whose total is bounded
    by a later module (8, then 9).  No op's threshold is a value an earlier hard op leaves exactly (0 / -1 / 1 / 0.25)."""
    n2i, a, b, c = names(v_out)
    stats_idx = {a: 0, b: 1, c: 2}
    kw = dict(name_to_index=n2i)
    st = dict(statistics=STATISTICS, name_to_index_stats=stats_idx)
    return [
        B.ReluBounding(variables=[a], **kw),
        B.LeakyReluBounding(variables=[b], **kw),
        B.HardtanhBounding(variables=[c], min_val=-1.0, max_val=1.0, **kw),
        B.LeakyHardtanhBounding(variables=[a], min_val=f32(-0.3), max_val=f32(0.7), **kw),
        B.NormalizedReluBounding(variables=[b], min_val=[-0.625], normalizer=["mean-std"], **kw, **st),  # t = 0.25
        B.LeakyNormalizedReluBounding(variables=[c], min_val=[-1.8], normalizer=["max"], **kw, **st),    # t = -0.6
        B.FractionBounding(variables=[a], min_val=f32(-0.2), max_val=0.5, total_var=a, **kw),
        B.LeakyFractionBounding(variables=[b], min_val=f32(0.3), max_val=f32(0.9), total_var=c, **kw),
        B.ReluBounding(variables=[c], **kw),
    ]


def old_chain(v_out: int):
    """The three classes of the reference checkout only (hard ops: the fused routes must give the module route's bits)."""
    n2i, a, b, c = names(v_out)
    kw = dict(name_to_index=n2i)
    return [
        B.ReluBounding(variables=[a, c], **kw),
        B.FractionBounding(variables=[a, b], min_val=0.0, max_val=1.0, total_var=a, **kw),
        B.HardtanhBounding(variables=[c], min_val=-0.25, max_val=0.5, **kw),
        B.FractionBounding(variables=[b], min_val=-1.0, max_val=1.0, total_var=c, **kw),
    ]


def inputs(rows: int, v_out: int, seed: int = 0):
    """Seeded N(0, 1.5^2) output rows and an incoming gradient N(0, 1)."""
    gen = torch.Generator().manual_seed(1000 * seed + 31 * rows + v_out)
    return torch.randn(rows, v_out, generator=gen) * 1.5, torch.randn(rows, v_out, generator=gen)


def op_list(modules, exact: bool = False):
    """``[(col, lo, hi, mul, slope)]`` with lo / hi / slope as the f32 values the device lists hold; ``exact``: as the modules
    hold them (f64 comparisons against the module route)."""
    ops, slopes = B.compile_boundings(modules), B.bounding_slopes(modules)
    slopes = [0.0] * len(ops) if slopes is None else slopes
    r = float if exact else f32
    return [(c, r(lo), r(hi), m, r(s)) for (c, lo, hi, m), s in zip(ops, slopes)]


def op_tensors(modules, device):
    """``((col, lo, hi, mul), slope, n_tape)`` device tensors of ``ops.bound_output`` / ``autograd.bound_output``."""
    ops = op_list(modules)
    t = lambda i, dt: torch.tensor([o[i] for o in ops], dtype=dt, device=device)  # noqa: E731
    return (t(0, torch.int32), t(1, torch.float32), t(2, torch.float32), t(3, torch.int32)), t(4, torch.float32), \
        len(ops) + sum(o[3] >= 0 for o in ops)


def module_chain(modules, x: torch.Tensor) -> torch.Tensor:
    y = x.clone()
    for m in modules:
        y = m(y)
    return y


def _f(v, lo, hi, s):
    v = torch.where(v < lo, lo + s * (v - lo) if s != 0 else torch.full_like(v, lo), v) if lo > -math.inf else v
    return torch.where(v > hi, hi + s * (v - hi) if s != 0 else torch.full_like(v, hi), v) if hi < math.inf else v


def apply_ops(y: torch.Tensor, ops):
    """Sequential restatement of the op walk with slopes, in ``y``'s dtype, in place; returns ``(y, tape)`` -- the tape as
    ``anemoi_bound_output_train`` writes it: per op the value read, then the multiplier read, ``[entry, rows]``."""
    tape = []
    for c, lo, hi, m, s in ops:
        v = y[..., c].clone()
        tape.append(v.reshape(-1))
        f = _f(v, lo, hi, s)
        if m >= 0:
            ym = y[..., m].clone()
            tape.append(ym.reshape(-1))
            f = f * ym
        y[..., c] = f
    return y, (torch.stack(tape) if tape else y.new_zeros((0, y[..., 0].numel())))


def reverse_walk(g: torch.Tensor, tape: torch.Tensor, ops) -> torch.Tensor:
    """Sequential restatement of ``anemoi_bound_output_backward`` in ``g``'s dtype: a new tensor."""
    dx = g.clone()
    flat = dx.view(-1, dx.shape[-1])
    e = tape.shape[0]
    for c, lo, hi, m, s in reversed(ops):
        ym = None
        if m >= 0:
            e -= 1
            ym = tape[e]
        e -= 1
        v = tape[e]
        go = flat[:, c].clone()
        d = torch.where((v > lo) & (v < hi), torch.ones_like(v), torch.full_like(v, s))
        if m >= 0:
            flat[:, c] = go * d * ym
            flat[:, m] += go * _f(v, lo, hi, s)
        else:
            flat[:, c] = go * d
    assert e == 0
    return dx


# ------------------------------------------------------------------------------------------------ contracts with bounds
def _walk_with_bound(x: torch.Tensor, ops, module_route: bool = False):
    """The op walk in f64 with the per-element bound; also what each op read: ``[(v, Ev, f, Ef, ym, Em)]``.
    ``module_route``: the bound of the MODULES evaluated in f32 instead of the kernel -- the normalised classes (finite lo != 0,
    hi = +inf) compute act(v - t) + t, two more roundings on every element: u (|v - t| + |f|)."""
    w = x.detach().cpu().to(F64).reshape(-1, x.shape[-1]).clone()
    e = torch.zeros_like(w)
    seen = []
    for c, lo, hi, m, s in ops:
        v, ev = w[:, c].clone(), e[:, c].clone()
        f = _f(v, lo, hi, s)
        ef = ev + U64 * (v.abs() + f.abs() + (abs(lo) if math.isfinite(lo) else 0.0))
        if s != 0.0:
            for bound, outside in ((lo, v - ev < lo), (hi, v + ev > hi)):
                if math.isfinite(bound):
                    r = 3.0 * U * (abs(bound) + s * ((v - bound).abs() + ev) + f.abs() + ev) + SLOPE_GAP * ((v - bound).abs() + ev)
                    ef = ef + torch.where(outside, r, torch.zeros_like(r))
        if module_route and math.isfinite(lo) and lo != 0.0 and hi == math.inf:
            ef = ef + U * ((v - lo).abs() + ev + f.abs())
        ym = em = None
        out, eo = f, ef
        if m >= 0:
            ym, em = w[:, m].clone(), e[:, m].clone()
            out = f * ym
            eo = f.abs() * em + ym.abs() * ef + ef * em + (U + U64) * out.abs()
        seen.append((v, ev, f, ef, ym, em))
        w[:, c], e[:, c] = out, eo
    return w, e, seen


def forward_ref(x: torch.Tensor, modules, module_route: bool = False):
    """``(want, bound)`` of the forward: the module chain in f64 on ``x`` as stored, and the propagated bound (of the kernel's
    walk; ``module_route``: of the modules themselves evaluated in f32)."""
    want = module_chain(modules, x.detach().cpu().to(F64)).reshape(-1, x.shape[-1])
    walked, bound, _ = _walk_with_bound(x, op_list(modules), module_route)
    nan = torch.isnan(want)
    assert torch.equal(nan, torch.isnan(walked)) and bool(((want - walked).abs()[~nan] <= bound[~nan]).all()), \
        "the f64 op walk left the f64 module chain"
    return want.reshape(x.shape), bound.reshape(x.shape)


def guarded_rows(x: torch.Tensor, modules) -> torch.Tensor:
    """bool ``[rows]``: rows where some op's reference input lies within max(GUARD, 4 x its propagated forward bound) of one of
    that op's finite thresholds -- the backward's derivative is discontinuous there."""
    ops = op_list(modules)
    _, _, seen = _walk_with_bound(x, ops)
    out = torch.zeros(seen[0][0].shape[0], dtype=torch.bool) if seen else torch.zeros(0, dtype=torch.bool)
    for (c, lo, hi, m, s), (v, ev, *_rest) in zip(ops, seen):
        guard = torch.clamp(4.0 * ev, min=GUARD)
        for bound in (lo, hi):
            if math.isfinite(bound):
                out |= (v - bound).abs() <= guard
    return out


def backward_ref(x: torch.Tensor, g: torch.Tensor, modules):
    """``(want, bound)`` of the backward: f64 autograd over the module chain, and the bound of the reverse walk."""
    x64 = x.detach().cpu().to(F64).requires_grad_()
    module_chain(modules, x64).backward(g.detach().cpu().to(F64))
    want = x64.grad.reshape(-1, x.shape[-1])
    ops = op_list(modules)
    _, _, seen = _walk_with_bound(x, ops)
    d = g.detach().cpu().to(F64).reshape(-1, g.shape[-1]).clone()
    e = torch.zeros_like(d)
    for (c, lo, hi, m, s), (v, ev, f, ef, ym, em) in zip(reversed(ops), reversed(seen)):
        go, ego = d[:, c].clone(), e[:, c].clone()
        slope = torch.where((v > lo) & (v < hi), torch.ones_like(v), torch.full_like(v, s))
        gc = go * slope
        leaks = (slope != 0) & (slope != 1)
        egc = slope * ego + torch.where(leaks, U * gc.abs() + SLOPE_GAP * go.abs(), torch.zeros_like(gc)) + U64 * gc.abs()
        if m >= 0:
            d[:, c] = gc * ym
            e[:, c] = ym.abs() * egc + gc.abs() * em + egc * em + (U + U64) * d[:, c].abs()
            term = go * f
            et = f.abs() * ego + go.abs() * ef + ego * ef + (U + U64) * term.abs()
            d[:, m] = d[:, m] + term
            e[:, m] = e[:, m] + et + (U + U64) * d[:, m].abs()
        else:
            d[:, c], e[:, c] = gc, egc
    return want.reshape(x.shape), e.reshape(x.shape), d.reshape(x.shape)


def check(got, want, bound, what: str, keep=None) -> float:
    """NaN exactly where the contract has NaN, every other element within ``bound`` of ``want`` (rows outside the bool mask
    ``keep`` are not compared).  Returns the largest fraction of a bound that was used."""
    g = got.detach().cpu().to(F64).reshape(want.shape)
    if keep is not None:
        g, want, bound = (t.reshape(-1, t.shape[-1])[keep] for t in (g, want, bound))
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(g), nan), f"{what}: NaN at other positions than the contract"
    diff, b = (g - want).abs()[~nan], bound[~nan]
    bad = ~(diff <= b)
    ratio = torch.where(diff == 0, torch.zeros_like(diff), diff / b.clamp_min(1e-300))
    if bool(bad.any()):
        i = int(torch.argmax(torch.where(bad, ratio, torch.full_like(ratio, -1.0))))
        raise AssertionError(f"{what}: {int(bad.sum())} of {diff.numel()} elements outside their bound; worst: got "
                             f"{float(g[~nan][i]):.9g}, want {float(want[~nan][i]):.9g}, |diff| {float(diff[i]):.3e} > bound "
                             f"{float(b[i]):.3e}")
    return float(ratio.max()) if ratio.numel() else 0.0
