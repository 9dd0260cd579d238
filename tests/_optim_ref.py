"""f64 restatement of one optimizer step of ``anemoi_models_amd.optim`` (norm, clip, skip, AdamW update) over a list of
tensors, and the two error bounds the GPU tests hold ``csrc/optim.hip`` to.  No GPU, no kernel: plain torch on the CPU.

u = 2^-24 is the unit roundoff of f32 (round to nearest).  Every f32 operation the kernels use -- add, multiply, fmaf, sqrtf,
division -- is correctly rounded, so each one multiplies its exact result by (1 + e), |e| <= u.  The factor 1.01 in both
bounds covers the second-order terms ((1 + u)^n - 1 <= 1.01 n u for n <= 10^4) and, for the norm, stage 2's f64 roundings.

The norm bound
--------------
``anemoi_multi_sumsq`` adds the squares g^2 >= 0.  Because every term is non-negative, every partial sum is bounded by the
total and the relative error of the result is at most (1 + u)^k - 1 where k is the largest number of f32 roundings any ONE
term passes through -- no cancellation can amplify it.  In the committed order (csrc/optim.hip) a term passes through

* its thread's chain: OPT_CHUNK / 256 fmaf's (a thread owns OPT_CHUNK / 256 elements of a chunk; ``fmaf(x, x, acc)`` rounds
  once, the square itself is exact inside it),
* the wave butterfly: 6 additions,
* the four waves of the workgroup added in order: 3 additions,

so D = OPT_CHUNK / 256 + 6 + 3 (= 25 for OPT_CHUNK = 4096), independent of the number of chunks: stage 2 adds the per-chunk
partials in f64 (at most n_chunks 2^-53 relative, far inside the 1.01) and rounds the total to f32 once.  That last rounding
is one of the "+ 2"; the other is spare.  Hence

    |sumsq_gpu - sumsq_ref| <= 1.01 (D + 2) u sumsq_ref,      D = sumsq_depth(OPT_CHUNK, n_chunks).

The update bounds
-----------------
The kernel's arithmetic, every line one f32 operation, none contracted (``#pragma clang fp contract(off)``), with the f32
scalars clip, decay = 1 - lr wd, step_size = lr / bc1, bc2s = sqrt(bc2) (the constants kernel), w1 = f32(1 - beta1),
b2 = f32(beta2), w2 = f32(1 - beta2), eps:

    g' = clip * g                                   1 rounding
    d  = g' - m                                     1
    m' = fmaf(d, w1, m)                             1        -> N_M = 3 roundings on the path of m'
    t  = w2 * g'                                    1
    bv = b2 * v                                     1
    v' = fmaf(t, g', bv)                            1        -> N_V = 5: g' enters the product twice (2), t, bv, the fmaf
    a  = p * decay                                  1
    s  = sqrtf(v')                                  1
    r  = s / bc2s                                   1
    D  = r + eps                                    1
    q  = m' / D                                     1
    p' = fmaf(-step_size, q, a)                     1        -> N_P = 6, counted from the STORED m' and v'

Reference: the same expressions in f64 from the same f32 inputs and the same f32 scalars (read back from the device's constants
block, which the tests check against f64 on its own).  For p' the inputs are the stored f32 m' and v' -- the values the kernel
itself continues with -- so the bound on p' does not inherit the cancellation in m'.

m': |err| <= u w1 |g'| + u w1 (|g'| + |m|) + u (|m| + w1 (|g'| + |m|)) <= 3 u T_m,   T_m = |m| + w1 (|g'| + |m|).
v': the product carries (1 + u)^3 (g' twice and t), bv one rounding, the fmaf one more over the sum: <= 4 u T_v <= 5 u T_v,
    T_v = b2 v + w2 g'^2 (all terms >= 0).
p': D is a sum of non-negative terms, so its relative error is at most 3 u (s, r, the add); q adds the division: 4 u; then
    |err| <= u |p decay| + 4 u step_size |q| + u (|p decay| + step_size |q|) <= 5 u T_p <= 6 u T_p,
    T_p = |p decay| + step_size |q|.
So each output is held to 1.01 n u T with n its rounding count, n <= 8 for all three (a larger count would mean an
approximation -- a fast reciprocal or rsqrt -- crept in).  Where a result falls into the subnormal range the relative model
fails by at most half the smallest subnormal per rounding; the bounds carry n 2^-149 for that.
"""

from __future__ import annotations

import math

import torch

U = 2.0 ** -24
TINY = 2.0 ** -149
N_M, N_V, N_P = 3, 5, 6


def f32(x: float) -> float:
    """x rounded to f32, as a Python float."""
    return float(torch.tensor(float(x), dtype=torch.float64).to(torch.float32))


def sumsq_depth(chunk: int, n_chunks: int) -> int:
    """Longest chain of f32 roundings a term of ``anemoi_multi_sumsq`` passes through (the chunk count does not enter:
    stage 2 adds in f64)."""
    return chunk // 256 + 6 + 3


def n_chunks(numels, chunk: int) -> int:
    return sum((int(n) + chunk - 1) // chunk for n in numels)


def sumsq(grads) -> float:
    return math.fsum(float((g.detach().double().cpu() ** 2).sum()) for g in grads)


def sumsq_bound(ref: float, chunk: int, chunks: int) -> float:
    return 1.01 * (sumsq_depth(chunk, chunks) + 2) * U * ref


def constants(sumsq32, step: float, lr: float, betas, weight_decay: float, max_norm=None, skip_nonfinite: bool = False):
    """The step's scalars in f64 from the f32 sum of squares (or None: no norm), the step count BEFORE the step and the
    group's hyper-parameters as torch takes them (lr: the float, or the f32 value of a device tensor).  What ``anemoi_adamw_constants`` writes, unrounded."""
    norm, clip, finite = 0.0, 1.0, True
    if sumsq32 is not None:
        norm = math.sqrt(sumsq32) if sumsq32 >= 0 else float("nan")
        finite = math.isfinite(norm)
        if max_norm is not None:
            c = max_norm / (norm + 1e-6)
            clip = c if (c != c or c <= 1.0) else 1.0
    skip = bool(skip_nonfinite and not finite)
    t = step + (0 if skip else 1)
    bc1, bc2 = 1.0 - betas[0] ** t, 1.0 - betas[1] ** t
    return dict(norm=norm, clip=clip, finite=finite, skip=skip, t=t, decay=1.0 - lr * weight_decay,
                step_size=lr / bc1 if bc1 != 0 else float("inf"), bc2s=math.sqrt(bc2), lr=lr)


def step_f64(params, grads, exp_avg, exp_avg_sq, steps, groups, max_norm=None, skip_nonfinite=False):
    """One whole step in f64, in place, over ``groups`` = list of (indices into the lists, dict(lr, betas, eps,
    weight_decay)); ``steps``: list of step counts per group, advanced in place.  Tensors with ``grad None`` are skipped; one
    norm over everything else.  Returns the scalars of the first group (norm, clip, skip ...)."""
    live = [g for g in grads if g is not None]
    s = sumsq(live) if (max_norm is not None or skip_nonfinite) else None
    first = None
    for gi, (idx, h) in enumerate(groups):
        if not any(grads[i] is not None for i in idx):
            continue
        c = constants(s, steps[gi], h["lr"], h["betas"], h["weight_decay"], max_norm, skip_nonfinite)
        first = first or c
        if c["skip"]:
            continue
        steps[gi] = c["t"]
        b1, b2 = h["betas"]
        for i in idx:
            if grads[i] is None:
                continue
            g = c["clip"] * grads[i]
            params[i].mul_(c["decay"])
            exp_avg[i].add_((g - exp_avg[i]) * (1.0 - b1))
            exp_avg_sq[i].mul_(b2).add_((1.0 - b2) * g * g)
            params[i].sub_(c["step_size"] * exp_avg[i] / (exp_avg_sq[i].sqrt() / c["bc2s"] + h["eps"]))
    return first


def moments_ref(g, m, v, clip: float, beta1: float, beta2: float):
    """(m_ref, m_bound, v_ref, v_bound) in f64 per element from the f32 inputs and the f32 scalars of the kernel."""
    w1, b2, w2 = f32(1.0 - beta1), f32(beta2), f32(1.0 - beta2)
    g, m, v = (t.detach().double().cpu() for t in (g, m, v))
    gc = clip * g
    m_ref = m + (gc - m) * w1
    v_ref = b2 * v + w2 * gc * gc
    m_bound = 1.01 * N_M * U * (m.abs() + w1 * (gc.abs() + m.abs())) + N_M * TINY
    v_bound = 1.01 * N_V * U * v_ref.abs() + N_V * TINY
    return m_ref, m_bound, v_ref, v_bound


def param_ref(p, m_new, v_new, decay: float, step_size: float, bc2s: float, eps: float):
    """(p_ref, p_bound) in f64 per element from the old f32 p, the STORED f32 moments and the f32 scalars."""
    p, m_new, v_new = (t.detach().double().cpu() for t in (p, m_new, v_new))
    q = m_new / (v_new.sqrt() / bc2s + f32(eps))
    a = p * decay
    return a - step_size * q, 1.01 * N_P * U * (a.abs() + step_size * q.abs()) + N_P * TINY
