"""f64 references, per-element error bounds and the checker for the GNN edge ops and the activation kernels.

Pure torch on the CPU; imports nothing from the GPU side.  Used by tests/test_gnn_ops_ref_cpu.py (which validates the
references against torch autograd, shows that a correct f32 / bf16 implementation reaches the bounds, and that the checker
rejects subtly wrong results) and by tests/test_gpu_gnn_ops.py (the kernels).

Every reference is computed in f64 from the operands AS STORED (a bf16 operand converts exactly).  Every bound is per element:
``|got - want| <= bound`` must hold for each element, and every element must be finite.  No global norm, nothing exempt.

Notation: eps32 = 2^-23 (spacing of f32 at 1; a rounded f32 operation errs by at most eps32 / 2 relative).  One bf16 store
is allowed 2^-8 relative: bf16 keeps 8 significant bits, so round-to-nearest errs by 2^-9 of the binade's upper end and by
up to 2^-8 of a value just above a power of two -- the kernels use 0.996 of this term (tests/test_gpu_gnn_ops.py).
"""

from __future__ import annotations

import math

import torch

EPS32 = 2.0 ** -23
BF16_STORE = 2.0 ** -8
ACTS = ("Identity", "GELU", "SiLU", "ReLU")

# Magnitudes planted (in both signs) into every activation case: zero, a value whose square underflows next to 1, the
# ordinary range, the range where exp(-x^2 / 2) and exp(-x) leave f32 (|x| around 13 and 87 .. 104), and the end of f32.
VALUE_SET = (0.0, 1e-8, 0.5, 3.0, 6.0, 10.0, 30.0, 87.0, 88.5, 89.0, 104.0, 1e4, 1e20, 3e38)

# The f32 activation bound is  A * max(1, |x|, |want|).
#   * csrc/common.hpp states |erf error| <= 1.5e-7 for fast_erf, i.e. about 1e-7 |x| for GELU = 0.5 x (1 + erf); __expf and
#     __frcp_rn add a few ulps (eps32 / 2 = 6e-8 each).
#   * TORCH_F32_WORST is the worst |y32 - y64| / max(1, |x|, |y64|) of torch's OWN f32 GELU / SiLU / ReLU and their autograd
#     derivatives on the CPU over +-VALUE_SET (measured by measure_torch_f32_worst(); test_gnn_ops_ref_cpu.py re-measures it
#     and fails if it moved by more than 1 %, either way).  Measured: 1.869e-7 (GELU at x = 3, two ulps of the result; GELU'
#     6.5e-8 at 0.5, SiLU 6.4e-8 and SiLU' 3.2e-8 at 6).  torch's f32 GELU overflows at 3e38 (it forms x (1 + erf) before halving); that
#     one element is left out of the measurement -- the kernels get no such allowance.
#   * A = max(4 * TORCH_F32_WORST, 4e-7) = 7.48e-7: the factor 4 covers the fast intrinsics, 4e-7 the documented erf bound
#     with margin.
TORCH_F32_WORST = 1.87e-7
A = max(4.0 * TORCH_F32_WORST, 4e-7)
# max |GELU''| = 2 phi(0) = 0.798, max |SiLU''| = 0.5: how far act' moves per unit of error in its argument
DACT_LIPSCHITZ = 0.8


def value_set_tensor(dtype=torch.float64) -> torch.Tensor:
    v = torch.tensor(VALUE_SET, dtype=torch.float64)
    return torch.cat([v, -v]).to(dtype)


# ------------------------------------------------------------------------------------------------ activations
def act64(x: torch.Tensor, act: str) -> torch.Tensor:
    """act(x) in f64 (x: any float dtype, converted exactly).  GELU through erfc, so that the left tail does not cancel."""
    x = x.double()
    if act == "Identity":
        return x.clone()
    if act == "GELU":  # 0.5 x (1 + erf(x / sqrt 2)) = 0.5 x erfc(-x / sqrt 2)
        return 0.5 * x * torch.special.erfc(-x * math.sqrt(0.5))
    if act == "SiLU":
        return x * torch.sigmoid(x)
    if act == "ReLU":
        return torch.where(x > 0, x, torch.zeros_like(x))
    raise KeyError(act)


def dact64(x: torch.Tensor, act: str) -> torch.Tensor:
    """act'(x) in f64.  ReLU'(0) = 0 (the kernel and torch agree)."""
    x = x.double()
    if act == "Identity":
        return torch.ones_like(x)
    if act == "GELU":  # Phi(x) + x phi(x)
        return 0.5 * torch.special.erfc(-x * math.sqrt(0.5)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    if act == "SiLU":  # s (1 + x (1 - s)), 1 - s = sigmoid(-x)
        s = torch.sigmoid(x)
        return s * (1.0 + x * torch.sigmoid(-x))
    if act == "ReLU":
        return (x > 0).double()
    raise KeyError(act)


def measure_torch_f32_worst() -> float:
    """Worst |y32 - y64| / max(1, |x|, |y64|) of torch's f32 activations and their derivatives over +-VALUE_SET."""
    import torch.nn.functional as F

    fns = {"GELU": F.gelu, "SiLU": F.silu, "ReLU": F.relu}
    x64 = value_set_tensor().float().double()  # the f32 values, exactly
    worst = 0.0
    for act, fn in fns.items():
        x32 = x64.float().requires_grad_()
        y32 = fn(x32)
        (d32,) = torch.autograd.grad(y32, x32, torch.ones_like(y32))
        for got, want in ((y32.detach(), act64(x64, act)), (d32, dact64(x64, act))):
            # torch's f32 GELU forms x (1 + erf) before halving and overflows at 3e38: that element measures nothing
            ok = torch.isfinite(got)
            assert int((~ok).sum()) <= 1 and bool(ok[x64.abs() < 1e38].all()), (act, got)
            scale = _floor1(x64, want)
            worst = max(worst, float(((got.double() - want).abs() / scale)[ok].max()))
    return worst


# ------------------------------------------------------------------------------------------------ bounds
def _is_bf16(dtype) -> bool:
    if dtype not in (torch.float32, torch.bfloat16):
        raise KeyError(dtype)
    return dtype == torch.bfloat16


def _floor1(*ts: torch.Tensor) -> torch.Tensor:
    out = torch.ones_like(ts[0])
    for t in ts:
        out = torch.maximum(out, t.abs())
    return out


def act_forward_ref(pre: torch.Tensor, act: str, residual=None):
    """(want, bound) of ``act(pre) (+ residual)`` stored in pre's dtype."""
    x = pre.double()
    want = act64(x, act)
    if residual is None:
        bound = A * _floor1(x, want)
    else:  # the sum is rounded once
        want = want + residual.double()
        bound = A * _floor1(x, residual.double())
    if _is_bf16(pre.dtype):
        bound = bound + BF16_STORE * want.abs()
    return want, bound


def act_backward_ref(pre: torch.Tensor, dy: torch.Tensor, act: str):
    """(want, bound) of ``dy * act'(pre)`` stored in pre's dtype."""
    x, d = pre.double(), dy.double()
    g = dact64(x, act)
    want = d * g
    bound = A * _floor1(x, g) * d.abs()
    if _is_bf16(pre.dtype):
        bound = bound + BF16_STORE * want.abs()
    return want, bound


def gather_add_act_ref(t, p_dst, p_src, dst, src, act: str):
    """(want, bound, pre) of ``act(t[e] + p_dst[dst[e]] + p_src[src[e]])`` stored in t's dtype; ``pre`` is the f64 argument."""
    a, b, c = t.double(), p_dst.double()[dst.long()], p_src.double()[src.long()]
    pre = a + b + c
    want = act64(pre, act)
    bound = A * _floor1(pre, want)
    if _is_bf16(t.dtype):
        bound = bound + BF16_STORE * want.abs()
    else:  # the two f32 additions
        bound = bound + 2.0 * EPS32 * (a.abs() + b.abs() + c.abs())
    return want, bound, pre


def _row_sums(v64: torch.Tensor, rowptr: torch.Tensor):
    n = rowptr.shape[0] - 1
    deg = (rowptr[1:] - rowptr[:-1]).long()
    row = torch.repeat_interleave(torch.arange(n), deg)
    return torch.zeros((n, v64.shape[1]), dtype=torch.float64).index_add_(0, row, v64), deg


def segment_sum_ref(v: torch.Tensor, rowptr: torch.Tensor):
    """(want, bound) of the per-row sums over ``rowptr``: the sequential-sum bound deg eps32 sum|v_e| (+ the bf16 store)."""
    v64 = v.double()
    want, deg = _row_sums(v64, rowptr)
    mag, _ = _row_sums(v64.abs(), rowptr)
    bound = deg.double()[:, None] * EPS32 * mag
    if _is_bf16(v.dtype):
        bound = bound + BF16_STORE * want.abs()
    return want, bound


def segment_sum_cat_ref(v, rowptr, x):
    """(want, bound) of ``[x | sums]``: the x half is a copy (bound 0)."""
    want, bound = segment_sum_ref(v, rowptr)
    return torch.cat([x.double(), want], dim=1), torch.cat([torch.zeros_like(want), bound], dim=1)


def transposed_csr(src: torch.Tensor, n_src: int):
    """(rowptr_t, order) of the source-major view of the CSR slots: ``order`` lists the slots grouped by source."""
    order = torch.argsort(src.long(), stable=True)
    rowptr_t = torch.zeros(n_src + 1, dtype=torch.int64)
    torch.cumsum(torch.bincount(src.long(), minlength=n_src), 0, out=rowptr_t[1:])
    return rowptr_t, order


def gather_add_act_backward_ref(t, p_dst, p_src, dst, src, rowptr, dout, act: str):
    """((d t, bound), (d p_dst, bound), (d p_src, bound)) of ``autograd.gather_add_act(...).backward(dout)``.

    d t = dout act'(pre).  The bound is the activation-derivative bound A max(1, |pre|, |act'|) times |dout|.  In bf16 the
    recomputed pre is stored in bf16 before act' (+ 0.8 * 2^-8 |pre| |dout|, 0.8 >= max |act''|), then comes the bf16 store.
    d p_dst / d p_src: the segment_sum bound on the reference's d t rows plus the row-wise sum of the d t bounds."""
    a, b, c = t.double(), p_dst.double()[dst.long()], p_src.double()[src.long()]
    pre, d = a + b + c, dout.double()
    g = dact64(pre, act)
    dt = d * g
    gb = A * _floor1(pre, g)
    # (Identity / ReLU: act' is piecewise constant, and the ReLU cases use operands whose sums are exact)
    if _is_bf16(t.dtype) and act not in ("Identity", "ReLU"):
        gb = gb + DACT_LIPSCHITZ * BF16_STORE * pre.abs()
    dt_bound = gb * d.abs()
    if _is_bf16(t.dtype):
        dt_bound = dt_bound + BF16_STORE * dt.abs()

    def node_grad(rp, rows):
        want, deg = _row_sums(dt[rows], rp)
        mag, _ = _row_sums(dt[rows].abs(), rp)
        carried, _ = _row_sums(dt_bound[rows], rp)
        bound = deg.double()[:, None] * EPS32 * mag + carried
        if _is_bf16(t.dtype):
            bound = bound + BF16_STORE * want.abs()
        return want, bound

    rowptr_t, order = transposed_csr(src, p_src.shape[0])
    return (dt, dt_bound), node_grad(rowptr.long(), slice(None)), node_grad(rowptr_t, order)


# ------------------------------------------------------------------------------------------------ checker
def check(got: torch.Tensor, want: torch.Tensor, bound: torch.Tensor, what: str, x=None) -> float:
    """Every element of ``got`` finite and within ``bound`` of ``want``.  Returns the worst |got - want| / bound (0 / 0 = 0:
    where the bound is zero the element must be exact).  ``x`` (the activation's argument): a failure also reports
    act_ratio(got, want, x), the figure that A bounds."""
    got = got.detach().cpu()
    if x is not None:
        what = f"{what} [worst |got - want| / max(1, |x|, |want|) = {act_ratio(got, want, x):.3e}]"
    assert got.shape == want.shape == bound.shape, f"{what}: shape {tuple(got.shape)}, expected {tuple(want.shape)}"
    if got.numel() == 0:
        return 0.0
    g = got.double()
    finite = torch.isfinite(g)
    if not bool(finite.all()):
        idx = tuple(int(i) for i in torch.nonzero(~finite)[0])
        raise AssertionError(f"{what}: {int((~finite).sum())} non-finite elements, first at {idx}: got {float(g[idx])}, "
                             f"want {float(want[idx]):.9g}")
    diff = (g - want).abs()
    bad = ~(diff <= bound)
    ratio = torch.where(diff == 0, torch.zeros_like(diff), diff / bound)
    worst = float(ratio.max())
    if bool(bad.any()):
        flat = int(torch.argmax(torch.where(bad, ratio, torch.full_like(ratio, -1.0))))
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), got.shape))
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements outside their bound; worst at {idx}: got "
                             f"{float(g[idx]):.9g}, want {float(want[idx]):.9g}, |diff| {float(diff[idx]):.3e} > bound "
                             f"{float(bound[idx]):.3e} (worst ratio {worst:.3g})")
    return worst


def act_ratio(got: torch.Tensor, want: torch.Tensor, x: torch.Tensor) -> float:
    """The figure A bounds: worst |got - want| / max(1, |x|, |want|) (reported per activation and dtype)."""
    if got.numel() == 0:
        return 0.0
    return float(((got.detach().cpu().double() - want).abs() / _floor1(x.double(), want)).max())


# ------------------------------------------------------------------------------------------------ graphs
N_SRC, N_DST = 37, 53
HUB_DST, HUB_DST_DEGREE = 7, 700
HUB_SRC, HUB_SRC_DEGREE = 11, 500
IDLE_SRC = 5


def make_graph(kind: str = "main", n_edges: int = 1500, n_dst: int = N_DST, seed: int = 0):
    """``(edge_index int64 [2, E], n_src, n_dst)``, n_src != n_dst, edges in shuffled order.

    "main": destination 0 and the last destination have no edges, HUB_DST has in-degree >= 700, IDLE_SRC no out-edges, HUB_SRC
    out-degree >= 500, the other ``n_edges - 1200`` edges are random.  "one_dst": a single destination.  "empty": E = 0."""
    g = torch.Generator().manual_seed(1000 + seed)
    if kind == "empty":
        return torch.zeros((2, 0), dtype=torch.int64), N_SRC, N_DST
    if kind == "one_dst":
        src = torch.randint(0, N_SRC - 1, (40,), generator=g)
        src = src + (src >= IDLE_SRC)
        return torch.stack([src, torch.zeros(40, dtype=torch.int64)]), N_SRC, 1
    assert kind == "main" and n_edges >= HUB_DST_DEGREE + HUB_SRC_DEGREE and n_dst > HUB_DST + 2

    def any_src(n):
        s = torch.randint(0, N_SRC - 1, (n,), generator=g)
        return s + (s >= IDLE_SRC)

    def any_dst(n):
        return torch.randint(1, n_dst - 1, (n,), generator=g)

    rest = n_edges - HUB_DST_DEGREE - HUB_SRC_DEGREE
    src = torch.cat([any_src(HUB_DST_DEGREE), torch.full((HUB_SRC_DEGREE,), HUB_SRC), any_src(rest)])
    dst = torch.cat([torch.full((HUB_DST_DEGREE,), HUB_DST), any_dst(HUB_SRC_DEGREE), any_dst(rest)])
    shuffle = torch.randperm(n_edges, generator=g)
    return torch.stack([src[shuffle], dst[shuffle]]), N_SRC, n_dst


def check_graph_shape(kind: str, rowptr: torch.Tensor, src: torch.Tensor, n_src: int) -> None:
    """The properties make_graph promises, read back from the plan the kernels get."""
    deg = (rowptr[1:] - rowptr[:-1]).long().cpu()
    out_deg = torch.bincount(src.long().cpu(), minlength=n_src)
    if kind == "main":
        assert deg[0] == 0 and deg[-1] == 0 and deg[HUB_DST] >= 700
        assert out_deg[IDLE_SRC] == 0 and out_deg[HUB_SRC] >= 500
    elif kind == "one_dst":
        assert deg.shape[0] == 1 and deg[0] == src.shape[0] > 0
    else:
        assert int(deg.sum()) == 0 and src.shape[0] == 0


def operands(n_edges: int, n_src: int, n_dst: int, c: int, dtype, act: str, seed: int = 0):
    """``t [E, C], p_dst [n_dst, C], p_src [n_src, C], dout [E, C]`` in ``dtype``.  ReLU: multiples of 2^-6 in [-2, 2] (every
    sum is exact in every dtype) with exact ``pre == 0`` planted by the caller (plant_zero_pre); otherwise unit normal."""
    g = torch.Generator().manual_seed(77 + seed + 13 * c)
    shapes = ((n_edges, c), (n_dst, c), (n_src, c), (n_edges, c))
    if act == "ReLU":
        return tuple((torch.randint(-128, 129, s, generator=g).double() / 64.0).to(dtype) for s in shapes)
    return tuple(torch.randn(s, generator=g).to(dtype) for s in shapes)


def plant_zero_pre(t, p_dst, p_src, dst, src, every: int = 7) -> int:
    """Make ``pre`` exactly zero at every ``every``-th edge's column ``e % C`` (exact-grid operands only).  Returns the count."""
    e = torch.arange(0, t.shape[0], every)
    if e.numel() == 0:
        return 0
    col = e % t.shape[1]
    val = -(p_dst.double()[dst.long()[e], col] + p_src.double()[src.long()[e], col])
    t[e, col] = val.to(t.dtype)
    assert bool((t.double()[e, col] == val).all())
    return int(e.numel())
