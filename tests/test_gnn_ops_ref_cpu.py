"""CPU checks of tests/_gnn_ops_ref.py, the yardstick of tests/test_gpu_gnn_ops.py.

Three statements:
  1. the f64 references are right: they agree with torch autograd in f64 (F.gelu / F.silu / index_add / .backward()) on every
     graph of the GPU grid;
  2. the bounds are reachable: the f32 / bf16 stand-ins of tests/_cpu_ops.py, driven through ``autograd.gather_add_act`` and
     ``autograd.segment_sum``, pass the same checker with the same bounds;
  3. the bounds are sharp: the checker rejects a correct result with one edge dropped, one wrong destination, a zeroed vector
     tail, a slice shifted by a lane, ReLU'(0) = 1, or a NaN at the largest input -- in both dtypes.
"""

import pytest
import torch
import torch.nn.functional as F

import _cpu_ops
import _gnn_ops_ref as R

DTYPES = [torch.float32, torch.bfloat16]
GRAPHS = ["main", "one_dst", "empty"]
_TORCH_ACT = {"Identity": lambda x: x, "GELU": F.gelu, "SiLU": F.silu, "ReLU": F.relu}


def _plan(kind):
    from anemoi_models_amd import runtime

    ei, n_src, n_dst = R.make_graph(kind)
    plan = runtime.build_edge_plan(ei, n_src, n_dst)
    R.check_graph_shape(kind, plan.rowptr, plan.col, n_src)
    return plan


def _operands(plan, c, dtype, act):
    t, pd, ps, dout = R.operands(plan.num_edges, plan.n_src, plan.n_dst, c, dtype, act)
    if act == "ReLU":
        planted = R.plant_zero_pre(t, pd, ps, plan.dst, plan.col)
        assert planted > 0 or plan.num_edges == 0
    return t, pd, ps, dout


# ------------------------------------------------------------------------------------------------ constants
def test_bound_constants():
    measured = R.measure_torch_f32_worst()
    print(f"torch f32 activations over the value set: worst ratio {measured:.3e} (recorded {R.TORCH_F32_WORST:.3e}), A {R.A:.3e}")
    assert abs(measured - R.TORCH_F32_WORST) <= 0.01 * R.TORCH_F32_WORST
    assert R.A == max(4.0 * R.TORCH_F32_WORST, 4e-7)
    assert R.EPS32 == 2.0 ** -23 and R.BF16_STORE == 2.0 ** -8
    # 0.8 >= max |GELU''| = 2 phi(0) and >= max |SiLU''| = 0.5, on a grid that contains both maxima
    x = torch.linspace(-12, 12, 48001, dtype=torch.float64).requires_grad_()
    for act in ("GELU", "SiLU"):
        (d2,) = torch.autograd.grad(R.dact64(x, act).sum(), x)
        assert float(d2.abs().max()) <= R.DACT_LIPSCHITZ


# ------------------------------------------------------------------------------------------------ 1. references
@pytest.mark.parametrize("act", R.ACTS)
def test_activation_reference_vs_torch_f64(act):
    x = torch.cat([torch.linspace(-40, 40, 4001, dtype=torch.float64), R.value_set_tensor()])
    if act == "ReLU":
        x = x[x != 0]  # (torch's f64 ReLU' at 0 is 0 as well; kept apart below)
    xr = x.clone().requires_grad_()
    y = _TORCH_ACT[act](xr) * 1.0
    (d,) = torch.autograd.grad(y, xr, torch.ones_like(y))
    # F.gelu in f64 evaluates 1 + erf, which cancels in the left tail: absolute agreement at f64 roundoff of |x|
    tol = 4e-16 * torch.clamp(x.abs(), min=1.0)
    assert bool(((R.act64(x, act) - y.detach()).abs() <= tol).all())
    assert bool(((R.dact64(x, act) - d).abs() <= tol).all())
    assert bool(torch.isfinite(R.act64(x, act)).all()) and bool(torch.isfinite(R.dact64(x, act)).all())
    z = torch.zeros(3, dtype=torch.float64)
    assert torch.equal(R.act64(z, act), z)
    assert torch.equal(R.dact64(z, "ReLU"), z)


@pytest.mark.parametrize("kind", GRAPHS)
@pytest.mark.parametrize("act", R.ACTS)
def test_edge_references_vs_torch_autograd_f64(kind, act):
    plan = _plan(kind)
    c = 5
    t32, pd32, ps32, dout32 = _operands(plan, c, torch.float32, act)
    t, pd, ps, dout = (x.double() for x in (t32, pd32, ps32, dout32))
    dst, src = plan.dst.long(), plan.col.long()
    tr, pdr, psr = (x.clone().requires_grad_() for x in (t, pd, ps))
    out = _TORCH_ACT[act](tr + pdr[dst] + psr[src])
    want, _, pre = R.gather_add_act_ref(t32, pd32, ps32, dst, src, act)
    assert torch.equal(pre, (t + pd[dst] + ps[src]))
    assert bool(((want - out.detach()).abs() <= 4e-16 * torch.clamp(pre.abs(), min=1.0)).all())
    out.backward(dout)
    (dt, _), (dpd, _), (dps, _) = R.gather_add_act_backward_ref(t32, pd32, ps32, dst, src, plan.rowptr, dout32, act)
    scale = 4e-16 * max(1, plan.num_edges)
    if act == "ReLU" and plan.num_edges:  # planted pre == 0: derivative 0, as torch has it
        assert int((pre == 0).sum()) > 0
    assert float((dt - tr.grad).abs().max() if dt.numel() else 0.0) <= 4e-16 * 8
    assert float((dpd - pdr.grad).abs().max()) <= scale * 8 and float((dps - psr.grad).abs().max()) <= scale * 8
    # segment_sum, its concatenated form and its backward
    v = dout
    sums, _ = R.segment_sum_ref(dout32, plan.rowptr)
    vr = v.clone().requires_grad_()
    ref = torch.zeros(plan.n_dst, c, dtype=torch.float64).index_add(0, dst, vr)
    assert float((sums - ref.detach()).abs().max()) <= scale * 8
    cat, cat_bound = R.segment_sum_cat_ref(dout32, plan.rowptr, pd32)
    assert torch.equal(cat[:, :c], pd) and torch.equal(cat[:, c:], sums) and bool((cat_bound[:, :c] == 0).all())
    g = torch.randn(plan.n_dst, c, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    ref.backward(g)
    assert torch.equal(vr.grad, g[dst])  # autograd.segment_sum's backward: dout[dst[e]]
    if kind == "empty":
        assert out.numel() == 0 and bool((sums == 0).all()) and bool((dpd == 0).all()) and bool((dps == 0).all())


# ------------------------------------------------------------------------------------------------ 2. reachable bounds
@pytest.mark.parametrize("kind", GRAPHS)
@pytest.mark.parametrize("dtype,c", [(torch.float32, 1), (torch.float32, 4), (torch.float32, 5), (torch.float32, 72),
                                     (torch.bfloat16, 6), (torch.bfloat16, 8), (torch.bfloat16, 9), (torch.bfloat16, 72)])
@pytest.mark.parametrize("act", R.ACTS)
def test_cpu_stand_ins_pass_the_bounds(monkeypatch, kind, dtype, c, act):
    from anemoi_models_amd import autograd

    _cpu_ops.install(monkeypatch)
    plan = _plan(kind)
    t, pd, ps, dout = _operands(plan, c, dtype, act)
    dst, src = plan.dst, plan.col
    tr, pdr, psr = (x.clone().requires_grad_() for x in (t, pd, ps))
    out = autograd.gather_add_act(tr, pdr, psr, plan, act)
    want, bound, _ = R.gather_add_act_ref(t, pd, ps, dst, src, act)
    R.check(out, want, bound, "gather_add_act")
    out.backward(dout)
    refs = R.gather_add_act_backward_ref(t, pd, ps, dst, src, plan.rowptr, dout, act)
    for name, got, (w, b) in zip(("d t", "d p_dst", "d p_src"), (tr.grad, pdr.grad, psr.grad), refs):
        assert got.dtype == dtype
        R.check(got, w, b, name)
    vr = dout.clone().requires_grad_()
    sums = autograd.segment_sum(vr, plan)
    R.check(sums, *R.segment_sum_ref(dout, plan.rowptr), "segment_sum")
    g = torch.randn(plan.n_dst, c, generator=torch.Generator().manual_seed(5)).to(dtype)
    sums.backward(g)
    assert torch.equal(vr.grad, g[dst.long()])
    cat = _cpu_ops.segment_sum(dout, plan.rowptr, cat_with=pd)
    R.check(cat, *R.segment_sum_cat_ref(dout, plan.rowptr, pd), "segment_sum_cat")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", R.ACTS)
def test_rounded_reference_passes_the_activation_bounds(dtype, act):
    """The correctly rounded f64 result is inside the act_forward / act_backward bounds on the whole value set."""
    x = R.value_set_tensor().to(dtype).reshape(4, -1)
    g = torch.Generator().manual_seed(2)
    res = torch.randn(x.shape, generator=g).to(dtype)
    dy = torch.randn(x.shape, generator=g).clamp(-1, 1).to(dtype)
    for r in (None, res):
        want, bound = R.act_forward_ref(x, act, r)
        assert bool(torch.isfinite(want).all())
        R.check(want.to(dtype), want, bound, "act_forward")
    want, bound = R.act_backward_ref(x, dy, act)
    assert bool(torch.isfinite(want).all())
    R.check(want.to(dtype), want, bound, "act_backward")


# ------------------------------------------------------------------------------------------------ 3. mutations
def _vec(dtype):
    return 4 if dtype == torch.float32 else 8


def _rejected(got, want, bound, what):
    with pytest.raises(AssertionError, match=what):
        R.check(got, want, bound, what)


@pytest.mark.parametrize("dtype", DTYPES)
def test_checker_rejects_a_dropped_edge(dtype):
    """One edge left out of one CSR row -- of the LONGEST row, where the bound is widest -- and of a short one."""
    plan = _plan("main")
    c = 16
    v = R.operands(plan.num_edges, plan.n_src, plan.n_dst, c, dtype, "GELU")[3]
    want, bound = R.segment_sum_ref(v, plan.rowptr)
    good = _cpu_ops.segment_sum(v, plan.rowptr)
    R.check(good, want, bound, "segment_sum")
    deg = (plan.rowptr[1:] - plan.rowptr[:-1]).long()
    short = int(torch.nonzero((deg > 0) & (deg < 40))[0])
    for row in (R.HUB_DST, short):
        for slot in (int(plan.rowptr[row]), int(plan.rowptr[row + 1]) - 1):  # the row's first and last edge
            bad = good.clone()
            bad[row] = (good[row].float() - v[slot].float()).to(dtype)
            _rejected(bad, want, bound, "segment_sum")
    # The same through the gradients of p_dst and p_src.  Their bound carries the row-wise sum of the d t bounds, which in bf16
    # grows by about 2^-8 |d t| per edge: one edge of 700 is inside it, so the long rows are tried in f32 only and a short row
    # (where one edge is far outside) in both dtypes.
    t, pd, ps, dout = _operands(plan, c, dtype, "SiLU")
    (dt, _), (dpd, dpd_b), (dps, dps_b) = R.gather_add_act_backward_ref(t, pd, ps, plan.dst, plan.col, plan.rowptr, dout, "SiLU")
    R.check(dpd.to(dtype), dpd, dpd_b, "d p_dst")
    R.check(dps.to(dtype), dps, dps_b, "d p_src")
    out_deg = torch.bincount(plan.col.long(), minlength=plan.n_src)
    short_src = int(torch.nonzero((out_deg > 0) & (out_deg < 60))[0])
    long_rows = dtype == torch.float32
    for row in ([R.HUB_DST] if long_rows else []) + [short]:
        bad = dpd.clone()
        bad[row] -= dt[int(plan.rowptr[row + 1]) - 1]
        _rejected(bad.to(dtype), dpd, dpd_b, "d p_dst")
    for row in ([R.HUB_SRC] if long_rows else []) + [short_src]:
        bad = dps.clone()
        bad[row] -= dt[int(torch.nonzero(plan.col == row)[-1])]
        _rejected(bad.to(dtype), dps, dps_b, "d p_src")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", ["Identity", "GELU", "SiLU"])
def test_checker_rejects_a_wrong_destination(dtype, act):
    plan = _plan("main")
    t, pd, ps, _ = _operands(plan, 8, dtype, act)
    want, bound, _ = R.gather_add_act_ref(t, pd, ps, plan.dst, plan.col, act)
    R.check(_cpu_ops.gather_add_act(t, pd, ps, plan.dst, plan.col, act), want, bound, "gather_add_act")
    for e in (0, plan.num_edges // 2, plan.num_edges - 1):
        dst = plan.dst.clone()
        dst[e] += 1  # (the last destination has no edges, so dst + 1 is a valid row)
        _rejected(_cpu_ops.gather_add_act(t, pd, ps, dst, plan.col, act), want, bound, "gather_add_act")


@pytest.mark.parametrize("dtype", DTYPES)
def test_checker_rejects_a_zeroed_tail_and_a_shifted_slice(dtype):
    vec = _vec(dtype)
    c = 64 * vec + vec  # a second slice with one active lane
    plan = _plan("one_dst")
    t, pd, ps, dout = _operands(plan, c, dtype, "GELU")
    want, bound, _ = R.gather_add_act_ref(t, pd, ps, plan.dst, plan.col, "GELU")
    good = _cpu_ops.gather_add_act(t, pd, ps, plan.dst, plan.col, "GELU")
    R.check(good, want, bound, "gather_add_act")
    bad = good.clone()
    bad[17, c - vec:] = 0  # the last VEC columns of one row left at zero
    _rejected(bad, want, bound, "gather_add_act")
    bad = good.clone()
    bad[:, 64 * vec:] = good[:, 64 * vec - vec: 64 * vec]  # the second slice read one lane early
    _rejected(bad, want, bound, "gather_add_act")
    want, bound = R.segment_sum_ref(dout, plan.rowptr)
    good = _cpu_ops.segment_sum(dout, plan.rowptr)
    R.check(good, want, bound, "segment_sum")
    bad = good.clone()
    bad[0, c - vec:] = 0
    _rejected(bad, want, bound, "segment_sum")
    bad = good.clone()
    bad[:, 64 * vec:] = good[:, 64 * vec - vec: 64 * vec]
    _rejected(bad, want, bound, "segment_sum")
    # the activation kernels: a dropped tail lane of the last row
    x = torch.randn(7, 3 * vec, generator=torch.Generator().manual_seed(9)).to(dtype)
    want, bound = R.act_forward_ref(x, "SiLU")
    bad = want.to(dtype)
    bad[-1, -vec:] = 0
    _rejected(bad, want, bound, "act_forward")


@pytest.mark.parametrize("dtype", DTYPES)
def test_checker_rejects_relu_gradient_one_at_zero(dtype):
    plan = _plan("main")
    t, pd, ps, dout = _operands(plan, 8, dtype, "ReLU")
    (dt, dt_b), (dpd, dpd_b), _ = R.gather_add_act_backward_ref(t, pd, ps, plan.dst, plan.col, plan.rowptr, dout, "ReLU")
    pre = R.gather_add_act_ref(t, pd, ps, plan.dst, plan.col, "ReLU")[2]
    at_zero = (pre == 0) & (dout.double() != 0)
    assert int(at_zero.sum()) > 0
    R.check(dt.to(dtype), dt, dt_b, "d t")
    bad = torch.where(at_zero, dout.double(), dt)  # ReLU' taken as 1 at pre == 0
    _rejected(bad.to(dtype), dt, dt_b, "d t")
    one = torch.zeros_like(at_zero)
    one[tuple(torch.nonzero(at_zero)[0])] = True  # a single such element
    _rejected(torch.where(one, dout.double(), dt).to(dtype), dt, dt_b, "d t")
    want, bound = R.act_backward_ref(pre.to(dtype), dout, "ReLU")
    _rejected(torch.where(at_zero, dout.double(), want).to(dtype), want, bound, "act_backward")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", R.ACTS)
def test_checker_rejects_a_nan_or_inf_at_the_largest_input(dtype, act):
    x = R.value_set_tensor().to(dtype).reshape(4, -1)
    dy = torch.full(x.shape, 0.75).to(dtype)
    for want, bound, what in ((*R.act_forward_ref(x, act), "act_forward"), (*R.act_backward_ref(x, dy, act), "act_backward")):
        for idx in (x.abs().argmax(), x.argmin()):
            for poison in (float("nan"), float("inf")):
                bad = want.to(dtype)
                bad.view(-1)[idx] = poison
                _rejected(bad, want, bound, what)
