"""The truncated residual connection on the HIP kernel (csrc/truncation.hip): anemoi_csr_project against f64 with a derived
per-element bound, its ownership and determinism properties, autograd.truncated_residual, and the models / training routes
that use it."""

import numpy as np
import pytest
import torch

import _truncation_ref as tr
from test_gpu_parity import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
FWD_TOL = {torch.float32: 1e-5, torch.bfloat16: 1e-2}  # the project's bounds (tests/test_gpu_cond_ln.py)
GRAD_TOL = {torch.float32: 1e-4, torch.bfloat16: 3e-2}
# the kernel gives W = 1, 2, 4, .., 64 lanes to a row (R = 64 / W rows per wave) and chunks P > 64 by 64: both sides of every step
P_CASES = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 130, 260]
SIZES = [(300, 77), (77, 300)]  # (n_in, n_out): n_out = 77 is a multiple of no R > 1, 300 of R = 2 and 4 only


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from anemoi_models_amd import _lib

    _lib.load()  # the native library must be present: no fallback
    assert torch.cuda.is_available()


_CSR = {}


def _csr(n_in, n_out):
    """One matrix per size, shared by every test: row lengths from {0, 1, 3, 63, 64, 65, 200}, each at least once."""
    if (n_in, n_out) not in _CSR:
        rng = np.random.default_rng(n_in * 1000 + n_out)
        lengths = tr.row_lengths(rng, n_out)
        assert set(lengths.tolist()) == {0, 1, 3, 63, 64, 65, 200}
        _CSR[(n_in, n_out)] = tr.random_csr(rng, n_out, n_in, lengths)
    return _CSR[(n_in, n_out)]


def _columns(rng, width, p):
    """``p`` distinct columns of ``width`` in a non-monotone order (never the identity for p > 1)."""
    cols = rng.permutation(width)[:p]
    if p > 1 and bool((np.diff(cols) > 0).all()):
        cols = cols[::-1].copy()
    return torch.from_numpy(cols.astype(np.int32))


def _case(n_in, n_out, slabs, v_in, p, seed=0):
    rng = np.random.default_rng(seed + 17 * p + v_in)
    v_in = max(v_in, p + 3)
    v_out = p + 4
    gen = torch.Generator().manual_seed(seed + p)
    x = torch.randn(slabs, 2, 1, n_in, v_in, generator=gen)  # [B, T = 2, Ens, n_in, V_in]: the kernel reads time slice 1 in place
    big = torch.randn(slabs + 2, 1, n_out, v_out, generator=gen)  # one sentinel slab before and one behind the output
    return {"x": x, "big": big, "cols_in": _columns(rng, v_in, p), "cols_out": _columns(rng, v_out, p),
            "mul": torch.rand(v_in, generator=gen) + 0.5, "add": torch.randn(v_in, generator=gen)}


def _run(case, csr, accumulate, affine, identity_cols=False):
    from anemoi_models_amd import ops

    x, big = case["x"].to(DEV), case["big"].to(DEV).clone()
    ci = None if identity_cols else case["cols_in"].to(DEV)
    co = None if identity_cols else case["cols_out"].to(DEV)
    aff = (case["mul"].to(DEV), case["add"].to(DEV)) if affine else None
    ops.csr_project(x[:, -1], big[1:-1], *(t.to(DEV) for t in csr), ci, co, aff, accumulate=accumulate,
                    p=case["cols_in"].numel())
    return big.cpu()


def _want(case, csr, n_in, accumulate, affine, identity_cols=False):
    p = case["cols_in"].numel()
    ci = torch.arange(p) if identity_cols else case["cols_in"].long()
    co = torch.arange(p) if identity_cols else case["cols_out"].long()
    xs = case["x"][:, -1].double()
    if affine:
        xs = xs * case["mul"].double() + case["add"].double()
    y0 = case["big"][1:-1][..., co] if accumulate else None
    want, bound = tr.project_with_bound(csr, n_in, xs[..., ci], y0)
    return want, bound, co


@pytest.mark.parametrize("p", P_CASES)
@pytest.mark.parametrize("n_in,n_out", SIZES)
def test_csr_project_vs_f64_store_accumulate_affine(n_in, n_out, p):
    """Every element within 1.01 (L_i + 4) 2^-24 (sum_k |val_k| |x'_k| + |y0|) of the f64 product -- the forward-error bound of
    an L-term f32 FMA recursion plus one rounding each for the affine map and the accumulate; empty rows exactly 0 / y0;
    columns outside cols_out and the slabs around the output keep their bits."""
    csr = _csr(n_in, n_out)
    empty = (csr[0][1:] == csr[0][:-1])
    assert bool(empty.any())
    for slabs in (1, 3):
        for v_in in (7, 140):
            case = _case(n_in, n_out, slabs, v_in, p)
            for accumulate in (False, True):
                for affine in (False, True):
                    got = _run(case, csr, accumulate, affine)
                    want, bound, co = _want(case, csr, n_in, accumulate, affine)
                    err = (got[1:-1][..., co].double() - want).abs()
                    worst = float((err / bound.clamp_min(1e-300)).max())
                    print(f"n_in={n_in} n_out={n_out} P={p} slabs={slabs} V_in={case['x'].shape[-1]} acc={accumulate} "
                          f"affine={affine}: worst error {worst:.3f} of the bound")
                    assert bool((err <= bound).all()), (slabs, v_in, accumulate, affine, worst)
                    rows = got[1:-1][:, :, empty][..., co]
                    if accumulate:
                        assert torch.equal(rows, case["big"][1:-1][:, :, empty][..., co])
                    else:
                        assert torch.equal(rows, torch.zeros_like(rows)) and not bool(torch.signbit(rows).any())
                    # ownership: nothing else is written
                    other = [c for c in range(got.shape[-1]) if c not in co.tolist()]
                    assert torch.equal(got[1:-1][..., other].view(torch.int32), case["big"][1:-1][..., other].view(torch.int32))
                    assert torch.equal(got[0].view(torch.int32), case["big"][0].view(torch.int32))
                    assert torch.equal(got[-1].view(torch.int32), case["big"][-1].view(torch.int32))


@pytest.mark.parametrize("p", [5, 64, 130])
def test_csr_project_identity_columns_and_strided_slabs(p):
    """NULL column lists are 0..P-1; the two slab levels take the strides of a transposed view (the ensemble inference route
    hands the state over as x.transpose(0, 2))."""
    from anemoi_models_amd import ops

    n_in, n_out = 300, 77
    csr = _csr(n_in, n_out)
    case = _case(n_in, n_out, 3, 140, p)
    for accumulate in (False, True):
        got = _run(case, csr, accumulate, True, identity_cols=True)
        want, bound, co = _want(case, csr, n_in, accumulate, True, identity_cols=True)
        assert bool(((got[1:-1][..., co].double() - want).abs() <= bound).all())
        assert torch.equal(got[1:-1][..., p:], case["big"][1:-1][..., p:])
    # [1, T, 3, n_in, V] seen as [3, T, 1, n_in, V] (a transposed view), written into [1, 3, n_out, P] seen as [3, 1, n_out, P]
    x = case["x"].transpose(0, 2).contiguous().to(DEV)  # [1, T, 3, ..]
    out_a = torch.zeros(1, 3, n_out, p, device=DEV)
    out_b = torch.zeros(3, 1, n_out, p, device=DEV)
    dev_csr = [t.to(DEV) for t in csr]
    ci = case["cols_in"].to(DEV)
    ops.csr_project(x[:, -1], out_a, *dev_csr, ci, None)
    xt = x.transpose(0, 2)
    assert not xt.is_contiguous()
    ops.csr_project(xt[:, -1], out_b, *dev_csr, ci, None)
    assert torch.equal(out_a[0], out_b[:, 0])
    ops.csr_project(xt[:, -1], out_a.transpose(0, 1), *dev_csr, ci, None, accumulate=True)  # the output view strided as well
    assert torch.equal(out_a[0], 2 * out_b[:, 0])


def test_csr_project_is_deterministic_and_slabs_are_independent():
    from anemoi_models_amd import ops

    n_in, n_out = 300, 77
    csr = [t.to(DEV) for t in _csr(n_in, n_out)]
    for p in (5, 33, 130):
        case = _case(n_in, n_out, 3, 140, p, seed=3)
        x, ci, co = case["x"].to(DEV), case["cols_in"].to(DEV), case["cols_out"].to(DEV)
        y0 = case["big"][1:-1].to(DEV)
        runs = [ops.csr_project(x[:, -1], y0.clone(), *csr, ci, co, accumulate=True) for _ in range(2)]
        assert torch.equal(runs[0], runs[1])
        single = y0.clone()
        for s in range(3):
            ops.csr_project(x[s:s + 1, -1], single[s:s + 1], *csr, ci, co, accumulate=True)
        assert torch.equal(single, runs[0])


# csrc/truncation.hip launches at most CSR_MAX_BLOCKS_X = 8192 workgroups of 4 waves along the rows and strides the rest: more
# than 32 768 row groups (of R rows) take the loop a second time -- the path every launch over config 3's 542 080 rows is on
GRID_STRIDE_GROUPS = 8192 * 4


@pytest.mark.parametrize("p,rows_per_wave", [(33, 1), (17, 2)])
def test_csr_project_beyond_the_grid_cap(p, rows_per_wave):
    """One row per wave (W = 64) and packed rows (W = 32, R = 2), each with 77 rows -- an odd count -- beyond one pass of the
    capped grid: the per-element f64 bound, empty rows and the sentinels of test_csr_project_vs_f64_store_accumulate_affine on
    every row, so a row that a stride skipped or met twice (which double-adds when accumulating) fails."""
    from anemoi_models_amd import ops

    n_in, n_out = 300, GRID_STRIDE_GROUPS * rows_per_wave + 77
    rng = np.random.default_rng(p)
    csr = tr.random_csr(rng, n_out, n_in, rng.choice((0, 1, 3, 5), size=n_out))
    empty = (csr[0][1:] == csr[0][:-1])
    case = _case(n_in, n_out, 1, 40, p, seed=5)
    co = case["cols_out"].long()
    dev_csr = [t.to(DEV) for t in csr]
    for accumulate, affine in ((False, False), (True, True)):
        got = _run(case, dev_csr, accumulate, affine)
        xs = case["x"][:, -1].double()
        if affine:
            xs = xs * case["mul"].double() + case["add"].double()
        y0 = case["big"][1:-1][..., co] if accumulate else None
        want, bound = tr.project_with_bound_sparse(csr, xs[..., case["cols_in"].long()], y0)
        err = (got[1:-1][..., co].double() - want).abs()
        bad = (err > bound).any(-1).nonzero()
        print(f"P={p} R={rows_per_wave} n_out={n_out} acc={accumulate}: worst error "
              f"{float((err / bound.clamp_min(1e-300)).max()):.3f} of the bound")
        assert bad.numel() == 0, f"{bad.shape[0]} rows off their bound, first {bad[0].tolist()}"
        rows = got[1:-1][:, :, empty][..., co]
        assert torch.equal(rows, case["big"][1:-1][:, :, empty][..., co] if accumulate else torch.zeros_like(rows))
        other = [c for c in range(got.shape[-1]) if c not in co.tolist()]
        assert torch.equal(got[1:-1][..., other].view(torch.int32), case["big"][1:-1][..., other].view(torch.int32))
        assert torch.equal(got[0].view(torch.int32), case["big"][0].view(torch.int32))
        assert torch.equal(got[-1].view(torch.int32), case["big"][-1].view(torch.int32))


def test_csr_project_edge_shapes_and_refusals():
    from anemoi_models_amd import ops

    csr = [t.to(DEV) for t in _csr(300, 77)]
    x = torch.randn(1, 1, 300, 8, device=DEV)
    # n_out = 0, no slabs: nothing to do
    empty_ptr = torch.zeros(1, dtype=torch.int64, device=DEV)
    none_i, none_v = torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(0, device=DEV)
    assert ops.csr_project(x, torch.zeros(1, 1, 0, 8, device=DEV), empty_ptr, none_i, none_v).shape == (1, 1, 0, 8)
    assert ops.csr_project(x[:0], torch.zeros(0, 1, 77, 8, device=DEV), *csr).numel() == 0
    # a matrix without entries: the store writes zeros into its columns only, the accumulate nothing
    ptr0 = torch.zeros(78, dtype=torch.int64, device=DEV)
    cols = torch.tensor([2, 0], dtype=torch.int32, device=DEV)
    out = torch.full((1, 1, 77, 3), 7.0, device=DEV)
    ops.csr_project(x, out, ptr0, none_i, none_v, cols, cols)
    assert bool((out[..., 1] == 7).all()) and bool((out[..., [0, 2]] == 0).all())
    ops.csr_project(x, out, ptr0, none_i, none_v, cols, cols, accumulate=True)
    assert bool((out[..., 1] == 7).all()) and bool((out[..., [0, 2]] == 0).all())
    out = torch.zeros(1, 1, 77, 8, device=DEV)
    with pytest.raises(ValueError):
        ops.csr_project(x.double(), out, *csr)
    with pytest.raises(ValueError):
        ops.csr_project(x, out, csr[0][:-1], csr[1], csr[2])
    with pytest.raises(ValueError):
        ops.csr_project(x, out, *csr, cols, torch.tensor([0, 1, 2], dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        ops.csr_project(x, out[..., ::2], *csr, p=4)  # columns must have unit stride
    with pytest.raises(ValueError):
        ops.csr_project(x, out.expand(2, 1, 77, 8), *csr)  # slab counts differ
    with pytest.raises(ValueError, match="overlap"):
        ops.csr_project(x.expand(2, 1, 300, 8), out.expand(2, 1, 77, 8), *csr)  # two slabs on one piece of memory
    with pytest.raises(RuntimeError):
        ops.csr_project(x.cpu(), out, *csr)
    # column values: inside the widths, the output side without repeats; x and out apart
    as_cols = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)  # noqa: E731
    with pytest.raises(ValueError, match="cols_in"):
        ops.csr_project(x, out, *csr, as_cols([0, 8]), as_cols([0, 1]))
    with pytest.raises(ValueError, match="cols_out"):
        ops.csr_project(x, out, *csr, as_cols([0, 1]), as_cols([-1, 1]))
    with pytest.raises(ValueError, match="repeats"):
        ops.csr_project(x, out, *csr, as_cols([1, 1]), as_cols([3, 3]))
    ops.csr_project(x, out, *csr, as_cols([1, 1]), as_cols([3, 4]))  # (an input column may feed two output columns)
    assert torch.equal(out[..., 3], out[..., 4]) and bool(out[..., 3].any())
    both = torch.zeros(1, 1, 300, 16, device=DEV)
    with pytest.raises(ValueError, match="overlap"):
        ops.csr_project(both[..., :8], both[:, :, :77, 8:], *csr)


# ------------------------------------------------------------------------------------------------------------ autograd
def _plan_matrices(g, g_c, seed=0, down_len=(0, 1, 3, 9), up_len=(0, 1, 3, 4)):
    rng = np.random.default_rng(seed)
    down = tr.random_csr(rng, g_c, g, rng.choice(down_len, size=g_c), 0.4)
    up = tr.random_csr(rng, g, g_c, rng.choice(up_len, size=g), 0.6)
    return {"down": (*down, (g_c, g)), "up": (*up, (g, g_c))}


@pytest.mark.parametrize("stages", ["both", "up"])
def test_truncated_residual_forward_and_backward_vs_f64(stages):
    """autograd.truncated_residual: y against the f64 restatement with the chained per-element bound; d out is the incoming
    gradient exactly; dx against f64 autograd with the same bound formed on the transposed matrices, and exactly zero outside
    the prognostic columns of the last time slice."""
    from anemoi_models_amd import autograd
    from anemoi_models_amd.layers.truncation import TruncationPlan

    b, t, e, g, g_c, v_in, v_out = 2, 2, 3, 300, 77, 9, 8
    data = _plan_matrices(g, g_c, 5)
    if stages == "up":  # one matrix alone: G x G
        rng = np.random.default_rng(6)
        data = {"up": (*tr.random_csr(rng, g, g, rng.choice((0, 1, 3, 65), size=g), 0.5), (g, g))}
    plan = TruncationPlan(data)
    gen = torch.Generator().manual_seed(1)
    out = torch.randn(b * e * g, v_out, generator=gen)
    x = torch.randn(b, t, e, g, v_in, generator=gen)
    dy = torch.randn(b, e, g, v_out, generator=gen)
    out_idx, in_idx = torch.tensor([6, 0, 3, 1, 4]), torch.tensor([2, 8, 0, 5, 3])
    o_dev, x_dev = out.to(DEV).requires_grad_(), x.to(DEV).requires_grad_()
    y = autograd.truncated_residual(o_dev, x_dev, plan, out_idx.to(DEV, torch.int32), in_idx.to(DEV, torch.int32), (b, e, g, v_out))
    y.backward(dy.to(DEV))
    assert torch.equal(o_dev.grad.cpu(), dy.reshape(out.shape))
    # forward
    mats = [(m.indptr, m.idx, m.val) for m in plan.stages]
    cur, err = x[:, -1].double()[..., in_idx], None
    for m, s in zip(mats, plan.stages):
        last = m is mats[-1]
        cur, err = tr.project_with_bound(m, s.shape[1], cur, out.reshape(b, e, g, v_out)[..., out_idx] if last else None, err)
    got = y.detach().cpu()
    assert bool(((got[..., out_idx].double() - cur).abs() <= err).all())
    rest = [c for c in range(v_out) if c not in out_idx.tolist()]
    assert torch.equal(got[..., rest], out.reshape(b, e, g, v_out)[..., rest])
    # backward: f64 autograd of the restatement, bound from the transposed chain
    x64 = x.double().requires_grad_()
    dense = [tr.dense(*m, s.shape[1]) for m, s in zip(mats, plan.stages)]
    tr.truncated_residual(out.reshape(b, e, g, v_out), x64, dense, out_idx, in_idx).backward(dy.double())
    cur, err = dy.double()[..., out_idx], None
    for s in reversed(plan.stages):
        st = s.transpose()
        assert st.shape == (s.shape[1], s.shape[0])
        cur, err = tr.project_with_bound((st.indptr, st.idx, st.val), st.shape[1], cur, None, err)
    dx = x_dev.grad.cpu()
    assert float((cur - x64.grad[:, -1][..., in_idx]).abs().max()) <= 1e-12 * float(cur.abs().max())
    assert bool(((dx[:, -1][..., in_idx].double() - x64.grad[:, -1][..., in_idx]).abs() <= err).all())
    others = [c for c in range(v_in) if c not in in_idx.tolist()]
    assert not bool(dx[:, :-1].any()) and not bool(dx[:, -1][..., others].any())
    # x without a gradient: none is computed
    y2 = autograd.truncated_residual(out.to(DEV).requires_grad_(), x.to(DEV), plan, out_idx.to(DEV, torch.int32),
                                     in_idx.to(DEV, torch.int32), (b, e, g, v_out))
    assert torch.equal(y2.detach(), y.detach())


# ------------------------------------------------------------------------------------------------------------ models
def _flat_model(graph, truncation_data=None, boundings=None, seed=3):
    from anemoi_models_amd.models import AnemoiModelEncProcDec
    from anemoi_models_amd.utils.indices import SimpleDataIndices
    from anemoi_models_amd.utils.presets import model_config

    torch.manual_seed(seed)
    cfg = model_config("GraphTransformer", 64, 2, 16)
    if boundings:
        cfg["model"]["bounding"] = [dict(b) for b in boundings]
    idx = SimpleDataIndices(n_prognostic=10, n_forcing=2, n_diagnostic=1)
    return AnemoiModelEncProcDec(model_config=type(cfg)(cfg), data_indices=idx, graph_data=graph,
                                 truncation_data=truncation_data).to(DEV), idx


def _identity(g):
    return (torch.arange(g + 1), torch.arange(g), torch.ones(g), (g, g))


def _expected(y0, x, model, data):
    """y0 - x_last[prog] + A_up A_down x_last[prog] in f64 on the CPU (``y0``: the same weights without truncation)."""
    oi = torch.as_tensor(model._internal_output_idx).long()
    ii = torch.as_tensor(model._internal_input_idx).long()
    skip = x[:, -1].double().cpu()[..., ii]
    proj = skip
    for key in ("down", "up"):
        if key in data:
            m = data[key]
            proj = torch.matmul(tr.dense(m[0], m[1], m[2], m[3][1]), proj)
    want = y0.double().cpu().clone()
    want[..., oi] += proj - skip
    return want


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_model_inference_with_truncation(graph_o32, monkeypatch, mode):
    monkeypatch.setenv("ANEMOI_AMD_DTYPE", mode)
    g = graph_o32["data"].num_nodes
    data = _plan_matrices(g, 400, 9)
    plain, idx = _flat_model(graph_o32)
    trunc, _ = _flat_model(graph_o32, data)
    trunc.load_state_dict(plain.state_dict())
    x = torch.randn(2, 2, 1, g, idx.num_input, generator=torch.Generator().manual_seed(4)).to(DEV)
    with torch.no_grad():
        y0, y = plain.eval()(x), trunc.eval()(x)
    err = rel_err(y, _expected(y0, x, trunc, data))
    print(f"flat model with truncation, {mode}: rel_err {err:.3e} against y0 - x + A_up A_down x")
    assert y.shape == y0.shape and err < 1e-5  # (both runs share a bit-identical decoder output: the f32 bound in bf16 too)
    assert not torch.equal(y, y0)


def test_model_inference_with_truncation_and_a_bounding(graph_o32, monkeypatch):
    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "fp32")
    g = graph_o32["data"].num_nodes
    data = _plan_matrices(g, 400, 9)
    relu = [{"_target_": "anemoi.models.layers.bounding.ReluBounding", "variables": ["prog_0", "prog_3"]}]
    free, idx = _flat_model(graph_o32)
    trunc, _ = _flat_model(graph_o32, data, relu)
    trunc.load_state_dict(free.state_dict())
    x = torch.randn(1, 2, 1, g, idx.num_input, generator=torch.Generator().manual_seed(4)).to(DEV)
    with torch.no_grad():
        y0, y = free.eval()(x), trunc.eval()(x)
        free_form = _expected(y0, x, trunc, data).float()
        want = free_form.clone()
        for bounding in trunc.boundings:  # the model's own bounding modules on the expected pre-bounding tensor
            want = bounding.cpu()(want)
    assert not torch.equal(want, free_form) and rel_err(y, want) < 1e-5


def test_ensemble_model_inference_with_truncation(graph_o32, monkeypatch):
    from test_gpu_cond_ln import NOISE
    from anemoi_models_amd.models import AnemoiEnsModelEncProcDec
    from anemoi_models_amd.utils.indices import SimpleDataIndices
    from anemoi_models_amd.utils.presets import model_config

    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "fp32")
    g = graph_o32["data"].num_nodes
    data = _plan_matrices(g, 400, 9)
    idx = SimpleDataIndices(n_prognostic=10, n_forcing=2, n_diagnostic=1)
    kw = dict(model_config=model_config("Transformer", 64, 2, noise_injector=NOISE), data_indices=idx, graph_data=graph_o32)
    torch.manual_seed(5)
    plain = AnemoiEnsModelEncProcDec(**kw).to(DEV).eval()
    trunc = AnemoiEnsModelEncProcDec(**kw, truncation_data=data).to(DEV).eval()
    trunc.load_state_dict(plain.state_dict())
    x = torch.randn(1, 2, 3, g, idx.num_input, generator=torch.Generator().manual_seed(6)).to(DEV)  # E = 3 members
    with torch.no_grad():
        torch.manual_seed(77)
        y0 = plain(x)
        torch.manual_seed(77)  # the same noise: the decoder outputs are bit-identical
        y = trunc(x)
    assert tuple(y.shape) == (1, 3, g, trunc.num_output_channels)
    assert rel_err(y, _expected(y0, x, trunc, data)) < 1e-5


def test_hierarchical_model_with_truncation(graph_hier, monkeypatch):
    """The hierarchical model reaches the truncated skip through the shared ``_finish``: inference against y0 - x + A_up A_down x;
    in training the skip is a constant of the parameters, so their gradients are those of the untruncated model bit for bit."""
    from anemoi_models_amd.models import AnemoiModelEncProcDecHierarchical
    from anemoi_models_amd.utils.indices import SimpleDataIndices
    from anemoi_models_amd.utils.presets import hierarchical_model_config

    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "fp32")
    g = graph_hier["data"].num_nodes
    data = _plan_matrices(g, 400, 9)
    idx = SimpleDataIndices(n_prognostic=10, n_forcing=2, n_diagnostic=1)
    kw = dict(model_config=hierarchical_model_config(64, 16), data_indices=idx, graph_data=graph_hier)
    torch.manual_seed(3)
    plain = AnemoiModelEncProcDecHierarchical(**kw).to(DEV)
    trunc = AnemoiModelEncProcDecHierarchical(**kw, truncation_data=data).to(DEV)
    assert list(plain.state_dict()) == list(trunc.state_dict())
    trunc.load_state_dict(plain.state_dict())
    x = torch.randn(1, 2, 1, g, idx.num_input, generator=torch.Generator().manual_seed(4)).to(DEV)
    with torch.no_grad():
        y0, y = plain.eval()(x), trunc.eval()(x)
    assert rel_err(y, _expected(y0, x, trunc, data)) < 1e-5
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    grads = []
    for m in (plain, trunc):
        m.train()
        m(x).backward(dy)
        grads.append({k: p.grad for k, p in m.named_parameters() if p.grad is not None})
    assert set(grads[0]) == set(grads[1]) and len(grads[0]) > 20
    for k, gr in grads[0].items():
        assert torch.equal(gr, grads[1][k]), k


def test_identity_matrices_give_the_bits_of_the_untruncated_route(graph_o32, monkeypatch):
    """A_down = A_up = I: inference and training (output and every parameter gradient) bit-equal to the model without
    truncation_data."""
    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "fp32")
    g = graph_o32["data"].num_nodes
    plain, idx = _flat_model(graph_o32)
    trunc, _ = _flat_model(graph_o32, {"down": _identity(g), "up": _identity(g)})
    trunc.load_state_dict(plain.state_dict())
    x = torch.randn(1, 2, 1, g, idx.num_input, generator=torch.Generator().manual_seed(4)).to(DEV)
    dy = torch.randn(1, 1, g, plain.num_output_channels, generator=torch.Generator().manual_seed(5)).to(DEV)
    with torch.no_grad():
        assert torch.equal(plain.eval()(x), trunc.eval()(x))
    grads = []
    for m in (plain, trunc):
        m.train()
        y = m(x)
        y.backward(dy)
        grads.append((y.detach(), {k: p.grad for k, p in m.named_parameters() if p.grad is not None}))
    assert torch.equal(grads[0][0], grads[1][0]) and set(grads[0][1]) == set(grads[1][1]) and len(grads[0][1]) > 20
    for k, gr in grads[0][1].items():
        assert torch.equal(gr, grads[1][1][k]), k


def test_predict_step_with_truncation_matches_the_hand_composition(graph_o32, golden_interface, monkeypatch):
    """predict_step with a plain InputNormalizer: the fused route (affine maps on the first and last kernels, the projection
    reading the raw state) against normalise -> model -> de-normalise composed by hand."""
    from conftest import split_prefix
    from anemoi_models_amd.interface import AnemoiModelInterface
    from anemoi_models_amd.utils.indices import SimpleDataIndices
    from anemoi_models_amd.utils.presets import model_config

    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "fp32")
    g = graph_o32["data"].num_nodes
    data = _plan_matrices(g, 400, 9)
    cfg = model_config("GraphTransformer", 64, 2, 16)
    cfg["data"] = {"forcing": ["forc_0", "forc_1"], "diagnostic": ["diag_0"],
                   "processors": {"normalizer": {"_target_": "anemoi.models.preprocessing.normalizer.InputNormalizer",
                                                 "config": {"default": "mean-std"}}}}
    cfg["model"]["model"] = {"_target_": "anemoi.models.models.encoder_processor_decoder.AnemoiModelEncProcDec"}
    stats = {k: v.numpy() for k, v in split_prefix(golden_interface, "stat.").items()}
    idx = SimpleDataIndices(n_prognostic=10, n_forcing=2, n_diagnostic=1)
    torch.manual_seed(2)
    iface = AnemoiModelInterface(config=type(cfg)(cfg), graph_data=graph_o32, statistics=stats, data_indices=idx, metadata={},
                                 truncation_data=data).to(DEV).eval()
    assert iface.model._truncation is not None
    batch = golden_interface["batch"].to(DEV)
    iface.predict_step(batch)  # (the first call checks the normalised batch for NaNs on the generic route)
    assert iface._normalizer_affines(batch) is not None
    got = iface.predict_step(batch)
    with torch.no_grad():
        xn = iface.pre_processors(batch, in_place=False)[:, 0:iface.multi_step, None, ...]
        want = iface.post_processors(iface.model(xn), in_place=False)
    assert got.shape == want.shape and rel_err(got, want) < 1e-5


# ------------------------------------------------------------------------------------------------------------ training
def _rollout_case(graph, seed=8):
    g = graph["data"].num_nodes
    gen = torch.Generator().manual_seed(seed)
    return {"data": _plan_matrices(g, 400, 9), "gen": gen, "g": g}


def _train_step(graph, case, x_cpu, targets_cpu, weights, fused_input_grad):
    """One 2-step rollout training step on a fresh model with an input that requires a gradient.  ``fused_input_grad``: the whole
    rollout runs inside ``training.rollout_input_grad()``, so step 1 -- whose input is the leaf -- keeps the kernel route as well
    (outside that context a leaf that requires a gradient takes the generic torch route by design)."""
    import contextlib

    from anemoi_models_amd import WeightedMSELoss, training
    from anemoi_models_amd.training import RolloutModel

    model, idx = _flat_model(graph, case["data"])
    model.train()
    loss_fn = WeightedMSELoss(*weights).to(DEV)
    x = x_cpu.to(DEV).requires_grad_()
    with training.rollout_input_grad() if fused_input_grad else contextlib.nullcontext():
        y = RolloutModel(model, idx, 2)(x)
    loss = loss_fn(y, targets_cpu.to(DEV))
    loss.backward()
    return loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}, x.grad.clone()


def test_rollout_training_fused_vs_composed_route_and_capture(graph_o32, monkeypatch):
    """A 2-step RolloutModel with truncation: the fused route (anemoi_csr_project in both steps, forward and backward: the
    gradient crosses the truncated skip of step 2 and reaches the leaf through that of step 1) against the composed torch route
    (index_select + torch.sparse.mm + add), the calls of each run counted; the fused route twice gives equal bits; one
    GraphedTrainStep capture replays to the bits of the eager step it captured."""
    from anemoi_models_amd import WeightedMSELoss, ops
    from anemoi_models_amd.runtime import GraphedTrainStep
    from anemoi_models_amd.training import RolloutModel

    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "fp32")
    case = _rollout_case(graph_o32)
    g, gen = case["g"], case["gen"]
    x = torch.randn(1, 2, 1, g, 12, generator=gen)
    targets = torch.randn(2, 1, 1, g, 11, generator=gen)
    weights = (torch.rand(g, generator=gen) + 0.1, torch.rand(11, generator=gen) + 0.5)

    calls = {"sparse_mm": 0, "csr_project": 0}
    real_mm, real_project = torch.sparse.mm, ops.csr_project

    def counted(name, fn):
        def wrapper(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapper

    monkeypatch.setattr(torch.sparse, "mm", counted("sparse_mm", real_mm))
    monkeypatch.setattr(ops, "csr_project", counted("csr_project", real_project))
    fused = _train_step(graph_o32, case, x, targets, weights, True)
    # 2 steps x 2 matrices forward, the same backward (both steps' inputs carry a gradient); nothing on the torch route
    assert calls == {"sparse_mm": 0, "csr_project": 8}
    again = _train_step(graph_o32, case, x, targets, weights, True)
    assert calls == {"sparse_mm": 0, "csr_project": 16}
    assert torch.equal(fused[0], again[0]) and torch.equal(fused[2], again[2])
    assert all(torch.equal(fused[1][k], again[1][k]) for k in fused[1])
    monkeypatch.setenv("ANEMOI_AMD_TRAIN_FUSED_FINISH", "0")
    composed = _train_step(graph_o32, case, x, targets, weights, False)
    monkeypatch.delenv("ANEMOI_AMD_TRAIN_FUSED_FINISH")
    assert calls == {"sparse_mm": 4, "csr_project": 16}  # two steps, two matrices: the torch route, nothing on the kernel
    monkeypatch.setattr(torch.sparse, "mm", real_mm)
    monkeypatch.setattr(ops, "csr_project", real_project)
    tol_f, tol_g = FWD_TOL[torch.float32], GRAD_TOL[torch.float32]
    l_err = abs(float(fused[0]) - float(composed[0])) / abs(float(composed[0]))
    print(f"truncated rollout, fused vs composed: loss rel err {l_err:.2e}")
    assert l_err <= tol_f
    assert set(fused[1]) == set(composed[1]) and len(fused[1]) > 20
    worst = 0.0
    for k, want in composed[1].items():
        worst = max(worst, rel_err(fused[1][k], want))
    dx_err = rel_err(fused[2], composed[2])
    print(f"truncated rollout, fused vs composed: worst parameter-gradient rel err {worst:.2e}, input gradient {dx_err:.2e}")
    assert worst <= tol_g and dx_err <= tol_g
    assert bool(fused[2][:, -1].any())

    # capture: a replay equals, bit for bit, the eager step of the same model and inputs (no input gradient: both steps on
    # the kernel, as in the step that is captured)
    model, idx = _flat_model(graph_o32, case["data"])
    model.train()
    roll = RolloutModel(model, idx, 2)
    loss_fn = WeightedMSELoss(*weights).to(DEV)
    xd, td = x.to(DEV), targets.to(DEV)

    def eager_step():  # (in a function: no autograd graph of it may be alive at the capture)
        for p in model.parameters():
            p.grad = None
        loss = loss_fn(roll(xd), td)
        loss.backward()
        return loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}

    want_loss, want = eager_step()
    graphed = GraphedTrainStep(roll, loss_fn, torch.zeros_like(xd), torch.zeros_like(td))
    loss = graphed(xd, td)
    assert torch.equal(loss, want_loss)
    for k, gr in want.items():
        assert torch.equal(model.get_parameter(k).grad, gr), k
