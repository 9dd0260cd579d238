"""GPU tests of the GNN edge ops and the activation kernels against the f64 references of tests/_gnn_ops_ref.py.

Kernels: ``gather_add_act_kernel`` / ``segment_sum_kernel`` (csrc/gnn.hip; 16-byte and scalar forms, f32 and bf16),
``act_forward_kernel`` / ``act_backward_vec_kernel`` / ``act_backward_kernel`` (csrc/backward.hip), and the autograd glue
``autograd.gather_add_act`` / ``autograd.segment_sum``.  Every comparison is per element against a bound derived from the data
(``_gnn_ops_ref``: derivations, the constant A and the CPU measurement behind it); tests/test_gnn_ops_ref_cpu.py shows that the
bounds are reachable and that one dropped edge, one wrong row, a zeroed tail, a shifted slice, ReLU'(0) = 1 or a NaN fails them.
Each case asserts from C, the row pitches and the pointers which kernel form it reaches.

Measured on an MI355X, worst over all cases of this file (A = 7.48e-7; 2^-8 = 3.9e-3 is what one bf16 store may cost):
  worst |got - want| / max(1, |x|, |want|)      Identity   GELU      SiLU      ReLU
    act_forward          f32                    0          1.87e-7   1.28e-7   0
    act_forward          bf16                   0          3.71e-3   3.21e-3   0
    act_backward (x |dy|) f32                   0          4.47e-7   2.07e-7   0
    act_backward (x |dy|) bf16                  0          3.85e-3   3.88e-3   0
    gather_add_act       f32 (two additions in) 2.38e-7    3.24e-7   2.73e-7   0
    gather_add_act       bf16                   3.89e-3    3.86e-3   3.79e-3   3.89e-3
  largest fraction of the bound that was used: f32 0.34 (act_backward GELU), 0.29 (gather_add_act, d t), 0.15 (segment_sum),
  0.06 (d p_dst / d p_src); bf16 0.996 (every store: round-to-nearest reaches 2^-8 just above a power of two), 0.53 (d p_dst /
  d p_src).  No output was NaN or infinite anywhere on the value set.
"""

import functools

import pytest
import torch

import _gnn_ops_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
WAVE_GRID_UNITS = 256 * 32 * 4  # csrc/gnn.hip::wave_grid: at most 8192 blocks of 4 waves, one (row, slice) unit per wave
BW_GRID_ITEMS = 256 * 16 * 256  # csrc/backward.hip::bw_grid: at most 4096 blocks of 256 threads, one item per thread


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from anemoi_models_amd import _lib

    _lib.load()  # the native library must be present: no fallback
    assert torch.cuda.is_available()


def _name(dtype):
    return "f32" if dtype == torch.float32 else "bf16"


def _vec(dtype):
    return 4 if dtype == torch.float32 else 8


def _vector_path(c, *tensors):
    """csrc/gnn.hip::vec_ok and the same test in anemoi_act_backward / anemoi_act_forward, restated on the tensors."""
    from anemoi_models_amd import ops

    v = _vec(tensors[0].dtype)
    return c % v == 0 and all(ops._ld(t) % v == 0 and t.data_ptr() % 16 == 0 for t in tensors)


def _slices(c, dtype, vector):
    return -(-c // (64 * (_vec(dtype) if vector else 1)))


# (dtype, C, vector path?, slices, partial last slice?)
WIDTHS = [
    pytest.param(torch.float32, 4, True, 1, True, id="f32-4-one_lane"),
    pytest.param(torch.float32, 256, True, 1, False, id="f32-256-one_full_slice"),
    pytest.param(torch.float32, 260, True, 2, True, id="f32-260-second_slice_one_lane"),
    pytest.param(torch.float32, 191, False, 3, True, id="f32-191-scalar_three_slices"),
    pytest.param(torch.float32, 1, False, 1, True, id="f32-1-scalar_one_column"),
    pytest.param(torch.bfloat16, 8, True, 1, True, id="bf16-8-one_lane"),
    pytest.param(torch.bfloat16, 512, True, 1, False, id="bf16-512-one_full_slice"),
    pytest.param(torch.bfloat16, 520, True, 2, True, id="bf16-520-second_slice_one_lane"),
    pytest.param(torch.bfloat16, 191, False, 3, True, id="bf16-191-scalar_three_slices"),
    pytest.param(torch.bfloat16, 6, False, 1, True, id="bf16-6-scalar_narrow"),
]
BACKWARD_WIDTHS = [w for w in WIDTHS if w.values[1] not in (256, 512)]


def _assert_path(c, dtype, vector, slices, partial, *tensors):
    assert _vector_path(c, *tensors) == vector
    assert _slices(c, dtype, vector) == slices
    assert (c % (64 * (_vec(dtype) if vector else 1)) != 0) == partial


class _Graph:
    def __init__(self, kind, n_edges, n_dst):
        from anemoi_models_amd import runtime

        ei, self.n_src, self.n_dst = R.make_graph(kind, n_edges, n_dst)
        self.plan = runtime.build_edge_plan(ei.to(DEV), self.n_src, self.n_dst)
        self.dst, self.src, self.rowptr = self.plan.dst.cpu(), self.plan.col.cpu(), self.plan.rowptr.cpu()
        self.n_edges = self.plan.num_edges
        assert self.n_src != self.n_dst and self.n_edges == ei.shape[1]
        R.check_graph_shape(kind, self.rowptr, self.src, self.n_src)


@functools.lru_cache(maxsize=None)
def _graph(kind="main", n_edges=1500, n_dst=R.N_DST):
    return _Graph(kind, n_edges, n_dst)


def _operands(g, c, dtype, act):
    t, pd, ps, dout = R.operands(g.n_edges, g.n_src, g.n_dst, c, dtype, act)
    if act == "ReLU" and g.n_edges:
        assert R.plant_zero_pre(t, pd, ps, g.dst, g.src) > 0
    return t, pd, ps, dout


def _report(what, dtype, act, got, want, x, of_bound):
    print(f"[{what} {_name(dtype)} {act}] worst |got - want| / max(1, |x|, |want|) = {R.act_ratio(got, want, x):.3e}, "
          f"{of_bound:.3f} of the bound")


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("dtype,c,vector,slices,partial", WIDTHS)
def test_gather_add_act(dtype, c, vector, slices, partial, act):
    from anemoi_models_amd import ops

    g = _graph()
    t, pd, ps, _ = _operands(g, c, dtype, act)
    td, pdd, psd = t.to(DEV), pd.to(DEV), ps.to(DEV)
    got = ops.gather_add_act(td, pdd, psd, g.plan.dst, g.plan.col, act=act)
    assert got.dtype == dtype and got.shape == (g.n_edges, c)
    _assert_path(c, dtype, vector, slices, partial, td, pdd, psd, got)
    want, bound, pre = R.gather_add_act_ref(t, pd, ps, g.dst, g.src, act)
    if act == "ReLU":
        assert int((pre == 0).sum()) > 0
    _report("gather_add_act", dtype, act, got, want, pre, R.check(got, want, bound, "gather_add_act", pre))


@pytest.mark.parametrize("dtype,c,vector,slices,partial", WIDTHS)
def test_segment_sum_and_cat(dtype, c, vector, slices, partial):
    from anemoi_models_amd import ops

    g = _graph()
    _, pd, _, v = _operands(g, c, dtype, "GELU")
    vd, xd = v.to(DEV), pd.to(DEV)
    got = ops.segment_sum(vd, g.plan.rowptr)
    assert got.dtype == dtype
    _assert_path(c, dtype, vector, slices, partial, vd, got)
    want, bound = R.segment_sum_ref(v, g.rowptr)
    print(f"[segment_sum {_name(dtype)} C={c}] {R.check(got, want, bound, 'segment_sum'):.3f} of the bound")
    assert bool((got[0] == 0).all()) and bool((got[-1] == 0).all())  # destinations without edges
    cat = ops.segment_sum(vd, g.plan.rowptr, cat_with=xd)
    assert cat.shape == (g.n_dst, 2 * c)
    assert _vector_path(c, vd, cat, xd) == vector
    R.check(cat, *R.segment_sum_cat_ref(v, g.rowptr, pd), "segment_sum_cat")
    assert torch.equal(cat[:, :c], xd) and torch.equal(cat[:, c:], got)


def _column_range(x, start, pad):
    """``x`` as the columns ``start : start + C`` of a wider device buffer of row pitch ``C + pad``."""
    buf = torch.full((x.shape[0], x.shape[1] + pad), 7.0, dtype=x.dtype, device=DEV)  # (a wrong offset reads 7s)
    view = buf[:, start:start + x.shape[1]]
    view.copy_(x)
    return buf, view


@pytest.mark.parametrize("layout", ["aligned_range", "range_from_column_1", "halves_of_one_buffer"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_strided_operands(dtype, layout):
    """``t`` / ``v`` as a column range of a wider buffer (16-byte aligned start and pitch: the vector path; from column 1: the
    scalar path, several slices), and ``p_dst`` / ``p_src`` as the two halves of one ``[N, 2C]`` buffer, as the model passes
    them.  Forward, segment sums and the gradients, which must land in the right columns and nowhere else."""
    from anemoi_models_amd import autograd, ops

    g, v, act = _graph(), _vec(dtype), "GELU"
    c = 64 * v + v
    t, pd, ps, dout = _operands(g, c, dtype, act)
    if layout == "halves_of_one_buffer":
        tbuf = tv = t.to(DEV)
        nbuf = torch.full((max(g.n_src, g.n_dst), 2 * c), 7.0, dtype=dtype, device=DEV)
        nbuf[: g.n_dst, :c] = pd.to(DEV)
        nbuf[: g.n_src, c:] = ps.to(DEV)
        nbuf.requires_grad_()
        pdv, psv = nbuf[: g.n_dst, :c], nbuf[: g.n_src, c:]
        vector = True
    else:
        start, vector = (v, True) if layout == "aligned_range" else (1, False)
        tbuf, tv = _column_range(t, start, 2 * v)
        pdv, psv = pd.to(DEV).requires_grad_(), ps.to(DEV).requires_grad_()
    tbuf.requires_grad_()
    if tv is not tbuf:
        tv = tbuf[:, start:start + c]
    got = ops.gather_add_act(tv.detach(), pdv.detach(), psv.detach(), g.plan.dst, g.plan.col, act=act)
    assert _vector_path(c, tv, pdv, psv, got) == vector and (vector or tv.data_ptr() % 16 != 0)
    assert _slices(c, dtype, vector) == (2 if vector else c // 64 + 1)
    want, bound, _ = R.gather_add_act_ref(t, pd, ps, g.dst, g.src, act)
    R.check(got, want, bound, "gather_add_act")
    # segment sums of the same strided rows, x of the concatenated form strided as well
    seg = ops.segment_sum(tv.detach(), g.plan.rowptr)
    assert _vector_path(c, tv, seg) == vector
    R.check(seg, *R.segment_sum_ref(t, g.rowptr), "segment_sum")
    cat = ops.segment_sum(tv.detach(), g.plan.rowptr, cat_with=pdv.detach())
    assert _vector_path(c, tv, cat, pdv) == vector
    assert torch.equal(cat[:, :c], pdv.detach()) and torch.equal(cat[:, c:], seg)
    # gradients
    autograd.gather_add_act(tv, pdv, psv, g.plan, act).backward(dout.to(DEV))
    refs = R.gather_add_act_backward_ref(t, pd, ps, g.dst, g.src, g.rowptr, dout, act)
    if layout == "halves_of_one_buffer":
        grads = (tbuf.grad, nbuf.grad[: g.n_dst, :c], nbuf.grad[: g.n_src, c:])
        assert bool((nbuf.grad[g.n_dst:, :c] == 0).all()) and bool((nbuf.grad[g.n_src:, c:] == 0).all())
    else:
        grads = (tbuf.grad[:, start:start + c], pdv.grad, psv.grad)
        assert bool((tbuf.grad[:, :start] == 0).all()) and bool((tbuf.grad[:, start + c:] == 0).all())
    for name, got, (w, b) in zip(("d t", "d p_dst", "d p_src"), grads, refs):
        R.check(got, w, b, name)


@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("kind", ["one_dst", "empty"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_destination_and_no_edges(dtype, kind, act):
    """n_dst = 1, and E = 0: the forward is empty, segment_sum gives zeros, cat_with gives [x | 0], the backward returns zero
    d p_dst and d p_src -- at a vector width and at a scalar width (whose backward takes the torch fallback)."""
    from anemoi_models_amd import autograd, ops

    g = _graph(kind, 0, 0)
    for c in (_vec(dtype), 3):
        t, pd, ps, dout = _operands(g, c, dtype, act)
        tr, pdr, psr = (x.to(DEV).requires_grad_() for x in (t, pd, ps))
        out = autograd.gather_add_act(tr, pdr, psr, g.plan, act)
        want, bound, _ = R.gather_add_act_ref(t, pd, ps, g.dst, g.src, act)
        assert out.shape == (g.n_edges, c) and out.dtype == dtype
        R.check(out, want, bound, "gather_add_act")
        assert torch.equal(out, ops.gather_add_act(tr.detach(), pdr.detach(), psr.detach(), g.plan.dst, g.plan.col, act=act))
        out.backward(dout.to(DEV))
        refs = R.gather_add_act_backward_ref(t, pd, ps, g.dst, g.src, g.rowptr, dout, act)
        for name, got, (w, b) in zip(("d t", "d p_dst", "d p_src"), (tr.grad, pdr.grad, psr.grad), refs):
            assert got is not None and got.dtype == dtype
            R.check(got, w, b, name)
        seg = ops.segment_sum(dout.to(DEV), g.plan.rowptr)
        R.check(seg, *R.segment_sum_ref(dout, g.rowptr), "segment_sum")
        cat = ops.segment_sum(dout.to(DEV), g.plan.rowptr, cat_with=pd.to(DEV))
        assert torch.equal(cat[:, :c], pd.to(DEV)) and torch.equal(cat[:, c:], seg)
        if kind == "empty":
            assert out.numel() == 0 and tr.grad.numel() == 0
            assert bool((seg == 0).all()) and bool((pdr.grad == 0).all()) and bool((psr.grad == 0).all())


@pytest.mark.parametrize("dtype,n,c,vector,slices,act", [
    pytest.param(torch.float32, 8200, 1028, True, 5, "SiLU", id="f32-vector-E8200-C1028"),
    pytest.param(torch.float32, 11000, 191, False, 3, "GELU", id="f32-scalar-E11000-C191"),
    pytest.param(torch.bfloat16, 11000, 191, False, 3, "SiLU", id="bf16-scalar-E11000-C191"),
])
def test_grid_stride_loop(dtype, n, c, vector, slices, act):
    """More (row, slice) units than ``wave_grid`` launches waves for: E = n_dst = n, so both the edge kernel and the segment
    sum go round their grid-stride loop."""
    from anemoi_models_amd import ops

    g = _graph("main", n, n)
    assert g.n_edges * slices > WAVE_GRID_UNITS and g.n_dst * slices > WAVE_GRID_UNITS
    t, pd, ps, _ = _operands(g, c, dtype, act)
    td, pdd, psd = t.to(DEV), pd.to(DEV), ps.to(DEV)
    got = ops.gather_add_act(td, pdd, psd, g.plan.dst, g.plan.col, act=act)
    assert _vector_path(c, td, pdd, psd, got) == vector and _slices(c, dtype, vector) == slices
    want, bound, pre = R.gather_add_act_ref(t, pd, ps, g.dst, g.src, act)
    _report("gather_add_act grid-stride", dtype, act, got, want, pre, R.check(got, want, bound, "gather_add_act", pre))
    del want, bound, pre
    seg = ops.segment_sum(td, g.plan.rowptr)
    assert _vector_path(c, td, seg) == vector
    R.check(seg, *R.segment_sum_ref(t, g.rowptr), "segment_sum")
    cat = ops.segment_sum(td, g.plan.rowptr, cat_with=pdd)
    assert torch.equal(cat[:, :c], pdd) and torch.equal(cat[:, c:], seg)


# ------------------------------------------------------------------------------------------------ backward
def _count_calls(monkeypatch, name):
    from anemoi_models_amd import ops

    calls, real = [], getattr(ops, name)

    def counted(*a, **k):
        calls.append(name)
        return real(*a, **k)

    monkeypatch.setattr(ops, name, counted)
    return calls


@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("dtype,c,vector,slices,partial", BACKWARD_WIDTHS)
def test_gather_add_act_backward(monkeypatch, dtype, c, vector, slices, partial, act):
    """d t, d p_dst, d p_src of ``autograd.gather_add_act`` for a random ``dout``; widths with C % (16 / element size) != 0 and
    an activation take the torch fallback for act', the others ``ops.act_backward``.  A second backward gives the same bits."""
    from anemoi_models_amd import autograd

    g = _graph()
    t, pd, ps, dout = _operands(g, c, dtype, act)
    refs = R.gather_add_act_backward_ref(t, pd, ps, g.dst, g.src, g.rowptr, dout, act)
    pre = R.gather_add_act_ref(t, pd, ps, g.dst, g.src, act)[2]
    kernel_calls = _count_calls(monkeypatch, "act_backward")
    runs = []
    for _ in range(2):
        tr, pdr, psr = (x.to(DEV).requires_grad_() for x in (t, pd, ps))
        autograd.gather_add_act(tr, pdr, psr, g.plan, act).backward(dout.to(DEV))
        runs.append((tr.grad, pdr.grad, psr.grad))
    assert len(kernel_calls) == (0 if act == "Identity" or c % _vec(dtype) != 0 else 2)
    assert (c % _vec(dtype) == 0) == vector
    for name, got, again, (w, b) in zip(("d t", "d p_dst", "d p_src"), runs[0], runs[1], refs):
        assert got.dtype == dtype
        of_bound = R.check(got, w, b, name, pre if name == "d t" else None)
        assert torch.equal(got, again), f"{name}: two backward passes differ"
        print(f"[backward {name} {_name(dtype)} {act} C={c}] {of_bound:.3f} of the bound")
    assert bool((runs[0][1][0] == 0).all()) and bool((runs[0][1][-1] == 0).all()) and bool((runs[0][2][R.IDLE_SRC] == 0).all())


@pytest.mark.parametrize("side", ["p_dst", "p_src"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_add_act_backward_one_side(dtype, side):
    from anemoi_models_amd import autograd

    g, act = _graph(), "SiLU"
    c = 64 * _vec(dtype) + _vec(dtype)
    t, pd, ps, dout = _operands(g, c, dtype, act)
    refs = R.gather_add_act_backward_ref(t, pd, ps, g.dst, g.src, g.rowptr, dout, act)
    tr, pdr, psr = t.to(DEV), pd.to(DEV).requires_grad_(side == "p_dst"), ps.to(DEV).requires_grad_(side == "p_src")
    autograd.gather_add_act(tr, pdr, psr, g.plan, act).backward(dout.to(DEV))
    assert tr.grad is None
    if side == "p_dst":
        assert psr.grad is None
        R.check(pdr.grad, *refs[1], "d p_dst")
    else:
        assert pdr.grad is None
        R.check(psr.grad, *refs[2], "d p_src")


@pytest.mark.parametrize("dtype", DTYPES)
def test_segment_sum_backward(dtype):
    from anemoi_models_amd import autograd

    g = _graph()
    for c in (_vec(dtype), 191):
        v = _operands(g, c, dtype, "GELU")[3].to(DEV).requires_grad_()
        out = autograd.segment_sum(v, g.plan)
        R.check(out, *R.segment_sum_ref(v.detach().cpu(), g.rowptr), "segment_sum")
        dout = torch.randn(g.n_dst, c, generator=torch.Generator().manual_seed(c)).to(dtype).to(DEV)
        out.backward(dout)
        assert torch.equal(v.grad, dout[g.plan.dst.long()])


# ------------------------------------------------------------------------------------------------ act_forward / act_backward
def _planted(rows, cols, dtype, seed):
    """Unit normal ``[rows, cols]`` inputs with +-VALUE_SET planted; a shape with fewer than 28 elements gets the set in turns.
    Yields ``(x, dy, residual)``; |dy| <= 1 at the planted elements, so that dy act'(3e38) stays inside f32."""
    g = torch.Generator().manual_seed(seed)
    vals, n = R.value_set_tensor(), rows * cols
    for k in range(0, vals.numel(), n):
        chunk = vals[k:k + n]
        x, dy, res = (torch.randn(rows, cols, generator=g, dtype=torch.float64) for _ in range(3))
        pos = torch.randperm(n, generator=g)[: chunk.numel()]
        x.view(-1)[pos] = chunk
        dy.view(-1)[pos] = dy.view(-1)[pos].clamp(-1, 1)
        yield x.to(dtype), dy.to(dtype), res.to(dtype)


def _shapes(dtype):
    v = _vec(dtype)
    return [(1, v), (7, 3 * v), (257, 40 * v + v)]


@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_act_forward(dtype, act):
    """``act(pre)`` and ``act(pre) + residual`` on contiguous operands and on aligned column ranges of wider buffers, with the
    value set planted: every output finite and within the bound."""
    from anemoi_models_amd import ops

    v, worst, of_bound = _vec(dtype), 0.0, 0.0
    for rows, cols in _shapes(dtype):
        assert (rows * cols) % 256 != 0 and cols % v == 0
        for x, _, res in _planted(rows, cols, dtype, rows + cols):
            for strided in (False, True):
                xd, rd = (_column_range(a, v, 2 * v)[1] if strided else a.to(DEV) for a in (x, res))
                assert _vector_path(cols, xd, rd) and (xd.stride(0) > cols) == strided
                for r, rdev in ((None, None), (res, rd)):
                    got = ops.act_forward(xd, act, rdev)
                    assert got.dtype == dtype and got.shape == (rows, cols) and _vector_path(cols, got)  # (a fresh result)
                    want, bound = R.act_forward_ref(x, act, r)
                    of_bound = max(of_bound, R.check(got, want, bound, f"act_forward {rows}x{cols} residual={r is not None}", x))
                    if r is None:
                        worst = max(worst, R.act_ratio(got, want, x))
    print(f"[act_forward {_name(dtype)} {act}] worst |got - want| / max(1, |x|, |want|) = {worst:.3e}, {of_bound:.3f} of the bound")


@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_act_backward(dtype, act):
    """``dy act'(pre)``: contiguous and aligned ranges (``act_backward_vec_kernel``), ranges starting at column 1 and a width
    off the 16-byte grid (``act_backward_kernel``)."""
    from anemoi_models_amd import ops

    v, worst, of_bound = _vec(dtype), 0.0, 0.0
    for rows, cols in _shapes(dtype) + [(7, 3 * v + 1)]:
        for x, dy, _ in _planted(rows, cols, dtype, rows + cols + 1):
            want, bound = R.act_backward_ref(x, dy, act)
            for start in (None, v, 1):
                xd, dyd = (a.to(DEV) if start is None else _column_range(a, start, 2 * v)[1] for a in (x, dy))
                got = ops.act_backward(xd, dyd, act)
                assert got.dtype == dtype and got.shape == (rows, cols)
                # (the library's test covers the result too: a fresh contiguous tensor, aligned and of pitch ``cols``)
                assert _vector_path(cols, xd, dyd, got) == (start != 1 and cols % v == 0)
                of_bound = max(of_bound, R.check(got, want, bound, f"act_backward {rows}x{cols} start={start}", x))
                worst = max(worst, R.act_ratio(got, want, x))
    print(f"[act_backward {_name(dtype)} {act}] worst |dy| -weighted error / max(1, |x|, |want|) = {worst:.3e}, "
          f"{of_bound:.3f} of the bound")


@pytest.mark.parametrize("dtype,rows,cols,vector,act", [
    pytest.param(torch.float32, 1100, 4096, True, "GELU", id="f32-vector-1100x4096"),
    pytest.param(torch.bfloat16, 1100, 8192, True, "SiLU", id="bf16-vector-1100x8192"),
    pytest.param(torch.float32, 1031, 1021, False, "SiLU", id="f32-scalar-1031x1021"),
    pytest.param(torch.bfloat16, 1031, 1021, False, "GELU", id="bf16-scalar-1031x1021"),
])
def test_act_grid_stride_loop(dtype, rows, cols, vector, act):
    """More items than ``bw_grid`` launches threads for: the vector kernels (forward with residual, backward) and the scalar
    backward kernel go round their grid-stride loop."""
    from anemoi_models_amd import ops

    assert rows * cols // (_vec(dtype) if vector else 1) > BW_GRID_ITEMS
    x, dy, res = next(_planted(rows, cols, dtype, rows))
    xd, dyd, rd = x.to(DEV), dy.to(DEV), res.to(DEV)
    got = ops.act_backward(xd, dyd, act)
    assert _vector_path(cols, xd, dyd, rd, got) == vector  # (the result is a fresh contiguous tensor of pitch ``cols``)
    R.check(got, *R.act_backward_ref(x, dy, act), "act_backward", x)
    if vector:
        R.check(ops.act_forward(xd, act, rd), *R.act_forward_ref(x, act, res), "act_forward", x)
    else:
        with pytest.raises(NotImplementedError, match="anemoi_act_forward"):
            ops.act_forward(xd, act, rd)


@pytest.mark.parametrize("dtype", DTYPES)
def test_act_forward_rejects_rows_off_the_16_byte_grid(dtype):
    """``act_forward`` has no scalar kernel: a width, a pitch or a start off the 16-byte grid raises the library's
    ANEMOI_ERR_UNSUPPORTED (NotImplementedError through ``_lib.check``) instead of returning anything."""
    from anemoi_models_amd import ops

    v = _vec(dtype)
    ok = torch.randn(7, 3 * v, generator=torch.Generator().manual_seed(1)).to(dtype)
    odd_width = torch.randn(7, 3 * v + 1, generator=torch.Generator().manual_seed(2)).to(dtype).to(DEV)
    odd_pitch = odd_width[:, : 3 * v]
    odd_start = _column_range(ok, 1, 2 * v)[1]
    assert odd_pitch.stride(0) % v != 0 and odd_start.data_ptr() % 16 != 0 and odd_start.stride(0) % v == 0
    for pre, res in ((odd_width, None), (odd_pitch, None), (odd_start, None), (ok.to(DEV), odd_pitch), (ok.to(DEV), odd_start)):
        assert not _vector_path(pre.shape[1], pre, *(() if res is None else (res,)))
        with pytest.raises(NotImplementedError, match="anemoi_act_forward"):
            ops.act_forward(pre, "GELU", res)
    torch.cuda.synchronize()
    R.check(ops.act_forward(ok.to(DEV), "GELU"), *R.act_forward_ref(ok, "GELU"), "act_forward")
