"""GPU tests of the LayerNorm family and the row / column kernels of the dense backward against the f64 references of
tests/_row_kernels_ref.py.

Kernels: ``layer_norm_kernel`` <ITEMS 1..8> / ``layer_norm_generic_kernel`` (plain, + residual, + statistics),
``row_stats_kernel`` <ITEMS 1..8> / ``row_stats_generic_kernel``, ``convert_pad_kernel``, ``row_scale_kernel``, ``row_dot_kernel``,
``add_kernel`` (csrc/elementwise.hip); ``layer_norm_backward_kernel`` <NC 8, 16, 32, 0>, ``col_sum_stage_kernel``,
``col_sum_final_kernel`` (csrc/backward.hip).  Every comparison is per element against a bound derived from the data
(``_row_kernels_ref``: the derivations); tests/test_row_kernels_ref_cpu.py shows that the bounds are reachable by a correct f32
implementation in two summation orders and that the variance over C - 1, a misplaced or tenfold eps, a dropped vector, shifted
gamma / beta, a missing xhat term, a missing row in d gamma / d beta, an ignored dres, a dropped chunk, a shift on the wrong
operand and a NaN fail them.  Each case restates the launcher's dispatch predicate on its tensors and asserts the kernel form
it reaches.  Inputs with a pitch carry NaN in their padding and in a margin around the matrix; every output is a view into a
buffer pre-filled with a bit pattern, and every byte outside the result is asserted unchanged.

Measured on an MI355X: the largest fraction of its bound that any element used, over all cases of this file (the module prints
the table again at its end; 1.000 means that an element sat on its bound, which the one-rounding bounds -- u |want| for an f32
addition, 2^-8 |want| for a bf16 store -- allow and round-to-nearest reaches just above a power of two):
                                        f32 operands   bf16 operands
    layer_norm                          0.855          0.995
    layer_norm + residual               0.943          0.983
    row_stats / layer_norm_with_stats   0.275          0.337   (f32 statistics; 0.243 on the exact rows = rsqrtf alone, about half an
                                                                ulp of the two it is allowed)
    layer_norm_backward  dx             0.522          0.995
    layer_norm_backward  d gamma (f32)  0.530          0.490
    layer_norm_backward  d beta  (f32)  0.698          0.006
    col_sum (f32)                       0.153          0.000   (the bf16 data are multiples of 2^-7: exact sums in f32)
    row_dot (f32)                       0.260          0.085
    row_scale                           0.972          0.996
    add                                 1.000          0.996
    convert_pad                         f32 -> bf16 0.996, the other three pairs exact
No output was NaN or infinite on any data set (constant rows, the zero row, the row at 1e18 included), every guard band was
clean, the statistics of ``layer_norm_with_stats`` equalled ``row_stats`` bit for bit and its output ``layer_norm`` at all 20
widths per dtype, and d gamma / d beta / the column sums were bit-identical across two calls.  The kernels needed no exemption.
"""

import pytest
import torch

import _row_kernels_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = R.F32, R.BF16
FLAT_GRID_ITEMS = 256 * 16 * 256  # csrc/elementwise.hip::flat_grid: at most 4096 blocks of 256 threads, one item per thread
MARGIN = 64  # elements before and after every guarded matrix (a multiple of 16 bytes in every dtype)
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from anemoi_models_amd import _lib

    _lib.load()  # the native library must be present: no fallback
    assert torch.cuda.is_available()
    yield
    for key in sorted(_WORST):
        print(f"[worst fraction of the bound] {key}: {_WORST[key]:.3f}")


def _note(kernel, dtype, fraction):
    key = f"{kernel} {R.name(dtype)}"
    _WORST[key] = max(_WORST.get(key, 0.0), fraction)
    return fraction


def _ids(params):
    return [f"{R.name(p[0])}-" + "-".join(str(v) for v in p[1:]) for p in params]


# ------------------------------------------------------------------------------------------------ guard bands
_INT = {F32: (torch.int32, 0x5A5A5A5A), BF16: (torch.int16, 0x5A5A)}


class Guarded:
    """A ``[rows, cols]`` view of pitch ``cols + pad`` that starts ``off`` elements past a 16-byte boundary, inside a larger
    buffer.  ``fill="pattern"`` (outputs): the buffer holds a fixed bit pattern and ``assert_clean`` demands that every byte
    outside the view still does.  ``fill="nan"`` (inputs): padding and margins are NaN, a read outside the operand poisons."""

    def __init__(self, rows, cols, dtype, pad=0, off=0, fill="pattern", data=None):
        itype, self.pattern = _INT[dtype]
        ld = cols + pad
        n = 2 * MARGIN + off + rows * ld
        if fill == "pattern":
            self.raw = torch.full((n,), self.pattern, dtype=itype, device=DEV)
            flat = self.raw.view(dtype)
        else:
            flat = torch.full((n,), float("nan"), dtype=dtype, device=DEV)
            self.raw = flat.view(itype)
        self.view = torch.as_strided(flat, (rows, cols), (ld, 1), MARGIN + off)
        idx = (MARGIN + off) + torch.arange(rows, device=DEV)[:, None] * ld + torch.arange(cols, device=DEV)[None, :]
        self.outside = torch.ones(n, dtype=torch.bool, device=DEV)
        self.outside[idx.reshape(-1)] = False
        if data is not None:
            self.view.copy_(data)
        assert self.view.data_ptr() % 16 == (off * flat.element_size()) % 16

    def assert_clean(self, what):
        touched = self.outside & (self.raw != self.pattern)
        assert not bool(touched.any()), f"{what}: {int(touched.sum())} elements outside the result were written, first at " \
                                        f"buffer offset {int(torch.nonzero(touched)[0])} (the result starts at {MARGIN})"


def _in(x, pad=0, off=0):
    """``x`` on the device; with a pitch or an offset inside NaNs."""
    if pad == 0 and off == 0:
        return x.to(DEV)
    return Guarded(x.shape[0], x.shape[1], x.dtype, pad, off, fill="nan", data=x.to(DEV)).view


def _out(rows, cols, dtype, pad=0, off=0):
    return Guarded(rows, cols, dtype, pad, off)


def _vector_out(n):
    return Guarded(1, n, F32)


# ------------------------------------------------------------------------------------------------ dispatch, restated
def _ld(t):
    from anemoi_models_amd import ops

    return ops._ld(t)


def _aligned(c, *tensors):
    """The launchers' test for the 16-byte forms: the width and every pitch a multiple of the vector, every base on 16 bytes."""
    v = R.vec(tensors[0].dtype)
    return c % v == 0 and all(t.data_ptr() % 16 == 0 and (t.dim() == 1 or _ld(t) % v == 0) for t in tensors)


def _ln_form(c, dtype, *tensors):
    """layer_norm_launch / row_stats_launch: ITEMS of the register form, 0 for the generic kernel."""
    items = -(-c // (64 * R.vec(dtype)))
    return items if _aligned(c, *tensors) and items <= 8 else 0


def _bw_form(c, *tensors):
    """layer_norm_backward_launch: (NC, dynamic LDS bytes)."""
    lds = 8 * c * 4
    if not _aligned(c, *tensors) or c > 2048:
        return 0, lds
    return (8 if c <= 512 else 16 if c <= 1024 else 32), lds


def _final_loops(n_part):
    """col_sum_final_kernel: (trips of the four-chain loop, trips of the remainder loop) of row group 0, the busiest one."""
    r, four = 0, 0
    while r + 48 < n_part:
        r, four = r + 64, four + 1
    return four, len(range(r, n_part, 16))


def test_guard_bands_notice_a_stray_write():
    g = _out(3, 5, BF16, pad=2)
    g.assert_clean("untouched")
    g.view.fill_(1.0)
    g.assert_clean("the result alone")
    for stray in (MARGIN - 1, MARGIN + 5, MARGIN + 3 * 7 - 2, g.raw.numel() - 1):  # before, pitch padding, after the last row, the end
        h = _out(3, 5, BF16, pad=2)
        h.raw[stray] = 0
        with pytest.raises(AssertionError, match="outside the result"):
            h.assert_clean("stray")
    x = _in(torch.ones(3, 5), pad=2, off=1)
    around = torch.as_strided(x, (3, 7), (7, 1), x.storage_offset())  # (the last row's padding lies in the margin)
    assert bool(torch.isnan(around[:, 5:]).all()) and bool((around[:, :5] == 1).all()) and x.data_ptr() % 16 == 4


# ------------------------------------------------------------------------------------------------ direct library calls
def _call(fn_name, *args):
    from anemoi_models_amd import _lib, ops

    _lib.check(getattr(_lib.load(), fn_name)(*args, ops._stream()), fn_name)


def _row_stats_into(x, stats, eps=R.EPS):
    from anemoi_models_amd import ops

    _call("anemoi_row_stats", ops.dtype_code(x.dtype), x.data_ptr(), _ld(x), stats.data_ptr(), x.shape[0], x.shape[1], eps)


def _ln_stats_into(x, w, b, out, stats, eps=R.EPS):
    from anemoi_models_amd import ops

    _call("anemoi_layer_norm_stats", ops.dtype_code(x.dtype), x.data_ptr(), _ld(x), w.data_ptr(), b.data_ptr(), out.data_ptr(),
          _ld(out), stats.data_ptr(), x.shape[0], x.shape[1], eps)


def _row_dot_into(a, b, shift, out):
    from anemoi_models_amd import ops

    _call("anemoi_row_dot", ops.dtype_code(a.dtype), a.data_ptr(), _ld(a), b.data_ptr(), _ld(b), ops._ptr(shift), out.data_ptr(),
          a.shape[0], a.shape[1])


def _convert_pad_into(src, dst):
    """``dst``: the full ``[rows, ld_out]`` result."""
    from anemoi_models_amd import ops

    _call("anemoi_convert_pad", ops.dtype_code(src.dtype), src.data_ptr(), _ld(src), ops.dtype_code(dst.dtype), dst.data_ptr(),
          dst.shape[1], src.shape[0], src.shape[1])


def _ln_backward_into(x, stats, w, dy, dres, dx, dgamma, dbeta):
    from anemoi_models_amd import _lib, ops

    rows, c = x.shape
    n_ws = _lib.load().anemoi_layer_norm_backward_workspace_floats(rows, c)
    ws = torch.empty(n_ws, dtype=F32, device=DEV)
    _call("anemoi_layer_norm_backward", ops.dtype_code(x.dtype), x.data_ptr(), _ld(x), stats.data_ptr(), w.data_ptr(), dy.data_ptr(),
          _ld(dy), ops._ptr(dres), 0 if dres is None else _ld(dres), dx.data_ptr(), _ld(dx), rows, c, dgamma.data_ptr(),
          dbeta.data_ptr(), ws.data_ptr(), n_ws)


# ------------------------------------------------------------------------------------------------ LayerNorm, statistics
def _layer_norm_case(dtype, rows, c, form, pads=(0, 0, 0), off=0, seed=0):
    """All four entry points on one matrix: ``layer_norm``, ``+ residual``, ``layer_norm_with_stats``, ``row_stats``.
    ``pads``: extra pitch of (x, out, residual); ``off``: elements between x's first element and a 16-byte boundary."""
    from anemoi_models_amd import ops

    x, (w, b), res = R.make_rows(rows, c, dtype, seed), R.affine(c), R.plain(rows, c, dtype, 11)
    xd, rd, wd, bd = _in(x, pads[0], off), _in(res, pads[2]), w.to(DEV), b.to(DEV)
    outs = [_out(rows, c, dtype, pads[1]) for _ in range(3)]
    stats = [_out(rows, 2, F32) for _ in range(2)]
    # (layer_norm and layer_norm_with_stats, layer_norm + residual, row_stats): what each launcher tests, on these tensors
    forms = (_ln_form(c, dtype, xd, outs[0].view, wd, bd), _ln_form(c, dtype, xd, outs[1].view, wd, bd, rd), _ln_form(c, dtype, xd))
    assert forms == (form if isinstance(form, tuple) else (form, form, form)), forms
    ops.layer_norm(xd, wd, bd, R.EPS, out=outs[0].view)
    ops.layer_norm(xd, wd, bd, R.EPS, out=outs[1].view, residual=rd)
    _ln_stats_into(xd, wd, bd, outs[2].view, stats[0].view)
    _row_stats_into(xd, stats[1].view)
    for k, g in enumerate(outs + stats):
        g.assert_clean(f"layer_norm family, output {k}, {rows}x{c}")
    what = f"{R.name(dtype)} {rows}x{c} pads={pads} off={off}"
    f_out = _note("layer_norm", dtype, R.check(outs[0].view, *R.layer_norm_ref(x, w, b), "layer_norm " + what))
    f_res = _note("layer_norm + residual", dtype,
                  R.check(outs[1].view, *R.layer_norm_ref(x, w, b, residual=res), "layer_norm + residual " + what))
    f_st = _note("row_stats (from %s)" % R.name(dtype), F32, R.check(stats[1].view, *R.row_stats_ref(x), "row_stats " + what))
    # one pass, two results: the same bits as the two separate kernels
    if forms[0] == forms[2]:  # (an odd pitch on the output alone: the generic kernel's sums against the register form's)
        assert torch.equal(stats[0].view, stats[1].view), "layer_norm_with_stats: statistics differ from row_stats"
    else:
        R.check(stats[0].view, *R.row_stats_ref(x), "layer_norm_with_stats, statistics " + what)
    assert torch.equal(outs[2].view, outs[0].view), "layer_norm_with_stats: output differs from layer_norm"
    for r in R.rows_of("constant", rows) + R.rows_of("zeros", rows):  # d = 0 exactly: the output is beta
        assert torch.equal(outs[0].view[r].float().cpu(), b.to(dtype).float())
    return f_out, f_res, f_st


def _ln_width_params():
    return [(dtype, c, items, partial) for dtype in R.DTYPES for c, items, partial in R.layer_norm_widths(dtype)]


@pytest.mark.parametrize("dtype,c,items,partial", _ln_width_params(), ids=_ids(_ln_width_params()))
def test_layer_norm_widths(dtype, c, items, partial):
    """Every ITEMS form with a full last pass and with one lane in it, the generic kernel past eight passes and for widths off
    the vector; every data set (ROW_KINDS) at every width; nine rows = two full blocks and one wave of a third."""
    v = R.vec(dtype)
    assert (c % (64 * v) != 0) == partial and (items == 0) == (c % v != 0 or c > 64 * v * 8)
    fr = _layer_norm_case(dtype, R.ALL_KINDS_ROWS, c, items)
    print(f"[layer_norm {R.name(dtype)} C={c} ITEMS={items}] of the bound: out {fr[0]:.3f}, + residual {fr[1]:.3f}, stats {fr[2]:.3f}")


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.name)
def test_layer_norm_rows_and_layouts(dtype):
    """Rows 1, 4, 5 (one wave, a full block, a second block with one wave); padded pitches on x, out and the residual in turn
    (still the register form); an odd pitch and a base 4 bytes off a 16-byte boundary (the generic kernel)."""
    v = R.vec(dtype)
    c = 64 * v + v
    worst = 0.0
    for rows in (1, 4, 5):
        for pads, off, form in (((0, 0, 0), 0, 2), ((v, 0, 0), 0, 2), ((0, 2 * v, 0), 0, 2), ((0, 0, 3 * v), 0, 2),
                                ((v, 2 * v, 3 * v), 0, 2),
                                ((1, 0, 0), 0, 0), ((0, 1, 0), 0, (0, 0, 2)), ((0, 0, 1), 0, (2, 0, 2)), ((v, 0, 0), 4 // (16 // v), 0)):
            if rows == 1 and form != 2 and off == 0:
                continue  # (one row has no pitch)
            worst = max(worst, *_layer_norm_case(dtype, rows, c, form, pads, off, seed=rows))
    print(f"[layer_norm layouts {R.name(dtype)}] {worst:.3f} of the bound")


# ------------------------------------------------------------------------------------------------ LayerNorm backward
def _backward_case(dtype, rows, c, nc, pads=(0, 0, 0, 0), off=0, twice=False):
    """With and without ``dres``; ``pads``: extra pitch of (x, dy, dx, dres).  The statistics are ``ops.row_stats`` of the x."""
    from anemoi_models_amd import ops

    x, (w, _), dy, dres = R.make_rows(rows, c, dtype), R.affine(c), R.make_dy(rows, c, dtype), R.plain(rows, c, dtype, 5)
    xd, dyd, drd, wd = _in(x, pads[0], off), _in(dy, pads[1]), _in(dres, pads[3]), w.to(DEV)
    stats = ops.row_stats(xd, R.EPS)
    _note("row_stats (from %s)" % R.name(dtype), F32, R.check(stats, *R.row_stats_ref(x), f"row_stats {rows}x{c}"))
    stats_cpu, worst = stats.cpu(), [0.0, 0.0, 0.0]
    for dr_cpu, dr in ((None, None), (dres, drd)):
        runs = []
        for _ in range(2 if twice else 1):
            dx, dg, db = _out(rows, c, dtype, pads[2]), _vector_out(c), _vector_out(c)
            tensors = (xd, dyd, dx.view, wd) + (() if dr is None else (dr,))
            form, lds = _bw_form(c, *tensors)
            assert form == nc and lds == 32 * c and lds <= 160 * 1024
            _ln_backward_into(xd, stats, wd, dyd, dr, dx.view, dg.view, db.view)
            for g, nm in ((dx, "dx"), (dg, "d gamma"), (db, "d beta")):
                g.assert_clean(f"layer_norm_backward {nm} {rows}x{c}")
            runs.append((dx.view, dg.view[0], db.view[0]))
        refs = R.layer_norm_backward_ref(x, stats_cpu, w, dy, dr_cpu)
        what = f"{R.name(dtype)} {rows}x{c} NC={nc} dres={dr is not None} pads={pads} off={off}"
        for k, (nm, key_dtype) in enumerate((("dx", dtype), ("d gamma", F32), ("d beta", F32))):
            kernel = f"layer_norm_backward {nm}" + ("" if k == 0 else f" (from {R.name(dtype)})")
            worst[k] = max(worst[k], _note(kernel, key_dtype, R.check(runs[0][k], *refs[k], f"{nm} {what}")))
            if twice:
                assert torch.equal(runs[0][k], runs[1][k]), f"{nm} {what}: two calls differ"
    return worst


def _bw_width_params():
    return [(dtype, c, nc) for dtype in R.DTYPES for c, nc in R.backward_widths(dtype)]


@pytest.mark.parametrize("dtype,c,nc", _bw_width_params(), ids=_ids(_bw_width_params()))
def test_layer_norm_backward_widths(dtype, c, nc):
    """NC = 8 (one lane, full), 16 (one lane in the second group, full), 32 (the same), the wide LDS route just past 64 KiB and
    at the limit of 160 KiB, and the unaligned LDS route at C = 191; every data set at every width; two calls, the same bits."""
    lds, v = 32 * c, R.vec(dtype)
    assert c <= R.BACKWARD_MAX_C and (c != 2048 or lds == 64 * 1024) and (c != 2048 + v or 64 * 1024 < lds < 65 * 1024)
    assert c != R.BACKWARD_MAX_C or lds == 160 * 1024  # (the whole LDS of a compute unit: one workgroup may take it)
    fr = _backward_case(dtype, R.ALL_KINDS_ROWS, c, nc, twice=True)
    print(f"[layer_norm_backward {R.name(dtype)} C={c} NC={nc}] of the bound: dx {fr[0]:.3f}, d gamma {fr[1]:.3f}, d beta {fr[2]:.3f}")


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.name)
def test_layer_norm_backward_rows_and_layouts(dtype):
    """Rows 1, 3 (idle waves), 32 (one full workgroup), 33 (a second one with one row), 65 (three); padded pitches on x, dy, dx
    and dres in turn; an odd pitch on each and a base 4 bytes off (the LDS route)."""
    v = R.vec(dtype)
    worst = [0.0, 0.0, 0.0]
    cases = [(rows, c, nc, (0, 0, 0, 0), 0) for rows in R.BACKWARD_ROWS for c, nc in ((8, 8), (191, 0))]
    cases += [(33, 520, 16, pads, 0) for pads in ((v, 0, 0, 0), (0, 2 * v, 0, 0), (0, 0, 3 * v, 0), (0, 0, 0, v))]
    cases += [(33, 520, 0, pads, 0) for pads in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0))] + [(5, 520, 0, (v, 0, 0, 0), 4 // (16 // v))]
    for rows, c, nc, pads, off in cases:
        fr = _backward_case(dtype, rows, c, nc, pads, off)
        worst = [max(a, b) for a, b in zip(worst, fr)]
    # an odd pitch on dres alone: dx without dres still takes the register form
    x, (w, _), dy, dres = R.make_rows(5, 520, dtype), R.affine(520), R.make_dy(5, 520, dtype), R.plain(5, 520, dtype, 5)
    xd, dyd, drd, wd = x.to(DEV), dy.to(DEV), _in(dres, 1), w.to(DEV)
    assert _bw_form(520, xd, dyd, wd)[0] == 16 and _bw_form(520, xd, dyd, wd, drd)[0] == 0
    from anemoi_models_amd import ops

    stats = ops.row_stats(xd, R.EPS)
    got = ops.layer_norm_backward(xd, stats, wd, dyd, drd)
    for g, ref in zip(got, R.layer_norm_backward_ref(x, stats.cpu(), w, dy, dres)):
        R.check(g, *ref, "layer_norm_backward, odd pitch on dres")
    print(f"[layer_norm_backward rows and layouts {R.name(dtype)}] of the bound: dx {worst[0]:.3f}, d gamma {worst[1]:.3f}, "
          f"d beta {worst[2]:.3f}")


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.name)
def test_layer_norm_backward_partial_counts(dtype):
    """col_sum_final_kernel behind the backward: n_part = workgroups on both sides of 16, 48 and 64 (the remainder loop alone,
    the four-chain loop entered, a second trip of it), and one case with rows_per_wg = 33 and a short last workgroup."""
    worst = [0.0, 0.0, 0.0]
    loops = {n: _final_loops(n) for n in R.BACKWARD_NPART}
    assert loops[1] == (0, 1) and loops[16] == (0, 1) and loops[17] == (0, 2) and loops[48] == (0, 3) and loops[49] == (1, 0)
    assert loops[63] == (1, 0) and loops[64] == (1, 0) and loops[65] == (1, 1) and loops[113] == (2, 0)
    for n in R.BACKWARD_NPART:
        rows = 32 * n
        assert R.backward_rows_per_wg(rows) == 32 and -(-rows // 32) == n
        worst = [max(a, b) for a, b in zip(worst, _backward_case(dtype, rows, 8, 8, twice=True))]
    rows = R.BACKWARD_MANY_ROWS
    per = R.backward_rows_per_wg(rows)
    assert per == 33 and rows % per != 0 and _final_loops(-(-rows // per)) == (15, 3)
    worst = [max(a, b) for a, b in zip(worst, _backward_case(dtype, rows, 8, 8, twice=True))]
    print(f"[layer_norm_backward partial counts {R.name(dtype)}] of the bound: dx {worst[0]:.3f}, d gamma {worst[1]:.3f}, "
          f"d beta {worst[2]:.3f}")


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.name)
def test_layer_norm_backward_refuses_rows_wider_than_the_lds(dtype):
    """C = 5120 + V needs more than 160 KiB of LDS: the library's ANEMOI_ERR_UNSUPPORTED before any launch."""
    from anemoi_models_amd import ops

    c = R.BACKWARD_MAX_C + R.vec(dtype)
    x = torch.ones(2, c, dtype=dtype, device=DEV)
    stats = ops.row_stats(x)
    with pytest.raises(NotImplementedError, match="too wide for the LDS"):
        ops.layer_norm_backward(x, stats, torch.ones(c, device=DEV), x)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ col_sum
@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.name)
def test_col_sum(dtype):
    """One block without a workspace (rows <= 16), two chunks (17, 19: a short last one), 512 chunks of 16 and chunks of 17
    with a short last one; 1, 255, 256, 257 columns (one thread, a block's last thread idle, full, a second column block); a
    padded pitch; two calls, the same bits."""
    from anemoi_models_amd import _lib, ops

    worst = 0.0
    for rows in R.COL_SUM_ROWS:
        chunk, blocks = R.col_sum_chunks(rows)
        assert (blocks <= 1) == (rows <= 16) and (rows != 8192 or (chunk, blocks) == (16, 512))
        assert rows != 8193 or (chunk == 17 and rows % chunk != 0 and _final_loops(blocks) == (7, 3))
        assert rows != 8192 or _final_loops(blocks) == (8, 0)
        assert rows not in (17, 19) or (blocks == 2 and rows % chunk in (1, 3) and _final_loops(blocks) == (0, 1))
        for cols in R.COL_SUM_COLS:
            assert _lib.load().anemoi_col_sum_workspace_floats(rows, cols) == (0 if blocks <= 1 else blocks * cols)
            x = R.col_data(rows, cols, dtype)
            want, bound = R.col_sum_ref(x)
            for pad in (0, 3):
                if pad and rows == 1:
                    continue
                xd, outs = _in(x, pad), [_vector_out(cols), _vector_out(cols)]
                for o in outs:
                    assert ops.col_sum(xd, out=o.view[0]).data_ptr() == o.view.data_ptr()
                    o.assert_clean(f"col_sum {rows}x{cols}")
                worst = max(worst, _note("col_sum (from %s)" % R.name(dtype), F32,
                                         R.check(outs[0].view[0], want, bound, f"col_sum {R.name(dtype)} {rows}x{cols} pad={pad}")))
                assert torch.equal(outs[0].view, outs[1].view)
    print(f"[col_sum {R.name(dtype)}] {worst:.3f} of the bound")


# ------------------------------------------------------------------------------------------------ row_dot, row_scale, add, convert_pad
def _row_form(cols, *tensors):
    return _aligned(cols, *tensors)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.name)
def test_row_dot_and_row_scale(dtype):
    """cols = V (one lane), 64 V 4 (one full trip of the four-deep unroll), 64 V 4 + V (a second trip with one lane), 191 (the
    scalar form); an odd pitch on each operand in turn (scalar); with and without ``shift``; ``row_scale`` in place."""
    from anemoi_models_amd import ops

    v, rows, alpha = R.vec(dtype), R.ALL_KINDS_ROWS, -0.375
    worst = [0.0, 0.0]
    for cols, vector in R.row_widths(dtype):
        a, b = R.plain(rows, cols, dtype, 31), R.make_rows(rows, cols, dtype, 1)
        shift = torch.randn(cols, generator=torch.Generator().manual_seed(cols)) + 0.5
        s = torch.randn(rows, generator=torch.Generator().manual_seed(3))
        sd, shd = s.to(DEV), shift.to(DEV)
        for pa, pb in ((0, 0), (v, 2 * v), (1, 0), (0, 1)):
            ad, bd = _in(a, pa), _in(b, pb)
            vec_form = vector and (pa, pb) in ((0, 0), (v, 2 * v))
            assert _row_form(cols, ad, bd) == vec_form
            for sh_cpu, sh in ((None, None), (shift, shd)):
                out = _vector_out(rows)
                _row_dot_into(ad, bd, sh, out.view)
                out.assert_clean("row_dot")
                what = f"{R.name(dtype)} C={cols} pitches +{pa} +{pb}"
                used = R.check(out.view[0], *R.row_dot_ref(a, b, sh_cpu), "row_dot " + what)
                worst[0] = max(worst[0], _note("row_dot (from %s)" % R.name(dtype), F32, used))
                assert torch.equal(ops.row_dot(ad, bd, sh), out.view[0])
            # row_scale: x with pitch pa, the result with pitch pb
            o = _out(rows, cols, dtype, pb)
            assert _row_form(cols, ad, o.view) == vec_form
            ops.row_scale(ad, sd, alpha, out=o.view)
            o.assert_clean("row_scale")
            want, bound = R.row_scale_ref(a, s, alpha)
            worst[1] = max(worst[1], _note("row_scale", dtype, R.check(o.view, want, bound, "row_scale " + what)))
        inplace = _out(rows, cols, dtype, v)
        inplace.view.copy_(a.to(DEV))
        ops.row_scale(inplace.view, sd, alpha, out=inplace.view)
        inplace.assert_clean("row_scale in place")
        R.check(inplace.view, want, bound, "row_scale in place")
    print(f"[row_dot, row_scale {R.name(dtype)}] of the bound: row_dot {worst[0]:.3f}, row_scale {worst[1]:.3f}")


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.name)
def test_add_and_convert_pad(dtype):
    from anemoi_models_amd import ops

    rows, worst = R.ALL_KINDS_ROWS, [0.0, 0.0]
    for cols, _ in R.row_widths(dtype):
        a, b = R.plain(rows, cols, dtype, 31), R.make_rows(rows, cols, dtype, 1)
        for pads in ((0, 0, 0), (1, 0, 0), (0, 2, 0), (0, 0, 3)):
            o = _out(rows, cols, dtype, pads[2])
            ops.add(_in(a, pads[0]), _in(b, pads[1]), out=o.view)
            o.assert_clean("add")
            worst[0] = max(worst[0], _note("add", dtype, R.check(o.view, *R.add_ref(a, b), f"add {R.name(dtype)} C={cols} pitches {pads}")))
        for dst in R.DTYPES:  # all four dtype pairs; the padding columns belong to the result and must be exactly zero
            ld = cols + 5
            o = _out(rows, ld, dst)
            _convert_pad_into(_in(a, 1), o.view)
            o.assert_clean("convert_pad")
            want, bound = R.convert_pad_ref(a, dst, ld)
            used = R.check(o.view, want, bound, f"convert_pad {R.name(dtype)} -> {R.name(dst)} C={cols}")
            worst[1] = max(worst[1], _note(f"convert_pad {R.name(dtype)} ->", dst, used))
            assert bool((o.view[:, cols:] == 0).all())
            assert torch.equal(ops.convert_pad(a.to(DEV), dst, ld), o.view)
    print(f"[add, convert_pad from {R.name(dtype)}] of the bound: add {worst[0]:.3f}, convert_pad {worst[1]:.3f}")


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.name)
def test_flat_grid_second_trip(dtype):
    """More items than ``flat_grid`` launches threads for, rows of one column: ``row_scale``, ``add`` and ``convert_pad`` go
    round their grid-stride loop a second time."""
    from anemoi_models_amd import ops

    rows = FLAT_GRID_ITEMS + 3
    a, b = R.plain(rows, 1, dtype, 41), R.plain(rows, 1, dtype, 42)
    s = torch.randn(rows, generator=torch.Generator().manual_seed(4))
    ad, bd = a.to(DEV), b.to(DEV)
    assert rows * 1 > FLAT_GRID_ITEMS and not _row_form(1, ad)  # one item per row in row_scale's scalar form and in add
    o = _out(rows, 1, dtype)
    ops.row_scale(ad, s.to(DEV), 0.5, out=o.view)
    o.assert_clean("row_scale")
    f_scale = _note("row_scale", dtype, R.check(o.view, *R.row_scale_ref(a, s, 0.5), "row_scale, second trip"))
    o = _out(rows, 1, dtype)
    ops.add(ad, bd, out=o.view)
    o.assert_clean("add")
    f_add = _note("add", dtype, R.check(o.view, *R.add_ref(a, b), "add, second trip"))
    half = rows // 2 + 2
    assert half * 2 > FLAT_GRID_ITEMS  # convert_pad: one item per element of the padded result
    other = BF16 if dtype == F32 else F32
    o = _out(half, 2, other)
    _convert_pad_into(ad[:half], o.view)
    o.assert_clean("convert_pad")
    f_pad = R.check(o.view, *R.convert_pad_ref(a[:half], other, 2), "convert_pad, second trip")
    print(f"[second trip {R.name(dtype)}] of the bound: row_scale {f_scale:.3f}, add {f_add:.3f}, convert_pad {f_pad:.3f}")


# ------------------------------------------------------------------------------------------------ wrappers, empty inputs, refusals
@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.name)
def test_wrappers_return_what_the_library_calls_return(dtype):
    """``ops.row_stats``, ``ops.layer_norm_with_stats``, ``ops.layer_norm_backward`` allocate their results: the same bits as
    the guarded direct calls above."""
    from anemoi_models_amd import ops

    rows, c = R.ALL_KINDS_ROWS, 64 * R.vec(dtype) + R.vec(dtype)
    x, (w, b), dy, dres = R.make_rows(rows, c, dtype), R.affine(c), R.make_dy(rows, c, dtype), R.plain(rows, c, dtype, 5)
    xd, wd, bd, dyd, drd = x.to(DEV), w.to(DEV), b.to(DEV), dy.to(DEV), dres.to(DEV)
    stats, out = _out(rows, 2, F32), _out(rows, c, dtype)
    _ln_stats_into(xd, wd, bd, out.view, stats.view)
    got_out, got_stats = ops.layer_norm_with_stats(xd, wd, bd, R.EPS)
    assert torch.equal(got_out, out.view) and torch.equal(got_stats, stats.view) and torch.equal(ops.row_stats(xd, R.EPS), stats.view)
    assert torch.equal(ops.layer_norm(xd, wd, bd, R.EPS), out.view)
    dx, dg, db = _out(rows, c, dtype), _vector_out(c), _vector_out(c)
    _ln_backward_into(xd, got_stats, wd, dyd, drd, dx.view, dg.view, db.view)
    got = ops.layer_norm_backward(xd, got_stats, wd, dyd, drd)
    assert torch.equal(got[0], dx.view) and torch.equal(got[1], dg.view[0]) and torch.equal(got[2], db.view[0])


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.name)
def test_zero_rows(dtype):
    """No rows: empty results, zero d gamma / d beta / column sums, no launch (an empty tensor has no storage to point at)."""
    from anemoi_models_amd import ops

    c = 24
    x = torch.empty(0, c, dtype=dtype, device=DEV)
    w, b = (t.to(DEV) for t in R.affine(c))
    assert ops.layer_norm(x, w, b).shape == (0, c) and ops.layer_norm(x, w, b, residual=x).shape == (0, c)
    out, stats = ops.layer_norm_with_stats(x, w, b)
    assert out.shape == (0, c) and out.dtype == dtype and stats.shape == (0, 2) and stats.dtype == F32
    assert ops.row_stats(x).shape == (0, 2)
    for dres in (None, x):
        dx, dg, db = ops.layer_norm_backward(x, stats, w, x, dres)
        assert dx.shape == (0, c) and dx.dtype == dtype and dg.dtype == db.dtype == F32
        assert torch.equal(dg, torch.zeros(c, device=DEV)) and torch.equal(db, torch.zeros(c, device=DEV))
    assert torch.equal(ops.col_sum(x), torch.zeros(c, device=DEV))
    into = torch.full((c,), 7.0, device=DEV)
    assert ops.col_sum(x, out=into) is into and bool((into == 0).all())
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.name)
def test_add_refuses_a_pitch_below_the_width(dtype):
    """``anemoi_add`` checks lda, ldb, ldy >= cols like every other entry point of the family: ANEMOI_ERR_INVALID, no launch."""
    from anemoi_models_amd import _lib, ops

    rows, cols = 4, 24
    a, b, y = (torch.ones(rows, cols, dtype=dtype, device=DEV) for _ in range(3))
    lib, code = _lib.load(), ops.dtype_code(dtype)
    for lds in ((cols - 1, cols, cols), (cols, cols - 1, cols), (cols, cols, cols - 1)):
        st = lib.anemoi_add(code, a.data_ptr(), lds[0], b.data_ptr(), lds[1], y.data_ptr(), lds[2], rows, cols, ops._stream())
        assert st == _lib.ANEMOI_ERR_INVALID
        with pytest.raises(ValueError, match="anemoi_add"):
            _lib.check(st, "anemoi_add")
    torch.cuda.synchronize()
    assert bool((y == 1).all())
    R.check(ops.add(a, b), *R.add_ref(a.cpu(), b.cpu()), "add")
