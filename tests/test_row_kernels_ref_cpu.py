"""CPU checks of tests/_row_kernels_ref.py, the yardstick of tests/test_gpu_row_kernels.py.

Three statements, each at every data set and shape of the GPU file:
  1. the references are right: the backward reference agrees with torch autograd in f64;
  2. the bounds are reachable: a correct f32 implementation (torch f32 arithmetic, bf16 with the explicit roundings) in two
     different summation orders -- torch's blocked pairwise ``sum`` and a strictly sequential sum from the last term to the
     first -- passes the checker; the fraction of the bound each uses is printed;
  3. the bounds have teeth: each subtly wrong result below fails the checker, in f32 and, where the output is f32, from bf16
     inputs too.

Mutants that a bf16 OUTPUT can hide behind its 2^-8 store term and that the f32 outputs must catch (test_layer_norm_mutants):
the variance over C - 1 (1 / (2 C) < 2^-8 from C > 128), a vector dropped from the mean or from the sum of squares of a wide
row, and ``eps`` outside the square root or ten times too large (nothing of rstd reaches the output of a constant row or of
C = 1, in either dtype).  The statistics of ``row_stats`` / ``layer_norm_with_stats`` are asserted to catch all five at every
width and from both input dtypes.  The backward's d gamma / d beta mutants (a missing row) touch only f32 outputs.

One listed mutant is provably invisible to any accuracy bound: the residual added before the first bf16 rounding (one rounding
instead of two) is closer to the exact result than the contract; test_residual_before_rounding_is_inside_the_bound states it.
"""

import pytest
import torch

import _row_kernels_ref as R

F32, BF16 = R.F32, R.BF16
ORDERS = ("pairwise", "sequential")


def _sum(t: torch.Tensor, dim: int, order: str) -> torch.Tensor:
    if order == "pairwise" or t.shape[dim] == 0:
        return t.sum(dim=dim)
    return torch.cumsum(t.flip(dim), dim=dim).select(dim, -1)  # strictly sequential, last term first


def _rt(t: torch.Tensor, dtype) -> torch.Tensor:
    """Round an f32 tensor to ``dtype`` and back."""
    return t.to(dtype).float()


# ------------------------------------------------------------------------------------------------ f32 implementations
def ln_f32(x, weight, bias, order, residual=None, mutant=None, eps=R.EPS):
    """(out in x's dtype, stats [R, 2] f32): the kernels' formulas in torch f32."""
    dtype, v = x.dtype, R.vec(x.dtype)
    xf = x.float()
    c = xf.shape[1]
    e = torch.tensor(eps, dtype=F32) * (10.0 if mutant == "eps_x10" else 1.0)
    keep = c - min(v, c)  # the columns before the last vector
    mean = _sum(xf[:, :keep] if mutant == "drop_vector_mean" else xf, 1, order) / c
    d = xf - mean[:, None]
    sq = d * d
    q = _sum(sq[:, :keep] if mutant == "drop_vector_sq" else sq, 1, order)
    var = q / (c - 1 if mutant == "c_minus_1" else c)
    rstd = 1.0 / (var.sqrt() + e) if mutant == "eps_outside" else torch.rsqrt(var + e)
    stats = torch.stack([rstd, -mean * rstd], dim=1)
    w, b = (weight.roll(v), bias.roll(v)) if mutant == "affine_shift" else (weight, bias)
    o = d * rstd[:, None] * w + b
    if residual is not None:
        o = (o + residual.float()) if mutant == "residual_first" else (_rt(o, dtype) + residual.float())
    if mutant == "nan":
        o[-1, -1] = float("nan")
        stats[-1, 0] = float("nan")
    return o.to(dtype), stats


def ln_backward_f32(x, stats, weight, dy, order, dres=None, mutant=None):
    xf, df, c = x.float(), dy.float(), x.shape[1]
    s, t = stats[:, :1].float(), stats[:, 1:].float()
    xh = xf * s + t
    g = df * weight
    inv_c = torch.tensor(1.0 / c, dtype=F32)
    sg = _sum(g, 1, order)[:, None] * inv_c
    sgx = _sum(g * xh, 1, order)[:, None] * inv_c
    dx = s * (g - sg - (0.0 if mutant == "no_xhat_term" else xh * sgx))
    if dres is not None and mutant != "dres_ignored":
        dx = dx + dres.float()
    tg, tb = df * xh, df.clone()
    # a workgroup loses the last row of its range: of the first, the middle and the last workgroup the one whose last row
    # carries most (the last row of a range may be a zero or a constant row, which adds nothing to d gamma)
    drop = R.boundary_rows(x.shape[0])
    if mutant == "dgamma_row":
        tg[max(drop, key=lambda r: float(tg[r].abs().sum()))] = 0.0
    if mutant == "dbeta_row":
        tb[max(drop, key=lambda r: float(tb[r].abs().sum()))] = 0.0
    if mutant == "nan":
        dx[0, 0] = float("nan")
    return dx.to(x.dtype), _sum(tg, 0, order), _sum(tb, 0, order)


def col_sum_f32(x, order, mutant=None):
    xf = x.float().clone()
    if mutant == "chunk":  # the partial of one chunk of rows is left out
        chunk, blocks = R.col_sum_chunks(x.shape[0])
        b = blocks // 2
        xf[b * chunk:(b + 1) * chunk] = 0.0
    return _sum(xf, 0, order)


def row_dot_f32(a, b, shift, order, mutant=None):
    af, bf = a.float(), b.float()
    if shift is not None:
        if mutant == "shift_on_a":
            af = af - shift[None, : a.shape[1]]
        else:
            bf = bf - shift[None, : a.shape[1]]
    return _sum(af * bf, 1, order)


def _frac(worst, key, value):
    worst[key] = max(worst.get(key, 0.0), value)


def _report(title, worst):
    print(f"[{title}] fraction of the bound used: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


# ------------------------------------------------------------------------------------------------ 1. references
@pytest.mark.parametrize("with_dres", [False, True])
def test_backward_reference_vs_torch_autograd_f64(with_dres):
    for c, rows in ((1, 9), (8, 33), (191, 9), (520, 9)):
        x = R.make_rows(rows, c, F32).double()
        w, b = (t.double() for t in R.affine(c))
        dy, dres = R.make_dy(rows, c, F32).double(), R.plain(rows, c, F32, 3).double()
        xr, wr, br = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
        # the two-pass definition through autograd (F.layer_norm's one-pass moments lose the huge and the large-mean rows
        # even in f64; it is compared on the ordinary rows below)
        d = xr - xr.mean(dim=1, keepdim=True)
        y = d * torch.rsqrt((d * d).mean(dim=1, keepdim=True) + R.eps32(R.EPS)) * wr + br
        (y * dy).sum().backward()
        if with_dres:
            xr.grad += dres
        rows_ok = R.rows_of("ordinary", rows)
        y_torch = torch.nn.functional.layer_norm(x[rows_ok], (c,), w, b, R.eps32(R.EPS))
        assert float((y_torch - y.detach()[rows_ok]).abs().max()) <= 1e-12 * float(1.0 + y_torch.abs().max())
        stats = R.exact_stats(x)
        (dx, _), (dg, _), (db, _) = R.layer_norm_backward_ref(x, stats, w, dy, dres if with_dres else None)
        # forward reference against torch, too
        want, _ = R.layer_norm_ref(x, w, b)
        scale = 1.0 + y.detach().abs()
        assert float(((want - y.detach()).abs() / scale).max()) <= 1e-9
        tol = 1e-9 * (1.0 + xr.grad.abs() + dx.abs())
        assert bool(((dx - xr.grad).abs() <= tol).all()), float((dx - xr.grad).abs().max())
        assert bool(((dg - wr.grad).abs() <= 1e-9 * (1.0 + dg.abs())).all())
        assert bool(((db - br.grad).abs() <= 1e-12 * (1.0 + db.abs())).all())


def test_small_kernel_references():
    a, b = R.plain(5, 7, F32, 1), R.plain(5, 7, F32, 2)
    shift, s = torch.randn(7), torch.randn(5)
    assert torch.allclose(R.row_dot_ref(a, b, shift)[0], (a.double() * (b.double() - shift.double())).sum(1))
    assert torch.equal(R.col_sum_ref(a)[0], a.double().sum(0))
    assert torch.equal(R.row_scale_ref(a, s, 0.5)[0], 0.5 * s.double()[:, None] * a.double())
    assert torch.equal(R.add_ref(a, b)[0], a.double() + b.double())
    want, bound = R.convert_pad_ref(a, BF16, 10)
    assert want.shape == (5, 10) and bool((want[:, 7:] == 0).all()) and bool((bound[:, 7:] == 0).all())
    assert float(R.convert_pad_ref(a.to(BF16), F32, 10)[1].max()) == 0.0


def test_exact_rows_are_recognised():
    """The constant, zero and "exact" rows have exact sums (bound: only the division, + eps and rsqrtf); the others do not."""
    for dtype in R.DTYPES:
        for c in (8, 191, 2048, 4104):
            x = R.make_rows(9, c, dtype)
            a = R.row_analysis(x)
            _, bound = R.row_stats_ref(x)
            for kind in ("constant", "zeros", "exact"):
                (r,) = R.rows_of(kind, 9)
                assert float(a.dm[r]) == 0.0 and float(bound[r, 0] / a.r[r]) < 4 * R.EPS32, (kind, c)
            for kind in ("ordinary", "mean_1e3", "huge") if dtype == F32 and c > 1 else ():
                # (in bf16 a row around 1e3 holds a few multiples of 4: exact as well, and recognised)
                assert all(float(a.dm[r]) > 0.0 for r in R.rows_of(kind, 9)), (kind, c)


def test_checker_names_row_and_column():
    want = torch.zeros(3, 4, dtype=torch.float64)
    got = want.clone()
    got[2, 1] = 1.0
    with pytest.raises(AssertionError, match="row 2, column 1"):
        R.check(got, want, torch.full_like(want, 0.5), "x")
    got[2, 1] = float("nan")
    with pytest.raises(AssertionError, match="non-finite.*row 2, column 1"):
        R.check(got, want, torch.full_like(want, 0.5), "x")
    assert R.check(want + 0.25, want, torch.full_like(want, 0.5), "x") == 0.5
    assert R.check(want, want, torch.zeros_like(want), "x") == 0.0


# ------------------------------------------------------------------------------------------------ 2. + 3. LayerNorm
def _ln_case(dtype, c, rows=R.ALL_KINDS_ROWS):
    x = R.make_rows(rows, c, dtype, 0 if rows == R.ALL_KINDS_ROWS else rows)  # (the GPU file's seeds)
    w, b = R.affine(c)
    return x, w, b, R.plain(rows, c, dtype, 11)


def _ln_widths(dtype):
    return [w[0] for w in R.layer_norm_widths(dtype)]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.name)
def test_layer_norm_f32_implementation_is_inside_the_bounds(dtype, order):
    worst = {}
    for c in _ln_widths(dtype):
        for rows in ((1, 4, 5, 9) if c == 65 * R.vec(dtype) else (9,)):  # (rows 1, 4, 5: the layouts of the GPU file)
            x, w, b, res = _ln_case(dtype, c, rows)
            out, stats = ln_f32(x, w, b, order)
            _frac(worst, "out", R.check(out, *R.layer_norm_ref(x, w, b), f"layer_norm C={c}"))
            _frac(worst, "stats", R.check(stats, *R.row_stats_ref(x), f"stats C={c}"))
            out_r, _ = ln_f32(x, w, b, order, residual=res)
            _frac(worst, "out+res", R.check(out_r, *R.layer_norm_ref(x, w, b, residual=res), f"layer_norm + residual C={c}"))
            for r in R.rows_of("constant", rows) + R.rows_of("zeros", rows):
                assert torch.equal(out[r].float(), _rt(b, dtype)), "a constant row gives beta"
    _report(f"layer_norm {R.name(dtype)} {order}", worst)


# mutant -> the widths at which it exists (affine_shift: a shift by one vector needs more than one vector)
LN_MUTANTS = ("c_minus_1", "eps_outside", "eps_x10", "drop_vector_mean", "drop_vector_sq", "affine_shift", "nan")
STATS_MUTANTS = ("c_minus_1", "eps_outside", "eps_x10", "drop_vector_mean", "drop_vector_sq", "nan")


def _fails(got, want, bound) -> bool:
    try:
        R.check(got, want, bound, "mutant")
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("mutant", LN_MUTANTS)
@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.name)
def test_layer_norm_mutants(dtype, mutant):
    """Every mutant fails at every width: through the f32 statistics where it touches them (the variance over C - 1, ``eps``
    outside the root or ten times too large, a vector dropped from the mean or the squares), through the output otherwise (a
    shifted gamma / beta).  In f32 the output catches the statistics mutants too, except at C = 1, where the output is beta
    whatever rstd is.  In bf16 the 2^-8 store term can hide each of the five in the OUTPUT (a relative change of 1 / (2 C)
    shows only where it moves a value across a rounding boundary): the widths at which it does are printed, nothing is asserted
    of them, and the statistics are asserted to catch the mutant at every width."""
    hidden = []
    for c in _ln_widths(dtype):
        if mutant in ("c_minus_1", "drop_vector_sq") and c == 1:
            continue  # (C = 1: a division by zero is not subtle, and d = 0 leaves no square to drop)
        if mutant == "affine_shift" and c <= R.vec(dtype):
            continue  # (one vector: nothing to shift)
        x, w, b, res = _ln_case(dtype, c)
        for order in ORDERS:
            out, stats = ln_f32(x, w, b, order, mutant=mutant)
            out_fails = _fails(out, *R.layer_norm_ref(x, w, b))
            if mutant in STATS_MUTANTS:
                assert _fails(stats, *R.row_stats_ref(x)), f"{mutant} C={c} {order}: the statistics let it through"
                if c == 1 and mutant in ("eps_outside", "eps_x10"):
                    assert not out_fails  # (d = 0: the output is beta whatever rstd is -- only the statistics can tell)
                elif dtype == F32:
                    assert out_fails, f"{mutant} C={c} {order}: the f32 output lets it through"
                elif not out_fails:
                    hidden.append(c)
            else:
                assert out_fails, f"{mutant} C={c} {order}: the output lets it through"
            out_r, _ = ln_f32(x, w, b, order, residual=res, mutant=mutant)
            if (dtype == F32 and c > 1) or mutant not in STATS_MUTANTS:
                assert _fails(out_r, *R.layer_norm_ref(x, w, b, residual=res)), f"{mutant} C={c} {order}: + residual"
    if dtype == BF16 and mutant in STATS_MUTANTS:
        print(f"[{mutant}] widths whose bf16 output hides it (the statistics catch it): {sorted(set(hidden))}")


def test_residual_before_rounding_is_inside_the_bound():
    """``bf16(o + r)`` instead of ``bf16(bf16(o) + r)``: one rounding fewer, closer to the exact result -- inside every bound
    that admits the contract (_row_kernels_ref: LayerNorm + residual).  Stated, not hidden; in f32 the two are the same."""
    differ = 0
    for c in _ln_widths(BF16):
        x, w, b, res = _ln_case(BF16, c)
        good, _ = ln_f32(x, w, b, "pairwise", residual=res)
        early, _ = ln_f32(x, w, b, "pairwise", residual=res, mutant="residual_first")
        want, bound = R.layer_norm_ref(x, w, b, residual=res)
        R.check(early, want, bound, "residual before the rounding")
        differ += int((good != early).sum())
        err_good = (good.double() - want).abs().sum()
        err_early = (early.double() - want).abs().sum()
        assert float(err_early) <= float(err_good)  # (summed over the matrix: one rounding errs less than two)
    assert differ > 0
    x, w, b, res = _ln_case(F32, 191)
    assert torch.equal(ln_f32(x, w, b, "pairwise", residual=res)[0], ln_f32(x, w, b, "pairwise", residual=res, mutant="residual_first")[0])


# ------------------------------------------------------------------------------------------------ 2. + 3. backward
def _bw_shapes(dtype):
    shapes = [(R.ALL_KINDS_ROWS, c) for c, _ in R.backward_widths(dtype)]
    shapes += [(rows, c) for rows in R.BACKWARD_ROWS for c in (8, 191)] + [(33, 520), (5, 520)]
    shapes += [(32 * n, 8) for n in R.BACKWARD_NPART] + [(R.BACKWARD_MANY_ROWS, 8)]
    return shapes


def _bw_case(dtype, rows, c, order="pairwise"):
    x = R.make_rows(rows, c, dtype)
    w, b = R.affine(c)
    stats = ln_f32(x, w, b, order)[1]  # f32 statistics, as the kernel is handed them
    return x, stats, w, R.make_dy(rows, c, dtype), R.plain(rows, c, dtype, 5)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.name)
def test_backward_f32_implementation_is_inside_the_bounds(dtype, order):
    worst = {}
    for rows, c in _bw_shapes(dtype):
        x, stats, w, dy, dres = _bw_case(dtype, rows, c, order)
        for dr in (None, dres):
            dx, dg, db = ln_backward_f32(x, stats, w, dy, order, dres=dr)
            (wx, bx), (wg, bg), (wb, bb) = R.layer_norm_backward_ref(x, stats, w, dy, dr)
            what = f"{rows}x{c} dres={dr is not None}"
            _frac(worst, "dx", R.check(dx, wx, bx, "dx " + what))
            _frac(worst, "dgamma", R.check(dg, wg, bg, "d gamma " + what))
            _frac(worst, "dbeta", R.check(db, wb, bb, "d beta " + what))
            assert bool(torch.isfinite(dx[R.rows_of("constant", rows)]).all())
    _report(f"layer_norm_backward {R.name(dtype)} {order}", worst)


@pytest.mark.parametrize("mutant,output", [("no_xhat_term", 0), ("dres_ignored", 0), ("dgamma_row", 1), ("dbeta_row", 2), ("nan", 0)])
@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.name)
def test_backward_mutants(dtype, mutant, output):
    for rows, c in _bw_shapes(dtype):
        if mutant == "no_xhat_term" and c == 1:
            continue
        x, stats, w, dy, dres = _bw_case(dtype, rows, c)
        for order in ORDERS:
            got = ln_backward_f32(x, stats, w, dy, order, dres=dres, mutant=mutant)
            refs = R.layer_norm_backward_ref(x, stats, w, dy, dres)
            assert _fails(got[output], *refs[output]), f"{mutant} {rows}x{c} {order}: not rejected"
            for k in range(3):
                if k != output:
                    R.check(got[k], *refs[k], f"{mutant}: untouched output {k}")


# ------------------------------------------------------------------------------------------------ 2. + 3. small kernels
def _pad_shapes():
    return [(rows, cols) for rows in R.COL_SUM_ROWS for cols in R.COL_SUM_COLS]


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.name)
def test_col_sum(dtype):
    worst = {}
    for rows, cols in _pad_shapes():
        x = R.col_data(rows, cols, dtype)
        want, bound = R.col_sum_ref(x)
        for order in ORDERS:
            _frac(worst, order, R.check(col_sum_f32(x, order), want, bound, f"col_sum {rows}x{cols}"))
            if R.col_sum_chunks(rows)[1] > 1:
                assert _fails(col_sum_f32(x, order, "chunk"), want, bound), f"a chunk left out, {rows}x{cols} {order}"
        nan = col_sum_f32(x, "pairwise")
        nan[-1] = float("nan")
        assert _fails(nan, want, bound)
    _report(f"col_sum {R.name(dtype)}", worst)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.name)
def test_row_dot_row_scale_add_convert_pad(dtype):
    worst = {}
    for cols, _ in R.row_widths(dtype):
        rows = 9
        a, b = R.plain(rows, cols, dtype, 31), R.make_rows(rows, cols, dtype, 1)
        shift = torch.randn(cols, generator=torch.Generator().manual_seed(cols)) + 0.5
        for sh in (None, shift):
            want, bound = R.row_dot_ref(a, b, sh)
            for order in ORDERS:
                _frac(worst, "row_dot", R.check(row_dot_f32(a, b, sh, order), want, bound, f"row_dot C={cols}"))
            if sh is not None:
                assert _fails(row_dot_f32(a, b, sh, "pairwise", "shift_on_a"), want, bound), f"shift on a, C={cols}"
            nan = row_dot_f32(a, b, sh, "pairwise")
            nan[0] = float("nan")
            assert _fails(nan, want, bound)
        s = torch.randn(rows, generator=torch.Generator().manual_seed(3))
        scaled = (torch.tensor(-0.375) * s)[:, None] * a.float()
        _frac(worst, "row_scale", R.check(scaled.to(dtype), *R.row_scale_ref(a, s, -0.375), "row_scale"))
        assert _fails(((0.625 * s)[:, None] * a.float()).to(dtype), *R.row_scale_ref(a, s, -0.375))
        _frac(worst, "add", R.check((a.float() + b.float()).to(dtype), *R.add_ref(a, b), "add"))
        assert _fails(a, *R.add_ref(a, b))
        for dst in R.DTYPES:
            want, bound = R.convert_pad_ref(a, dst, cols + 3)
            got = torch.zeros(rows, cols + 3, dtype=dst)
            got[:, :cols] = a.to(dst)
            _frac(worst, "convert_pad", R.check(got, want, bound, "convert_pad"))
            got[0, cols] = 1e-30  # the padding must be exactly zero
            assert _fails(got, want, bound)
    _report(f"row kernels {R.name(dtype)}", worst)
