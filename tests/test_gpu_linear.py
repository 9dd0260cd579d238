"""GPU tests of the fused Linear family (csrc/gemm.hip behind ``ops.linear`` with and without ``ln=`` / ``stats_eps=``,
``ops.linear_dual``, ``ops.linear_actgrad``, ``ops.linear_heads``) against the f64 references of tests/_linear_ref.py: every
element of every output finite and inside a bound derived from the data (``_linear_ref``: the derivations; ``exact`` data:
bound 0, compared by bits).  tests/test_linear_ref_cpu.py shows that emulations of the kernels' arithmetic stay inside these
bounds and that the wrong kernels listed there do not, and that the case table reaches every route.

Every case restates the launcher's dispatch on its own tensors (``_linear_ref.route``) and asserts the route it names; a case
whose route differs FAILS.  The restatement is then held against the launcher's own plan for the same pointers
(``anemoi_linear_route``: kernel, launches, tiles, workgroups, tail, stagger), so the route a case names is the one that ran.
Operands sit in NaN-guarded buffers (rows before and after x, W, the residual and pre, the pad
columns K..ldx and N..ldr, the entries behind the bias, the column sums and the statistics); ``y`` (and, through the library
entry points, ``pre``) sit in buffers holding a bit pattern that must be untouched outside the view, the pad N..ldy included.
Every case runs twice and must repeat bit for bit.

Measured on an MI355X: the largest fraction of its bound that any element used (lowest - highest over the epilogues of the
row; the module prints the full table, per kernel set, epilogue and output, at its end):
    kernels                              output     y               pre     stats           y vs LayerNorm
    128x128                              bf16       0.588 - 0.992   -       0.089           0.537
    128x128                              f32        0.013 - 0.173   -       -               0.256
    128x128 + skinny kernel              bf16       0.822 - 0.995   -       -               0.409
    128x128 + 128x128 tail               bf16       0.841 - 0.996   -       -               0.443
    128x128 batched                      bf16/f32   0.980 / 0.010   -       -               -
    four-wave MH=3                       bf16       0.609 - 0.990   -       0.053 - 0.069   0.521
    four-wave MH=3 + in-launch tail      bf16       0.257 - 0.994   -       0.065 - 0.089   0.320
    four-wave MH=4 (incl. DUAL / GMUL)   bf16       0.584 - 0.995   0.995   0.050 - 0.076   -
    four-wave MH=4 + in-launch tail      bf16       0.986 - 0.995   0.995   -               -
    four-wave MH=4 + ops.py rows         bf16       0.981 - 0.993   0.989   -               -
    four-wave MH=5 / MH=6                bf16       0.679 - 0.996   -       0.054 - 0.077   -
    four-wave MH=8 (incl. DUAL / GMUL)   bf16       0.693 - 0.995   0.994   0.061 - 0.090   -
    four-wave MH=8, launches A + B, tail bf16       0.898           -       0.082           -     (9475 x 4096 x 2048, fold + residual)
    four-wave MH=8 batched               bf16       0.990           -       -               -
    ops.py fallback (128x128 + act)      bf16       0.381 - 0.930   0.994   -               -
    every ``exact`` case (all routes, the two-launch split and mt nt >= 1024 among them): 0.000, bit for bit; the staggered
    launch (8192 x 4096 x 512, GELU) and the mt nt >= 1024 launch on ``spike`` data are part of the MH=8 row.
Reading the table.  bf16 outputs sit at 0.98 - 0.996: the store's 2^-8 is reached, everything else is small beside it (the low
ends are the fold + GELU rows, where the cancellation term of the fold widens the bound, ReLU' rows, and the y = 300 / 302 rows,
whose rounding error is at most half of their bf16 spacing).  f32 outputs use 0.01 - 0.17: gamma(K) S is the worst case of K
roundings in a row, the kernels' errors add like a random walk and the bf16 MFMA rounds less often than once per product; no
published figure allows a smaller K factor, so the bound stays as derived and these routes rely on the ``exact`` cases (bound 0)
for index errors and on the CPU file's mutants (dropped slab / chunk, tanh GELU) for value errors.  The fused statistics use
0.05 - 0.09 of a bound derived from the depth of the kernels' own summation tree (34 + C / 128 additions; _linear_ref).
Device activations through ``ops.act_forward`` (f32) against f64 on 2^20 points of [-24, 24], 2^16 of [-90, 90] and +-VALUE_SET,
relative to |x|: SiLU (x * __frcp_rn(1 + __expf(-x))) 1.414e-7, bound 2 x that; erf-form GELU 2.48e-7 in all, 1.63e-7 beside the
three roundings gamma(3) |GELU x|, bound 2e-7 as documented (test_device_activation_figures asserts both).
Findings: none in the kernels -- every route, the remainder column groups (nt = 17, 18, 23), nt < 8 with a ragged last column
tile, every tile height, the half-tile second launch (statistics and residual offset by m_a), the stand-alone skinny kernel and
the batched walk were bit-exact on ``exact`` data and inside the bounds otherwise; no guard band was written, no NaN guard was
read, every repeat was bit-identical, ``linear_dual``'s pre equalled ``ops.linear`` and ``stats_eps=`` left y unchanged.  One
shape of the proposed table moved: 1024 x 6144 x 128 takes MH = 4 whole tiles (192 tiles, one round), not MH = 3.
``ops.linear(stats_eps=)``, ``ops.linear_dual`` and ``ops.linear_actgrad`` allocate ``stats_out`` / ``pre`` / ``y`` themselves, so the
library entry points (``anemoi_linear_stats`` with its workspace, ``anemoi_linear_dual``, ``anemoi_linear_actgrad``) are also called
directly on pattern-filled buffers: nothing outside the views may be written and the results must equal the wrappers' bit for
bit.  ``ops.linear_heads`` keeps the dtype, so the bf16 -> f32 batched form goes through ``anemoi_linear_batched`` itself.
"""

import types

import pytest
import torch

import _linear_ref as R
from test_linear_ref_cpu import assert_same_route, case_library_route

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = R.F32, R.BF16
_WORST = {}
_INT = {F32: (torch.int32, 0x5A5A5A5A), BF16: (torch.int16, 0x5A5A)}
SMALL = 2e8  # m n k up to which the second fold check (against LayerNorm itself) is made


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from anemoi_models_amd import _lib

    _lib.load()  # the native library must be present: no fallback
    assert torch.cuda.is_available()
    yield
    for key in sorted(_WORST):
        print(f"[worst fraction of the bound] {key}: {_WORST[key]:.3f}")


def _note(key, fraction):
    _WORST[key] = max(_WORST.get(key, 0.0), fraction)
    return fraction


class Guarded:
    """A ``[rows, cols]`` view of pitch ``cols + pad`` inside a larger buffer: guard rows (a multiple of 64 elements, so the view
    keeps the buffer's 16-byte alignment) before and after, ``pad`` guard columns.  ``data`` given (inputs): the guards are NaN,
    a read outside the operand poisons the result.  Otherwise (outputs) the buffer holds a bit pattern and ``assert_clean``
    demands that every element outside the view still does."""

    def __init__(self, rows, cols, dtype, pad=0, data=None):
        itype, self.pattern = _INT[dtype]
        ld = cols + pad
        margin = (2 * ld + 63) // 64 * 64
        n = 2 * margin + rows * ld
        if data is None:
            self.raw = torch.full((n,), self.pattern, dtype=itype, device=DEV)
            flat = self.raw.view(dtype)
        else:
            flat = torch.full((n,), float("nan"), dtype=dtype, device=DEV)
            self.raw = flat.view(itype)
        self.view = torch.as_strided(flat, (rows, cols), (ld, 1), margin)
        self.ld, self.margin, self.rows, self.cols = ld, margin, rows, cols
        if data is not None:
            self.view.copy_(data)
        assert self.view.data_ptr() % 16 == 0

    def assert_clean(self, what):
        inside = torch.zeros(self.raw.numel(), dtype=torch.bool, device=DEV)
        torch.as_strided(inside, (self.rows, self.cols), (self.ld, 1), self.margin).fill_(True)
        touched = ~inside & (self.raw != self.pattern)
        assert not bool(touched.any()), f"{what}: {int(touched.sum())} elements outside the result were written, first at " \
                                        f"buffer offset {int(torch.nonzero(touched)[0])} (view starts at {self.margin}, pitch {self.ld})"


def test_guard_bands_notice_a_stray_write():
    g = Guarded(5, 7, BF16, pad=3)
    g.view.fill_(1.0)
    g.assert_clean("inside only")
    g.raw.view(BF16)[g.margin + 7] = 2.0  # the first pad column of row 0
    with pytest.raises(AssertionError):
        g.assert_clean("pad column")


def _vec(t):
    return None if t is None else Guarded(1, t.numel(), F32, data=t.reshape(1, -1).to(DEV))


def _call(c, o):
    """One run of the case on guarded buffers.  ({name: CPU tensor}, route)."""
    from anemoi_models_amd import _lib, ops

    h = max(c.h, 1)
    gx = Guarded(c.m, c.k * h, c.dtype, c.pads[0], data=o.x.to(DEV))
    gw = Guarded(h * c.n, c.k, c.dtype, 0, data=o.w.reshape(h * c.n, c.k).to(DEV))
    gb, gcs = _vec(o.bias), _vec(o.colsum)
    gst = None if o.stats is None else Guarded(c.m, 2, F32, data=o.stats.to(DEV))
    second = o.res if o.res is not None else o.pre
    gr = None if second is None else Guarded(c.m, c.n, c.dtype, c.pads[2], data=second.to(DEV))
    gy = Guarded(c.m, c.n * h, c.out, c.pads[1])
    bias = None if gb is None else gb.view[0]
    ptrs = (gy.view.data_ptr(), 0 if gb is None else bias.data_ptr(), 0 if gr is None else gr.view.data_ptr(),
            0 if gcs is None else gcs.view.data_ptr())
    rt = R.case_route(c, ptrs)
    assert R.route_str(rt) == c.expect, f"{R.case_id(c)}: the launcher takes {R.route_str(rt)}, the case names {c.expect}"
    # ... and the launcher's own plan on these pointers (anemoi_linear_route) is the restated one, launch for launch
    st, lib_rt, rows = case_library_route(c, ptrs, x=gx.view.data_ptr(), w=gw.view.data_ptr())
    assert_same_route(rt, st, lib_rt, c.m, c.n, c.h, rows, R.case_id(c))
    out = {}
    what = R.case_id(c)
    if c.kind == "linear":
        ln = (gst.view, gcs.view[0]) if c.fold else None
        y = ops.linear(gx.view, gw.view, bias, act=c.act, residual=None if gr is None else gr.view, out=gy.view, ln=ln,
                       stats_eps=R.EPS if c.stats else None)
        assert y.data_ptr() == gy.view.data_ptr()
        if c.stats:
            st = ops.row_stats(y, R.EPS)
            assert st is y._anemoi_row_stats[1] and st.shape == (c.m, 2) and st.dtype == F32
            out["stats"] = st
            # the wrapper allocates the statistics and the workspace: the entry point itself with both (and a second y) in
            # pattern-filled buffers -- nothing before row 0, behind row M or beside the pairs may be written
            slots = max(c.n // 128, 1)
            gso, gws, gy2 = Guarded(c.m, 2, F32), Guarded(c.m * slots, 2, F32), Guarded(c.m, c.n, c.out, c.pads[1])
            torch.cuda.synchronize()
            rc = _lib.load().anemoi_linear_stats(
                ops.dtype_code(c.dtype), gx.view.data_ptr(), gx.ld, gw.view.data_ptr(), ops._ptr(bias),
                None if gcs is None else gcs.view.data_ptr(), None if gst is None else gst.view.data_ptr(),
                None if gr is None else gr.view.data_ptr(), 0 if gr is None else gr.ld, gy2.view.data_ptr(), gy2.ld, c.m, c.n, c.k,
                gws.view.data_ptr(), gws.view.numel() * 4, R.EPS, gso.view.data_ptr(), ops._stream())
            assert rc == 0
            torch.cuda.synchronize()
            for g, nm in ((gso, "stats_out"), (gws, "workspace"), (gy2, "y")):
                g.assert_clean(f"{what} (library call) {nm}")
            assert torch.equal(gy2.view, y) and torch.equal(gso.view, st), f"{what}: the library call differs from the wrapper"
    elif c.kind == "heads" and c.out == c.dtype:
        y = ops.linear_heads(gx.view, gw.view.view(h, c.n, c.k), out=gy.view)
    elif c.kind == "heads":  # bf16 -> f32 (the weight gradient's form): ops.linear_heads keeps the dtype, so the entry point itself
        st = _lib.load().anemoi_linear_batched(ops.dtype_code(c.dtype), ops.dtype_code(c.out), gx.view.data_ptr(), gx.ld, c.k,
                                               gw.view.data_ptr(), c.n * c.k, gy.view.data_ptr(), gy.ld, c.n, h, c.m, c.n, c.k,
                                               ops._stream())
        assert st == 0
        y = gy.view
    elif c.kind == "dual":
        pre, y = ops.linear_dual(gx.view, gw.view, bias, c.act)
        out["pre"] = pre
    else:
        y = ops.linear_actgrad(gx.view, gw.view, gr.view, c.act)
    torch.cuda.synchronize()
    if c.kind in ("dual", "actgrad") and rt.kernel == "w4":
        # the wrappers allocate their results: the library entry point itself, on pattern-filled buffers, for the rows it takes
        rows = c.m if rt.tail != "py" else rt.main_rows
        gy2, code = Guarded(rows, c.n, BF16, 8), ops.dtype_code(BF16)
        lib = _lib.load()
        if c.kind == "dual":
            gp = Guarded(rows, c.n, BF16, 16)
            st = lib.anemoi_linear_dual(code, gx.view.data_ptr(), gx.ld, gw.view.data_ptr(), ops._ptr(bias), gp.view.data_ptr(),
                                        gp.ld, gy2.view.data_ptr(), gy2.ld, rows, c.n, c.k, _lib.ACT_CODES[c.act], ops._stream())
        else:
            st = lib.anemoi_linear_actgrad(code, gx.view.data_ptr(), gx.ld, gw.view.data_ptr(), gr.view.data_ptr(), gr.ld,
                                           gy2.view.data_ptr(), gy2.ld, rows, c.n, c.k, _lib.ACT_CODES[c.act], ops._stream())
        assert st == 0, f"{what}: the library refused a shape ops.py hands it ({st})"
        torch.cuda.synchronize()
        gy2.assert_clean(what + " (library call) y")
        assert torch.equal(gy2.view, y[:rows]), f"{what}: the library call on padded buffers differs from the wrapper's result"
        if c.kind == "dual":
            gp.assert_clean(what + " (library call) pre")
            assert torch.equal(gp.view, out["pre"][:rows])
    out["y"] = y
    if c.kind in ("linear", "heads"):
        gy.assert_clean(what)
    return {k: v.detach().clone() for k, v in out.items()}, rt


def _check_device(got, want, bound, what):
    """_linear_ref.check for tensors that stay on the device (the multi-round cases)."""
    g = got.double()
    assert bool(torch.isfinite(g).all()), f"{what}: non-finite elements"
    diff = (g - want).abs()
    ratio = torch.where(diff == 0, torch.zeros_like(diff), diff / bound)
    bad = ~(diff <= bound)
    if bool(bad.any()):
        i = int(torch.argmax(torch.where(bad, ratio, torch.full_like(ratio, -1.0))))
        r, cc = divmod(i, got.shape[1])
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements outside their bound; worst at ({r}, {cc}): got "
                             f"{float(g[r, cc]):.9g}, want {float(want[r, cc]):.9g}, bound {float(bound[r, cc]):.3e}")
    return float(ratio.max())


def _family(rt):
    """Row of the worst-fraction table: the kernels that computed the case (the per-case lines name the full route)."""
    if rt.kernel == "py":
        return "ops.py fallback (128x128 + act pass)"
    tail = {"none": "", "skinny": " + skinny kernel", "k128": " + 128x128 tail", "py": " + ops.py rows"}.get(rt.tail, " + in-launch tail")
    if rt.kernel == "k128":
        return "128x128" + tail + (" batched" if rt.batched else "")
    return f"four-wave MH={rt.mh}" + (" two launches" if rt.second and rt.m_a > 0 else "") + tail + (" batched" if rt.batched else "")


def _epilogue(c):
    return c.kind + ("+" + c.act if c.act != "Identity" else "") + ("+res" if c.res else "") + ("+fold" if c.fold else "") + \
        ("" if c.out == c.dtype else ">f32") + (" f32" if c.dtype == F32 else "") + (" exact" if c.data == "exact" else "")


def _run_case(c):
    o = R.operands(c)
    got, rt = _call(c, o)
    again, _ = _call(c, o)
    for k in got:
        assert torch.equal(got[k], again[k]), f"{R.case_id(c)}: {k} differs between two runs"
    big = R.is_big(c)
    acc_s = R.products(c, o, DEV) if big else None
    ref = R.reference(c, o, rt, device=DEV if big else "cpu", acc_s=acc_s)
    if big:  # the device's f64 product (torch's BLAS), confirmed on a row sample by the CPU's
        rows = R.sample_rows(c, rt)
        acc_d, s_d = acc_s
        acc_c, s_c = R.products(c, o, "cpu", rows)
        assert bool(((acc_d[rows.to(DEV)].cpu() - acc_c).abs() <= 1e-12 * s_c).all()), "device f64 product != CPU f64 product"
        assert bool(((s_d[rows.to(DEV)].cpu() - s_c).abs() <= 1e-12 * s_c).all())
    route_key = _family(rt)
    for k, (want, bound) in ref.items():
        if c.data == "exact":
            assert float(want.abs().max()) <= 256 and float(bound.max()) == 0.0
        what = f"{R.case_id(c)} {k}"
        f = _check_device(got[k], want, bound, what) if big else R.check(got[k], want, bound, what)
        _note(f"{route_key} | {_epilogue(c)} | {k}", f)
        print(f"{what}: {f:.3f} of the bound")
    if c.fold and c.data != "exact" and c.m * c.n * c.k <= SMALL:  # against LayerNorm itself
        z_true, extra = R.fold_true_ref(c, o)
        want = R.act64(z_true, c.act) + (o.res.double() if o.res is not None else 0.0)
        f = R.check(got["y"], want, ref["y"][1] + R.LIP[c.act] * extra, f"{R.case_id(c)} y against LayerNorm(x) W^T + b")
        _note(f"{route_key} | {_epilogue(c)} | y vs LayerNorm", f)
    if c.stats:
        want, bound = R.stats_ref(got["y"].cpu(), c.n, rt, c.m)
        f = R.check(got["stats"], want, bound, f"{R.case_id(c)} stats")
        _note(f"{route_key} | {_epilogue(c)} | stats", f)
        print(f"{R.case_id(c)} stats: {f:.3f} of the bound")
        plain = types.SimpleNamespace(**{**vars(c), "stats": False})
        y_plain, _ = _call(plain, o)
        assert torch.equal(y_plain["y"], got["y"]), "stats_eps= changed y"
    return o, got, rt


@pytest.mark.parametrize("c", R.generic_cases(), ids=R.case_id)
def test_generic_kernel(c):
    _run_case(c)


@pytest.mark.parametrize("c", R.w4_cases(), ids=R.case_id)
def test_four_wave_kernel_and_tails(c):
    _run_case(c)


@pytest.mark.parametrize("c", R.dual_cases(), ids=R.case_id)
def test_dual_and_actgrad(c):
    from anemoi_models_amd import ops

    o, got, rt = _run_case(c)
    if c.kind == "dual" and c.m in (1031, 1033) and c.n == 264:  # once at a tail case, once with ragged tiles and ops.py's rows
        want = ops.linear(o.x.to(DEV), o.w.to(DEV), o.bias.to(DEV))
        assert torch.equal(got["pre"], want), "linear_dual's pre differs from ops.linear"


@pytest.mark.parametrize("kind", ["dual", "actgrad"])
def test_unsupported_shapes_are_refused_and_the_fallback_is_right(kind):
    """M % 256 = 9 handed to the library entry point itself: ANEMOI_ERR_UNSUPPORTED, nothing written; ops.py's split of the same
    shape (tiles + its own rows) is the 1033-row case of test_dual_and_actgrad, checked against the same reference."""
    from anemoi_models_amd import _lib, ops

    c = R.Case(kind, 1033, 264, 128, "w4/mh4/split/py/rn/nt2/rem2", act="GELU")
    assert any(R.case_id(c) == R.case_id(d) for d in R.dual_cases())
    o = R.operands(c)
    x, w = o.x.to(DEV), o.w.to(DEV)
    gy, gp = Guarded(c.m, c.n, BF16), Guarded(c.m, c.n, BF16)
    code, lib = ops.dtype_code(BF16), _lib.load()
    if kind == "dual":
        st = lib.anemoi_linear_dual(code, x.data_ptr(), c.k, w.data_ptr(), None, gp.view.data_ptr(), c.n, gy.view.data_ptr(), c.n,
                                    c.m, c.n, c.k, _lib.ACT_CODES[c.act], ops._stream())
    else:
        pre = o.pre.to(DEV)
        st = lib.anemoi_linear_actgrad(code, x.data_ptr(), c.k, w.data_ptr(), pre.data_ptr(), c.n, gy.view.data_ptr(), c.n, c.m,
                                       c.n, c.k, _lib.ACT_CODES[c.act], ops._stream())
    torch.cuda.synchronize()
    assert st == R.ERR_UNSUPPORTED
    assert bool((gy.raw == gy.pattern).all()) and bool((gp.raw == gp.pattern).all()), "a refused call wrote something"


@pytest.mark.parametrize("c", R.heads_cases(), ids=R.case_id)
def test_linear_heads(c):
    _run_case(c)


@pytest.mark.parametrize("c", R.big_cases(), ids=R.case_id)
def test_multi_round_launches(c):
    _run_case(c)


def test_device_activation_figures():
    """The device's SiLU and erf-form GELU (csrc/common.hpp::act_apply -- what the 128 x 128 kernel, the skinny passes and, for
    SiLU, every epilogue call) against f64 on a dense grid, relative to |x|: the SiLU figure that no guide gives (_linear_ref
    uses twice the recorded one), and the documented 2e-7 |x| of the erf form beside the three roundings of 0.5 x (1 + erf)."""
    from anemoi_models_amd import ops

    import _gnn_ops_ref as G

    x = torch.cat([torch.linspace(-24.0, 24.0, 1 << 20, dtype=torch.float64), torch.linspace(-90.0, 90.0, 1 << 16, dtype=torch.float64),
                   G.value_set_tensor()]).float()
    x = x[x != 0]
    x = x[:x.numel() // 4 * 4].contiguous()
    ax = x.double().abs()
    err = {}
    for act in ("SiLU", "GELU"):
        got = ops.act_forward(x.reshape(1, -1).to(DEV), act).cpu().double().reshape(-1)
        assert bool(torch.isfinite(got).all())
        want = G.act64(x.double(), act)
        err[act] = (got - want).abs(), want.abs()
    silu = float((err["SiLU"][0] / ax).max())
    gelu_all = float((err["GELU"][0] / ax).max())
    gelu = float(((err["GELU"][0] - R.gamma(3) * err["GELU"][1]) / ax).max())
    print(f"[device SiLU] worst |error| / |x| = {silu:.3e} (recorded {R.SILU_MEASURED:.3e}, bound {R.SILU_REL:.3e})")
    print(f"[device GELU, erf form] worst |error| / |x| = {gelu_all:.3e}; beside gamma(3) |GELU x|: {gelu:.3e} (bound {R.GELU_ERF_REL:.1e})")
    assert silu <= R.SILU_REL and gelu <= R.GELU_ERF_REL
    assert silu <= 1.05 * R.SILU_MEASURED, "the recorded SiLU figure is out of date: re-derive SILU_REL from the new one"
