"""GPU tests of the thin Linear (csrc/gemm_thin.hip behind ``ops.linear_thin`` / ``anemoi_linear_thin``): every element of
every output against the f64 reference of tests/_linear_ref.py on the same bf16 operands, inside the bound that file derives
-- nothing here widens or restates it.

Which bound.  ``_linear_ref.reference`` takes a route description and bounds the arithmetic that route performs.  The thin
kernel is held to the 128 x 128 route's description for the case's K and epilogue (``_linear_ref._generic``): any-order f32
accumulation gamma(K) |x| |W|^T, one rounding for the bias, gamma(3) terms for the LayerNorm fold, one bf16 store.  With a
residual and a bf16 result the thin kernel rounds, adds in f32 and rounds again, as the persistent kernel and the skinny pass
do (csrc/gemm.hip, "bf16 result, then + residual"); ``_linear_ref`` has that arithmetic under the 128 x 128 route as well --
the rows its skinny pass computes (``tail="skinny"``: every row here, all M < 256) -- and that is the description used for
those cases.  Statistics-only results are held to ``_linear_ref.stats_ref`` of the STORED product of the same kernel (the
two-pass bound ``ops.row_stats`` is held to), and compared with ``ops.row_stats`` of that product.

Shapes: M in {1, 15, 16, 17, 63, 197} (below a 16-row block, ragged, 4 waves x 3 blocks + 5); every (N, K) of the kernel table;
H in {1, 3, 16} problems over column blocks with ldx, ldy, ldr 8 elements beyond the widths.  Operands sit in NaN-guarded
buffers, outputs in pattern-filled ones that must stay untouched outside the view; every case runs twice and must repeat bit
for bit; ``exact`` data (small integers: bound 0) pins every index of the column permutation and of the K split."""

import ctypes

import pytest
import torch

import _linear_ref as R
from test_gpu_linear import Guarded

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = R.F32, R.BF16
MS = (1, 15, 16, 17, 63, 4 * 16 * 3 + 5)
SHAPES = ((256, 64), (64, 256), (256, 256), (80, 1024), (16, 1024), (16, 256), (256, 128))  # (N, K)
BATCHED = ((256, 64), (64, 256), (256, 256), (16, 256), (256, 128))
MODES = {
    "plain": dict(bias=False),
    "bias": dict(bias=True),
    "fold": dict(fold=True),
    "res": dict(bias=False, res=True),
    "f32": dict(bias=False, out=F32),
    "fold_f32": dict(fold=True, out=F32),  # the decoder's extraction
    "bias_res": dict(bias=True, res=True),  # the head product
}
PAD = 8


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from anemoi_models_amd import _lib

    _lib.load()
    assert torch.cuda.is_available()


def _case(m, n, k, h, data, bias=True, res=False, fold=False, out=None):
    return R.Case("heads" if h else "linear", m, n, k, "thin", res=res, fold=fold, data=data, out=out, bias=bias, h=h,
                  pads=(PAD, PAD, PAD))


def _operands(c):
    """``_linear_ref.operands`` of the case; for several problems the bias and the residual cover all H N columns."""
    o = R.operands(c)
    h = max(c.h, 1)
    if h > 1:
        g = torch.Generator().manual_seed(c.m * 31 + c.n * 7 + c.k + h)
        if c.bias:
            o.bias = (torch.randint(-64, 65, (h * c.n,), generator=g).float() if c.data == "exact"
                      else (torch.randn(h * c.n, generator=g) * 0.5 + 0.1).float())
        if c.res:
            o.res = (torch.randint(-64, 65, (c.m, h * c.n), generator=g).double() if c.data == "exact"
                     else torch.randn((c.m, h * c.n), generator=g, dtype=torch.float64) * 2.0).to(BF16)
    return o


def _route(c):
    """The 128 x 128 route's description for the case; round / add / round rows where the thin kernel does that (docstring)."""
    h = max(c.h, 1)
    two = c.res and c.out == BF16
    return R._generic(c.m, c.n * h, c.n * h + PAD, c.n * h + PAD, (0, 0, 0, 0), c.res, c.fold, "skinny" if two else "none")


def _vec(t):
    return None if t is None else Guarded(1, t.numel(), F32, data=t.reshape(1, -1).to(DEV))


def _run(c, o, stats_eps=None):
    from anemoi_models_amd import ops

    h = max(c.h, 1)
    gx = Guarded(c.m, c.k * h, BF16, PAD, data=o.x.to(DEV))
    gw = Guarded(h * c.n, c.k, BF16, 0, data=o.w.reshape(h * c.n, c.k).to(DEV))
    gb, gcs = _vec(o.bias), _vec(o.colsum)
    gst = None if o.stats is None else Guarded(c.m, 2, F32, 0, data=o.stats.to(DEV))
    gr = None if o.res is None else Guarded(c.m, c.n * h, BF16, PAD, data=o.res.to(DEV))
    w = gw.view.view(h, c.n, c.k) if c.h else gw.view
    kw = dict(residual=None if gr is None else gr.view,
              ln=None if gst is None else (gst.view, gcs.view.view(-1)))
    bias = None if gb is None else gb.view.view(-1)
    if stats_eps is not None:
        got = ops.linear_thin(gx.view, w, bias, stats_eps=stats_eps, out_dtype=c.out, **kw)
        assert got is not None, "the thin kernel refused a shape of its table"
        return got
    outs = []
    for _ in range(2):
        gy = Guarded(c.m, c.n * h, c.out, PAD)
        got = ops.linear_thin(gx.view, w, bias, out=gy.view, **kw)
        assert got is not None, "the thin kernel refused a shape of its table"
        torch.cuda.synchronize()
        gy.assert_clean(f"y of {R.case_id(c)}")
        outs.append(gy.view.clone())
    assert torch.equal(outs[0].view(torch.int16 if c.out == BF16 else torch.int32),
                       outs[1].view(torch.int16 if c.out == BF16 else torch.int32)), "two launches differ"
    return outs[0]


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("n,k", SHAPES)
def test_every_element_against_f64(n, k, mode):
    worst = 0.0
    for data in ("ordinary", "exact"):
        for m in MS:
            for h in ((0, 3, 16) if (n, k) in BATCHED and "fold" not in mode else (0,)):
                if h and data == "exact" and m not in (17, MS[-1]):
                    continue  # (the batched walk adds offsets only: two row counts pin them)
                c = _case(m, n, k, h, data, **MODES[mode])
                o = _operands(c)
                got = _run(c, o)
                want, bound = R.reference(c, o, _route(c))["y"]
                worst = max(worst, R.check(got, want, bound, R.case_id(c)))
    print(f"[thin {n}x{k} {mode}] worst fraction of the bound: {worst:.3f}")


@pytest.mark.parametrize("n,k", SHAPES)
def test_statistics_only_against_row_stats_of_the_stored_product(n, k):
    from anemoi_models_amd import ops

    worst = 0.0
    # alone, with a bias, with the LayerNorm fold, and of the f32 product (no bf16 rounding in front of the statistics)
    for mode in (dict(bias=False), dict(bias=True), dict(fold=True), dict(bias=True, out=F32), dict(fold=True, out=F32)):
        for m in MS:
            c = _case(m, n, k, 0, "ordinary", **mode)
            o = _operands(c)
            y = _run(c, o)  # the product as this kernel stores it (in the case's output dtype)
            got = _run(c, o, stats_eps=R.EPS)
            assert got.shape == (m, 2) and got.dtype == torch.float32
            want, bound = R.stats_ref(y, n, _route(c), m, R.EPS)
            worst = max(worst, R.check(got, want, bound, f"stats of {R.case_id(c)}"))
            rs = ops.row_stats(y.contiguous(), R.EPS)
            R.check(rs, want, bound, f"ops.row_stats of {R.case_id(c)}")
            assert bool(((got - rs).abs().double().cpu() <= 2 * bound).all())
            again = _run(c, o, stats_eps=R.EPS)
            assert torch.equal(got.view(torch.int32), again.view(torch.int32))
    print(f"[thin {n}x{k} statistics only] worst fraction of the bound: {worst:.3f}")


def test_refused_calls_launch_nothing():
    from anemoi_models_amd import _lib, ops

    x = torch.randn(64, 1024, device=DEV).to(BF16)
    ops.PROFILE = []
    try:
        for n, k in ((128, 128), (80, 512), (64, 64), (256, 1024), (24, 256)):
            w = torch.randn(n, k, device=DEV).to(BF16)
            assert ops.linear_thin(x[:, :k], w) is None
        # combinations the table's shapes do not take: batched K-split, batched fold, statistics with a residual
        w = torch.randn(4, 80, 1024, device=DEV).to(BF16)
        assert ops.linear_thin(torch.randn(64, 4096, device=DEV).to(BF16), w) is None
        w = torch.randn(4, 64, 256, device=DEV).to(BF16)
        st, cs = torch.ones(64, 2, device=DEV), torch.zeros(64, device=DEV)
        assert ops.linear_thin(x, w, ln=(st, cs)) is None
        w = torch.randn(256, 256, device=DEV).to(BF16)
        assert ops.linear_thin(x[:, :256], w, residual=torch.zeros(64, 256, device=DEV, dtype=BF16), stats_eps=1e-5) is None
        assert ops.linear_thin(x.float()[:, :256], w.float()) is None  # f32 operands
        # the status code itself
        a = _lib.LinearThinArgs()
        a.struct_bytes = ctypes.sizeof(_lib.LinearThinArgs)
        y = torch.empty(64, 128, device=DEV, dtype=BF16)
        w = torch.randn(128, 128, device=DEV).to(BF16)
        a.out_dtype, a.x, a.w, a.y, a.ldx, a.ldy, a.M, a.N, a.K = _lib.BF16, x.data_ptr(), w.data_ptr(), y.data_ptr(), 1024, 128, 64, 128, 128
        assert _lib.load().anemoi_linear_thin(ctypes.byref(a), ops._stream()) == _lib.ANEMOI_ERR_UNSUPPORTED
        assert ops.PROFILE == []
        # operands the 16-byte accesses cannot take (pitch, base address) are refused too: the caller's route may take them
        w = torch.randn(64, 256, device=DEV).to(BF16)
        assert ops.linear_thin(torch.zeros(64, 260, device=DEV, dtype=BF16)[:, :256], w) is None
        assert ops.linear_thin(torch.zeros(64, 264, device=DEV, dtype=BF16)[:, 4:260], w) is None
        assert ops.linear_thin(x[:, :256], w, out=torch.zeros(64, 68, device=DEV, dtype=BF16)[:, :64]) is None
        assert ops.linear_thin(x[:, :256], w, residual=torch.zeros(64, 72, device=DEV, dtype=BF16)[:, 4:68]) is None
        assert ops.PROFILE == []
        # through the entry point itself such a block is an invalid call
        a.N, a.K, a.ldx, a.ldy, a.w, a.y = 64, 256, 1028, 64, w.data_ptr(), y.data_ptr()
        assert _lib.load().anemoi_linear_thin(ctypes.byref(a), ops._stream()) == _lib.ANEMOI_ERR_INVALID
        assert ops.PROFILE == []
        assert ops.linear_thin(x[:, :256], w) is not None and [r[0] for r in ops.PROFILE] == ["linear"]
        assert ops.PROFILE[0][3].get("thin") is True
    finally:
        ops.PROFILE = None


def test_linear_heads_takes_the_residual_and_the_switch_restores_the_two_launches(monkeypatch):
    """``ops.linear_heads(g, w, out=, residual=)`` at the raw-row encoder's head shapes: one thin launch with the switch on, no
    ``add``; ``ANEMOI_AMD_THIN=0``: ``anemoi_linear_batched`` then ``add``, the bits of the two separate calls."""
    from anemoi_models_amd import ops

    m, h = 197, 16
    for n, k in ((64, 256), (256, 64)):
        c = _case(m, n, k, h, "ordinary", bias=False, res=True)
        o = _operands(c)
        x, w, r = o.x.to(DEV), o.w.to(DEV), o.res.to(DEV)

        def run(flag):
            monkeypatch.setenv("ANEMOI_AMD_THIN", flag)
            out = torch.zeros(m, h * n + PAD, device=DEV, dtype=BF16)
            ops.PROFILE = []
            try:
                ops.linear_heads(x, w, out=out[:, :h * n], residual=r)
                names = [(rec[0], bool(rec[3].get("thin"))) for rec in ops.PROFILE]
            finally:
                ops.PROFILE = None
            assert not out[:, h * n:].any()
            return out[:, :h * n].clone(), names

        on, names_on = run("1")
        off, names_off = run("0")
        assert names_on == [("linear", True)] and names_off == [("linear", False), ("add", False)]
        monkeypatch.setenv("ANEMOI_AMD_THIN", "0")
        parent = ops.add(ops.linear_heads(x, w), r)  # the two launches as the callers made them before
        assert torch.equal(off, parent)
        want, bound = R.reference(c, o, _route(c))["y"]
        R.check(on, want, bound, f"linear_heads {n}x{k} thin")
        R.check(off, want, bound, f"linear_heads {n}x{k} batched + add")
