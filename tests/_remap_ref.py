"""f64 contracts, per-element error bounds, cases and the checker of the three remapper kernels (csrc/remap.hip behind
``ops.assemble_nodes(remap=)``, ``ops.residual_remapped``, ``ops.unmap_output``), and plain-torch f32 evaluations of the same
formulas with their mutants.

Pure torch on the CPU.  Used by tests/test_remap_io_cpu.py (f32 torch stays inside the bounds, the mutants do not) and by
tests/test_gpu_remap_io.py (the kernels).  Every contract is computed in f64 from the operands AS STORED (f32 state, f32
tables); every bound is per element, built as tests/_row_kernels_ref.py builds its bounds:

  u = 2^-24 per rounded f32 operation, relative to its result (an fma only removes a rounding);
  a function f of an argument known to within Ea:  sup |f'| over [a - Ea, a + Ea] times Ea (mean value theorem; the
    supremum in closed form per function below), plus the function's own error;
  the function's own error, from the table of the OpenCL C specification ("Relative error as ULPs"), which ROCm's device
    library implements (see _row_kernels_ref.py), in ulp = EPS32 of the result:
      log1p 2, sqrt 3, cos 4, sin 4, expm1 3, atan2 6, x / y 2.5, fmod 0;
  one bf16 store: 2^-8 of |want| + (the f32 bound).

Forward  f(x) = post_mul * op(pre_mul * x + pre_add) + post_add
  a = pre_mul x + pre_add:  Ea = u (|pre_mul x| + |a|)   (0 without the pair: nothing is computed)
  copy: Ew = Ea.   log1p: sup |f'| = 1 / (1 + a - Ea).   sqrt: 1 / (2 sqrt(a - Ea)).   boxcox (sqrt(a) - 1) / 0.5: twice the
  sqrt bound plus u |w| for the subtraction (the division by 0.5 is exact).
  cos / sin of r = a k, k = pi / 180: the kernel holds k as an f32 constant and rounds the product, Er = k Ea + 2 u |r|;
    |f'| <= min(1, |f'(r)| + Er).
  z = post_mul w + post_add:  Ez = |post_mul| Ew (1 + 2 u) + u (|post_mul w| + |z|).
Residual  y + f:  Ef + u (|want| + Ef).
Inverse  z = (inv((y - post_add) / post_mul) - pre_add) / pre_mul
  v = (y - post_add) / post_mul:  Ev = u |y - post_add| / |post_mul| + 2.5 EPS32 |v|   (0 without the pair)
  expm1: sup |f'| = exp(v + Ev).   square: 2 (|v| + Ev), one rounding.   inv_boxcox h = 0.5 v + 1, h^2: Eh = Ev / 2 + u |h|,
  Ew = (2 |h| + Eh) Eh + u h^2.
  atan2deg of (c, s) = (cosine, sine column), rho = hypot(c, s):  |d atan2| <= (|s| Ec + |c| Es) / max(rho - Ec - Es, 0)^2,
    plus 6 ulp of the angle; times the f32 constant 180 / pi (2 u of the product); fmod is exact; + 360 of a negative
    result rounds once (u 360).  The comparison is ON THE CIRCLE: min(|d|, P - |d|) with the period P = 360 / |pre_mul| of the
    column's final units -- every element is compared.
  z = (w - pre_add) / pre_mul:  Ez = (Ew + u |w - pre_add|) / |pre_mul| + 2.5 EPS32 (|z| + Ew / |pre_mul|).
NaN: the positions of NaN in the result must EQUAL those of the contract (a NaN input, log1p below -1, sqrt of a negative
number); the test data keeps every finite argument further than its Ea from a domain's edge.
"""

from __future__ import annotations

import math

import torch

from _gnn_ops_ref import BF16_STORE, EPS32

U = EPS32 / 2.0
ULP = {"log1p": 2.0, "sqrt": 3.0, "cos": 4.0, "sin": 4.0, "expm1": 3.0, "atan2": 6.0, "div": 2.5}
K = math.pi / 180.0
F64 = torch.float64


def _pair(p, cols=None):
    if p is None:
        return None
    mul, add = (t.detach().cpu().to(F64) for t in p)
    return (mul, add) if cols is None else (mul[cols], add[cols])


def _sqrt(a, ea):
    w = torch.sqrt(a)
    lo = (a - ea).clamp_min(0.0)
    slope = torch.where(ea > 0, 0.5 / torch.sqrt(lo), torch.zeros_like(a))
    return w, slope * ea + ULP["sqrt"] * EPS32 * w.abs()


def op_ref(op: str, a, ea, a1=None, ea1=None):
    """``(op(a), bound)`` for an argument known to within ``ea`` (f64 tensors)."""
    if op == "copy":
        return a, ea
    if op == "log1p":
        w = torch.log1p(a)
        return w, ea / (1.0 + a - ea).clamp_min(0.0) + ULP["log1p"] * EPS32 * w.abs()
    if op == "sqrt":
        return _sqrt(a, ea)
    if op == "boxcox":
        s, es = _sqrt(a, ea)
        w = (s - 1.0) / 0.5
        return w, 2.0 * es + U * w.abs()
    if op in ("cos", "sin"):
        r = a * K
        er = K * ea + 2.0 * U * r.abs()
        w, slope = (torch.cos(r), torch.sin(r).abs()) if op == "cos" else (torch.sin(r), torch.cos(r).abs())
        return w, (slope + er).clamp_max(1.0) * er + ULP[op] * EPS32 * w.abs()
    if op == "expm1":
        w = torch.expm1(a)
        return w, torch.exp(a + ea) * ea + ULP["expm1"] * EPS32 * w.abs()
    if op == "square":
        w = a * a
        return w, 2.0 * (a.abs() + ea) * ea + U * w
    if op == "inv_boxcox":
        h = 0.5 * a + 1.0
        eh = 0.5 * ea + U * h.abs()
        return h * h, (2.0 * h.abs() + eh) * eh + U * h * h
    if op == "atan2deg":
        ang = torch.atan2(a1, a)
        rho = (torch.hypot(a, a1) - ea - ea1).clamp_min(0.0)
        e_ang = (a1.abs() * ea + a.abs() * ea1) / (rho * rho) + ULP["atan2"] * EPS32 * ang.abs()
        e_ang = torch.where((ea + ea1) > 0, e_ang, ULP["atan2"] * EPS32 * ang.abs())
        deg = ang * (180.0 / math.pi)
        return torch.remainder(deg, 360.0), e_ang * (180.0 / math.pi) + 2.0 * U * deg.abs() + U * 360.0
    raise ValueError(op)


def forward_ref(x, ops_, pre, post):
    """``x`` f64 ``[..., V_int]`` (already gathered: column j holds the raw column src[j]) -> ``(f(x), bound)``."""
    a, ea = x, torch.zeros_like(x)
    if pre is not None:
        a = pre[0] * x + pre[1]
        ea = U * ((pre[0] * x).abs() + a.abs())
    w, ew = torch.empty_like(a), torch.empty_like(a)
    for j, op in enumerate(ops_):
        w[..., j], ew[..., j] = op_ref(op, a[..., j], ea[..., j])
    if post is None:
        return w, ew
    z = post[0] * w + post[1]
    return z, post[0].abs() * ew * (1.0 + 2.0 * U) + U * ((post[0] * w).abs() + z.abs())


def _names(codes, table):
    inverse = {v: k for k, v in table.items()}
    return [inverse[int(c)] for c in codes]


def tables(remap):
    """The tables of an ``ops.Remapping`` on the host: names and f64 pairs."""
    from anemoi_models_amd.ops import REMAP_OPS

    return {"src": remap.h_src.long(), "op": _names(remap.h_op, REMAP_OPS), "res": remap.h_res.long(),
            "s0": remap.h_s0.long(), "s1": remap.h_s1.long(), "inv_op": _names(remap.h_inv_op, REMAP_OPS),
            "pre": _pair(remap.pre), "post": _pair(remap.post), "inv_pre": _pair(remap.inv_pre),
            "inv_post": _pair(remap.inv_post)}


def _store(want, b32, dtype):
    return b32 + BF16_STORE * (want.abs() + b32) if dtype == torch.bfloat16 else b32


def assemble_ref(x, latlons, trainable, remap, ldo: int, dtype):
    """Contract of ``anemoi_assemble_nodes_remapped``: ``(want, bound)`` f64 ``[B * Ens * G, ldo]``."""
    t = tables(remap)
    b, nt, ens, g, _ = x.shape
    f, ef = forward_ref(x.double()[..., t["src"]], t["op"], t["pre"], t["post"])  # [B, T, Ens, G, V_int]
    v_int = f.shape[-1]
    feat = f.permute(0, 2, 3, 1, 4).reshape(b * ens * g, nt * v_int)
    efeat = ef.permute(0, 2, 3, 1, 4).reshape(b * ens * g, nt * v_int)
    want = torch.zeros((b * ens * g, ldo), dtype=F64)
    bound = torch.zeros_like(want)
    want[:, : nt * v_int], bound[:, : nt * v_int] = feat, efeat
    col = nt * v_int
    for extra in (latlons, trainable):
        if extra is not None:
            want[:, col : col + extra.shape[1]] = extra.double().repeat(b * ens, 1)
            col += extra.shape[1]
    return want, _store(want, bound, dtype)


def residual_ref(y, x, remap):
    """Contract of ``anemoi_residual_remapped``: ``(want, bound)`` f64, shaped like ``y`` ``[B, Ens, G, V_int_out]``."""
    t = tables(remap)
    f, ef = forward_ref(x.double()[:, -1][..., t["src"]], t["op"], t["pre"], t["post"])  # [B, Ens, G, V_int]
    want, bound = y.double().clone(), torch.zeros(y.shape, dtype=F64)
    for c, j in enumerate(t["res"].tolist()):
        if j >= 0:
            want[..., c] = y.double()[..., c] + f[..., j]
            bound[..., c] = ef[..., j] + U * (want[..., c].abs() + ef[..., j])
    return want, bound


def unmap_ref(y, remap):
    """Contract of ``anemoi_unmap_output``: ``(want, bound, period)`` f64 ``[..., V_out]``; ``period`` is 0 for a column that is
    compared on the line and the length of the circle for an ``atan2deg`` column."""
    t = tables(remap)
    v, ev = y.double(), torch.zeros(y.shape, dtype=F64)
    if t["inv_post"] is not None:
        mul, add = t["inv_post"]
        v = (y.double() - add) / mul
        ev = U * (y.double() - add).abs() / mul.abs() + ULP["div"] * EPS32 * v.abs()
    n_out = len(t["inv_op"])
    want = torch.empty(tuple(y.shape[:-1]) + (n_out,), dtype=F64)
    bound, period = torch.empty_like(want), torch.zeros(n_out, dtype=F64)
    for c, op in enumerate(t["inv_op"]):
        a, a1 = int(t["s0"][c]), int(t["s1"][c])
        if op == "atan2deg":
            want[..., c], bound[..., c] = op_ref(op, v[..., a], ev[..., a], v[..., a1], ev[..., a1])
            period[c] = 360.0
        else:
            want[..., c], bound[..., c] = op_ref(op, v[..., a], ev[..., a])
    if t["inv_pre"] is not None:
        mul, add = t["inv_pre"]
        z = (want - add) / mul
        bound = (bound + U * (want - add).abs()) / mul.abs() + ULP["div"] * EPS32 * (z.abs() + bound / mul.abs())
        want, period = z, period / mul.abs()
    return want, bound, period


def check(got, want, bound, what: str, period=None) -> float:
    """NaN exactly where the contract has NaN; every other element finite and within ``bound`` of ``want`` -- on the circle of
    length ``period[c]`` where that is positive.  Returns the largest fraction of a bound that was used."""
    g = got.detach().cpu().double()
    assert g.shape == want.shape == bound.shape, f"{what}: shape {tuple(g.shape)}, expected {tuple(want.shape)}"
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(g), nan), f"{what}: NaN at {int((torch.isnan(g) != nan).sum())} other positions than the contract"
    diff = (g - want).abs()
    if period is not None:
        p = period.expand_as(diff)
        diff = torch.where(p > 0, torch.minimum(diff, (p - diff).abs()), diff)
    diff, b = diff[~nan], bound[~nan]
    assert bool(torch.isfinite(g[~nan]).all()), f"{what}: non-finite elements where the contract is finite"
    bad = ~(diff <= b)
    ratio = torch.where(diff == 0, torch.zeros_like(diff), diff / b)
    if bool(bad.any()):
        i = int(torch.argmax(torch.where(bad, ratio, torch.full_like(ratio, -1.0))))
        raise AssertionError(f"{what}: {int(bad.sum())} of {diff.numel()} elements outside their bound; worst: got "
                             f"{float(g[~nan][i]):.9g}, want {float(want[~nan][i]):.9g}, |diff| {float(diff[i]):.3e} > bound "
                             f"{float(b[i]):.3e}")
    return float(ratio.max()) if ratio.numel() else 0.0


# ------------------------------------------------------------------------------------------------ cases
SHAPES = ((2, 2, 2, 37, 6), (1, 2, 1, 65, 7), (1, 1, 1, 300, 12))  # (B, T, Ens, G, V_raw)


def make_case(shape, extra: int, affine: bool, seed: int = 0, device="cpu"):
    """A remapping of ``V_raw`` raw input columns to ``V_int = V_raw + extra`` (1 or 2) internal ones and its data.

    Raw columns: 0 a direction (cos and sin: ONE SOURCE FEEDS TWO COLUMNS), 1 log1p, 2 sqrt, 3 boxcox, the last one a FORCING
    that is a second direction when ``extra == 2`` (remapped, ABSENT FROM THE OUTPUT), plain columns between.  Internal input:
    the kept columns first -- they SHIFT POSITION -- then the cos / sin pairs.  Internal output: the non-forcing internal
    columns; raw output: raw columns but the forcing.  ``affine``: non-identity pre pair (forward) and pre pair (inverse), else
    a post pair on both -- each test runs both.  Data: directions in [0, 360), mono columns in [0.01, 4), NaN at some points of
    every kind of column and values outside the domain (-3) in the log1p, sqrt and boxcox columns."""
    from anemoi_models_amd.ops import Remapping

    b, t, ens, g, v_raw = shape
    gen = torch.Generator().manual_seed(seed)
    forcing = v_raw - 1
    remapped = [0] + ([forcing] if extra == 2 else [])
    keep = [c for c in range(v_raw) if c not in remapped]
    mono = {1: "log1p", 2: "sqrt", 3: "boxcox"}
    src = keep + [c for r in remapped for c in (r, r)]
    op = [mono.get(c, "copy") for c in keep] + ["cos", "sin"] * len(remapped)
    v_int = len(src)
    assert v_int == v_raw + extra
    int_in_forcing = {j for j, c in enumerate(src) if c == forcing}
    int_out = [j for j in range(v_int) if j not in int_in_forcing]  # internal output column k <- internal input column int_out[k]
    res = [-1 if src[j] == 4 else j for j in int_out]  # raw column 4 gets no residual (as a diagnostic would not)
    raw_out = [c for c in range(v_raw) if c != forcing]
    s0, s1, inv_op = [], [], []
    inverse = {"log1p": "expm1", "sqrt": "square", "boxcox": "inv_boxcox"}
    for c in raw_out:
        if c == 0:
            s0.append(int_out.index(src.index(0)))
            s1.append(s0[-1] + 1)
            inv_op.append("atan2deg")
        else:
            s0.append(int_out.index(src.index(c)))
            s1.append(-1)
            inv_op.append(inverse.get(mono.get(c), "copy"))

    def pair(n):
        return (0.5 + torch.rand(n, generator=gen), torch.randn(n, generator=gen) * 0.25)

    kw = {}
    if affine:
        mul, add = pair(v_int)
        trig = torch.tensor([o in ("cos", "sin") for o in op])
        plain = torch.tensor([o == "copy" for o in op])
        # a pre pair must keep the arguments inside the converters' domains: shift only plain and direction columns
        kw["pre"] = (torch.where(trig | plain, mul, torch.ones(v_int)), torch.where(plain, add, torch.zeros(v_int)))
        kw["inv_pre"] = pair(len(raw_out))
    else:
        kw["post"] = pair(v_int)
        kw["inv_post"] = pair(len(int_out))
    remap = Remapping(device, v_raw, src, op, res, s0, s1, inv_op, **kw)

    x = torch.randn((b, t, ens, g, v_raw), generator=gen)
    for c in remapped:
        x[..., c] = torch.rand((b, t, ens, g), generator=gen) * 360.0
    for c in mono:
        x[..., c] = 0.01 + torch.rand((b, t, ens, g), generator=gen) * 3.99
        x[..., c][torch.rand((b, t, ens, g), generator=gen) < 0.05] = -3.0
    x[torch.rand(x.shape, generator=gen) < 0.03] = float("nan")
    y = torch.randn((b, ens, g, len(int_out)), generator=gen)  # internal output: cos / sin columns of any radius
    y[torch.rand(y.shape, generator=gen) < 0.03] = float("nan")
    return remap, x, y


# ------------------------------------------------------------------------------------------------ f32 torch and its mutants
def forward_f32(x, ops_, pre, post, mutant: str = ""):
    """The forward formula in f32 torch with the kernel's one f32 constant pi / 180; ``x`` ``[..., V_int]`` gathered."""
    if mutant == "pairs_exchanged":
        pre, post = post, pre
    a = x if pre is None else x * pre[0] + pre[1]
    w = torch.empty_like(a)
    for j, op in enumerate(ops_):
        if mutant == "cos_sin_swapped":
            op = {"cos": "sin", "sin": "cos"}.get(op, op)
        col = a[..., j]
        if op in ("cos", "sin"):
            r = col if mutant == "no_degree_factor" else col * torch.tensor(K, dtype=torch.float32)
            w[..., j] = torch.cos(r) if op == "cos" else torch.sin(r)
        else:
            w[..., j] = {"copy": lambda v: v, "log1p": torch.log1p, "sqrt": torch.sqrt,
                         "boxcox": lambda v: (torch.sqrt(v) - 1) / 0.5}[op](col)
    return w if post is None else w * post[0] + post[1]


def inverse_f32(y, t, mutant: str = ""):
    """The inverse formula in f32 torch on the tables ``t`` of :func:`tables` (pairs as f32)."""
    post = None if t["inv_post"] is None else tuple(p.float() for p in t["inv_post"])
    pre = None if t["inv_pre"] is None else tuple(p.float() for p in t["inv_pre"])
    if mutant == "pairs_exchanged":
        # (the tables have different lengths: exchange their roles column by column)
        post, pre = (None if pre is None else tuple(p[torch.arange(y.shape[-1]) % p.numel()] for p in pre),
                     None if post is None else tuple(p[torch.arange(len(t["inv_op"])) % p.numel()] for p in post))
    v = y if post is None else (y - post[1]) / post[0]
    cols = []
    for c, op in enumerate(t["inv_op"]):
        a, a1 = v[..., int(t["s0"][c])], v[..., int(t["s1"][c])]
        if op == "atan2deg":
            if mutant == "cos_sin_swapped":
                a, a1 = a1, a
            ang = torch.atan2(a1, a)
            cols.append(torch.remainder(ang if mutant == "no_degree_factor" else ang * torch.tensor(1.0 / K, dtype=torch.float32), 360))
        elif op == "expm1":
            cols.append(torch.exp(a) if mutant == "exp_for_expm1" else torch.expm1(a))
        else:
            cols.append({"copy": lambda q: q, "square": lambda q: q * q, "inv_boxcox": lambda q: (q * 0.5 + 1) ** 2}[op](a))
    w = torch.stack(cols, dim=-1)
    return w if pre is None else (w - pre[1]) / pre[0]


# ------------------------------------------------------------------------------------------------ the interface cases
def build_case_interface(graph, gold, case, fix=None, processors=None, remapped="case",
                         model_target="anemoi.models.models.encoder_processor_decoder.AnemoiModelEncProcDec", config=None):
    """The interface of tests/golden/make_golden_remappers.py case ``case`` on config 1 (``gold``: interface_gt.npz, whose
    statistics and -- with ``fix``, the loaded fixture -- weights it shares; the widened tensors of a cos_sin case come from
    ``fix``).  ``processors`` / ``remapped`` override the case's chain and ``config.data.remapped``, ``config`` /
    ``model_target`` the model."""
    import sys

    from conftest import GOLDEN
    from conftest import split_prefix

    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)
    import make_golden_remappers as fixture

    from anemoi_models_amd.interface import AnemoiModelInterface
    from anemoi_models_amd.utils.indices import SimpleDataIndices
    from anemoi_models_amd.utils.presets import model_config

    procs, case_remapped, bounding = fixture.CASES[case]
    remapped = case_remapped if remapped == "case" else remapped
    cfg = model_config("GraphTransformer", 64, 4, 16) if config is None else config
    cfg["data"] = fixture.data_config(processors or procs, remapped)
    cfg["model"]["model"] = {"_target_": model_target}
    if bounding is not None:
        cfg["model"]["bounding"] = [dict(b) for b in bounding]
    cfg = type(cfg)(cfg)
    stats = {k: v.numpy() for k, v in split_prefix(gold, "stat.").items()}
    idx = SimpleDataIndices(n_prognostic=10, n_forcing=2, n_diagnostic=1, remapped=remapped)
    iface = AnemoiModelInterface(config=cfg, graph_data=graph, statistics=stats, data_indices=idx, metadata={})
    if fix is not None:
        sd = split_prefix(gold, "sd.")
        if remapped:
            sd.update(split_prefix(fix, "sd_multi."))
        iface.load_state_dict(sd)
    return iface


def column_errors(got, want, direction_columns=()):
    """Per output column: max error over the column's max magnitude; a direction column on the circle, against 360."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    out = []
    for c in range(want.shape[-1]):
        d = (got[..., c] - want[..., c]).abs()
        if c in direction_columns:
            out.append(float(torch.minimum(d, (360.0 - d).abs()).max()) / 360.0)
        else:
            out.append(float(d.max()) / float(want[..., c].abs().max()))
    return out
