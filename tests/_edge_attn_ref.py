"""f64 references, per-element error bounds, data sets, graphs and case lists for the FOLDED graph-transformer edge phase:
``ops.gt_edge_attention_folded`` (csrc/edge_attention.hip: the plain kernel and the four list kernels -- groups, runs, tiles,
sched) and its backward ``autograd._edge_backward`` (csrc/edge_backward.hip: destination sweep, source sweep, attribute
gradient); behind them, each with its own derivation in the comment above its section: the explicit-edge conv ``ops.gt_conv`` with
its dropout, forward and backward (``autograd.gt_conv``: dq, dk, dv, d e), the unfolded kernel ``ops.gt_edge_attention`` (fast and
generic path) and the raw-row kernel ``ops.gt_edge_attention_raw``.

Pure torch on the CPU; imports nothing from the GPU side.  Used by tests/test_edge_attn_ref_cpu.py (validates the references
against f64 autograd of the explicit expression and against ``oracle.pyg_semantics``, shows that emulations of the kernels'
arithmetic stay inside the bounds and that subtly wrong results do not) and by tests/test_gpu_edge_attn.py (the kernels).

The operation, on the operands AS STORED (a bf16 operand converts exactly), c = 1 / sqrt(D), per destination i, head h and
in-edge e = (j -> i) at CSR position e with the f32 attribute row a_e [up] (constant 1 in column up - 1):
    s_e = c (q_i,h . k_j,h + u_i,h . a_e),   m = max_e s_e,   l = sum_e exp(s_e - m),   alpha_e = exp(s_e - m) / (l + 1e-16),
    out_i,h = sum_e alpha_e v_j,h (+ x_r),   t_i,h = sum_e alpha_e a_e,   lse_i,h = m + log(l + 1e-16);
    a destination without in-edges: out = x_r (or 0), t = 0, lse = -inf.
Backward (the closed forms at the top of edge_backward.hip), given dout, dt:
    da_e = dout_i,h . v_j,h + dt_i,h . a_e,   w_e = alpha_e da_e,   Dsum_i,h = sum_e w_e,   ds_e = w_e - alpha_e Dsum_i,h,
    dq_i,h = c sum_e ds_e k_j,h,  du_i,h = c sum_e ds_e a_e,  dk_j,h = c sum_{e from j} ds_e q_i,h,  dv_j,h = sum_{e from j} alpha_e dout_i,h,
    d a_e = sum_h (c ds_e u_i,h + alpha_e dt_i,h),   d x_r = dout.
``evaluate`` / ``evaluate_backward`` state exactly these expressions once, for any torch dtype: in f64 they are the reference,
in f32 they are "torch's own f32 evaluation of the same expressions" the constants below are measured on.

Every bound is per element: |got - want| <= bound and got finite, nothing exempt; where the bound is 0 the element must be
exact (``_mhsa_ref.check``).  Notation as tests/_mhsa_ref.py: u = 2^-24 (``U``), gamma(n) = n u / (1 - n u), EPS32 = 2 u,
BF16_STORE = 2^-8 for the one rounding of a bf16 store, applied to |want| + (the bound in front of it).

Scores.  bf16: the D products are exact (v_dot2_f32_bf16) and summed in f32; f32: D FMAs.  A lane sums VEC channel terms and its
APL attribute FMAs (f32 attributes), log2(LPH) cross-lane adds follow: at most D + up + log2(16) roundings on terms whose
absolute sum is sqrt(D) M, M_i,h = c max_e (sum_d |q||k| + sum_a |u||a|).  The f32 scale 1 / sqrtf(D) is two roundings off c,
the product one more, the subtraction of the running maximum one on a number <= 2 M, and __expf is exp2 of a rounded product
with a rounded log2 e (two more on <= 2 M) around a hardware exponential of one ulp (EPS32 relative).  An absolute error of the
exponent is the same relative error of the weight:
    eta_i,h = gamma(D + up + 12) M_i,h + 2 EPS32                    (relative, every weight of the row, c = 12, k = 2)
Forward.  The weights stay f32.  The online maximum rescales the accumulators once per chunk of U_EDGES = 4 edges with a factor
that is the same float for the numerator and the normaliser, so its own error cancels in out and t; what does not cancel is one
rounding per rescale and per FMA: deg + deg / 4 roundings, and 4 for l + 1e-16, the reciprocal and the product:
    eps_i,h = eta + gamma(deg + deg / 4 + 4),   E32 = eps / (1 - eps) (A + |attn|),   A = sum_e alpha_e |v_j| (|a_e| for t)
(as in _mhsa_ref: num^ / (l^ / l) with both relative errors <= eps), then x_r is added in f32: U (|want| + E32), exact when
there is no x_r, and the store: bf16 BF16_STORE (|want| + bound), f32 nothing.  An isolated destination has A = 0: the bound is
the x_r store alone, which is exact -- out = x_r, t = 0 bit for bit, and lse = -inf is demanded by ``check_lse``.
    lse = m + __logf(l + 1e-16):  in l the rescale factors do NOT cancel; a factor is an __expf of m_old - m_new (one ulp, and
    3 u |m_old - m_new| from the subtraction and the product; the differences telescope to <= 2 M), one per chunk:
    eps_lse = eps + (deg / 4) EPS32 + gamma(8) M;   bound = eps_lse / (1 - eps_lse) + 4 EPS32 (|lse| + M)      (log, sum: as _mhsa_ref)
Backward.  alpha^ = __expf(s^ - lse_stored) = alpha (1 + e), |e| <= relP = x / (1 - x), x = eta + lse_err, where lse_err is what
is known about the stored lse: the forward lse bound, or the actual deviation where the test supplies the lse.
    da^_e:   Eda = gamma(D + up + 4) (sum_d |dout||v| + sum_a |dt||a|)
    w^_e:    Ew  = |w| (relP + U) + alpha (1 + relP) Eda
    Dsum^:   EDs = sum_e Ew + gamma(deg) sum_e (|w| + Ew)                             = relP sum|w| + gamma(deg) sum|w| + ...
    dq = c (A - Dsum B), A = sum w k, B = sum alpha k -- two sums that cancel, so the bound carries their magnitudes:
             EA = sum_e Ew |k| + gamma(deg + 2) sum_e (|w| + Ew) |k|,   EB = relP sum_e alpha |k| + gamma(deg + 2) (1 + relP) sum_e alpha |k|
             Edq = c [EA + EDs (Babs + EB) + |Dsum| EB + 4 U (Aabs + EA + (|Dsum| + EDs) (Babs + EB))]     (du: a_e for k_j)
    It is NOT gamma |true dq|: a destination with one in-edge has a true ds = 0 and a computed w (1 - alpha^).
    ds^_e = fma(-alpha^, Dsum^, w^):  Eds = Ew + alpha relP |Dsum| + alpha (1 + relP) EDs + U (|w| + alpha |Dsum|)
    dk_j:    c [sum_e Eds |q| + gamma(odeg + 2) sum_e (|ds| + Eds) |q|]                 (over the out-edges of j, U = 4 there too)
    dv_j:    sum_e alpha relP |dout| + gamma(odeg + 1) (1 + relP) sum_e alpha |dout|
    d a_e:   sum_h [c Eds |u| + alpha relP |dt|] + gamma(2 H + 2) sum_h [c (|ds| + Eds) |u| + alpha (1 + relP) |dt|]      (f32 result)
then the store.  Where every term vanishes (an isolated destination's dq / du, dk / dv of a source without out-edges) the bound
is 0 and the element must be an exact zero.  dxr is a copy of dout: bit-equal.

What published figures do not cover -- __expf, __logf, the summation order -- is MEASURED on something else than the kernels:
torch's own f32 evaluation of the expressions above on the CPU against the f64 reference over ``F32_MEASURE_CASES``, as the worst
fraction of the derived roundoff bound (``TORCH_F32``; the CPU test re-measures it and fails if it moves by more than 1 %).  The
kernels get ``F32_FACTOR`` = 4 times that (the project's margin, _mhsa_ref) on the roundoff part; single roundings that are
known exactly (the x_r add, the store) and the operand part (what lse_err adds) stay as derived.  No constant comes from a GPU.

What no accuracy bound can reject: the 1e-16 in the normaliser (l >= 1, so it is 1e-16 relative, far below u) and a backward that
is more accurate than this contract (ds formed directly).  The CPU test asserts exactly that instead of pretending otherwise.
"""

from __future__ import annotations

import math
import types

import torch

from _mhsa_ref import BF16, BF16_STORE, EPS32, F32, F32_FACTOR, U, check, fails, gamma  # noqa: F401  (re-exported)
from _raw_rows_ref import degree_graph

U_EDGES = 4  # the kernels' gather batch: one online rescale per chunk of four edges
# torch's f32 evaluation on the CPU against the f64 reference: worst fraction of the DERIVED roundoff bound (measure_torch_f32)
TORCH_F32 = {"out": 0.0704, "t": 0.05707, "lse": 0.08237, "dq": 0.02697, "du": 0.02734, "dk": 0.04467, "dv": 0.1857,
             "dattr": 0.05678}


def name(dtype) -> str:
    return "f32" if dtype == F32 else "bf16"


# ------------------------------------------------------------------------------------------------ segments
def seg_sum(x, idx, n):
    return torch.zeros((n,) + tuple(x.shape[1:]), dtype=x.dtype).index_add_(0, idx, x)


def seg_max(x, idx, n, init=float("-inf")):
    out = torch.full((n,) + tuple(x.shape[1:]), init, dtype=x.dtype)
    if x.shape[0] == 0:
        return out
    return out.scatter_reduce(0, idx.view(-1, *([1] * (x.dim() - 1))).expand_as(x), x, "amax", include_self=True)


# ------------------------------------------------------------------------------------------------ the operation
def Problem(q, k, v, xr, u, attr, rowptr, col, h, up):
    """The operands as stored (any float dtype; ``attr`` f32 [E, up] in CSR order), with the graph expanded."""
    n_dst, c = q.shape
    deg = (rowptr[1:] - rowptr[:-1]).long()
    dst = torch.repeat_interleave(torch.arange(n_dst), deg)
    src = col.long()
    odeg = torch.bincount(src, minlength=k.shape[0])
    return types.SimpleNamespace(q=q, k=k, v=v, xr=xr, u=u, attr=attr, rowptr=rowptr, col=col, h=h, up=up, d=c // h, c=c,
                                 n_dst=n_dst, n_src=k.shape[0], deg=deg, odeg=odeg, dst=dst, src=src, dtype=q.dtype,
                                 n_edges=int(src.shape[0]))


def _heads(x, h, dt):
    return x.to(dt).reshape(x.shape[0], h, x.shape[1] // h)


def evaluate(p, dt=torch.float64, scale=None, edge_weight=None):
    """The forward expressions of the module docstring in dtype ``dt``.  ``out`` [n_dst, C], ``t`` [n_dst, H up], ``lse``
    [n_dst, H], and what the bounds and the backward need.  ``edge_weight`` [E]: multiplicity of every edge (mutants)."""
    h, n = p.h, p.n_dst
    q, k, v, uu = _heads(p.q, h, dt), _heads(p.k, h, dt), _heads(p.v, h, dt), _heads(p.u, h, dt)
    a = p.attr.to(dt)
    c = (1.0 / math.sqrt(p.d)) if scale is None else scale
    kj, vj, qi, ui = k[p.src], v[p.src], q[p.dst], uu[p.dst]
    s = ((qi * kj).sum(-1) + (ui * a[:, None, :]).sum(-1)) * c  # [E, H]
    if edge_weight is not None:
        s = s + torch.log(edge_weight.to(dt))[:, None]
    m = seg_max(s, p.dst, n)
    ex = torch.exp(s - m[p.dst])
    l = seg_sum(ex, p.dst, n)
    alpha = ex / (l[p.dst] + 1e-16)
    attn = seg_sum(alpha[:, :, None] * vj, p.dst, n).reshape(n, p.c)
    t = seg_sum(alpha[:, :, None] * a[:, None, :], p.dst, n).reshape(n, h * p.up)
    out = attn if p.xr is None else attn + p.xr.to(dt)
    lse = m + torch.log(l + 1e-16)  # (-inf for a destination without in-edges)
    r = types.SimpleNamespace(out=out, t=t, lse=lse, attn=attn, alpha=alpha, s=s, c=c, q=q, k=k, v=v, u=uu, a=a)
    if dt == torch.float64:
        r.A = seg_sum(alpha[:, :, None] * vj.abs(), p.dst, n).reshape(n, p.c)
        r.At = seg_sum(alpha[:, :, None] * a.abs()[:, None, :], p.dst, n).reshape(n, h * p.up)
        sabs = ((qi.abs() * kj.abs()).sum(-1) + (ui.abs() * a.abs()[:, None, :]).sum(-1)) * abs(c)
        r.M = seg_max(sabs, p.dst, n, init=0.0)
    return r


def evaluate_backward(p, f, dout, dtt, dt=torch.float64, alpha=None):
    """The backward expressions in dtype ``dt`` in the kernels' form (dq = c (A - Dsum B)); ``f`` = ``evaluate(p, dt)``;
    ``alpha`` replaces the forward's weights (the emulation hands in the ones rebuilt from a perturbed lse)."""
    h, n = p.h, p.n_dst
    do, dth = _heads(dout, h, dt), _heads(dtt, h, dt)
    al = f.alpha if alpha is None else alpha
    kj, vj, qi = f.k[p.src], f.v[p.src], f.q[p.dst]
    a3 = f.a[:, None, :]
    da = (do[p.dst] * vj).sum(-1) + (dth[p.dst] * a3).sum(-1)
    w = al * da
    dsum = seg_sum(w, p.dst, n)
    ds = w - al * dsum[p.dst]
    big_a, big_b = seg_sum(w[:, :, None] * kj, p.dst, n), seg_sum(al[:, :, None] * kj, p.dst, n)
    dq = ((big_a - dsum[:, :, None] * big_b) * f.c).reshape(n, p.c)
    au, bu = seg_sum(w[:, :, None] * a3, p.dst, n), seg_sum(al[:, :, None] * a3, p.dst, n)
    du = ((au - dsum[:, :, None] * bu) * f.c).reshape(n, h * p.up)
    dk = (seg_sum(ds[:, :, None] * qi, p.src, p.n_src) * f.c).reshape(p.n_src, p.c)
    dv = seg_sum(al[:, :, None] * do[p.dst], p.src, p.n_src).reshape(p.n_src, p.c)
    dattr = (f.c * ds[:, :, None] * f.u[p.dst] + al[:, :, None] * dth[p.dst]).sum(1)
    return types.SimpleNamespace(dq=dq, du=du, dk=dk, dv=dv, dattr=dattr, da=da, w=w, dsum=dsum, ds=ds, do=do, dth=dth,
                                 dxr=dout.to(dt))


# ------------------------------------------------------------------------------------------------ bounds
def eta(p, f):
    return gamma(p.d + p.up + 12) * f.M + 2.0 * EPS32


def _store(want, b32, dtype):
    return b32 + BF16_STORE * (want.abs() + b32) if dtype == BF16 else b32


def _per_head(x, width):
    """[n, H] -> [n, H width]."""
    return x[:, :, None].expand(x.shape[0], x.shape[1], width).reshape(x.shape[0], -1)


def forward_derived(p, f):
    """The roundoff of the f32 results in front of the x_r add and the store: (E32 out, E32 t, lse bound)."""
    deg = p.deg.double()[:, None]
    eps = eta(p, f) + gamma(deg + torch.floor(deg / U_EDGES) + 4)
    rel = eps / (1.0 - eps)
    e_out = _per_head(rel, p.d) * (f.A + f.attn.abs())
    e_t = _per_head(rel, p.up) * (f.At + f.t.abs())
    eps_l = eps + torch.ceil(deg / U_EDGES) * EPS32 + gamma(8) * f.M
    lse_abs = torch.where(torch.isfinite(f.lse), f.lse.abs(), torch.zeros_like(f.lse))
    e_lse = eps_l / (1.0 - eps_l) + 4.0 * EPS32 * (lse_abs + f.M)
    return e_out, e_t, e_lse


def forward_bounds(p, f, dtype=None):
    """(out bound [n_dst, C], t bound [n_dst, H up], lse bound [n_dst, H]) of a kernel that stores ``dtype``."""
    dtype = p.dtype if dtype is None else dtype
    e_out, e_t, e_lse = forward_derived(p, f)
    e_out, e_t, e_lse = (e_out * (F32_FACTOR * TORCH_F32["out"]), e_t * (F32_FACTOR * TORCH_F32["t"]),
                         e_lse * (F32_FACTOR * TORCH_F32["lse"]))
    if p.xr is not None:
        e_out = e_out + U * (f.out.abs() + e_out)
    return _store(f.out, e_out, dtype), _store(f.t, e_t, dtype), e_lse


def check_lse(got, want, bound, what) -> float:
    """lse per element: -inf exactly where the destination has no in-edge, inside the bound elsewhere."""
    got = got.detach().cpu().double()
    iso = torch.isinf(want) & (want < 0)
    assert bool((got[iso] == float("-inf")).all()), f"{what}: lse of a destination without in-edges is not -inf"
    if bool((~iso).any()):
        return check(got[~iso], want[~iso], bound[~iso], what)
    return 0.0


def lse_fails(got, want, bound) -> bool:
    got = got.detach().double()
    iso = torch.isinf(want) & (want < 0)
    return not bool((got[iso] == float("-inf")).all()) or fails(got[~iso], want[~iso], bound[~iso])


def _backward_derived(p, f, b, lse_err):
    h, n = p.h, p.n_dst
    x = eta(p, f) + lse_err
    relp_n = x / (1.0 - x)  # [n, H]
    relp = relp_n[p.dst]  # [E, H]
    al = f.alpha
    kj, vj, qi = f.k[p.src].abs(), f.v[p.src].abs(), f.q[p.dst].abs()
    a3 = f.a.abs()[:, None, :]
    do, dth = b.do.abs(), b.dth.abs()
    deg = p.deg.double()[:, None]
    odeg = p.odeg.double()[:, None]
    eda = gamma(p.d + p.up + 4) * ((do[p.dst] * vj).sum(-1) + (dth[p.dst] * a3).sum(-1))
    ew = b.w.abs() * (relp + U) + al * (1.0 + relp) * eda
    eds_n = seg_sum(ew, p.dst, n) + gamma(deg) * seg_sum(b.w.abs() + ew, p.dst, n)  # [n, H]
    g2 = gamma(deg + 2)[:, :, None]

    def dst_side(xj):  # xj [E, H, width] absolute values of what is summed (k_j or a_e)
        aabs, babs = seg_sum(b.w.abs()[:, :, None] * xj, p.dst, n), seg_sum(al[:, :, None] * xj, p.dst, n)
        ea = seg_sum(ew[:, :, None] * xj, p.dst, n) + g2 * seg_sum((b.w.abs() + ew)[:, :, None] * xj, p.dst, n)
        eb = relp_n[:, :, None] * babs + g2 * (1.0 + relp_n[:, :, None]) * babs
        dsa, edsn = b.dsum.abs()[:, :, None], eds_n[:, :, None]
        e = ea + edsn * (babs + eb) + dsa * eb + 4.0 * U * (aabs + ea + (dsa + edsn) * (babs + eb))
        return (abs(f.c) * e).reshape(n, -1)

    bdq = dst_side(kj)
    bdu = dst_side(a3.expand(-1, h, -1))
    eds = ew + al * relp * b.dsum.abs()[p.dst] + al * (1.0 + relp) * eds_n[p.dst] + U * (b.w.abs() + al * b.dsum.abs()[p.dst])
    go2, go1 = gamma(odeg + 2)[:, :, None], gamma(odeg + 1)[:, :, None]
    bdk = abs(f.c) * (seg_sum(eds[:, :, None] * qi, p.src, p.n_src) + go2 * seg_sum((b.ds.abs() + eds)[:, :, None] * qi, p.src, p.n_src))
    bdv = seg_sum((al * relp)[:, :, None] * do[p.dst], p.src, p.n_src) + go1 * seg_sum((al * (1.0 + relp))[:, :, None] * do[p.dst], p.src, p.n_src)
    ui = f.u[p.dst].abs()
    bda = (abs(f.c) * eds[:, :, None] * ui + (al * relp)[:, :, None] * dth[p.dst]).sum(1) + gamma(2 * h + 2) * (
        abs(f.c) * (b.ds.abs() + eds)[:, :, None] * ui + (al * (1.0 + relp))[:, :, None] * dth[p.dst]).sum(1)
    return {"dq": bdq, "du": bdu, "dk": bdk.reshape(p.n_src, p.c), "dv": bdv.reshape(p.n_src, p.c), "dattr": bda}


BACKWARD_KEYS = ("dq", "du", "dk", "dv", "dattr")


def backward_bounds(p, f, b, lse_err, dtype=None):
    """{dq, du, dk, dv, dattr}: bounds; ``lse_err`` [n_dst, H] >= |lse_stored - lse| (0 for isolated destinations)."""
    dtype = p.dtype if dtype is None else dtype
    full = _backward_derived(p, f, b, lse_err)
    base = _backward_derived(p, f, b, torch.zeros_like(lse_err))
    out = {}
    for key in BACKWARD_KEYS:
        e = base[key] * (F32_FACTOR * TORCH_F32[key]) + (full[key] - base[key])
        out[key] = e if key == "dattr" else _store(getattr(b, key), e, dtype)
    return out


def finite_lse_err(e_lse, lse):
    return torch.where(torch.isfinite(lse), e_lse, torch.zeros_like(e_lse))


# ------------------------------------------------------------------------------------------------ graphs
REQUIRED_DEGREES = (0, 1, 2, 3, 4, 5, 7, 8, 9, 16, 45)
N_SRC = 40
IDLE_SRC = N_SRC - 1  # a source without out-edges
HUB_SRC = (0, 1)  # sources of out-degree >= 5 (0: shared by most destinations)


def irregular_degrees(n_dst: int, seed: int):
    """The required degrees in a seeded order, filled up to ``n_dst`` with degrees 0 ... 10; the last destination isolated."""
    g = torch.Generator().manual_seed(1000 + seed)
    extra = torch.randint(0, 11, (max(n_dst - len(REQUIRED_DEGREES) - 1, 0),), generator=g).tolist()
    deg = list(REQUIRED_DEGREES) + extra
    order = torch.randperm(len(deg), generator=g).tolist()
    return [deg[i] for i in order] + [0]


def make_graph(kind: str, seed: int = 0):
    """(rowptr int32, col int32, n_src).  "irr": 24 ... 40 destinations with every required in-degree; "n1" / "n5" / "n9": that many
    destinations (fewer than XCDs: some of the kernels' destination ranges are empty); "e0": five destinations, no edge;
    "deg3": 1024 destinations of in-degree 3 whose source triples are shared (groups of 8 and more, one single destination)."""
    if kind == "deg3":
        return _deg3_graph(seed)
    if kind == "e0":
        return torch.zeros(6, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), N_SRC
    degs = {"irr": irregular_degrees(28 + 4 * (seed % 4), seed), "n1": [9], "n5": [5, 0, 45, 1, 4], "n9": [3, 16, 0, 8, 1, 45, 7, 2, 0]}[kind]
    rowptr, col, _ = degree_graph(degs, N_SRC - 1, 77 + seed)  # (never the idle source)
    col = col.clone()
    for i, dg in enumerate(degs):
        e0 = int(rowptr[i])
        if dg >= 2 and i % 2 == 0:
            col[e0 + 1] = HUB_SRC[0]  # (position 1: the first edges stay distinct, a foreign first edge shows)
        if dg >= 3 and i % 2 == 1:
            col[e0 + dg - 1] = HUB_SRC[1]
    return rowptr, col, N_SRC


def _deg3_graph(seed: int):
    """Blocks of 2, 3, 2, 4 consecutive destinations with one source triple (b, b + 7, b + 31) each (runs of two for the run
    kernel); the triples repeat every 30 blocks, so a triple's ~34 destinations lie apart in the order (groups of 8 for the group
    kernel); the last destination has a triple of its own.  Every destination lists its triple in an order of its own."""
    n, n_src = 1024, 64
    g = torch.Generator().manual_seed(4000 + seed)
    base, i = [], 0
    while len(base) < n - 1:
        base += [i % 30] * (2, 3, 2, 4)[i % 4]
        i += 1
    base = torch.tensor(base[:n - 1] + [31])
    tri = torch.stack([base, base + 7, base + 31], 1)
    order = torch.stack([torch.randperm(3, generator=g) for _ in range(n)])
    col = torch.gather(tri, 1, order).reshape(-1).int()
    return torch.arange(0, 3 * n + 1, 3, dtype=torch.int32), col, n_src


def canonical_order(rowptr, col):
    """Permutation of the CSR positions that sorts every destination's in-edges by ascending source (stable): the order in
    which the group and run kernels of uniform-degree-3 graphs sum."""
    n = rowptr.shape[0] - 1
    dst = torch.repeat_interleave(torch.arange(n), (rowptr[1:] - rowptr[:-1]).long())
    return torch.argsort(dst * (int(col.max()) + 1) + col.long(), stable=True)


# ------------------------------------------------------------------------------------------------ data sets
DATA = ("flat", "spread", "late_max", "cold", "residual")
RESIDUAL_SCALE = 64.0
COLD_LEVEL = -12.0


def _seed(kind, c):
    base = DATA.index(kind) + 1 if kind in DATA else 9
    return ((base * 1009 + c.d) * 1013 + c.h) * 1019 + c.up * 7 + (0 if c.dtype == F32 else 3) + 31 * c.gseed


def late_max_position(deg: int, i: int) -> int:
    """Where destination i of in-degree ``deg`` carries its largest score: the last in-edge (odd i), the first edge of the last
    chunk of four (even i)."""
    return deg - 1 if i % 2 else (deg - 1) // U_EDGES * U_EDGES


def make_problem(c):
    """The operands of case ``c`` as stored: built in f64 from the case's seed, then cast (attributes f32)."""
    rowptr, col, n_src = make_graph(c.graph, c.gseed)
    n_dst, e = rowptr.shape[0] - 1, col.shape[0]
    h, d, up = c.h, c.d, c.up
    cc = h * d
    g = torch.Generator().manual_seed(_seed(c.data, c))
    f64 = torch.float64

    def uni(*shape):
        return torch.rand(*shape, generator=g, dtype=f64) * 2.0 - 1.0

    if c.data == "spread":
        q = torch.randn(n_dst, cc, generator=g, dtype=f64) * 1.6
        k = torch.randn(n_src, cc, generator=g, dtype=f64)
        u = torch.randn(n_dst, h * up, generator=g, dtype=f64) * 0.3
        attr = torch.randn(e, up, generator=g, dtype=f64)
    else:
        amp = 0.7 / d ** 0.25
        q, k = uni(n_dst, cc) * amp, uni(n_src, cc) * amp
        u = uni(n_dst, h * up) * 0.3
        attr = uni(e, up)
    v = torch.randn(n_src, cc, generator=g, dtype=f64)
    xr = torch.randn(n_dst, cc, generator=g, dtype=f64)
    if e:
        attr[:, up - 1] = 1.0  # the constant-1 column (the bias carrier)
    if c.data == "residual":
        xr = xr * RESIDUAL_SCALE
    if c.data == "cold":
        u.view(n_dst, h, up)[:, :, up - 1] = -float(math.ceil(15.0 * math.sqrt(d)))  # (an integer <= 256: a bf16 number)
    if c.data == "late_max":
        u.view(n_dst, h, up)[:, :, 0] = 2.0
        deg = (rowptr[1:] - rowptr[:-1]).tolist()
        for i, dg in enumerate(deg):
            if dg >= 2:
                nats = 20.0 + 40.0 * ((i * 7) % 11) / 10.0
                attr[int(rowptr[i]) + late_max_position(dg, i), 0] = round(nats * math.sqrt(d) / 2.0 * 4.0) / 4.0
    cast = lambda x: x.to(c.dtype)  # noqa: E731
    return Problem(cast(q), cast(k), cast(v), cast(xr) if c.xr else None, cast(u), attr.float(), rowptr, col, h, up)


def make_grads(c, p):
    g = torch.Generator().manual_seed(_seed("grads", c))
    dout = torch.randn(p.n_dst, p.c, generator=g, dtype=torch.float64).to(c.dtype)
    dtt = torch.randn(p.n_dst, p.h * p.up, generator=g, dtype=torch.float64).to(c.dtype)
    return dout, dtt


# ------------------------------------------------------------------------------------------------ dispatch restated
def vec(dtype) -> int:
    return 4 if dtype == F32 else 8


def lanes_per_head(dtype, d: int) -> int:
    return d // vec(dtype)


def attrs_per_lane(up: int, lph: int) -> int:
    """edge_common.hpp::attrs_per_lane."""
    raw = -(-up // lph)
    for a in (2, 4, 8, 12, 16):
        if a >= raw and up % a == 0:
            return a
    return up


def n_slices(dtype, c: int) -> int:
    return -(-c // (64 * vec(dtype)))


def plain_kernel(dtype, d: int, up: int, xr: bool) -> str:
    """The instantiation the plain launcher takes (dispatch_folded / launch_folded); raises where there is none."""
    lph = lanes_per_head(dtype, d)
    if d % vec(dtype) or lph not in (1, 2, 4, 8, 16) or up not in (4, 8, 12, 16):
        raise ValueError("no instantiation")
    no_xr = dtype == BF16 and not xr
    return f"folded<{name(dtype)},LPH={lph},UP={up},APL={attrs_per_lane(up, lph)},XR={'false' if no_xr else 'true'}>"


def list_kernel_shape(dtype, d: int, up: int, n_dst: int) -> bool:
    return dtype == BF16 and d in (32, 64) and up in (4, 8, 12, 16) and n_dst != 0


ENTRY = {"plain": "anemoi_gt_edge_attention_folded", "groups": "anemoi_gt_edge_attention_folded_groups",
         "runs": "anemoi_gt_edge_attention_folded_runs", "tiles": "anemoi_gt_edge_attention_folded_tiles",
         "sched": "anemoi_gt_edge_attention_folded_sched"}


# ------------------------------------------------------------------------------------------------ cases
def Case(dtype, d, h, up, data, graph="irr", xr=True, lse=True, gseed=0, route="plain", pad_out=False):
    return types.SimpleNamespace(dtype=dtype, d=d, h=h, up=up, data=data, graph=graph, xr=xr, lse=lse, gseed=gseed,
                                 route=route, pad_out=pad_out)


def case_id(c) -> str:
    t = f"{name(c.dtype)}-D{c.d}-H{c.h}-UP{c.up}-{c.data}-{c.graph}{c.gseed}"
    t += "" if c.xr else "-noxr"
    t += "" if c.lse else "-nolse"
    t += "-padK" if c.pad_out else ""
    return t + ("" if c.route == "plain" else f"-{c.route}")


F32_D, BF16_D, UPS = (4, 8, 16, 32, 64), (8, 16, 32, 64, 128), (4, 8, 12, 16)
MULTI_SLICE = ((F32, 64, 5), (BF16, 64, 9), (BF16, 64, 16), (BF16, 32, 16))  # C = 320, 576, 1024, 512


def plain_instantiation_cases():
    """Every instantiation of the plain kernel, H = 3 (one slice), x_r on: 40 shapes, ``flat`` and ``spread`` alternating so
    that every D and every UP meets both."""
    out = []
    for dtype, ds in ((F32, F32_D), (BF16, BF16_D)):
        for i, d in enumerate(ds):
            for j, up in enumerate(UPS):
                out.append(Case(dtype, d, 3, up, ("flat", "spread")[(i + j) % 2], gseed=(i + j) % 4))
    return out


def plain_further_cases():
    out = [Case(BF16, 64, 3, 12, "flat", xr=False), Case(F32, 16, 3, 12, "flat", xr=False),  # XR = false / x_r == nullptr
           Case(BF16, 32, 3, 8, "flat", lse=False), Case(F32, 8, 3, 4, "spread", lse=False)]
    for dtype, d, h in MULTI_SLICE:
        out += [Case(dtype, d, h, 12, "flat", gseed=1), Case(dtype, d, h, 16, "spread", gseed=2)]
    for graph in ("n1", "n5", "n9", "e0"):
        out += [Case(BF16, 64, 3, 12, "flat", graph=graph), Case(F32, 16, 3, 8, "flat", graph=graph)]
    for data in ("late_max", "cold", "residual"):
        out += [Case(BF16, 64, 3, 12, data), Case(BF16, 16, 3, 16, data, gseed=3), Case(F32, 32, 3, 4, data, gseed=1),
                Case(F32, 4, 3, 12, data, gseed=2)]
    out += [Case(BF16, 64, 3, 12, "flat", pad_out=True), Case(F32, 16, 3, 12, "flat", pad_out=True)]
    return out


def list_cases():
    """bf16 D = 64 with C = 1024 and D = 32 with C = 512; one C = 128 case for the sched kernel (and the tile kernel's one slice)."""
    out = []
    for d, h in ((64, 16), (32, 16)):
        for route in ("sched", "tiles"):
            out += [Case(BF16, d, h, 12, "flat", gseed=1, route=route), Case(BF16, d, h, 16, "spread", gseed=2, route=route)]
        for route in ("groups", "runs"):
            out += [Case(BF16, d, h, 12, "flat", graph="deg3", route=route), Case(BF16, d, h, 4, "spread", graph="deg3", route=route, xr=False)]
    out += [Case(BF16, 32, 4, 8, "flat", gseed=3, route="sched"), Case(BF16, 32, 4, 4, "flat", gseed=3, route="tiles")]
    return out


def backward_cases():
    """f32 D in {4, 16, 64}, bf16 D in {8, 32, 64, 128}, UP in {4, 12, 16}; one multi-slice case each; the four data sets."""
    out = []
    datas = ("flat", "spread", "residual", "late_max")
    i = 0
    for dtype, ds in ((F32, (4, 16, 64)), (BF16, (8, 32, 64, 128))):
        for d in ds:
            for up in (4, 12, 16):
                out.append(Case(dtype, d, 3, up, datas[i % 4], gseed=i % 4))
                i += 1
    out += [Case(F32, 64, 5, 12, "flat", gseed=1), Case(BF16, 64, 9, 12, "flat", gseed=1)]
    # H = 4: H up is a multiple of 16 bytes in bf16 for every UP, so these also run through autograd.gt_edge_attention
    out += [Case(BF16, 8, 4, 4, "flat", gseed=2), Case(BF16, 32, 4, 12, "spread", gseed=3), Case(BF16, 64, 4, 4, "residual", gseed=3)]
    out += [Case(BF16, 64, 3, 12, "flat", graph=graph) for graph in ("n1", "n5")]
    return out


F32_MEASURE_CASES = [Case(F32, d, 3, up, data, gseed=s) for d, up, s in ((4, 12, 0), (16, 4, 1), (32, 16, 2), (64, 8, 3))
                     for data in ("flat", "spread", "late_max", "cold")]


def measure_torch_f32():
    """Worst fraction of the DERIVED roundoff bounds that torch's f32 evaluation of the same expressions uses (TORCH_F32)."""
    worst = {key: 0.0 for key in TORCH_F32}

    def frac(got, want, bound):
        diff = (got.double() - want).abs()
        r = torch.where(diff == 0, torch.zeros_like(diff), diff / bound)
        return float(r[torch.isfinite(want)].max()) if bool(torch.isfinite(want).any()) else 0.0

    for c in F32_MEASURE_CASES:
        p = make_problem(c)
        dout, dtt = make_grads(c, p)
        f = evaluate(p)
        b = evaluate_backward(p, f, dout, dtt)
        f32 = evaluate(p, torch.float32)
        b32 = evaluate_backward(p, f32, dout, dtt, torch.float32)
        e_out, e_t, e_lse = forward_derived(p, f)
        base = _backward_derived(p, f, b, torch.zeros_like(e_lse))
        pairs = {"out": (f32.attn, f.attn, e_out), "t": (f32.t, f.t, e_t), "lse": (f32.lse, f.lse, e_lse)}
        pairs.update({key: (getattr(b32, key), getattr(b, key), base[key]) for key in BACKWARD_KEYS})
        for key, (got, want, bound) in pairs.items():
            worst[key] = max(worst[key], frac(got, want, bound))
    return worst


# ------------------------------------------------------------------------------------------------ explicit-edge conv, forward
# ``ops.gt_conv`` (gt_conv_kernel): the per-edge features e_e [E, C] (CSR order) are given and added to BOTH k and v:
#     k'_e = k_j + e_e,  v'_e = v_j + e_e,  s_e = c q_i . k'_e,  alpha as above (+ 1e-16),  out_i = sum_e alpha_e kk_e v'_e (+ x_r),
#     kk_e,h = keep_e,h / (1 - p) (dropout: the kernels' keep mask over the CSR positions, tests/_cpu_ops.py::edge_dropout_keep_mask;
#     the normaliser and lse see every edge),  lse = m + log(l + 1e-16).
# Bounds, as for the folded kernel with these differences: k' and v' are formed in f32 (one rounding each, exact for most bf16
# pairs), so the D products are not exact and the score takes D FMAs: eta = gamma(D + 13) M' + 2 EPS32 with M' = c max_e sum |q||k'|;
# the online maximum rescales at EVERY edge (l = l corr + pe, acc = fma(pv, v', acc corr)): two roundings per edge, one for v'
# and one for pv = pe kk:  eps = eta + gamma(2 deg + 6),  E32 = eps / (1 - eps) (A + |attn|),  A = sum_e alpha_e kk_e |v'_e|;
# lse: a rescale factor per edge,  eps_lse = eps + deg EPS32 + gamma(8) M'.  p = 1: A = 0, out is x_r exactly.
TORCH_F32_CONV = {"out": 0.05802, "lse": 0.06068}
CONV_SEED = 20240917


def ConvProblem(q, k, v, e, xr, rowptr, col, h):
    p = Problem(q, k, v, xr, None, None, rowptr, col, h, 0)
    p.e = e
    return p


def evaluate_conv(p, dt=torch.float64, keep=None, pdrop=0.0, e_in_v=True):
    """The conv's forward expressions in dtype ``dt``; ``keep`` [E, H] of 0 / 1 with ``pdrop``; ``e_in_v=False``: the mutant that
    adds the edge features to k alone."""
    h, n = p.h, p.n_dst
    q, k, v, e = _heads(p.q, h, dt), _heads(p.k, h, dt), _heads(p.v, h, dt), _heads(p.e, h, dt)
    c = 1.0 / math.sqrt(p.d)
    kj = k[p.src] + e
    vj = v[p.src] + e if e_in_v else v[p.src]
    s = (q[p.dst] * kj).sum(-1) * c
    m = seg_max(s, p.dst, n)
    ex = torch.exp(s - m[p.dst])
    l = seg_sum(ex, p.dst, n)
    alpha = ex / (l[p.dst] + 1e-16)
    kk = torch.ones_like(alpha) if keep is None else keep.to(dt) * (1.0 / (1.0 - pdrop) if pdrop < 1.0 else 0.0)
    attn = seg_sum((alpha * kk)[:, :, None] * vj, p.dst, n).reshape(n, p.c)
    out = attn if p.xr is None else attn + p.xr.to(dt)
    r = types.SimpleNamespace(out=out, attn=attn, lse=m + torch.log(l + 1e-16), alpha=alpha, s=s, kk=kk)
    if dt == torch.float64:
        r.A = seg_sum((alpha * kk)[:, :, None] * vj.abs(), p.dst, n).reshape(n, p.c)
        r.M = seg_max((q[p.dst].abs() * kj.abs()).sum(-1) * c, p.dst, n, init=0.0)
    return r


def conv_forward_derived(p, f):
    deg = p.deg.double()[:, None]
    eps = gamma(p.d + 13) * f.M + 2.0 * EPS32 + gamma(2.0 * deg + 6)
    e_out = _per_head(eps / (1.0 - eps), p.d) * (f.A + f.attn.abs())
    eps_l = eps + deg * EPS32 + gamma(8) * f.M
    lse_abs = torch.where(torch.isfinite(f.lse), f.lse.abs(), torch.zeros_like(f.lse))
    return e_out, eps_l / (1.0 - eps_l) + 4.0 * EPS32 * (lse_abs + f.M)


def conv_forward_bounds(p, f):
    e_out, e_lse = conv_forward_derived(p, f)
    e_out, e_lse = e_out * (F32_FACTOR * TORCH_F32_CONV["out"]), e_lse * (F32_FACTOR * TORCH_F32_CONV["lse"])
    if p.xr is not None:
        e_out = e_out + U * (f.out.abs() + e_out)
    return _store(f.out, e_out, p.dtype), e_lse


def make_conv_problem(c):
    """q, k, v, x_r and the graph of ``make_problem``; the edge features from a seed of their own, of k's magnitude."""
    p = make_problem(c)
    g = torch.Generator().manual_seed(_seed("grads", c) + 17)
    if c.data == "spread":
        e = torch.randn(p.n_edges, p.c, generator=g, dtype=torch.float64)
    else:
        e = (torch.rand(p.n_edges, p.c, generator=g, dtype=torch.float64) * 2.0 - 1.0) * (0.7 / c.d ** 0.25)
    return ConvProblem(p.q, p.k, p.v, e.to(c.dtype), p.xr, p.rowptr, p.col, p.h)


def conv_cases():
    """f32 D = 4 and 32, bf16 D = 8 and 64 (H = 3), ``flat`` and ``spread``; each at p = 0, 0.25 and 1 (ConvCase.p)."""
    out = []
    for dtype, d in ((F32, 4), (F32, 32), (BF16, 8), (BF16, 64)):
        for i, pd in enumerate((0.0, 0.25, 1.0)):
            c = Case(dtype, d, 3, 4, ("flat", "spread")[i % 2], gseed=i + 1)
            c.p = pd
            out.append(c)
    out += [Case(BF16, 64, 3, 4, "flat", graph="n5"), Case(F32, 32, 3, 4, "flat", graph="n1")]
    out[-2].p, out[-1].p = 0.25, 0.0
    return out


def conv_case_id(c) -> str:
    return f"conv-{name(c.dtype)}-D{c.d}-{c.data}-{c.graph}{c.gseed}-p{c.p}"


def measure_torch_f32_conv():
    worst = {"out": 0.0, "lse": 0.0}
    for c in [Case(F32, d, 3, 4, data, gseed=s) for d, s in ((4, 0), (16, 1), (32, 2), (64, 3)) for data in ("flat", "spread")]:
        p = make_conv_problem(c)
        f, f32 = evaluate_conv(p), evaluate_conv(p, torch.float32)
        e_out, e_lse = conv_forward_derived(p, f)
        for key, got, want, bound in (("out", f32.attn, f.attn, e_out), ("lse", f32.lse, f.lse, e_lse)):
            diff = (got.double() - want).abs()
            r = torch.where(diff == 0, torch.zeros_like(diff), diff / bound)
            worst[key] = max(worst[key], float(r[torch.isfinite(want)].max()))
    return worst


# ------------------------------------------------------------------------------------------------ explicit-edge conv, backward
# ``autograd.gt_conv`` (gt_conv_bwd_dst_kernel, gt_conv_bwd_src_kernel).  With k' = k_j + e_e, v' = v_j + e_e, kk = keep / (1 - p):
#     da_e = dout_i . v'_e,   w_e = alpha_e kk_e da_e,   Dsum_i = sum_e w_e,   ds_e = w_e - alpha_e Dsum_i,
#     dq_i = c (sum_e w_e k'_e - Dsum_i sum_e alpha_e k'_e),   dk_j = c sum_{e from j} ds_e q_i,   dv_j = sum_{e from j} alpha_e kk_e dout_i,
#     d e_e = c ds_e q_i + alpha_e kk_e dout_i   (the per-edge terms of dk and dv),   d x_r = dout.
# Bounds: the folded backward's, term for term, with relP from the conv's eta (gamma(D + 13) M' + 2 EPS32 + lse_err), one more
# rounding in every dot product and sum for k' / v' formed in f32 and for the product with kk, no attribute terms, and
#     d e_e:  c Eds |q| + alpha kk (relP + U) |dout| + 3 U (c (|ds| + Eds) |q| + alpha kk (1 + relP) |dout|)      then the store.
# p = 1: every term vanishes, the gradients are exact zeros.
CONV_BACKWARD_KEYS = ("dq", "dk", "dv", "de")
TORCH_F32_CONV_BWD = {"dq": 0.06241, "dk": 0.07738, "dv": 0.2233, "de": 0.2565}


def evaluate_conv_backward(p, f, dout, dt=torch.float64, alpha=None):
    h, n = p.h, p.n_dst
    q, k, v, e, do = (_heads(x, h, dt) for x in (p.q, p.k, p.v, p.e, dout))
    c = 1.0 / math.sqrt(p.d)
    al = f.alpha.to(dt) if alpha is None else alpha
    kk = f.kk.to(dt)
    kj, vj, qi, doi = k[p.src] + e, v[p.src] + e, q[p.dst], do[p.dst]
    da = (doi * vj).sum(-1)
    w = al * kk * da
    dsum = seg_sum(w, p.dst, n)
    ds = w - al * dsum[p.dst]
    dq = ((seg_sum(w[:, :, None] * kj, p.dst, n) - dsum[:, :, None] * seg_sum(al[:, :, None] * kj, p.dst, n)) * c).reshape(n, p.c)
    gk, gv = (c * ds)[:, :, None] * qi, (al * kk)[:, :, None] * doi
    dk, dv = seg_sum(gk, p.src, p.n_src).reshape(p.n_src, p.c), seg_sum(gv, p.src, p.n_src).reshape(p.n_src, p.c)
    return types.SimpleNamespace(dq=dq, dk=dk, dv=dv, de=(gk + gv).reshape(p.n_edges, p.c), w=w, dsum=dsum, ds=ds, da=da, c=c,
                                 kj=kj, vj=vj, qi=qi, doi=doi, al=al, kk=kk)


def _conv_backward_derived(p, f, b, lse_err):
    n, c = p.n_dst, b.c
    x = gamma(p.d + 13) * f.M + 2.0 * EPS32 + lse_err
    relp_n = x / (1.0 - x)
    relp = relp_n[p.dst]
    al, kk = b.al, b.kk
    kj, vj, qi, doi = b.kj.abs(), b.vj.abs(), b.qi.abs(), b.doi.abs()
    deg, odeg = p.deg.double()[:, None], p.odeg.double()[:, None]
    eda = gamma(p.d + 5) * (doi * vj).sum(-1)
    ew = b.w.abs() * (relp + 3.0 * U) + al * kk * (1.0 + relp) * eda
    eds_n = seg_sum(ew, p.dst, n) + gamma(deg) * seg_sum(b.w.abs() + ew, p.dst, n)
    g3 = gamma(deg + 3)[:, :, None]
    aabs, babs = seg_sum(b.w.abs()[:, :, None] * kj, p.dst, n), seg_sum(al[:, :, None] * kj, p.dst, n)
    ea = seg_sum(ew[:, :, None] * kj, p.dst, n) + g3 * seg_sum((b.w.abs() + ew)[:, :, None] * kj, p.dst, n)
    eb = relp_n[:, :, None] * babs + g3 * (1.0 + relp_n[:, :, None]) * babs
    dsa, edsn = b.dsum.abs()[:, :, None], eds_n[:, :, None]
    bdq = (c * (ea + edsn * (babs + eb) + dsa * eb + 4.0 * U * (aabs + ea + (dsa + edsn) * (babs + eb)))).reshape(n, p.c)
    eds = ew + al * relp * b.dsum.abs()[p.dst] + al * (1.0 + relp) * eds_n[p.dst] + 2.0 * U * (b.w.abs() + al * b.dsum.abs()[p.dst])
    go2 = gamma(odeg + 2)[:, :, None]
    egk = c * eds[:, :, None] * qi
    egv = (al * kk * (relp + U))[:, :, None] * doi
    mgk, mgv = c * (b.ds.abs() + eds)[:, :, None] * qi, (al * kk * (1.0 + relp))[:, :, None] * doi
    bdk = seg_sum(egk, p.src, p.n_src) + go2 * seg_sum(mgk, p.src, p.n_src)
    bdv = seg_sum(egv, p.src, p.n_src) + go2 * seg_sum(mgv, p.src, p.n_src)
    bde = egk + egv + 3.0 * U * (mgk + mgv)
    return {"dq": bdq, "dk": bdk.reshape(p.n_src, p.c), "dv": bdv.reshape(p.n_src, p.c), "de": bde.reshape(p.n_edges, p.c)}


def conv_backward_bounds(p, f, b, lse_err):
    full = _conv_backward_derived(p, f, b, lse_err)
    base = _conv_backward_derived(p, f, b, torch.zeros_like(lse_err))
    return {key: _store(getattr(b, key), base[key] * (F32_FACTOR * TORCH_F32_CONV_BWD[key]) + (full[key] - base[key]), p.dtype)
            for key in CONV_BACKWARD_KEYS}


def conv_keep(c, p):
    """The kernels' keep mask of a conv case (tests/_cpu_ops.py restates csrc/common.hpp::edge_dropout_keep)."""
    from _cpu_ops import edge_dropout_keep_mask

    return edge_dropout_keep_mask(CONV_SEED, c.p, p.n_edges, p.h) if c.p > 0.0 else None


def _conv_measure_cases():
    out = []
    for d, s in ((4, 0), (16, 1), (32, 2), (64, 3)):
        for data, pd in (("flat", 0.0), ("spread", 0.25)):
            c = Case(F32, d, 3, 4, data, gseed=s)
            c.p = pd
            out.append(c)
    return out


def measure_torch_f32_conv_backward():
    worst = {key: 0.0 for key in CONV_BACKWARD_KEYS}
    for c in _conv_measure_cases():
        p = make_conv_problem(c)
        keep = conv_keep(c, p)
        dout, _ = make_grads(c, p)
        f, f32 = evaluate_conv(p, keep=keep, pdrop=c.p), evaluate_conv(p, torch.float32, keep=keep, pdrop=c.p)
        b, b32 = evaluate_conv_backward(p, f, dout), evaluate_conv_backward(p, f32, dout, torch.float32)
        base = _conv_backward_derived(p, f, b, torch.zeros_like(f.lse))
        for key in CONV_BACKWARD_KEYS:
            diff = (getattr(b32, key).double() - getattr(b, key)).abs()
            worst[key] = max(worst[key], float(torch.where(diff == 0, torch.zeros_like(diff), diff / base[key]).max()))
    return worst


# ------------------------------------------------------------------------------------------------ unfolded kernel
# ``ops.gt_edge_attention`` (gt_edge_attention_kernel: fast path; gt_edge_attention_generic_kernel): e_e = W_e a_e + b (W_e [C, edge_dim],
# b [C], a_e the first edge_dim columns of the f32 attribute row) added to BOTH k and v, the softmax of the conv, out (+ x_r), no lse.
# The fast path never forms e: it scores with u = W_h^T q (D FMAs, a head reduction) and u . a, and finishes with
# out = (acc + b l + W t) / (l + 1e-16); the generic kernel forms e per edge and channel (edge_dim FMAs), k + e, v + e, and rescales at
# every edge.  One bound covers both, in the magnitudes either form sums:  E_e = |W_e| |a_e| + |b|,
#     M'' = c max_e sum_d |q| (|k| + E_e),   eta = gamma(2 D + edge_dim + 14) M'' + 2 EPS32,   A = sum_e alpha_e (|v_j| + E_e),
#     eps = eta + gamma(2 deg + edge_dim + 8),   E32 = eps / (1 - eps) (A + |attn|),   then the x_r add and the store as above.
TORCH_F32_UNFOLDED = {"out": 0.03739}


def unfolded_route(dtype, d: int, c: int, edge_dim: int, ea_ld: int, pitches_aligned: bool = True) -> str:
    """edge_attention_launch restated: "fast<LPH, EDP>" (">64K" where W_e in LDS needs the raised limit) or "generic"."""
    v = vec(dtype)
    edp = (edge_dim + 3) // 4 * 4
    lds = (edp + 1) * c * 4
    fast = (pitches_aligned and ea_ld % 4 == 0 and ea_ld >= edp and d % v == 0 and d // v in (1, 2, 4, 8, 16) and edp <= 16
            and lds <= 160 * 1024 and c % v == 0)
    if not fast:
        assert d <= 64
        return "generic"
    return f"fast<LPH={d // v},EDP={edp}>" + (">64K" if lds > 64 * 1024 else "")


def make_unfolded_problem(c):
    """q, k, v, x_r and the graph of ``make_problem``; W_e, b and the attribute rows ([E, EDP + 4]: zero in the pad columns the
    fast path multiplies by its zero weights, NaN in the four columns behind them) from a seed of their own."""
    p = make_problem(c)
    g = torch.Generator().manual_seed(_seed("grads", c) + 29 + c.edge_dim)
    edp = (c.edge_dim + 3) // 4 * 4
    a = torch.full((p.n_edges, edp + 4), float("nan"))
    a[:, :edp] = 0.0
    a[:, :c.edge_dim] = torch.rand(p.n_edges, c.edge_dim, generator=g) * 2.0 - 1.0
    scale = (0.7 / c.d ** 0.25 if c.data != "spread" else 1.0) / math.sqrt(c.edge_dim)
    w = (torch.randn(p.c, c.edge_dim, generator=g) * scale).float()
    b = (torch.randn(p.c, generator=g) * 0.1).float()
    q = ConvProblem(p.q, p.k, p.v, None, p.xr, p.rowptr, p.col, p.h)
    q.attr, q.w, q.b, q.edge_dim = a, w, b, c.edge_dim
    return q


def evaluate_unfolded(p, dt=torch.float64, e_in_v=True, bias=True):
    a = p.attr[:, :p.edge_dim].to(dt)
    p.e = a @ p.w.to(dt).T + (p.b.to(dt) if bias else 0.0)
    f = evaluate_conv(p, dt, e_in_v=e_in_v)
    if dt == torch.float64:
        h, n = p.h, p.n_dst
        eabs = _heads(a.abs() @ p.w.double().abs().T + p.b.double().abs(), h, dt)
        q, k, v = _heads(p.q, h, dt), _heads(p.k, h, dt), _heads(p.v, h, dt)
        f.M = seg_max((q[p.dst].abs() * (k[p.src].abs() + eabs)).sum(-1) / math.sqrt(p.d), p.dst, n, init=0.0)
        f.A = seg_sum(f.alpha[:, :, None] * (v[p.src].abs() + eabs), p.dst, n).reshape(n, p.c)
    return f


def unfolded_derived(p, f):
    deg = p.deg.double()[:, None]
    eps = gamma(2 * p.d + p.edge_dim + 14) * f.M + 2.0 * EPS32 + gamma(2.0 * deg + p.edge_dim + 8)
    return _per_head(eps / (1.0 - eps), p.d) * (f.A + f.attn.abs())


def unfolded_bounds(p, f):
    e = unfolded_derived(p, f) * (F32_FACTOR * TORCH_F32_UNFOLDED["out"])
    if p.xr is not None:
        e = e + U * (f.out.abs() + e)
    return _store(f.out, e, p.dtype)


def UCase(dtype, d, h, edge_dim, data="flat", gseed=1, unaligned=False, graph="irr"):
    c = Case(dtype, d, h, 4, data, graph=graph, gseed=gseed)
    c.edge_dim, c.unaligned = edge_dim, unaligned
    return c


def unfolded_case_id(c) -> str:
    return f"unfolded-{name(c.dtype)}-D{c.d}-H{c.h}-ed{c.edge_dim}-{c.data}-{c.graph}{c.gseed}" + ("-unaligned" if c.unaligned else "")


def unfolded_cases():
    out = []
    for dtype, ds in ((F32, (4, 16)), (BF16, (8, 64))):
        for i, d in enumerate(ds):
            out += [UCase(dtype, d, 3, ed, ("flat", "spread")[(i + j) % 2], gseed=j + 1) for j, ed in enumerate((3, 11, 13))]
    out.append(UCase(BF16, 64, 16, 16, "flat"))  # W_e in LDS: 17 x 1024 x 4 bytes > 64 KiB
    for dtype in (F32, BF16):
        out += [UCase(dtype, 12, 8, 11, "flat", gseed=2), UCase(dtype, 5, 3, 3, "spread", gseed=3),
                UCase(dtype, 16 if dtype == F32 else 8, 3, 20, "flat", gseed=1), UCase(dtype, 16 if dtype == F32 else 8, 3, 11, "flat", gseed=2, unaligned=True)]
    out.append(UCase(F32, 16, 3, 3, "flat", graph="n5"))
    return out


def measure_torch_f32_unfolded():
    worst = 0.0
    for c in [UCase(F32, d, 3, ed, data, gseed=s) for d, ed, s in ((4, 3, 0), (16, 11, 1), (32, 13, 2), (64, 16, 3)) for data in ("flat", "spread")]:
        p = make_unfolded_problem(c)
        f, f32 = evaluate_unfolded(p), evaluate_unfolded(p, torch.float32)
        diff = (f32.attn.double() - f.attn).abs()
        worst = max(worst, float(torch.where(diff == 0, torch.zeros_like(diff), diff / unfolded_derived(p, f)).max()))
    return {"out": worst}


# ------------------------------------------------------------------------------------------------ raw-row kernel
# ``ops.gt_edge_attention_raw`` (gt_edge_attention_raw_kernel, bf16, 16 heads): the sources are raw rows x_j [Ks] with rstd_j,
#     s_e = c (rstd_j qt_i,h . x_j + u_i,h . a_e),   g_i,h = sum_e alpha_e rstd_j x_j   (column sum_col: sum_e alpha_e),   t as above.
# ``_raw_rows_ref.kernel_reference`` in f64 is the reference.  Arithmetic: qt . x on the matrix pipe (exact bf16 products, Ks f32
# additions), one FMA with rstd, up attribute FMAs, the scale:  eta = gamma(Ks + up + 12) M + 2 EPS32,  M = c max_e (rstd sum|qt||x| +
# sum|u||a|).  The weight pe rstd is rounded to f32 and then to bf16 (rb = BF16_STORE) BEFORE the second MFMA, which sums 16 edges
# per step in f32 and is rescaled once per step; the normaliser sums the unrounded pe (the bound holds for either choice: as in
# _mhsa_ref the normaliser's own relative error e' may be anything up to eps, 0 included):
#     eps_g = rb + U + eta + gamma(deg + deg / 16 + 8),   E32 = eps_g / (1 - eps_g) (A + |g|),   A = sum_e alpha_e rstd_j |x_j|
#     t (f32 weights, four partial sums joined across lanes):  eps_t = rb + eta + gamma(deg + deg / 16 + 10),  A_t = sum_e alpha_e |a_e|
#     (rb for t as well: its weights are unrounded, but a normaliser over ROUNDED weights is off by up to rb and nothing in t's
#     numerator cancels that -- a first draft without it was refuted by the CPU emulation with the rounded normaliser)
#     column sum_col = l / (l + 1e-16): 4 U around 1 (exactly 0 for a destination without in-edges);   then the bf16 store.
# These are derived bounds throughout (no measured factor): the bf16 weight and the bf16 store dominate them.
RAW_DEGREES = (0, 1, 15, 16, 17, 31, 32, 33, 104)
RAW_H, RAW_N_SRC = 16, 60


def RawCase(ks, up, d, sum_col="last"):
    return types.SimpleNamespace(ks=ks, up=up, d=d, sum_col=(ks - 1 if sum_col == "last" else -1))


def raw_case_id(c) -> str:
    return f"raw-Ks{c.ks}-up{c.up}-D{c.d}-sumcol{c.sum_col}"


def raw_cases():
    out = [RawCase(ks, up, 64 if (i + j) % 2 else 32) for i, ks in enumerate((64, 128, 256)) for j, up in enumerate((4, 16))]
    return out + [RawCase(128, 8, 32), RawCase(128, 12, 64), RawCase(64, 4, 32, sum_col=None)]


def make_raw_problem(c):
    g = torch.Generator().manual_seed(9000 + c.ks * 31 + c.up * 7 + c.d)
    rowptr, col, _ = degree_graph(list(RAW_DEGREES) + [3, 0], RAW_N_SRC, 55 + c.ks + c.up)
    n, e = rowptr.shape[0] - 1, col.shape[0]
    x = torch.randn(RAW_N_SRC, c.ks, generator=g, dtype=torch.float64)
    if c.sum_col >= 0:
        x[:, c.sum_col] = 0.0  # (a zero column of x carries sum alpha)
    qt = torch.randn(n, RAW_H * c.ks, generator=g, dtype=torch.float64) * (1.5 / math.sqrt(c.ks))
    u = torch.randn(n, RAW_H * c.up, generator=g, dtype=torch.float64) * 0.3
    attr = torch.randn(e, c.up, generator=g, dtype=torch.float64)
    attr[:, c.up - 1] = 1.0
    rstd = torch.rand(RAW_N_SRC, generator=g, dtype=torch.float64) * 1.5 + 0.5
    stats = torch.stack([rstd, -rstd * torch.randn(RAW_N_SRC, generator=g, dtype=torch.float64)], dim=1).float().contiguous()
    deg = (rowptr[1:] - rowptr[:-1]).long()
    return types.SimpleNamespace(qt=qt.bfloat16(), x=x.bfloat16(), stats=stats, u=u.bfloat16(), attr=attr.float(), rowptr=rowptr, col=col,
                                 n_dst=n, n_src=RAW_N_SRC, n_edges=e, deg=deg, dst=torch.repeat_interleave(torch.arange(n), deg),
                                 src=col.long(), ks=c.ks, up=c.up, d=c.d, h=RAW_H, sum_col=c.sum_col)


def evaluate_raw(p, rstd_on=True):
    """(g [n_dst, H Ks], t [n_dst, H up]) by ``_raw_rows_ref.kernel_reference`` in f64, with what the bounds need."""
    from _raw_rows_ref import kernel_reference

    n, h = p.n_dst, p.h
    qt, x, u, a = p.qt.double().view(n, h, p.ks), p.x.double(), p.u.double().view(n, h, p.up), p.attr.double()
    rstd = p.stats[:, 0].double() if rstd_on else torch.ones(p.n_src, dtype=torch.float64)
    g, t = kernel_reference(qt, x, rstd, u, a, p.rowptr, p.col, p.d, p.sum_col)
    c = 1.0 / math.sqrt(p.d)
    xj, rj = x[p.src], rstd[p.src]
    s = (rj[:, None] * torch.einsum("ehk,ek->eh", qt[p.dst], xj) + torch.einsum("eha,ea->eh", u[p.dst], a)) * c
    m = seg_max(s, p.dst, n)
    ex = torch.exp(s - m[p.dst])
    alpha = ex / (seg_sum(ex, p.dst, n)[p.dst] + 1e-16)
    sabs = (rj[:, None] * torch.einsum("ehk,ek->eh", qt[p.dst].abs(), xj.abs()) + torch.einsum("eha,ea->eh", u[p.dst].abs(), a.abs())) * c
    return types.SimpleNamespace(g=g.reshape(n, -1), t=t.reshape(n, -1), alpha=alpha, s=s, M=seg_max(sabs, p.dst, n, init=0.0),
                                 A=seg_sum(alpha[:, :, None] * (rj[:, None] * xj.abs())[:, None, :], p.dst, n).reshape(n, -1),
                                 At=seg_sum(alpha[:, :, None] * a.abs()[:, None, :], p.dst, n).reshape(n, -1))


def raw_bounds(p, f):
    deg = p.deg.double()[:, None]
    eta_r = gamma(p.ks + p.up + 12) * f.M + 2.0 * EPS32
    steps = torch.ceil(deg / 16.0)
    eps_g = BF16_STORE + U + eta_r + gamma(deg + steps + 8)
    eps_t = BF16_STORE + eta_r + gamma(deg + steps + 10)
    e_g = _per_head(eps_g / (1.0 - eps_g), p.ks) * (f.A + f.g.abs())
    if p.sum_col >= 0:
        cols = torch.arange(p.h) * p.ks + p.sum_col
        e_g[:, cols] = torch.where(p.deg[:, None] > 0, torch.full((p.n_dst, p.h), 4.0 * U, dtype=torch.float64), torch.zeros(p.n_dst, p.h, dtype=torch.float64))
    e_t = _per_head(eps_t / (1.0 - eps_t), p.up) * (f.At + f.t.abs())
    return _store(f.g, e_g, BF16), _store(f.t, e_t, BF16)
