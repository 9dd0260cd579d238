"""GPU tests of the folded graph-transformer edge phase (csrc/edge_attention.hip behind ``ops.gt_edge_attention_folded``,
csrc/edge_backward.hip behind ``autograd._edge_backward``), of the explicit-edge conv forward and backward (``ops.gt_conv``,
``autograd.gt_conv``), of the unfolded kernel (``ops.gt_edge_attention``, fast and generic path) and of the raw-row kernel
(``ops.gt_edge_attention_raw``) against the f64 references of tests/_edge_attn_ref.py: ``out``, ``t``,
``lse``, ``dq``, ``du``, ``dk``, ``dv`` and ``d attr`` PER ELEMENT, every element finite and inside a bound derived from the data
(``_edge_attn_ref``: the derivations).  tests/test_edge_attn_ref_cpu.py shows, without a GPU, that emulations of the kernels'
arithmetic stay inside these bounds at every case of this file and that a dropped, doubled or foreign edge, a wrong scale,
swapped heads, a rotated or misplaced t column, a wrong x_r, an lse in other units and seven wrong backwards do not.

Every operand and every result sits in a ``Guarded`` buffer (tests/test_gpu_mhsa.py): NaN rows and columns around the inputs,
a bit pattern around the outputs that must be untouched, pitches wider than the data (k | v and dk | dv share one buffer with a
guard band between them, as the kernels want one pitch for both).  Every case names the kernel it expects: the plain kernel's
instantiation by restating the dispatch (``_edge_attn_ref.plain_kernel``), and the entry point whose kernel ran by the launch
trail -- a list kernel that fell back to the plain one shows there.

Measured on an MI355X: the largest fraction of its bound that any element used, over all cases of this file (the module prints
the table again at its end).  bf16 results sit at 0.99: that is the rounding of the store, half a unit of bf16's last place.
                                        out      t        lse
    plain forward, f32                  0.909    0.313    0.344   (out: the one rounding of the f32 x_r add on ``residual``)
    plain forward, bf16                 0.996    0.990    0.313
    sched forward                       0.996    0.989    0.325   (bit-identical to the plain kernel)
    tiles forward                       0.996    0.989    0.428   (bit-identical to the plain kernel)
    groups forward                      0.996    0.996    0.312   (bit-identical to the plain kernel on the source-ordered CSR)
    runs forward                        0.996    0.996    0.312   (likewise, and to the group kernel)
                                        dq       du       dk       dv       d attr
    backward alone, f32                 0.329    0.247    0.273    0.334    0.420   (operand: the rounded reference lse)
    backward alone, bf16                0.993    0.992    0.989    0.993    0.373
    backward, the forward's lse, f32    0.114    0.128    0.116    0.181    0.171   (bounds widened by the forward's lse bound)
    backward, the forward's lse, bf16   0.992    0.990    0.988    0.992    0.235
                                        out      lse
    conv forward, f32                   0.834    0.295   (with dropout 0.642 / 0.400)
    conv forward, bf16                  0.994    0.362   (with dropout 0.995 / 0.341)
                                        dq       dk       dv       d e
    conv backward, f32                  0.123    0.210    0.289    0.304   (with dropout 0.124 / 0.098 / 0.108 / 0.141)
    conv backward, bf16                 0.994    0.992    0.986    0.990   (with dropout 0.962 / 0.987 / 0.976 / 0.976)
                                        out
    unfolded fast path, f32 / bf16      0.331 / 0.995
    unfolded generic kernel, f32 / bf16 0.182 / 0.993
                                        g        t
    raw-row kernel                      0.647    0.294   (derived bounds: the bf16 weight of the second MFMA and the bf16 store)
No guard band was written, every repeat of a forward call was bit-identical, isolated destinations gave out = x_r, t = 0,
lse = -inf and exact zeros in dq / du, sources without out-edges exact zeros in dk / dv, dxr equalled dout bit for bit, the
packed layouts and the autograd functions gave the bits of the direct call; the conv at p = 1 returned x_r exactly and exact
zero gradients; the raw-row kernel's sum_col column was exactly 1 (0 for isolated rows) and its second run bit-identical.

What failed, and the kernel change it led to.  ``test_list_kernels[bf16-D32-H16-UP12-flat-deg30-groups]``: out and t equalled
the plain kernel's bit for bit, lse differed in 97 of 16 384 elements (1698 on the ``spread`` case; the run kernel the same; the
D = 64 cases passed).  Cause, read from the compiler's assembly: in the group and run kernels ``sum * scale - m`` had been
contracted into one v_fma_f32 (a single rounding) in all 32 instantiations, while the plain, scheduled and tile kernels round
the product first (v_mul_f32, v_sub_f32).  With scale = 1 / 8 the product is exact and both agree; with 1 / sqrt(32) the
weights differ in their last f32 bit, which the bf16 store of out / t hides and lse shows.  Both were inside the bounds; the
finding is the broken bit-identity of the route table.  Fix: ``edge_common.hpp::exponent_of`` forms the difference with
contraction off, used by all five folded kernels (it changes code in the group and run kernels alone).  Afterwards: the 32 instantiations have v_sub_f32 where the v_fma_f32
was, the same instruction count and one VGPR fewer; every other kernel's assembly is unchanged; of 35 forward cases run on the
library before and after (all 18 list cases, 17 plain ones) 31 are bit-identical, and the four that differ are the D = 32
group / run cases, by the amounts above (out: 5 of 524 288 bf16 elements on ``spread``, none on ``flat``).
"""

import pytest
import torch

import _edge_attn_ref as R
from test_gpu_mhsa import Guarded

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = R.F32, R.BF16
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from anemoi_models_amd import _lib

    _lib.load()  # the native library must be present: no fallback
    assert torch.cuda.is_available()
    yield
    print("[worst fraction of the bound, per kernel and output]")
    for key in sorted(_WORST):
        print(f"    {key}: {_WORST[key]:.3f}")


def _note(key, fraction):
    _WORST[key] = max(_WORST.get(key, 0.0), fraction)
    return fraction


def _pad(width, dtype):
    """Guard columns that keep the pitch a multiple of 16 bytes: at least one vector, never none."""
    v = R.vec(dtype)
    return v + (-width) % v


def _nan_gap(a, b, dtype):
    return torch.cat([a, torch.full((a.shape[0], R.vec(dtype)), float("nan"), dtype=dtype), b], dim=1)


def _plan(p):
    from anemoi_models_amd import runtime

    return runtime.EdgePlan(p.rowptr.to(DEV), p.col.to(DEV), torch.arange(p.n_edges, dtype=torch.int32, device=DEV), p.n_src, p.n_dst)


class Operands:
    """The guarded inputs of a problem on the device."""

    def __init__(self, p):
        dt, c = p.dtype, p.c
        self.q = Guarded(p.n_dst, c, dt, _pad(c, dt), data=p.q.to(DEV))
        self.kv = Guarded(p.n_src, 2 * c + R.vec(dt), dt, R.vec(dt), data=_nan_gap(p.k, p.v, dt).to(DEV))
        self.k, self.v = self.kv.view[:, :c], self.kv.view[:, c + R.vec(dt):]
        self.xr = None if p.xr is None else Guarded(p.n_dst, c, dt, _pad(c, dt), data=p.xr.to(DEV))
        self.u = Guarded(p.n_dst, p.h * p.up, dt, _pad(p.h * p.up, dt), data=p.u.to(DEV))
        self.attr = Guarded(p.n_edges, p.up, F32, 0, data=p.attr.to(DEV)).view if p.n_edges else torch.zeros(0, p.up, device=DEV)
        self.rowptr, self.col = p.rowptr.to(DEV), p.col.to(DEV)


def _forward(c, p, ops_in, lists=None, route="plain"):
    """One launch of ``ops.gt_edge_attention_folded`` into guarded results; asserts the entry point by the trail and the
    guards.  (out, t, lse or None) on the CPU."""
    from anemoi_models_amd import ops, trail

    width = p.c + p.h * p.up
    ld = ops.round_up(width, ops.k_multiple(p.dtype)) if c.pad_out else width
    gout = Guarded(p.n_dst, ld, p.dtype, _pad(ld, p.dtype))
    if ld > width:
        gout.view[:, width:].zero_()  # (what the wrapper does when it allocates: the kernel must leave the K padding alone)
    glse = Guarded(p.n_dst, p.h, F32, 0) if c.lse else None
    with trail.record() as tr:
        got = ops.gt_edge_attention_folded(ops_in.q.view, ops_in.k, ops_in.v, None if ops_in.xr is None else ops_in.xr.view,
                                           ops_in.u.view, ops_in.attr, ops_in.rowptr, ops_in.col, p.h, p.up, out=gout.view,
                                           ld_out=ld, lse=None if glse is None else glse.view, **(lists or {}))
    assert got.data_ptr() == gout.view.data_ptr()
    want_names = [R.ENTRY[route] + ":out"] + ([R.ENTRY[route] + ":lse"] if c.lse else [])
    assert tr.names() == want_names, f"{R.case_id(c)}: the trail names {tr.names()}"
    assert (tr.entries[0].rows, tr.entries[0].cols) == (p.n_dst, width)
    gout.assert_clean(R.case_id(c) + " out")
    res = gout.view.cpu()
    if ld > width:
        assert not bool(res[:, width:].any()), f"{R.case_id(c)}: the K padding of out was written"
    lse = None
    if glse is not None:
        glse.assert_clean(R.case_id(c) + " lse")
        lse = glse.view.cpu().clone()
    return res[:, :p.c].clone(), res[:, p.c:width].clone(), lse


def _check_forward(c, p, f, out, t, lse, tag):
    bo, bt, bl = R.forward_bounds(p, f)
    fo = _note(f"{tag} out", R.check(out, f.out, bo, f"{R.case_id(c)} out"))
    ft = _note(f"{tag} t", R.check(t, f.t, bt, f"{R.case_id(c)} t"))
    fl = _note(f"{tag} lse", R.check_lse(lse, f.lse, bl, f"{R.case_id(c)} lse")) if lse is not None else float("nan")
    print(f"{R.case_id(c)}: out {fo:.3f}, t {ft:.3f}, lse {fl:.3f} of the bound")
    iso = p.deg == 0
    if bool(iso.any()):  # (the bounds are zero there already; said again in the open)
        assert torch.equal(out[iso], p.xr[iso] if p.xr is not None else torch.zeros_like(out[iso]))
        assert not bool(t[iso].any())
        assert lse is None or bool((lse[iso] == float("-inf")).all())


# ------------------------------------------------------------------------------------------------ the plain kernel
@pytest.mark.parametrize("c", R.plain_instantiation_cases() + R.plain_further_cases(), ids=R.case_id)
def test_plain_folded_kernel(c):
    p = R.make_problem(c)
    kernel = R.plain_kernel(c.dtype, c.d, c.up, c.xr)  # (raises where the dispatch has no instantiation)
    assert R.n_slices(c.dtype, p.c) == (1 if c.h == 3 else -(-p.c // (64 * R.vec(c.dtype))))
    f = R.evaluate(p)
    ops_in = Operands(p)
    out, t, lse = _forward(c, p, ops_in)
    print(f"{R.case_id(c)}: {kernel}, {R.n_slices(c.dtype, p.c)} slice(s), {p.n_dst} destinations, {p.n_edges} edges")
    _check_forward(c, p, f, out, t, lse, f"plain forward {R.name(c.dtype)}")
    out2, t2, lse2 = _forward(c, p, ops_in)
    assert torch.equal(out2, out) and torch.equal(t2, t) and (lse is None or torch.equal(lse2, lse)), "a repeat of the call differs"
    if c.pad_out:  # the wrapper allocating the padded buffer itself: the same bits, and ITS zero fill of the K padding
        from anemoi_models_amd import ops

        width = p.c + p.h * p.up
        ld = ops.round_up(width, ops.k_multiple(p.dtype))
        own = ops.gt_edge_attention_folded(ops_in.q.view, ops_in.k, ops_in.v, ops_in.xr.view, ops_in.u.view, ops_in.attr, ops_in.rowptr,
                                           ops_in.col, p.h, p.up, ld_out=ld).cpu()
        assert own.shape == (p.n_dst, ld) and ld > width and not bool(own[:, width:].any())
        assert torch.equal(own[:, :p.c], out) and torch.equal(own[:, p.c:width], t)


# ------------------------------------------------------------------------------------------------ the list kernels
def _canonical(p):
    """The same graph with every destination's in-edges in ascending source order (attribute rows moved along)."""
    order = R.canonical_order(p.rowptr, p.col)
    return R.Problem(p.q, p.k, p.v, p.xr, p.u, p.attr[order].contiguous(), p.rowptr, p.col[order].contiguous(), p.h, p.up)


@pytest.mark.parametrize("c", R.list_cases(), ids=R.case_id)
def test_list_kernels(c, monkeypatch):
    """sched, tiles (irregular graph), groups, runs (uniform degree 3): against the f64 reference, and bit for bit against the
    plain kernel on the same guarded operands -- groups and runs sum a destination's three edges in ascending source order,
    so their plain twin runs on the CSR in that order (the same operation, the same order of summation)."""
    p = R.make_problem(c)
    assert R.list_kernel_shape(c.dtype, c.d, c.up, p.n_dst)
    plan = _plan(p)
    if c.route == "sched":
        sched = plan.schedule(BF16, p.c)
        assert sched is not None and sched.shape[0] == 8
        lists = {"sched": sched}
    elif c.route == "tiles":
        assert p.c % 128 == 0
        tiles = plan.tiles(BF16, p.c, p.h, p.up)
        assert tiles is not None
        lists = {"tiles": tiles}
    else:
        monkeypatch.setenv("ANEMOI_AMD_EDGE_GROUPS", "1" if c.route == "groups" else "0")
        runs = plan.runs3()
        assert runs is not None and len(runs) == (3 if c.route == "groups" else 2)
        if c.route == "groups":
            sizes = (runs[0][1:] - runs[0][:-1]).cpu()
            assert int(sizes.max()) == 8 and int(sizes.min()) == 1  # a group of 8 and a single destination
        lists = {"runs": runs}
    f = R.evaluate(p)
    ops_in = Operands(p)
    out, t, lse = _forward(c, p, ops_in, lists, c.route)  # (the trail shows that the list kernel ran and did not fall back)
    _check_forward(c, p, f, out, t, lse, f"{c.route} forward")
    out2, t2, lse2 = _forward(c, p, ops_in, lists, c.route)
    assert torch.equal(out2, out) and torch.equal(t2, t) and torch.equal(lse2, lse), "a repeat of the call differs"
    twin = ops_in if c.route in ("sched", "tiles") else Operands(_canonical(p))
    po, pt, pl = _forward(c, p, twin)
    for what, a, b in (("out", out, po), ("t", t, pt), ("lse", lse, pl)):
        assert torch.equal(a, b), f"{R.case_id(c)}: {what} differs from the plain kernel in {int((a != b).sum())} elements"


# ------------------------------------------------------------------------------------------------ backward
class Grads:
    """Guarded gradient buffers of one layout.  ``separate``: one buffer each (dk | dv share a pitch); ``processor``: the column
    ranges of one ``d(x_r | q | k | v | u)`` (n_src == n_dst); ``mapper``: ``d(x_r | q | u)`` and ``d(k | v)``."""

    def __init__(self, p, layout):
        dt, c, hu, v = p.dtype, p.c, p.h * p.up, R.vec(p.dtype)
        self.layout = layout
        if layout == "separate":
            self.bufs = {"dq": Guarded(p.n_dst, c, dt, _pad(c, dt)), "du": Guarded(p.n_dst, hu, dt, _pad(hu, dt)),
                         "dxr": Guarded(p.n_dst, c, dt, _pad(c, dt)), "dkv": Guarded(p.n_src, 2 * c + v, dt, v)}
            kv = self.bufs["dkv"].view
            self.dq, self.du, self.dxr, self.dk, self.dv = self.bufs["dq"].view, self.bufs["du"].view, self.bufs["dxr"].view, kv[:, :c], kv[:, c + v:]
            self.gaps = [kv[:, c:c + v]]
        elif layout == "processor":
            assert p.n_src == p.n_dst
            self.bufs = {"dsq": Guarded(p.n_dst, 4 * c + hu, dt, _pad(4 * c + hu, dt))}
            s = self.bufs["dsq"].view
            self.dxr, self.dq, self.dk, self.dv, self.du = s[:, :c], s[:, c:2 * c], s[:, 2 * c:3 * c], s[:, 3 * c:4 * c], s[:, 4 * c:]
            self.gaps = []
        else:
            self.bufs = {"dsq": Guarded(p.n_dst, 2 * c + hu, dt, _pad(2 * c + hu, dt)), "dkv": Guarded(p.n_src, 2 * c, dt, _pad(2 * c, dt))}
            s, kv = self.bufs["dsq"].view, self.bufs["dkv"].view
            self.dxr, self.dq, self.du, self.dk, self.dv = s[:, :c], s[:, c:2 * c], s[:, 2 * c:], kv[:, :c], kv[:, c:]
            self.gaps = []

    def assert_clean(self, what):
        for key, g in self.bufs.items():
            g.assert_clean(f"{what} {self.layout} {key}")
        for gap in self.gaps:  # the band between dk and dv inside their shared buffer
            pattern = next(iter(self.bufs.values())).pattern
            raw = gap.view(torch.int16 if gap.dtype == BF16 else torch.int32)
            assert bool((raw == pattern).all()), f"{what}: the columns between dk and dv were written"

    def results(self):
        return {"dq": self.dq.cpu().clone(), "du": self.du.cpu().clone(), "dk": self.dk.cpu().clone(), "dv": self.dv.cpu().clone(),
                "dxr": self.dxr.cpu().clone()}


def _backward(c, p, ops_in, gd, gdt, glse, layout, plan):
    """``autograd._edge_backward`` on guarded operands into the guarded buffers of ``layout``; asserts the three entry points
    by the trail and every guard."""
    from anemoi_models_amd import autograd, trail

    g = Grads(p, layout)
    with trail.record() as tr:
        dattr = autograd._edge_backward(ops_in.q.view, ops_in.k, ops_in.v, gd.view, ops_in.u.view, gdt.view, glse.view, ops_in.attr,
                                        plan, p.h, p.up, g.dq, g.dk, g.dv, g.du, True, dxr=g.dxr)
    dst, src = "anemoi_gt_edge_attention_folded_backward_dst", "anemoi_gt_edge_attention_folded_backward_src"
    assert tr.names() == [dst + ":dq", dst + ":du", dst + ":dxr", dst + ":dsum", src + ":dk", src + ":dv", "anemoi_gt_edge_attr_grad:out"], tr.names()
    g.assert_clean(R.case_id(c))
    res = g.results()
    res["dattr"] = dattr.cpu()
    return res


def _check_backward(c, p, f, b, res, lse_err, tag, what):
    bb = R.backward_bounds(p, f, b, lse_err)
    fr = {key: _note(f"{tag} {key}", R.check(res[key], getattr(b, key), bb[key], f"{R.case_id(c)} {what} {key}")) for key in R.BACKWARD_KEYS}
    print(f"{R.case_id(c)} {what}: " + ", ".join(f"{k} {v:.3f}" for k, v in fr.items()) + " of the bound")
    # exact zeros where nothing flows (the bounds are zero there; said again in the open: these land in torch.empty buffers)
    assert not bool(res["dq"][p.deg == 0].any()) and not bool(res["du"][p.deg == 0].any())
    assert not bool(res["dk"][p.odeg == 0].any()) and not bool(res["dv"][p.odeg == 0].any())


@pytest.mark.parametrize("c", R.backward_cases(), ids=R.case_id)
def test_folded_backward(c):
    from anemoi_models_amd import autograd

    p = R.make_problem(c)
    R.plain_kernel(c.dtype, c.d, c.up, True)  # (the backward's dispatch takes the same D / VEC and UP)
    dout, dtt = R.make_grads(c, p)
    f = R.evaluate(p)
    b = R.evaluate_backward(p, f, dout, dtt)
    ops_in, plan = Operands(p), _plan(p)
    gd = Guarded(p.n_dst, p.c, p.dtype, _pad(p.c, p.dtype), data=dout.to(DEV))
    gdt = Guarded(p.n_dst, p.h * p.up, p.dtype, _pad(p.h * p.up, p.dtype), data=dtt.to(DEV))
    tag = f"backward {R.name(c.dtype)}"
    # 1. the rounded reference lse: lse_err is its actual deviation, the bound is at its tightest
    lse_st = f.lse.float()
    glse = Guarded(p.n_dst, p.h, F32, 0, data=lse_st.to(DEV))
    layouts = ["separate", "mapper"] + (["processor"] if p.n_src == p.n_dst else [])
    first = None
    for layout in layouts:
        res = _backward(c, p, ops_in, gd, gdt, glse, layout, plan)
        assert torch.equal(res["dxr"].view(torch.int16 if c.dtype == BF16 else torch.int32),
                           dout.view(torch.int16 if c.dtype == BF16 else torch.int32)), "dxr is not dout bit for bit"
        if first is None:
            first = res
            err = R.finite_lse_err((lse_st.double() - f.lse).abs(), f.lse)
            _check_backward(c, p, f, b, res, err, tag + " alone", "reference lse")
        else:
            for key in first:
                assert torch.equal(res[key], first[key]), f"{R.case_id(c)}: {key} of the {layout} layout differs from the separate one"
    # 2. the forward kernel's own lse: the bound widened by the forward's lse bound
    _, _, lse_k = _forward(c, p, ops_in)
    bo, bt, bl = R.forward_bounds(p, f)
    res = _backward(c, p, ops_in, gd, gdt, Guarded(p.n_dst, p.h, F32, 0, data=lse_k.to(DEV)), "separate", plan)
    _check_backward(c, p, f, b, res, R.finite_lse_err(bl, f.lse), tag + " own lse", "own lse")
    # ... and the same through autograd.gt_edge_attention, where the wrapper's own (unpadded) buffers have pitches the kernels
    # take: H up and C + H up multiples of 16 bytes (bf16 with an odd H: up = 16 alone; the H = 4 cases; every f32 case)
    v = R.vec(c.dtype)
    if (p.h * p.up) % v == 0 and (p.c + p.h * p.up) % v == 0:
        leaves = [t.to(DEV).requires_grad_() for t in (p.q, p.k, p.v, p.xr, p.u)]
        kv = torch.cat([leaves[1], leaves[2]], dim=1)  # (k and v must share a pitch)
        attr = p.attr.to(DEV).requires_grad_()
        full = autograd.gt_edge_attention(leaves[0], kv[:, :p.c], kv[:, p.c:], leaves[3], leaves[4], attr, plan, p.h, p.up)
        R.check(full.detach()[:, :p.c], f.out, bo, f"{R.case_id(c)} autograd out")
        R.check(full.detach()[:, p.c:], f.t, bt, f"{R.case_id(c)} autograd t")
        full.backward(torch.cat([dout, dtt], dim=1).to(DEV))
        got = {"dq": leaves[0].grad, "dk": leaves[1].grad, "dv": leaves[2].grad, "dxr": leaves[3].grad, "du": leaves[4].grad, "dattr": attr.grad}
        for key, g in got.items():
            assert torch.equal(g.cpu(), res[key]), f"{R.case_id(c)}: autograd.gt_edge_attention {key} differs from the direct call"


@pytest.mark.parametrize("c", [R.Case(BF16, 64, 4, 12, "flat", gseed=3), R.Case(F32, 16, 3, 12, "spread", gseed=3),
                               R.Case(BF16, 32, 16, 16, "residual", gseed=3)], ids=R.case_id)
def test_packed_autograd_functions_give_the_bits_of_the_direct_call(c):
    """``autograd.gt_edge_attention_packed`` (mapper: ``x_r | q | u`` + ``k | v``) and ``_GTEdgeAttentionSelf`` (processor: one
    ``x_r | q | k | v | u``) against ``autograd._edge_backward`` called directly with the lse of the same forward."""
    from anemoi_models_amd import autograd, ops, runtime

    p = R.make_problem(c)
    assert p.n_src == p.n_dst
    dout, dtt = R.make_grads(c, p)
    plan = _plan(p)
    dfull = torch.cat([dout, dtt], dim=1).to(DEV)
    attr = p.attr.to(DEV)
    # the direct call, on the operands of the packed buffers
    sq5 = torch.cat([p.xr, p.q, p.k, p.v, p.u], dim=1).to(DEV)
    cc = p.c
    lse = torch.empty(p.n_dst, p.h, device=DEV)
    lists = runtime.edge_lists(plan, p.dtype, cc, p.h, p.up, training=True)._asdict()
    fwd = ops.gt_edge_attention_folded(sq5[:, cc:2 * cc], sq5[:, 2 * cc:3 * cc], sq5[:, 3 * cc:4 * cc], sq5[:, :cc], sq5[:, 4 * cc:], attr,
                                       plan.rowptr, plan.col, p.h, p.up, lse=lse, **lists)
    ops_in = Operands(p)
    gd = Guarded(p.n_dst, cc, p.dtype, _pad(cc, p.dtype), data=dout.to(DEV))
    gdt = Guarded(p.n_dst, p.h * p.up, p.dtype, _pad(p.h * p.up, p.dtype), data=dtt.to(DEV))
    glse = Guarded(p.n_dst, p.h, F32, 0, data=lse)
    direct = _backward(c, p, ops_in, gd, gdt, glse, "separate", plan)
    # processor
    x = sq5.clone().requires_grad_()
    a = attr.clone().requires_grad_()
    y = autograd._GTEdgeAttentionSelf.apply(x, a, plan, p.h, p.up)
    assert torch.equal(y, fwd)
    y.backward(dfull)
    g = x.grad.cpu()
    for key, cols in (("dxr", slice(0, cc)), ("dq", slice(cc, 2 * cc)), ("dk", slice(2 * cc, 3 * cc)), ("dv", slice(3 * cc, 4 * cc)),
                      ("du", slice(4 * cc, None))):
        assert torch.equal(g[:, cols], direct[key]), f"_GTEdgeAttentionSelf {key}"
    assert torch.equal(a.grad.cpu(), direct["dattr"])
    # mapper
    sq = torch.cat([p.xr, p.q, p.u], dim=1).to(DEV).requires_grad_()
    kv = torch.cat([p.k, p.v], dim=1).to(DEV).requires_grad_()
    a = attr.clone().requires_grad_()
    y = autograd.gt_edge_attention_packed(sq, kv, a, plan, p.h, p.up)
    assert torch.equal(y, fwd)
    y.backward(dfull)
    g, gkv = sq.grad.cpu(), kv.grad.cpu()
    for key, got in (("dxr", g[:, :cc]), ("dq", g[:, cc:2 * cc]), ("du", g[:, 2 * cc:]), ("dk", gkv[:, :cc]), ("dv", gkv[:, cc:])):
        assert torch.equal(got, direct[key]), f"gt_edge_attention_packed {key}"
    assert torch.equal(a.grad.cpu(), direct["dattr"])


# ------------------------------------------------------------------------------------------------ explicit-edge conv, forward
@pytest.mark.parametrize("c", R.conv_cases(), ids=R.conv_case_id)
def test_conv_forward_and_lse(c):
    """``ops.gt_conv`` (gt_conv_kernel <DROP = false / true>) on guarded operands: out and lse per element at p = 0, 0.25 (the
    kernels' keep mask restated by tests/_cpu_ops.py) and 1 (x_r exactly).  The wrapper allocates out itself."""
    from _cpu_ops import edge_dropout_keep_mask
    from anemoi_models_amd import ops, trail

    p = R.make_conv_problem(c)
    lph = p.d // R.vec(c.dtype)
    assert p.d % R.vec(c.dtype) == 0 and lph in (1, 2, 4, 8, 16)
    drop = min(int(c.p * 32768.0 + 0.5), 32768) != 0  # (the DROP instantiation)
    keep = edge_dropout_keep_mask(R.CONV_SEED, c.p, p.n_edges, p.h) if c.p > 0.0 else None
    f = R.evaluate_conv(p, keep=keep, pdrop=c.p)
    bo, bl = R.conv_forward_bounds(p, f)
    ops_in = Operands(R.Problem(p.q, p.k, p.v, p.xr, torch.zeros(p.n_dst, p.h * 4, dtype=c.dtype), torch.zeros(p.n_edges, 4), p.rowptr, p.col, p.h, 4))
    ge = Guarded(p.n_edges, p.c, c.dtype, _pad(p.c, c.dtype), data=p.e.to(DEV))

    def run(seed):
        glse = Guarded(p.n_dst, p.h, F32, 0)
        with trail.record() as tr:
            out = ops.gt_conv(ops_in.q.view, ops_in.k, ops_in.v, ge.view, ops_in.rowptr, ops_in.col, p.h, x_r=ops_in.xr.view,
                              lse=glse.view, dropout_p=c.p, dropout_seed=seed)
        assert tr.names() == ["anemoi_gt_conv:out", "anemoi_gt_conv:lse"], tr.names()
        glse.assert_clean(R.conv_case_id(c) + " lse")
        return out.cpu(), glse.view.cpu().clone()

    out, lse = run(R.CONV_SEED)
    tag = f"conv forward {R.name(c.dtype)}" + (" dropout" if drop else "")
    fo = _note(f"{tag} out", R.check(out, f.out, bo, f"{R.conv_case_id(c)} out"))
    fl = _note(f"{tag} lse", R.check_lse(lse, f.lse, bl, f"{R.conv_case_id(c)} lse"))
    print(f"{R.conv_case_id(c)}: gt_conv_kernel<{R.name(c.dtype)},LPH={lph},DROP={drop}>: out {fo:.3f}, lse {fl:.3f} of the bound")
    iso = p.deg == 0
    assert torch.equal(out[iso], p.xr[iso]) and bool((lse[iso] == float("-inf")).all())
    if c.p >= 1.0:
        assert torch.equal(out, p.xr)
    out2, lse2 = run(R.CONV_SEED)
    assert torch.equal(out2, out) and torch.equal(lse2, lse), "a repeat of the call differs"
    if 0.0 < c.p < 1.0:
        other, lse3 = run(R.CONV_SEED + 1)
        assert not torch.equal(other, out) and torch.equal(lse3, lse)  # (the normaliser sees every edge: lse has no mask)


@pytest.mark.parametrize("c", R.conv_cases(), ids=R.conv_case_id)
def test_conv_backward(c):
    """``autograd.gt_conv`` (gt_conv_bwd_dst_kernel, gt_conv_bwd_src_kernel <DROP>): dq, dk, dv and d e per element with the mask
    of the forward, bounds widened by the forward's lse bound; d x_r is dout; p = 1 gives exact zeros."""
    from anemoi_models_amd import autograd, trail

    p = R.make_conv_problem(c)
    keep = R.conv_keep(c, p)
    dout, _ = R.make_grads(c, p)
    f = R.evaluate_conv(p, keep=keep, pdrop=c.p)
    b = R.evaluate_conv_backward(p, f, dout)
    bo, bl = R.conv_forward_bounds(p, f)
    bb = R.conv_backward_bounds(p, f, b, R.finite_lse_err(bl, f.lse))
    q, kv, e, xr = (t.to(DEV).requires_grad_() for t in (p.q, torch.cat([p.k, p.v], dim=1), p.e, p.xr))
    with trail.record() as tr:
        out = autograd.gt_conv(q, kv[:, :p.c], kv[:, p.c:], e, xr, _plan(p), p.h, dropout_p=c.p, seed=R.CONV_SEED)
        out.backward(dout.to(DEV))
    want = ["anemoi_gt_conv:out", "anemoi_gt_conv:lse", "anemoi_gt_conv_backward_dst:dq", "anemoi_gt_conv_backward_dst:dsum",
            "anemoi_gt_conv_backward_src:dk", "anemoi_gt_conv_backward_src:dv"]
    assert tr.names() == want, tr.names()
    R.check(out.detach(), f.out, bo, f"{R.conv_case_id(c)} autograd out")
    got = {"dq": q.grad.cpu(), "dk": kv.grad[:, :p.c].cpu(), "dv": kv.grad[:, p.c:].cpu(), "de": e.grad.cpu()}
    tag = f"conv backward {R.name(c.dtype)}" + (" dropout" if c.p > 0.0 else "")
    fr = {key: _note(f"{tag} {key}", R.check(got[key], getattr(b, key), bb[key], f"{R.conv_case_id(c)} {key}")) for key in R.CONV_BACKWARD_KEYS}
    print(f"{R.conv_case_id(c)}: " + ", ".join(f"{k} {v:.3f}" for k, v in fr.items()) + " of the bound")
    assert torch.equal(xr.grad.cpu(), dout)
    assert not bool(got["dq"][p.deg == 0].any()) and not bool(got["dk"][p.odeg == 0].any()) and not bool(got["dv"][p.odeg == 0].any())
    if c.p >= 1.0:
        assert not any(bool(g.any()) for g in got.values())


# ------------------------------------------------------------------------------------------------ unfolded kernel
@pytest.mark.parametrize("c", R.unfolded_cases(), ids=R.unfolded_case_id)
def test_unfolded_kernel(c):
    """``ops.gt_edge_attention`` on guarded operands and a guarded result: the fast path (every EDP, the > 64 KiB LDS
    instantiation) and the generic kernel (D = 12, D = 5, edge_dim = 20, a pitch off the 16-byte grid), the route restated from
    the launcher's conditions on the tensors handed over; out per element, isolated rows exactly x_r."""
    from anemoi_models_amd import ops, trail

    p = R.make_unfolded_problem(c)
    dt, cc, v = c.dtype, p.c, R.vec(c.dtype)
    pad = (v + 1 + (-cc) % v) if c.unaligned else _pad(cc, dt)  # (unaligned: a pitch that is no multiple of 16 bytes)
    gq = Guarded(p.n_dst, cc, dt, pad, data=p.q.to(DEV))
    gkv = Guarded(p.n_src, 2 * cc + v, dt, pad, data=_nan_gap(p.k, p.v, dt).to(DEV))
    gx = Guarded(p.n_dst, cc, dt, pad, data=p.xr.to(DEV))
    ga = Guarded(p.n_edges, (p.edge_dim + 3) // 4 * 4, F32, 4, data=p.attr[:, :(p.edge_dim + 3) // 4 * 4].to(DEV))  # (NaN pad columns)
    gout = Guarded(p.n_dst, cc, dt, pad)
    k, vv = gkv.view[:, :cc], gkv.view[:, cc + v:]
    aligned = all(t.data_ptr() % 16 == 0 and t.stride(0) % v == 0 for t in (gq.view, k, vv, gx.view, gout.view))
    route = R.unfolded_route(dt, c.d, cc, p.edge_dim, ga.ld, aligned)
    want_generic = c.unaligned or c.d in (5, 12) or p.edge_dim > 16
    assert (route == "generic") == want_generic and (c.h != 16 or route.endswith(">64K")), route
    w, b = p.w.to(DEV), p.b.to(DEV)

    def run():
        with trail.record() as tr:
            got = ops.gt_edge_attention(gq.view, k, vv, gx.view, ga.view, p.edge_dim, w, b, p.rowptr.to(DEV), p.col.to(DEV), p.h, out=gout.view)
        assert got.data_ptr() == gout.view.data_ptr() and tr.names() == ["anemoi_gt_edge_attention:out"]
        gout.assert_clean(R.unfolded_case_id(c))
        return gout.view.cpu().clone()

    out = run()
    f = R.evaluate_unfolded(p)
    tag = f"unfolded {'generic' if route == 'generic' else 'fast'} {R.name(dt)}"
    fo = _note(f"{tag} out", R.check(out, f.out, R.unfolded_bounds(p, f), f"{R.unfolded_case_id(c)} out"))
    print(f"{R.unfolded_case_id(c)}: {route}: out {fo:.3f} of the bound")
    assert torch.equal(out[p.deg == 0], p.xr[p.deg == 0])
    assert torch.equal(run(), out), "a repeat of the call differs"


# ------------------------------------------------------------------------------------------------ raw-row kernel
@pytest.mark.parametrize("c", R.raw_cases(), ids=R.raw_case_id)
def test_raw_row_kernel(c):
    """``ops.gt_edge_attention_raw`` (gt_edge_attention_raw_kernel <Ks, UP>) on guarded operands and results, in-degrees 0, 1, 15,
    16, 17, 31, 32, 33, 104: g per element with the sum_col column, t per element, isolated rows exactly zero, a second run
    bit-identical."""
    from anemoi_models_amd import ops, trail

    p = R.make_raw_problem(c)
    assert c.ks in (64, 128, 256) and c.up in (4, 8, 12, 16) and p.h == 16
    f = R.evaluate_raw(p)
    bg, bt = R.raw_bounds(p, f)
    hk, hu = p.h * p.ks, p.h * p.up
    gq = Guarded(p.n_dst, hk, BF16, 8, data=p.qt.to(DEV))
    gx = Guarded(p.n_src, p.ks, BF16, 8, data=p.x.to(DEV))
    gu = Guarded(p.n_dst, hu, BF16, 8, data=p.u.to(DEV))
    ga = Guarded(p.n_edges, p.up, F32, 0, data=p.attr.to(DEV))
    stats, rowptr, col = p.stats.to(DEV), p.rowptr.to(DEV), p.col.to(DEV)

    def run():
        gg, gt = Guarded(p.n_dst, hk, BF16, 8), Guarded(p.n_dst, hu, BF16, 8)
        with trail.record() as tr:
            got = ops.gt_edge_attention_raw(gq.view, gx.view, stats, gu.view, ga.view, rowptr, col, p.h, p.d, p.up, p.sum_col, gt.view, g=gg.view)
        assert got.data_ptr() == gg.view.data_ptr()
        assert tr.names() == ["anemoi_gt_edge_attention_raw:out", "anemoi_gt_edge_attention_raw:t_out"], tr.names()
        gg.assert_clean(R.raw_case_id(c) + " g")
        gt.assert_clean(R.raw_case_id(c) + " t")
        return gg.view.cpu().clone(), gt.view.cpu().clone()

    g, t = run()
    fg = _note("raw-row g", R.check(g, f.g, bg, f"{R.raw_case_id(c)} g"))
    ft = _note("raw-row t", R.check(t, f.t, bt, f"{R.raw_case_id(c)} t"))
    print(f"{R.raw_case_id(c)}: gt_edge_attention_raw_kernel<{c.ks},{c.up}>: g {fg:.3f}, t {ft:.3f} of the bound")
    assert not bool(g[p.deg == 0].any()) and not bool(t[p.deg == 0].any())
    if p.sum_col >= 0:
        sums = g.view(p.n_dst, p.h, p.ks)[:, :, p.sum_col]
        assert bool((sums[p.deg > 0] == 1.0).all())  # (l / (l + 1e-16) within 4 U of 1 is 1 in bf16)
    g2, t2 = run()
    assert torch.equal(g2, g) and torch.equal(t2, t), "a second run differs"
