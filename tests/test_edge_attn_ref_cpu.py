"""CPU-side proof for tests/test_gpu_edge_attn.py: the references of tests/_edge_attn_ref.py are right, its bounds hold for
faithful implementations and reject wrong ones -- before any GPU run.

* The f64 reference (forward and the closed-form backward) agrees with f64 autograd of an independent explicit expression built
  on ``oracle.pyg_semantics`` (segment_softmax with its 1e-16, scatter_sum), and lse with torch.logsumexp per destination.
* Emulations of the kernels' arithmetic in torch -- f32, online softmax rescaled once per chunk of four edges, operands as
  stored, one store; the backward in the ``A - Dsum B`` form with the weights rebuilt from an lse perturbed by its bound -- stay
  inside the bounds on every case of the GPU file.  The worst fractions are printed.
* Subtly wrong results do not.  Edges: the last in-edge dropped, the edge at position 4 dropped (degrees 5 and 9), an edge
  counted twice, the next destination's first edge read.  Scale and heads: no scale, the scale of another D, two heads
  swapped.  Attributes: the constant-1 column left out of the score (visible in lse alone: a per-destination constant
  cancels in the softmax), t columns rotated within a head, a t written by a lane that owns no attribute.  Residual: x_r twice,
  missing, from the neighbouring row.  lse in log2 units, lse without the maximum.  Backward: ds without - alpha Dsum, Dsum
  rebuilt from the bf16 ``out - x_r`` (on ``residual``), dk without the scale, dv weighted with ds, d attr without alpha dt, d attr
  over H - 1 heads, dq of an isolated destination non-zero.  On ``flat`` every AFFECTED DESTINATION of every case must fail for
  the edge mutants; on the other sets at least one destination fails and the test names it.
* The explicit-edge conv's forward: the reference against the project's f32 restatement (tests/_cpu_ops.py, dropout mask
  included), the emulated kernel (rescale at every edge) inside the bounds, and four mutants outside: the edge feature added to
  k but not to v, the mask in another edge order, keep not scaled by 1 / (1 - p), the normaliser over the kept edges only.
* The conv's backward (dq, dk, dv, d e): the closed forms against f64 autograd, the emulated kernels inside the bounds from an
  lse off by its bound, seven mutants outside (ds without - alpha Dsum, dk without the scale, dv weighted with ds, d e without
  either of its terms, a backward without the keep mask or with another one).
* The unfolded kernel: the reference against tests/_cpu_ops.py, the fast path's u / t form and the generic kernel's explicit e in
  f32 inside the bound; outside: the lin_edge feature added to k but not to v, lin_edge without its bias, x_r of the next row.
* The raw-row kernel: the emulation with bf16-rounded weights inside the bounds whether the normaliser sums rounded or
  unrounded weights; outside: the tail slots of a 16-edge step weighted non-zero (every destination whose degree is no multiple
  of 16), rstd dropped, the sum_col column not carrying sum alpha, heads swapped.
* What no accuracy bound can reject is asserted as such: a normaliser without the 1e-16 and a backward that forms ds directly
  (more accurate than the contract) are INSIDE the bounds.
"""

import math

import pytest
import torch

import _edge_attn_ref as R

F32, BF16 = R.F32, R.BF16
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for key in sorted(_WORST):
        print(f"[worst fraction of the bound] {key}: {_WORST[key]:.3f}")


def _note(key, fraction):
    _WORST[key] = max(_WORST.get(key, 0.0), fraction)


def _all_forward_cases():
    return R.plain_instantiation_cases() + R.plain_further_cases() + R.list_cases()


_STATE = {}


def _state(c):
    """Problem, reference and bounds of a case, computed once and shared (never modified)."""
    key = R.case_id(c)
    if key not in _STATE:
        p = R.make_problem(c)
        f = R.evaluate(p)
        _STATE[key] = (p, f, R.forward_bounds(p, f))
    return _STATE[key]


# ------------------------------------------------------------------------------------------------ references
def _explicit(p, q, k, v, xr, u, attr):
    """out, t of f64 leaves through oracle.pyg_semantics (independent of _edge_attn_ref.evaluate)."""
    from oracle.pyg_semantics import scatter_sum, segment_softmax

    h, d, up = p.h, p.d, p.up
    qh, kh, vh, uh = q.view(-1, h, d), k.view(-1, h, d), v.view(-1, h, d), u.view(-1, h, up)
    s = (torch.einsum("ehd,ehd->eh", qh[p.dst], kh[p.src]) + torch.einsum("eha,ea->eh", uh[p.dst], attr)) / math.sqrt(d)
    alpha = segment_softmax(s, p.dst, p.n_dst)
    out = scatter_sum((alpha[:, :, None] * vh[p.src]).reshape(-1, h * d), p.dst, p.n_dst) + xr
    t = scatter_sum((alpha[:, :, None] * attr[:, None, :]).reshape(-1, h * up), p.dst, p.n_dst)
    return out, t, s


@pytest.mark.parametrize("c", [R.Case(F32, 8, 3, 12, "spread"), R.Case(BF16, 16, 2, 4, "flat", graph="n9"),
                               R.Case(BF16, 8, 3, 16, "late_max", gseed=1), R.Case(F32, 4, 3, 8, "cold", gseed=2)], ids=R.case_id)
def test_reference_agrees_with_pyg_semantics_and_f64_autograd(c):
    p = R.make_problem(c)
    f = R.evaluate(p)
    dout, dtt = R.make_grads(c, p)
    b = R.evaluate_backward(p, f, dout, dtt)
    leaves = [x.double().clone().requires_grad_() for x in (p.q, p.k, p.v, p.xr, p.u, p.attr)]
    out, t, s = _explicit(p, *leaves)
    tol = lambda w: 1e-12 * (1.0 + float(w.abs().max()))  # noqa: E731
    assert float((out.detach() - f.out).abs().max()) < tol(f.out) and float((t.detach() - f.t).abs().max()) < tol(f.t)
    for i in range(p.n_dst):
        e0, e1 = int(p.rowptr[i]), int(p.rowptr[i + 1])
        want = torch.logsumexp(s.detach()[e0:e1], dim=0) if e1 > e0 else torch.full((p.h,), float("-inf"), dtype=torch.float64)
        if e1 > e0:
            assert float((f.lse[i] - want).abs().max()) < 1e-12 * (1.0 + float(want.abs().max()))
        else:
            assert bool((f.lse[i] == want).all()) and not bool(f.t[i].any()) and torch.equal(f.out[i], p.xr[i].double())
    ((out * dout.double()).sum() + (t * dtt.double()).sum()).backward()
    for key, leaf in zip(("dq", "dk", "dv", "dxr", "du", "dattr"), leaves):
        want = getattr(b, key)
        assert float((leaf.grad - want).abs().max()) < tol(want), key
    # isolated destinations and idle sources: exact zeros in the reference itself
    assert not bool(b.dq[p.deg == 0].any()) and not bool(b.du[p.deg == 0].any())
    assert not bool(b.dk[p.odeg == 0].any()) and not bool(b.dv[p.odeg == 0].any())


def test_graphs_have_what_the_cases_rely_on():
    for seed in range(4):
        rowptr, col, n_src = R.make_graph("irr", seed)
        deg = (rowptr[1:] - rowptr[:-1]).tolist()
        assert set(R.REQUIRED_DEGREES) <= set(deg) and 24 <= len(deg) <= 40 and deg[-1] == 0
        odeg = torch.bincount(col.long(), minlength=n_src)
        assert int(odeg[R.IDLE_SRC]) == 0 and int(odeg[R.HUB_SRC[0]]) >= 5 and int(odeg[R.HUB_SRC[1]]) >= 5
        dst = torch.repeat_interleave(torch.arange(len(deg)), torch.tensor(deg))
        assert len(set(dst[col.long() == R.HUB_SRC[0]].tolist())) >= 5  # one source shared by many destinations
    rowptr, col, n_src = R.make_graph("deg3")
    tri = col.view(-1, 3).long().sort(dim=1).values
    assert bool((tri[:, 1:] != tri[:, :-1]).all())
    key = (tri[:, 0] * n_src + tri[:, 1]) * n_src + tri[:, 2]
    counts = torch.unique(key, return_counts=True)[1]
    assert int(counts.max()) >= 8 and int(counts.min()) == 1 and rowptr.shape[0] - 1 >= 1.5 * counts.shape[0]


def test_data_sets_are_what_they_claim():
    for c in R.plain_instantiation_cases() + R.plain_further_cases():
        p, f, _ = _state(c)
        if p.n_edges == 0:
            continue
        share = f.alpha * p.deg[p.dst][:, None]
        if c.data in ("flat", "residual"):
            assert float(share.min()) >= math.exp(-2.0), R.case_id(c)  # every in-edge carries >= e^-2 / deg of its row
        if c.data == "cold":
            assert float(f.s.max()) < R.COLD_LEVEL
        if c.data == "late_max":
            for i in torch.nonzero(p.deg >= 2).flatten().tolist():
                e0, dg = int(p.rowptr[i]), int(p.deg[i])
                s = f.s[e0:e0 + dg]
                pos = R.late_max_position(dg, i)
                rest = torch.cat([s[:pos], s[pos + 1:]])
                gap = s[pos] - rest.amax(dim=0)
                assert 15.0 < float(gap.min()) and float(gap.max()) < 65.0


def test_torch_f32_constants_are_what_was_measured():
    got = R.measure_torch_f32()
    print({k: float(f"{v:.4g}") for k, v in got.items()})
    for key, v in R.TORCH_F32.items():
        assert abs(got[key] - v) <= 0.01 * v, f"TORCH_F32[{key!r}] = {v}, measured {got[key]:.5g}"


# ------------------------------------------------------------------------------------------------ emulation
def _edges(p, mutant=None):
    """(dst, src, attribute row, affected destinations) of the edge list the emulated kernel walks."""
    dst, src, row = p.dst.clone(), p.src.clone(), torch.arange(p.n_edges)
    pos = torch.arange(p.n_edges) - p.rowptr.long()[:-1][dst]
    deg_e = p.deg[dst]
    if mutant is None:
        return dst, src, row, None
    if mutant == "drop_last":
        keep = pos != deg_e - 1
        return dst[keep], src[keep], row[keep], torch.nonzero(p.deg >= 1).flatten()
    if mutant == "drop_pos4":
        keep = ~((pos == 4) & ((deg_e == 5) | (deg_e == 9)))
        return dst[keep], src[keep], row[keep], torch.nonzero((p.deg == 5) | (p.deg == 9)).flatten()
    if mutant == "double":
        first = torch.nonzero(pos == 0).flatten()
    elif mutant == "foreign":  # destination i also reads the first edge of the next destination that has one
        first_of = torch.full((p.n_dst + 1,), -1, dtype=torch.long)
        first_of[dst[pos == 0]] = torch.nonzero(pos == 0).flatten()
        nxt, last = [], -1
        for i in range(p.n_dst - 1, -1, -1):
            nxt.append(last)
            if int(first_of[i]) >= 0:
                last = int(first_of[i])
        nxt = torch.tensor(nxt[::-1])
        who = torch.nonzero(nxt >= 0).flatten()
        extra_dst, first = who, nxt[who]
    else:
        raise ValueError(mutant)
    extra_dst = dst[first] if mutant == "double" else extra_dst
    dst2, src2, row2 = torch.cat([dst, extra_dst]), torch.cat([src, src[first]]), torch.cat([row, row[first]])
    order = torch.argsort(dst2, stable=True)
    return dst2[order], src2[order], row2[order], torch.unique(extra_dst)


def emu_forward(p, mutant=None, scale=None, score_attr=None, eps=1e-16):
    """The plain kernel's arithmetic in torch f32: scores, the online softmax rescaled once per chunk of four edges, f32
    weights, x_r added in f32, one store.  (out, t, lse, l, m, affected destinations)."""
    h, n, d, up = p.h, p.n_dst, p.d, p.up
    f32 = torch.float32
    dst, src, row, affected = _edges(p, mutant)
    q, k, v, u = (x.float().reshape(x.shape[0], h, -1) for x in (p.q, p.k, p.v, p.u))
    a = p.attr[row]
    a_score = a if score_attr is None else score_attr[row]
    sc = torch.tensor(1.0 / math.sqrt(d) if scale is None else scale, dtype=f32)
    s = ((q[dst] * k[src]).sum(-1) + (u[dst] * a_score[:, None, :]).sum(-1)) * sc
    deg = torch.bincount(dst, minlength=n)
    start = torch.cumsum(deg, 0) - deg
    pos = torch.arange(dst.shape[0]) - start[dst]
    m = torch.full((n, h), float("-inf"), dtype=f32)
    l = torch.zeros(n, h, dtype=f32)
    acc, tacc = torch.zeros(n, h, d, dtype=f32), torch.zeros(n, h, up, dtype=f32)
    for chunk in range(-(-int(deg.max()) // R.U_EDGES) if dst.shape[0] else 0):
        sel = torch.nonzero(pos // R.U_EDGES == chunk).flatten()
        mb = torch.maximum(m, R.seg_max(s[sel], dst[sel], n))
        has = torch.zeros(n, dtype=torch.bool)
        has[dst[sel]] = True
        corr = torch.where(has[:, None], torch.exp(m - mb), torch.ones_like(m))
        corr = torch.where(torch.isnan(corr), torch.zeros_like(corr), corr)
        l, acc, tacc = l * corr, acc * corr[:, :, None], tacc * corr[:, :, None]
        for uu in range(R.U_EDGES):
            e = sel[pos[sel] % R.U_EDGES == uu]
            pe = torch.exp(s[e] - mb[dst[e]])
            l = l.index_add(0, dst[e], pe)
            acc = acc.index_add(0, dst[e], pe[:, :, None] * v[src[e]])
            tacc = tacc.index_add(0, dst[e], pe[:, :, None] * a[e][:, None, :])
        m = mb
    inv = 1.0 / (l + torch.tensor(eps, dtype=f32))
    o = (acc * inv[:, :, None]).reshape(n, h * d)
    if p.xr is not None:
        o = o + p.xr.float()
    t = (tacc * inv[:, :, None]).reshape(n, h * up)
    lse = m + torch.log(l + torch.tensor(eps, dtype=f32))
    return o.to(p.dtype), t.to(p.dtype), lse, l, m, affected


def _fractions(c, p, f, bounds, out, t, lse, tag):
    bo, bt, bl = bounds
    _note(f"emulated {tag} out", R.check(out, f.out, bo, f"{R.case_id(c)} out"))
    _note(f"emulated {tag} t", R.check(t, f.t, bt, f"{R.case_id(c)} t"))
    _note(f"emulated {tag} lse", R.check_lse(lse, f.lse, bl, f"{R.case_id(c)} lse"))


@pytest.mark.parametrize("c", _all_forward_cases(), ids=R.case_id)
def test_forward_emulation_stays_inside_the_bounds(c):
    p, f, bounds = _state(c)
    out, t, lse, *_ = emu_forward(p)
    _fractions(c, p, f, bounds, out, t, lse, R.name(c.dtype))
    iso = p.deg == 0
    assert not bool(t[iso].any()) and bool((lse[iso] == float("-inf")).all())
    assert torch.equal(out[iso], p.xr[iso] if p.xr is not None else torch.zeros_like(out[iso]))
    # what no accuracy bound can reject: the normaliser without its 1e-16 (l >= 1: 1e-16 relative) -- inside, and said so
    if p.n_edges:
        out0, t0, lse0, *_ = emu_forward(p, eps=0.0)
        ok = p.deg > 0
        assert not R.fails(out0[ok], f.out[ok], bounds[0][ok]) and not R.fails(t0[ok], f.t[ok], bounds[1][ok])
        assert not R.fails(lse0[ok], f.lse[ok], bounds[2][ok])


def _emu_backward(p, f, dout, dtt, lse_stored):
    f32 = R.evaluate(p, torch.float32)
    alpha = torch.exp(f32.s - lse_stored[p.dst])
    b32 = R.evaluate_backward(p, f32, dout, dtt, torch.float32, alpha=alpha)
    return {key: (getattr(b32, key) if key == "dattr" else getattr(b32, key).to(p.dtype)) for key in R.BACKWARD_KEYS}


def _backward_state(c):
    p, f, bounds = _state(c)
    dout, dtt = R.make_grads(c, p)
    b = R.evaluate_backward(p, f, dout, dtt)
    return p, f, bounds, dout, dtt, b


@pytest.mark.parametrize("c", R.backward_cases(), ids=R.case_id)
def test_backward_emulation_stays_inside_the_bounds(c):
    p, f, bounds, dout, dtt, b = _backward_state(c)
    g = torch.Generator().manual_seed(5)
    sign = torch.randint(0, 2, f.lse.shape, generator=g).double() * 2.0 - 1.0
    for what, lse_stored in (("rounded reference lse", f.lse.float()),
                             ("lse off by its bound", (f.lse + sign * R.finite_lse_err(bounds[2], f.lse)).float())):
        err = R.finite_lse_err((lse_stored.double() - f.lse).abs(), f.lse)
        bb = R.backward_bounds(p, f, b, err)
        got = _emu_backward(p, f, dout, dtt, lse_stored)
        for key in R.BACKWARD_KEYS:
            _note(f"emulated backward {R.name(c.dtype)} {key} ({what})",
                  R.check(got[key], getattr(b, key), bb[key], f"{R.case_id(c)} {key} {what}"))
        assert not bool(got["dq"][p.deg == 0].any()) and not bool(got["dk"][p.odeg == 0].any())
    # what no accuracy bound can reject: a backward that forms ds directly, in f64, from the true weights -- inside, of course
    bb = R.backward_bounds(p, f, b, torch.zeros_like(f.lse))
    direct = (R.seg_sum(b.ds[:, :, None] * f.k[p.src], p.dst, p.n_dst) * f.c).reshape(p.n_dst, p.c)
    assert not R.fails(direct.to(p.dtype), b.dq, bb["dq"])


# ------------------------------------------------------------------------------------------------ mutants
def _row_fails(got, want, bound):
    g = got.double()
    return ~(torch.isfinite(g) & ((g - want).abs() <= bound)).all(dim=1)


def _lse_row_fails(got, want, bound):
    g = got.double()
    iso = torch.isinf(want) & (want < 0)
    ok = torch.where(iso, g == float("-inf"), torch.isfinite(g) & ((g - want).abs() <= bound))
    return ~ok.all(dim=1)


def _forward_mutants(c, p, f):
    """{label: (out, t, lse, affected destinations or None)}: the emulated kernel with one thing wrong."""
    h, d, up, n = p.h, p.d, p.up, p.n_dst
    out, t, lse, l, m, _ = emu_forward(p)
    res = {}
    for label in ("drop_last", "drop_pos4", "double", "foreign"):
        o2, t2, l2, _, _, aff = emu_forward(p, label)
        if aff is not None and aff.numel():
            res[label] = (o2, t2, l2, aff)
    has = torch.nonzero(p.deg >= 2).flatten()
    o2, t2, l2, *_ = emu_forward(p, scale=1.0)
    res["no_scale"] = (o2, t2, l2, None)
    o2, t2, l2, *_ = emu_forward(p, scale=1.0 / math.sqrt(2 * d))
    res["scale_of_2D"] = (o2, t2, l2, None)
    perm = [1, 0] + list(range(2, h))
    res["heads_swapped"] = (out.view(n, h, d)[:, perm].reshape(n, -1), t.view(n, h, up)[:, perm].reshape(n, -1), lse[:, perm], None)
    no_bias = p.attr.clone()
    no_bias[:, up - 1] = 0.0
    o2, t2, l2, *_ = emu_forward(p, score_attr=no_bias)
    res["bias_column_not_in_score"] = (o2, t2, l2, None)
    res["t_rotated"] = (out, t.view(n, h, up).roll(1, dims=2).reshape(n, -1), lse, None)
    lph = R.lanes_per_head(c.dtype, d)
    apl = R.attrs_per_lane(up, lph)
    # (``late_max``: every head's weight sits on the same one edge, so every head has the same t and the copy is the truth)
    if lph * apl > up and c.data != "late_max":  # the first lane without an attribute stores its (a_ld = 0) accumulators behind the head's columns
        t3 = t.view(n, h, up).clone()
        t3[:, 1:, :apl] = t.view(n, h, up)[:, :-1, :apl]
        res["t_from_a_lane_without_attribute"] = (out, t3.reshape(n, -1), lse, None)
    if p.xr is not None:
        xr = p.xr.float()
        res["x_r_twice"] = ((out.float() + xr).to(p.dtype), t, lse, None)
        res["x_r_missing"] = ((out.float() - xr).to(p.dtype), t, lse, None)
        if n > 1:
            res["x_r_of_the_next_row"] = ((out.float() - xr + xr.roll(-1, dims=0)).to(p.dtype), t, lse, None)
    res["lse_in_log2_units"] = (out, t, lse / math.log(2.0), None)
    res["lse_without_the_maximum"] = (out, t, torch.log(l + 1e-16), None)
    return res, has


@pytest.mark.parametrize("c", [c for c in _all_forward_cases() if c.graph != "e0"], ids=R.case_id)
def test_forward_mutants_fail_the_bounds(c):
    p, f, (bo, bt, bl) = _state(c)
    muts, _ = _forward_mutants(c, p, f)
    must = {"drop_last", "double", "no_scale", "scale_of_2D", "heads_swapped", "bias_column_not_in_score", "t_rotated",
            "lse_in_log2_units", "lse_without_the_maximum"}
    must |= {"x_r_twice", "x_r_missing"} if c.xr else set()
    must |= {"x_r_of_the_next_row"} if c.xr and p.n_dst > 1 else set()
    must |= {"foreign"} if p.n_dst > 1 else set()
    must |= {"drop_pos4"} if bool(((p.deg == 5) | (p.deg == 9)).any()) else set()
    if R.lanes_per_head(c.dtype, c.d) * R.attrs_per_lane(c.up, R.lanes_per_head(c.dtype, c.d)) > c.up and c.data != "late_max":
        must.add("t_from_a_lane_without_attribute")
    if p.n_edges == int((p.deg > 0).sum()):  # every destination has at most one in-edge: alpha = 1 whatever the score
        must -= {"no_scale", "scale_of_2D"}
    assert must <= set(muts), sorted(must - set(muts))
    lse_only = {"bias_column_not_in_score", "lse_in_log2_units", "lse_without_the_maximum"}
    for label, (out, t, lse, aff) in muts.items():
        if not c.lse and label in lse_only:
            continue  # (a call without lse cannot show them: the constant-1 column cancels in the softmax)
        rows = _row_fails(out, f.out, bo) | _row_fails(t, f.t, bt)
        rows_all = rows | (_lse_row_fails(lse, f.lse, bl) if c.lse else torch.zeros_like(rows))
        assert bool(rows_all.any()), f"{R.case_id(c)}: mutant {label} passes"
        worst = int(torch.nonzero(rows_all).flatten()[0])
        if c.data == "flat" and aff is not None:
            # ``flat``: every in-edge carries >= e^-2 / deg of its row, so every affected destination shows it in out or t
            # (its only in-edge counted twice: alpha stays 1, lse alone moves, by ln 2)
            if label == "double":
                aff = aff[p.deg[aff] >= 2]
            assert bool(rows[aff].all()), f"{R.case_id(c)}: mutant {label} passes at destinations {aff[~rows[aff]].tolist()}"
            if label == "double" and c.lse:
                assert bool(rows_all[p.deg == 1].all())
        elif c.data == "flat" and label in ("x_r_twice", "x_r_missing", "heads_swapped"):
            sees = torch.ones_like(rows) if c.xr else p.deg > 0  # (without x_r an isolated row is zero in every head)
            assert bool(rows[sees].all()), f"{R.case_id(c)}: mutant {label} passes at destinations {torch.nonzero(~rows & sees).flatten().tolist()}"
        elif c.data == "flat" and label == "t_rotated":
            assert bool(rows[p.deg > 0].all()), f"{R.case_id(c)}: mutant {label} passes at some destination with in-edges"
        elif c.data != "flat":
            print(f"{R.case_id(c)}: {label} rejected at destination {worst} (in-degree {int(p.deg[worst])})")


@pytest.mark.parametrize("c", R.backward_cases(), ids=R.case_id)
def test_backward_mutants_fail_the_bounds(c):
    p, f, bounds, dout, dtt, b = _backward_state(c)
    # the widest bounds the GPU test uses: lse_err = the forward lse bound
    bb = R.backward_bounds(p, f, b, R.finite_lse_err(bounds[2], f.lse))
    n, h = p.n_dst, p.h
    cast = lambda x: x.to(p.dtype)  # noqa: E731
    kj, qi, a3 = f.k[p.src], f.q[p.dst], f.a[:, None, :]
    muts = {}
    muts["ds_without_alpha_Dsum"] = ("dq", cast((R.seg_sum(b.w[:, :, None] * kj, p.dst, n) * f.c).reshape(n, -1)))
    muts["dk_without_the_scale"] = ("dk", cast(b.dk / f.c))
    muts["dv_weighted_with_ds"] = ("dv", cast(R.seg_sum(b.ds[:, :, None] * b.do[p.dst], p.src, p.n_src).reshape(p.n_src, -1)))
    muts["dattr_without_alpha_dt"] = ("dattr", (f.c * b.ds[:, :, None] * f.u[p.dst]).sum(1).float())
    muts["dattr_over_H-1_heads"] = ("dattr", (f.c * b.ds[:, :, None] * f.u[p.dst] + f.alpha[:, :, None] * b.dth[p.dst])[:, :h - 1].sum(1).float())
    if bool((p.deg == 0).any()):
        stale = b.dq.clone()
        stale[p.deg == 0] = 1e-3  # stale memory of plausible magnitude
        muts["dq_of_an_isolated_destination_non-zero"] = ("dq", cast(stale))
        idle = b.dv.clone()
        idle[p.odeg == 0] = 1e-3
        muts["dv_of_an_idle_source_non-zero"] = ("dv", cast(idle))
    if c.data == "residual" and c.dtype == BF16:
        # Dsum rebuilt as dout . (out - x_r) from the ROUNDED out: in bf16 the difference cancels against the 64 x residual
        attn_r = (f.out.to(p.dtype).double() - p.xr.double()).view(n, h, p.d)
        dsum = (b.do * attn_r).sum(-1) + (b.dth * f.t.to(p.dtype).double().view(n, h, p.up)).sum(-1)
        ds = b.w - f.alpha * dsum[p.dst]
        muts["Dsum_from_the_rounded_out"] = ("dq", cast((R.seg_sum(ds[:, :, None] * kj, p.dst, n) * f.c).reshape(n, -1)))
    for label, (key, got) in muts.items():
        want, bound = getattr(b, key), bb[key]
        rows = _row_fails(got, want, bound)
        assert bool(rows.any()), f"{R.case_id(c)}: backward mutant {label} passes"
        if c.data != "flat":
            print(f"{R.case_id(c)}: {label} rejected at row {int(torch.nonzero(rows)[0])} of {key}")
    assert c.data != "residual" or c.dtype != BF16 or "Dsum_from_the_rounded_out" in muts


# ------------------------------------------------------------------------------------------------ explicit-edge conv, forward
def _conv_keep(c, p, seed=R.CONV_SEED):
    from _cpu_ops import edge_dropout_keep_mask

    return edge_dropout_keep_mask(seed, c.p, p.n_edges, p.h) if c.p > 0.0 else None


def emu_conv(p, keep, pdrop, norm_over_kept=False, scale_keep=True):
    """gt_conv_kernel's arithmetic in torch f32: k + e and v + e formed in f32, the online softmax rescaled at every edge, the
    weight times keep / (1 - p), x_r added in f32, one store."""
    h, n, d = p.h, p.n_dst, p.d
    f32 = torch.float32
    q, k, v, e = (x.float().reshape(x.shape[0], h, d) for x in (p.q, p.k, p.v, p.e))
    kj, vj = k[p.src] + e, v[p.src] + e
    s = (q[p.dst] * kj).sum(-1) * torch.tensor(1.0 / math.sqrt(d), dtype=f32)
    kk = torch.ones_like(s) if keep is None else keep.float() * torch.tensor((1.0 / (1.0 - pdrop) if pdrop < 1.0 else 0.0) if scale_keep else 1.0, dtype=f32)
    pos = torch.arange(p.n_edges) - p.rowptr.long()[:-1][p.dst]
    m = torch.full((n, h), float("-inf"), dtype=f32)
    l, acc = torch.zeros(n, h, dtype=f32), torch.zeros(n, h, d, dtype=f32)
    for step in range(int(p.deg.max()) if p.n_edges else 0):
        ed = torch.nonzero(pos == step).flatten()
        i = p.dst[ed]
        mn = torch.maximum(m[i], s[ed])
        corr = torch.exp(m[i] - mn)
        pe = torch.exp(s[ed] - mn)
        counted = pe * keep[ed].float() if norm_over_kept and keep is not None else pe
        l[i] = l[i] * corr + counted
        acc[i] = (pe * kk[ed])[:, :, None] * vj[ed] + acc[i] * corr[:, :, None]
        m[i] = mn
    o = (acc * (1.0 / (l + 1e-16))[:, :, None]).reshape(n, h * d)
    if norm_over_kept:
        o = torch.where(torch.isfinite(o), o, torch.zeros_like(o))
    if p.xr is not None:
        o = o + p.xr.float()
    return o.to(p.dtype), m + torch.log(l + 1e-16)


def test_conv_torch_f32_constants_are_what_was_measured():
    got = R.measure_torch_f32_conv()
    for key, v in R.TORCH_F32_CONV.items():
        assert abs(got[key] - v) <= 0.01 * v, f"TORCH_F32_CONV[{key!r}] = {v}, measured {got[key]:.5g}"


@pytest.mark.parametrize("c", R.conv_cases(), ids=R.conv_case_id)
def test_conv_reference_emulation_and_mutants(c):
    import _cpu_ops

    p = R.make_conv_problem(c)
    keep = _conv_keep(c, p)
    f = R.evaluate_conv(p, keep=keep, pdrop=c.p)
    bo, bl = R.conv_forward_bounds(p, f)
    # the reference against the project's f32 restatement of the conv (oracle.pyg_semantics underneath), dropout mask included
    want = _cpu_ops.gt_conv(p.q.float(), p.k.float(), p.v.float(), p.e.float(), p.rowptr, p.col, p.h, x_r=p.xr.float(), dropout_p=c.p,
                            dropout_seed=R.CONV_SEED)
    assert float((want.double() - f.out).abs().max()) <= 2e-5 * (1.0 + float(f.out.abs().max()))
    if keep is not None and c.p < 1.0:
        assert abs(float(keep.mean()) - (1.0 - c.p)) < 0.06
    # the emulated kernel is inside the bounds
    out, lse = emu_conv(p, keep, c.p)
    _note(f"emulated conv {R.name(c.dtype)} out", R.check(out, f.out, bo, f"{R.conv_case_id(c)} out"))
    _note(f"emulated conv {R.name(c.dtype)} lse", R.check_lse(lse, f.lse, bl, f"{R.conv_case_id(c)} lse"))
    if c.p >= 1.0:
        assert torch.equal(out, p.xr)  # everything dropped: x_r, exactly
        return
    # mutants: the lin_edge feature added to k but not to v
    g = R.evaluate_conv(p, keep=keep, pdrop=c.p, e_in_v=False)
    assert R.fails(g.out.to(p.dtype), f.out, bo), "e added to k alone passes"
    if keep is None:
        return
    # the mask indexed by the caller's edge order instead of the CSR position (here: the reversed order)
    g = R.evaluate_conv(p, keep=keep.flip(0), pdrop=c.p)
    assert R.fails(g.out.to(p.dtype), f.out, bo), "a mask in another edge order passes"
    # keep not scaled by 1 / (1 - p); the normaliser taken over the kept edges only
    assert R.fails(emu_conv(p, keep, c.p, scale_keep=False)[0], f.out, bo), "an unscaled keep passes"
    o2, l2 = emu_conv(p, keep, c.p, norm_over_kept=True)
    assert R.fails(o2, f.out, bo) and R.lse_fails(l2, f.lse, bl), "a normaliser over the kept edges passes"


# ------------------------------------------------------------------------------------------------ explicit-edge conv, backward
def test_conv_backward_torch_f32_constants_are_what_was_measured():
    got = R.measure_torch_f32_conv_backward()
    for key, v in R.TORCH_F32_CONV_BWD.items():
        assert abs(got[key] - v) <= 0.01 * v, f"TORCH_F32_CONV_BWD[{key!r}] = {v}, measured {got[key]:.5g}"


@pytest.mark.parametrize("c", R.conv_cases(), ids=R.conv_case_id)
def test_conv_backward_reference_emulation_and_mutants(c):
    p = R.make_conv_problem(c)
    keep = R.conv_keep(c, p)
    dout, _ = R.make_grads(c, p)
    f = R.evaluate_conv(p, keep=keep, pdrop=c.p)
    b = R.evaluate_conv_backward(p, f, dout)
    # the closed forms against f64 autograd of the explicit expression (oracle.pyg_semantics)
    from oracle.pyg_semantics import scatter_sum, segment_softmax

    leaves = [x.double().clone().requires_grad_() for x in (p.q, p.k, p.v, p.e, p.xr)]
    q, k, v, e = (x.view(x.shape[0], p.h, p.d) for x in leaves[:4])
    s = ((q[p.dst] * (k[p.src] + e)).sum(-1)) / math.sqrt(p.d)
    al = segment_softmax(s, p.dst, p.n_dst) * f.kk
    out = scatter_sum((al[:, :, None] * (v[p.src] + e)).reshape(-1, p.c), p.dst, p.n_dst) + leaves[4]
    (out * dout.double()).sum().backward()
    for key, leaf in zip(("dq", "dk", "dv", "de"), leaves):
        want = getattr(b, key)
        assert float((leaf.grad - want).abs().max()) < 1e-12 * (1.0 + float(want.abs().max())), key
    assert torch.equal(leaves[4].grad, dout.double())
    # the emulated kernels (f32, A - Dsum B, weights rebuilt from an lse off by the forward's bound) inside the bounds
    _, bl = R.conv_forward_bounds(p, f)
    g = torch.Generator().manual_seed(11)
    sign = torch.randint(0, 2, f.lse.shape, generator=g).double() * 2.0 - 1.0
    lse_st = (f.lse + sign * R.finite_lse_err(bl, f.lse)).float()
    err = R.finite_lse_err((lse_st.double() - f.lse).abs(), f.lse)
    bb = R.conv_backward_bounds(p, f, b, err)
    f32 = R.evaluate_conv(p, torch.float32, keep=keep, pdrop=c.p)
    b32 = R.evaluate_conv_backward(p, f32, dout, torch.float32, alpha=torch.exp(f32.s - lse_st[p.dst]))
    for key in R.CONV_BACKWARD_KEYS:
        _note(f"emulated conv backward {R.name(c.dtype)} {key}",
              R.check(getattr(b32, key).to(p.dtype), getattr(b, key), bb[key], f"{R.conv_case_id(c)} {key}"))
    if c.p >= 1.0:
        assert not any(bool(getattr(b, key).any()) for key in R.CONV_BACKWARD_KEYS)  # everything dropped: exact zeros
        return
    if p.n_edges == int((p.deg > 0).sum()):
        return  # (one in-edge per destination: ds = 0 whatever is wrong with it)
    # mutants, against the widest bounds the GPU test uses (lse_err = the forward's lse bound)
    bb = R.conv_backward_bounds(p, f, b, R.finite_lse_err(bl, f.lse))
    cast = lambda x: x.to(p.dtype)  # noqa: E731
    n = p.n_dst
    muts = {"ds_without_alpha_Dsum": ("dq", (R.seg_sum(b.w[:, :, None] * b.kj, p.dst, n) * b.c).reshape(n, -1)),
            "dk_without_the_scale": ("dk", b.dk / b.c),
            "dv_weighted_with_ds": ("dv", R.seg_sum(b.ds[:, :, None] * b.doi, p.src, p.n_src).reshape(p.n_src, -1)),
            "de_without_the_dv_term": ("de", ((b.c * b.ds)[:, :, None] * b.qi).reshape(p.n_edges, -1)),
            "de_without_the_dk_term": ("de", ((b.al * b.kk)[:, :, None] * b.doi).reshape(p.n_edges, -1))}
    if keep is not None:
        nokeep = R.evaluate_conv_backward(p, R.evaluate_conv(p), dout)
        muts["backward_without_the_keep_mask"] = ("dv", nokeep.dv)
        other = R.evaluate_conv_backward(p, R.evaluate_conv(p, keep=keep.flip(0), pdrop=c.p), dout)
        muts["backward_with_another_mask"] = ("de", other.de)
    for label, (key, got) in muts.items():
        assert R.fails(cast(got), getattr(b, key), bb[key]), f"{R.conv_case_id(c)}: conv backward mutant {label} passes"


# ------------------------------------------------------------------------------------------------ unfolded kernel
def emu_unfolded_fast(p):
    """The fast path's arithmetic in torch f32: u = W_h^T q and the bias term per destination, scores q . k + u . a + u_b, the
    sums of pe v, pe a and pe, out = (acc + b l + W t) / (l + 1e-16) + x_r, one store."""
    h, n, d = p.h, p.n_dst, p.d
    q, k, v = (x.float().reshape(x.shape[0], h, d) for x in (p.q, p.k, p.v))
    w, b, a = p.w.reshape(h, d, -1), p.b.reshape(h, d), p.attr[:, :p.edge_dim]
    u = torch.einsum("hda,nhd->nha", w, q)
    ub = torch.einsum("hd,nhd->nh", b, q)
    s = ((q[p.dst] * k[p.src]).sum(-1) + (u[p.dst] * a[:, None, :]).sum(-1) + ub[p.dst]) * torch.tensor(1.0 / math.sqrt(d))
    m = R.seg_max(s, p.dst, n)
    pe = torch.exp(s - m[p.dst])
    l = R.seg_sum(pe, p.dst, n)
    acc = R.seg_sum(pe[:, :, None] * v[p.src], p.dst, n)
    t = R.seg_sum(pe[:, :, None] * a[:, None, :], p.dst, n)
    o = (acc + b[None] * l[:, :, None] + torch.einsum("hda,nha->nhd", w, t)) * (1.0 / (l + 1e-16))[:, :, None]
    return (o.reshape(n, -1) + p.xr.float()).to(p.dtype)


def test_unfolded_torch_f32_constant_is_what_was_measured():
    got = R.measure_torch_f32_unfolded()["out"]
    assert abs(got - R.TORCH_F32_UNFOLDED["out"]) <= 0.01 * R.TORCH_F32_UNFOLDED["out"], got


@pytest.mark.parametrize("c", R.unfolded_cases(), ids=R.unfolded_case_id)
def test_unfolded_reference_emulations_and_mutants(c):
    import _cpu_ops

    p = R.make_unfolded_problem(c)
    f = R.evaluate_unfolded(p)
    bo = R.unfolded_bounds(p, f)
    want = _cpu_ops.gt_edge_attention(p.q.float(), p.k.float(), p.v.float(), p.xr.float(), p.attr, p.edge_dim, p.w, p.b, p.rowptr, p.col, p.h)
    assert float((want.double() - f.out).abs().max()) <= 2e-5 * (1.0 + float(f.out.abs().max()))
    # both kernels' forms in f32: the fast path's u / t form, the generic kernel's explicit e
    _note(f"emulated unfolded fast {R.name(c.dtype)} out", R.check(emu_unfolded_fast(p), f.out, bo, f"{R.unfolded_case_id(c)} fast form"))
    g32 = R.evaluate_unfolded(p, torch.float32)
    _note(f"emulated unfolded generic {R.name(c.dtype)} out", R.check(g32.out.to(p.dtype), f.out, bo, f"{R.unfolded_case_id(c)} explicit form"))
    iso = p.deg == 0
    assert torch.equal(emu_unfolded_fast(p)[iso], p.xr[iso])
    # mutants: the lin_edge feature added to k but not to v, its bias left out, no scale
    assert R.fails(R.evaluate_unfolded(p, e_in_v=False).out.to(p.dtype), f.out, bo), "e added to k alone passes"
    assert R.fails(R.evaluate_unfolded(p, bias=False).out.to(p.dtype), f.out, bo), "lin_edge without its bias passes"
    shifted = R.evaluate_unfolded(p).out - p.xr.double() + p.xr.double().roll(1, dims=0)
    assert p.n_dst == 1 or R.fails(shifted.to(p.dtype), f.out, bo), "x_r of the neighbouring row passes"
    R.evaluate_unfolded(p)  # (leaves p.e as the reference's)


# ------------------------------------------------------------------------------------------------ raw-row kernel
def emu_raw(p, rounded_normaliser=False, tail_weight=0.0, rstd_on=True, sum_col_is_sum=True):
    """The raw-row kernel's arithmetic in torch f32: scores rstd (qt . x) + u . a, weights pe rstd rounded to bf16 before the
    aggregate, the normaliser over the unrounded (or the rounded) pe, bf16 stores.  ``tail_weight``: the mutant that gives the
    empty slots of a 16-edge step (which repeat the segment's last edge) a weight."""
    n, h = p.n_dst, p.h
    qt, x, u, a = p.qt.float().view(n, h, p.ks), p.x.float(), p.u.float().view(n, h, p.up), p.attr
    rs = p.stats[:, 0] if rstd_on else torch.ones(p.n_src)
    xj, rj = x[p.src], rs[p.src]
    s = (rj[:, None] * torch.einsum("ehk,ek->eh", qt[p.dst], xj) + torch.einsum("eha,ea->eh", u[p.dst], a)) * torch.tensor(1.0 / math.sqrt(p.d))
    m = R.seg_max(s, p.dst, n)
    pe = torch.exp(s - m[p.dst])
    l = R.seg_sum(pe.bfloat16().float() if rounded_normaliser else pe, p.dst, n)
    wgt = (pe * rj[:, None]).bfloat16().float()
    g = R.seg_sum(wgt[:, :, None] * xj[:, None, :], p.dst, n)
    t = R.seg_sum(pe[:, :, None] * a[:, None, :], p.dst, n)
    if tail_weight:
        last = (p.rowptr.long()[1:] - 1)[p.deg > 0]
        slots = ((-p.deg[p.deg > 0]) % 16).float()
        g[p.deg > 0] += (tail_weight * slots)[:, None, None] * (wgt[last][:, :, None] * xj[last][:, None, :])
    inv = 1.0 / (l + 1e-16)
    g = g * inv[:, :, None]
    if p.sum_col >= 0 and sum_col_is_sum:
        g[:, :, p.sum_col] = l * inv
    return g.reshape(n, -1).bfloat16(), (t * inv[:, :, None]).reshape(n, -1).bfloat16()


@pytest.mark.parametrize("c", R.raw_cases(), ids=R.raw_case_id)
def test_raw_row_reference_emulation_and_mutants(c):
    p = R.make_raw_problem(c)
    assert set(R.RAW_DEGREES) <= set(p.deg.tolist())
    f = R.evaluate_raw(p)
    bg, bt = R.raw_bounds(p, f)
    for rounded in (False, True):  # the bound holds whether the normaliser sums rounded or unrounded weights
        g, t = emu_raw(p, rounded_normaliser=rounded)
        tag = "rounded" if rounded else "unrounded"
        _note(f"emulated raw g ({tag} normaliser)", R.check(g, f.g, bg, f"{R.raw_case_id(c)} g {tag}"))
        _note(f"emulated raw t ({tag} normaliser)", R.check(t, f.t, bt, f"{R.raw_case_id(c)} t {tag}"))
        assert not bool(g[p.deg == 0].any()) and not bool(t[p.deg == 0].any())
    # mutants
    g, _ = emu_raw(p, tail_weight=1.0)
    rows = ~((g.double() - f.g).abs() <= bg).all(dim=1)
    tails = (p.deg > 0) & (p.deg % 16 != 0)
    assert bool(rows[tails].all()), "tail slots of a 16-edge step weighted non-zero pass"
    assert R.fails(emu_raw(p, rstd_on=False)[0], f.g, bg), "rstd dropped passes"
    if p.sum_col >= 0:
        assert R.fails(emu_raw(p, sum_col_is_sum=False)[0], f.g, bg), "sum_col not carrying sum alpha passes"
    gs, ts = emu_raw(p)
    assert R.fails(gs.view(p.n_dst, p.h, -1)[:, [1, 0] + list(range(2, p.h))].reshape(p.n_dst, -1), f.g, bg), "heads swapped pass"
