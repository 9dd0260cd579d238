"""CPU checks of tests/_linear_ref.py, the reference side of tests/test_gpu_linear.py:
  * the restated dispatch reaches every route on the case table (every tile height whole and ragged, every tail template, the
    stand-alone skinny kernel, the 128 x 128 tail, nt in {1, < 8, 16, 17..23, 24}, split, stagger, the skipped cost model, the
    batched walk, both vector states of the 128 x 128 kernel) and every case names the route it gets;
  * the restated dispatch IS the library's: ``anemoi_linear_route`` (the entry points' own validation and plan, no GPU) gives
    the same route on every case of the table and on a sweep of 443 520 argument sets, launch for launch; the two lab
    switches reach the plan (a fresh child process each);
  * emulations of the kernels' arithmetic stay inside the bounds on every data kind: bf16 products exact in f32, f32
    accumulation in slab order, the skinny passes' lane-strided fmaf chain and butterfly, the epilogue in f32 with the
    documented polynomials (as numbers, _linear_ref.GELU_Q / DGELU_Q), round / add residual / round again -- at every case small
    enough, on row samples of the others;
  * the wrong kernels listed in ``MUTANTS`` leave the bounds at the cases named for them; ``exact`` data catches the index
    mutants with bound 0.
One mutant is INSIDE the bounds by derivation, and asserted to be: one rounding where round / add / round is specified (closer
to the truth than the contract, as for LayerNorm + residual in _row_kernels_ref).  Statistics of the unrounded y move the
variance by about 2^-16 / 3 relative: above the depth-derived summation bound of the fused statistics, so that mutant is
rejected on ordinary rows as well as on the cancellation rows (y = 300 / 302).  ``act`` of the rounded ``pre`` in dual is
OUTSIDE: its error reaches 1.13 x 2^-8 |z| + 2^-8 |y| against a bound of 2^-8 |y| (1 + small).
"""

import types

import pytest
import torch

import _linear_ref as R

F32, BF16 = R.F32, R.BF16
SMALL = 2e8


def bf(t):
    return t.bfloat16().float()


def _horner(t, q):
    acc = torch.full_like(t, q[0])
    for coef in q[1:]:
        acc = acc * t + torch.tensor(coef, dtype=torch.float32)
    return acc


def gelu_poly(x, q=R.GELU_Q):
    xc = x.clamp(-4.5, 4.5)
    return x * (xc * _horner(xc * xc, q) + 0.5)


def dgelu_poly(x, q=R.DGELU_Q):
    xc = x.clamp(-4.0, 4.0)
    return xc * _horner(xc * xc, q) + 0.5


# a coefficient off in its fourth digit: 0.39871 -> 0.3990 (forward), 0.79756 -> 0.7980 (derivative)
GELU_Q_WRONG = R.GELU_Q[:-1] + (0.3990,)
DGELU_Q_WRONG = R.DGELU_Q[:-1] + (0.7980,)


def act32(x, act, poly_rows, mut=None):
    if act == "GELU":
        if mut == "tanh_gelu":
            return torch.nn.functional.gelu(x, approximate="tanh")
        erf_form = 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752440))
        return torch.where(poly_rows[:, None], gelu_poly(x, GELU_Q_WRONG if mut == "gelu_q_digit" else R.GELU_Q), erf_form)
    if act == "SiLU":
        return x * torch.sigmoid(x)
    if act == "ReLU":
        return x.clamp_min(0.0)
    return x


def dact32(x, act, py_rows, mut=None):
    if act == "GELU":
        if mut == "dgelu_no_xphi":
            return 0.5 * (1.0 + torch.erf(x * 0.70710678118654752440))
        return torch.where(py_rows[:, None], R.dact64(x, act).float(),
                           dgelu_poly(x, DGELU_Q_WRONG if mut == "dgelu_q_digit" else R.DGELU_Q))
    if act == "SiLU":
        sg = torch.sigmoid(x)
        return sg if mut == "dsilu_sigmoid" else sg * (x * (1.0 - sg) + 1.0)
    return (x > 0).float()


def slab_product(x, w, slab, mut=None):
    """f32 accumulation in slab order (products of bf16 values are exact in f32)."""
    acc = torch.zeros((x.shape[0], w.shape[0]), dtype=torch.float32)
    n_slabs = x.shape[1] // slab
    for s in range(n_slabs - (1 if mut == "drop_slab" else 0)):
        acc = acc + x[:, s * slab:(s + 1) * slab].float() @ w[:, s * slab:(s + 1) * slab].float().T
        if mut == "acc_bf16":
            acc = bf(acc)
    return acc


def skinny_product(x, w, mut=None):
    """skinny_column(s): lane l takes the 8-element chunks at k = 8 l + 512 j, a fmaf chain per lane, then the xor butterfly."""
    x, w = x.float(), w.float()
    r, k = x.shape
    kp = (k + 511) // 512 * 512
    xp, wp = torch.zeros((r, kp)), torch.zeros((w.shape[0], kp))
    xp[:, :k], wp[:, :k] = x, w
    if mut == "drop_chunk":
        xp[:, 8:16] = 0.0
    xp, wp = xp.reshape(r, 1, kp // 512, 64, 8), wp.reshape(1, w.shape[0], kp // 512, 64, 8)
    acc = torch.zeros((r, w.shape[0], 64))
    for j in range(kp // 512):
        for i in range(8):
            acc = acc + xp[:, :, j, :, i] * wp[:, :, j, :, i]  # exact product, one rounding: fmaf
    lanes = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, :, lanes ^ off]
    return acc[:, :, 0]


def emulate(c, o, rt, rows=None, mut=None):
    """A correct (mut None) or subtly wrong kernel set in f32; {name: tensor in the output dtype}."""
    ridx = torch.arange(c.m) if rows is None else rows
    slab = 64 if c.dtype == BF16 else 32
    x = o.x[ridx]
    main = rt.main_rows if rt.kernel == "w4" else c.m // 256 * 256
    skinny = (ridx >= main) & (rt.tail.startswith("in") or rt.tail == "skinny")
    poly, two = R._row_flags(c, rt)
    poly, two = poly[ridx], two[ridx]
    py = torch.zeros(c.m, dtype=torch.bool)
    if rt.kernel == "py":
        py[:] = True
    elif rt.tail == "py":
        py[main:] = True
    py = py[ridx]
    heads = []
    for j in range(max(c.h, 1)):
        w = o.w if not c.h else o.w[(j - 1) % c.h if mut == "w_prev" else j]
        xj = x[:, j * c.k:(j + 1) * c.k]
        acc = slab_product(xj, w, slab, mut)
        if bool(skinny.any()):
            acc[skinny] = skinny_product(xj[skinny], w, mut)
        heads.append(acc)
    acc = torch.cat(heads, dim=1)
    n = acc.shape[1]
    cols = torch.arange(n)
    b = torch.zeros(n) if o.bias is None else o.bias.clone()
    if mut == "bias_shift4":
        b = torch.roll(b, -4)
    elif mut == "bias_shift8":
        b = torch.roll(b, -8)
    elif mut == "bias_tile_rel":
        b = b[cols % 256]
    store = bf if c.out == BF16 else (lambda t: t)
    out = {}
    if c.kind == "actgrad":
        pre = o.pre[ridx].float()
        g = dact32(pre, c.act, py, mut)
        out["y"] = bf(torch.where(py[:, None], bf(acc), acc) * g)
        return out
    if c.fold:
        sidx = ridx.clone()
        tm = 32 * rt.mh if rt.mh else 128
        if mut == "stats_tile_rel":
            sidx = ridx % tm
        elif mut == "stats_b_no_offset":
            sidx = torch.where((ridx >= rt.m_a) & (ridx < main), ridx - rt.m_a, ridx)
        elif mut == "tail_stats_0_7":
            sidx = torch.where(ridx >= main, ridx - main, ridx)
        st = o.stats[sidx]
        cs = torch.roll(o.colsum, -4) if mut == "colsum_shift" else o.colsum
        t2 = st[:, 1:] * cs[None, :]
        if mut == "fold_no_shift":
            t2 = torch.zeros_like(t2)
        z = torch.where(poly[:, None] | (rt.kernel == "w4") & ~skinny[:, None], acc * st[:, :1] + (t2 + b[None, :]),
                        (acc * st[:, :1] + t2) + b[None, :])
    else:
        z = acc + b[None, :]
    if c.kind == "dual":
        a = act32(z, c.act, poly & ~py, mut)
        out["pre"] = bf(a) if mut == "pre_activated" else bf(z)
        rounded = act32(bf(z), c.act, poly & ~py, mut)
        out["y"] = bf(rounded) if mut == "act_rounded_pre" else bf(torch.where(py[:, None], rounded, a))
        return out
    if o.res is None:
        a = act32(z, c.act, poly, mut)
        unrounded = a
    else:
        r = o.res[(ridx + 1) % c.m if mut == "res_next_row" else (ridx - 1) % c.m if mut == "res_prev_row" else ridx].float()
        if mut == "res_before_act":
            a = act32(z + r, c.act, poly, mut)
            unrounded = a
        else:
            a = act32(z, c.act, poly, mut)
            tw = two if mut is None or mut not in ("single_round", "double_round") else \
                (torch.zeros_like(two) if mut == "single_round" else torch.ones_like(two))
            unrounded = torch.where(tw[:, None] & (c.out == BF16), bf(a), a) + r
    y = store(unrounded)
    out["y"] = y.to(c.out)
    if c.stats:
        src = unrounded if mut == "stats_unrounded" else y
        inv_c = torch.tensor(1.0 / (n + (8 if mut == "stats_ldy" else 0)), dtype=torch.float32)
        s, ss = src.sum(dim=1), (src * src).sum(dim=1)
        mean = s * inv_c
        var1 = (ss * inv_c - mean * mean).clamp_min(0.0)
        d = src - mean[:, None]
        var2 = (d * d).sum(dim=1) * inv_c
        tiled = ridx < main
        if rt.rs:
            var = torch.where(tiled & (var1 < 1e-3 * ss * inv_c), var2, var1)
        else:
            var = var2
        rstd = torch.rsqrt(var + torch.tensor(R.EPS, dtype=torch.float32))
        out["stats"] = torch.stack([rstd, -mean * rstd], dim=1)
    return out


def _rows_for(c, rt):
    if c.m * c.n * c.k * max(c.h, 1) <= SMALL:
        return None
    return R.sample_rows(c, rt, 32)


_CACHE = {}


def _setup(c):
    key = R.case_id(c)
    if key not in _CACHE:
        if len(_CACHE) > 6:
            _CACHE.clear()
        o = R.operands(c)
        rt = R.case_route(c)
        rows = _rows_for(c, rt)
        _CACHE[key] = (o, rt, rows, R.reference(c, o, rt, rows=rows))
    return _CACHE[key]


def _stats_want(c, rt, y, rows):
    """stats_ref on a row sample: the bound's route flags follow the original row numbers."""
    if rows is None:
        return R.stats_ref(y, c.n, rt, c.m)
    main = int((rows < rt.main_rows).sum())
    sub = types.SimpleNamespace(**{**vars(rt), "main_rows": main})
    return R.stats_ref(y, c.n, sub, len(rows))


# ------------------------------------------------------------------------------------------------ routes
def test_every_case_names_its_route():
    for c in R.all_cases():
        assert R.route_str(R.case_route(c)) == c.expect, R.case_id(c)
    assert len({R.case_id(c) for c in R.all_cases()}) == len(R.all_cases())


def test_case_table_reaches_every_route():
    rts = [(c, R.case_route(c)) for c in R.all_cases()]
    w4 = [(c, rt) for c, rt in rts if rt.kernel == "w4"]
    plain = [(c, rt) for c, rt in w4 if c.kind == "linear"]
    assert {(rt.mh, rt.ragged_m) for _, rt in plain if not rt.second} >= {(h, r) for h in (3, 4, 5, 6, 8) for r in (False, True)}
    for h in (3, 4, 5, 6, 8):  # every height with every epilogue of the list, whole and ragged
        for r in (False, True):
            epis = {(c.act, c.res, c.fold, c.stats) for c, rt in plain if rt.mh == h and rt.ragged_m == r and not rt.second}
            assert len(epis) >= 5, (h, r, epis)
    for kind in ("linear", "dual", "actgrad"):
        assert {rt.tail for c, rt in w4 if c.kind == kind} >= {"in1", "in2", "in4", "in8"}, kind
    assert {(c.fold, c.res) for c, rt in w4 if rt.tail.startswith("in") and c.kind == "linear"} >= {(False, False), (True, False),
                                                                                                   (False, True), (True, True)}
    assert {rt.tail for c, rt in rts if rt.kernel == "k128"} >= {"none", "skinny", "k128"}
    nts = {rt.nt for _, rt in w4}
    assert 1 in nts and nts & set(range(2, 8)) and 16 in nts and len(nts & set(range(17, 24))) >= 3 and 24 in nts
    assert {rt.rem for _, rt in w4 if 17 <= rt.nt <= 23} >= {9, 10, 15}
    assert any(rt.nt < 8 and rt.ragged_n for _, rt in w4) and any(rt.nt > 16 and rt.ragged_n for _, rt in w4)
    assert any(rt.second and rt.m_a > 0 and c.fold and c.res and c.stats for c, rt in w4)  # launch A + launch B
    assert any(rt.second and rt.m_a == 0 and c.kind == kind for c, rt in w4 for kind in ("dual",))  # whole-problem split
    assert any(rt.second and rt.m_a == 0 and c.kind == "actgrad" for c, rt in w4)
    assert any(rt.stagger for _, rt in w4) and any(not rt.model and not rt.batched and c.kind == "linear" for c, rt in w4)
    assert any(rt.batched and rt.ragged_m and rt.ragged_n and c.h == 3 for c, rt in w4)
    assert any(rt.batched and rt.kernel == "k128" and c.dtype == F32 for c, rt in rts)
    assert any(rt.batched and rt.kernel == "k128" and c.dtype == BF16 and c.out == F32 for c, rt in rts)
    assert any(rt.batched and rt.kernel == "k128" and c.k < 128 for c, rt in rts)
    assert any(rt.batched and rt.kernel == "k128" and c.n % 8 for c, rt in rts)
    for dtype, out in ((F32, F32), (BF16, BF16), (BF16, F32)):
        assert {rt.vec_ok for c, rt in rts if rt.kernel == "k128" and (c.dtype, c.out) == (dtype, out) and not c.h} == {True, False}
    assert any(rt.rs for _, rt in w4) and any(c.stats and not rt.rs for c, rt in rts)
    assert any(rt.kernel == "py" for _, rt in rts) and any(rt.tail == "py" for _, rt in rts)
    assert {c.data for c in R.all_cases()} >= {"ordinary", "exact", "cancel", "spike", "fold_mean", "b300"}


def test_tile_walk_covers_every_tile_once():
    """tile_coords as restated: a permutation of the tile grid for every column count of the table (remainder groups 9..15 wide)."""
    for nt in sorted({R.case_route(c).nt for c in R.all_cases() if R.case_route(c).kernel == "w4"}):
        for mt in (1, 4, 11):
            seen = {R.tile_coords(t, nt, mt) for t in range(mt * nt)}
            assert seen == {(i, j) for i in range(mt) for j in range(nt)}, (nt, mt)


# ------------------------------------------------------------------------------------------------ the library's own route
# ``anemoi_linear_route`` runs the validation and the plan of the entry points on integers (no GPU, nothing launched): the
# restatement above is held against it, so "the launcher takes X" in tests/test_gpu_linear.py describes the launcher itself.
FAKE = dict(x=0x10000000, w=0x20000000, y=0x30000000, bias=0x40000000, residual=0x50000000, colsum=0x60000000,
            stats=0x70000000, workspace=0x80000000, stats_out=0x90000000)  # 16-byte aligned stand-ins: only looked at, never read


def library_route(dtype, out_dtype, M, N, K, ldx, ldy, ldr, ptrs, act="Identity", res=False, fold=False, stats=False, epi=0,
                  batch=0, x=FAKE["x"], w=FAKE["w"]):
    """The arguments of ``_linear_ref.route`` handed to the library the way ops.py hands them over; ``ptrs`` = (y, bias, residual
    or pre, colsum) are real addresses here, 0 = absent.  (status, raw route, rows handed to the library)."""
    from anemoi_models_amd import _lib, ops

    code = {F32: _lib.F32, BF16: _lib.BF16}
    y, b, r, cs = ptrs
    a = dict(dtype=code[dtype], out_dtype=code[out_dtype], x=x, w=w, y=y, bias=b, ldx=ldx, ldy=ldy, M=M, N=N, K=K,
             act=_lib.ACT_CODES[act])
    if batch > 0:  # ops.linear_heads: problem h at x + h K, w + h N K, y + h N
        return _lib.linear_route("batched", **{**a, "batch": batch, "stride_x": K, "stride_w": N * K, "stride_y": N}) + (M,)
    if epi != 0:  # ops.linear_dual allocates pre (pitch N); ops.linear_actgrad is given it
        rows = ops._fused_epilogue_rows(dtype, M, N, K, ldx, 0 if epi == 1 else ldr)
        if rows == 0:
            return None, None, 0
        a.update(M=rows, out_dtype=code[dtype], residual=r or FAKE["residual"], ldr=N if epi == 1 else ldr)
        if epi == 2:
            a["bias"] = 0
        return _lib.linear_route("dual" if epi == 1 else "actgrad", **a) + (rows,)
    if res:
        a.update(residual=r, ldr=ldr)
    if fold:
        a.update(colsum=cs, stats=FAKE["stats"])
    if stats and act == "Identity" and out_dtype == dtype:  # ops.linear(stats_eps=): the workspace it allocates
        a.update(workspace=FAKE["workspace"], workspace_bytes=M * max(N // 128, 1) * 8, stats_out=FAKE["stats_out"])
        return _lib.linear_route("stats", **a) + (M,)
    return _lib.linear_route("ln" if fold else "linear", **a) + (M,)


def library_route_restated(st, r, M, N, batch, rows):
    """The library's route in the terms of ``_linear_ref.route`` (``rows`` of ``M`` were handed over; the rest is ops.py's)."""
    from anemoi_models_amd import _lib

    py = types.SimpleNamespace(kernel="py", tail="none", batched=False, vec_ok=False, main_rows=0, m_a=0, rs=False)
    if rows == 0 or st == _lib.ANEMOI_ERR_UNSUPPORTED:
        return py
    assert st == _lib.ANEMOI_OK, (st, _lib.load().anemoi_last_error())
    tail = {_lib.LINEAR_REST_NONE: "none", _lib.LINEAR_REST_SKINNY: "skinny", _lib.LINEAR_REST_128: "k128",
            _lib.LINEAR_REST_IN_LAUNCH: "in%d" % (1 if r.rest_rows == 1 else 2 if r.rest_rows == 2 else 4 if r.rest_rows <= 4 else 8)}[r.rest]
    if rows < M:
        assert tail == "none"
        tail = "py"
    assert r.main_rows + (r.rest_rows if r.rest else 0) == rows and (r.rest == 0 or r.rest_row0 == r.main_rows)
    if r.kernel == _lib.LINEAR_KERNEL_128:
        assert r.n_launches == 0 and r.rs_rows == 0
        return types.SimpleNamespace(kernel="k128", vec_ok=bool(r.vec_ok), tail=tail, batched=batch > 0, main_rows=0, m_a=0, rs=False)
    assert r.kernel == _lib.LINEAR_KERNEL_PERSISTENT and r.n_launches in (1, 2) and r.vec_ok == 1 and r.rs_rows in (0, r.main_rows)
    first, last, second = r.launch[0], r.launch[r.n_launches - 1], bool(r.split)
    assert (r.n_launches == 1 or second) and sum(r.launch[i].rows for i in range(r.n_launches)) == r.main_rows
    groups = max(r.nt // R.SUPER_N, 1)
    return types.SimpleNamespace(
        kernel="w4", mh=first.mh, second=second, tail=tail, ragged_m=last.rows % (128 if second else 32 * last.mh) != 0,
        ragged_n=N % R.BIG != 0, nt=r.nt, rem=r.nt - (groups - 1) * R.SUPER_N, vec_ok=True, stagger=first.stagger_phases > 1,
        model=bool(r.model), rs=r.rs_rows > 0, batched=batch > 0, main_rows=r.main_rows,
        m_a=r.main_rows if not second else (first.rows if r.n_launches == 2 else 0))


def restated_launches(rt, batch):
    """(mh, first row, rows, tiles) per launch of a restated persistent route."""
    mt = -(-rt.main_rows // R.BIG)
    if not rt.second:
        return [(rt.mh, 0, rt.main_rows, max(batch, 1) * -(-rt.main_rows // (32 * rt.mh)) * rt.nt)]
    mt_a = rt.m_a // R.BIG
    return ([(8, 0, rt.m_a, mt_a * rt.nt)] if mt_a else []) + [(4, rt.m_a, rt.main_rows - rt.m_a, (mt - mt_a) * 2 * rt.nt)]


def assert_same_route(rt, st, r, M, N, batch, rows, what):
    """The restated route ``rt`` equals the library's (status ``st``, raw route ``r``): every field ``route_str`` prints, ``m_a``,
    ``main_rows``, the row sums, and per launch of the persistent kernel its height, rows, tiles, workgroups and stagger; the
    rows of the in-launch pass ride on the last launch."""
    lib = library_route_restated(st, r, M, N, batch, rows)
    assert R.route_str(lib) == R.route_str(rt), f"{what}: the library takes {R.route_str(lib)}, the restatement {R.route_str(rt)}"
    assert (lib.main_rows, lib.m_a, lib.rs) == (rt.main_rows, rt.m_a, rt.rs), what
    if rt.kernel != "w4":
        return
    want = restated_launches(rt, batch)
    assert r.n_launches == len(want), what
    for i, (mh, row0, nrows, tiles) in enumerate(want):
        l = r.launch[i]
        assert (l.mh, l.row0, l.rows, l.tiles, l.blocks) == (mh, row0, nrows, tiles, min(256, -(-tiles // 8) * 8)), (what, i)
        assert l.tail_rows == (r.rest_rows if i == len(want) - 1 and lib.tail.startswith("in") else 0), (what, i)
        assert (l.stagger_phases > 1) == (rt.stagger and i == 0), (what, i)


def _case_ptrs(c):
    return (FAKE["y"], FAKE["bias"] if c.bias and c.kind != "actgrad" else 0,
            FAKE["residual"] if c.res or c.kind == "actgrad" else 0, FAKE["colsum"] if c.fold else 0)


def case_library_route(c, ptrs, **xw):
    """``library_route`` on the arguments ``_linear_ref.case_route`` restates."""
    ldx, ldy, ldr = (c.k * c.h if c.h else c.k) + c.pads[0], (c.n * c.h if c.h else c.n) + c.pads[1], c.n + c.pads[2]
    epi = {"linear": 0, "dual": 1, "actgrad": 2, "heads": 0}[c.kind]
    return library_route(c.dtype, c.out, c.m, c.n, c.k, ldx, ldy, ldr, ptrs, c.act, c.res or epi == 2, c.fold, c.stats, epi, c.h, **xw)


def test_the_library_routes_every_case_as_restated():
    for c in R.all_cases():
        ptrs = _case_ptrs(c)
        rt = R.case_route(c, ptrs)
        assert R.route_str(rt) == c.expect, R.case_id(c)
        st, r, rows = case_library_route(c, ptrs)
        assert_same_route(rt, st, r, c.m, c.n, c.h, rows, R.case_id(c))
        if c.kind in ("dual", "actgrad"):  # the rows ops.py hands over: all, the whole tiles, or none (restated as py)
            assert rows == (0 if rt.kernel == "py" else rt.main_rows if rt.tail == "py" else c.m), R.case_id(c)


SWEEP_M = (1024, 1025, 1032, 1033, 2569, 5121, 10242, 20481, 40960, 40962, 65545)
SWEEP_N = (256, 264, 512, 1024, 2048, 2240, 4096, 4288, 4352, 6144)
SWEEP_K = (64, 128, 256, 512, 1216, 2048, 4096)


def test_the_library_routes_a_sweep_as_restated():
    """bf16 -> bf16 over SWEEP_M x SWEEP_N x SWEEP_K x activation x residual x fold x row sums x {pitches as tight as they go,
    padded by 8} x {y, bias, residual, colsum each 16-byte aligned or off by 8 bytes, where the operand exists}: 443 520 sets
    of integer arguments."""
    n = 0
    for M in SWEEP_M:
        for N in SWEEP_N:
            for K in SWEEP_K:
                for act in R.ACTS:
                    for res in (False, True):
                        for fold in (False, True):
                            offs = [(oy, ob, orr, oc) for oy in (0, 8) for ob in (0, 8) for orr in (0, 8)[:1 + res]
                                    for oc in (0, 8)[:1 + fold]]
                            for stats in (False, True):
                                for pad in (0, 8):
                                    for off in offs:
                                        ptrs = (FAKE["y"] + off[0], FAKE["bias"] + off[1], (FAKE["residual"] + off[2]) * res,
                                                (FAKE["colsum"] + off[3]) * fold)
                                        args = (BF16, BF16, M, N, K, K + pad, N + pad, N + pad, ptrs, act, res, fold, stats)
                                        st, r, rows = library_route(*args)
                                        assert_same_route(R.route(*args), st, r, M, N, 0, rows, args)
                                        n += 1
    assert n == 11 * 10 * 7 * 4 * (4 + 8 + 8 + 16) * 2 * 2 == 443520


@pytest.mark.parametrize("switch,value,shape,default,forced", [
    ("ANEMOI_AMD_GEMM_MH", "5", (1056, 256, 128), "1 3 0", "1 5 0"),  # a small-problem shape: one launch of 96-row tiles
    ("ANEMOI_AMD_GEMM_STAGGER", "0,0,2", (8192, 4096, 512), "1 8 2", "1 8 0"),  # 512 tiles, K = 512: staggered as shipped
])
def test_lab_switches_reach_the_plan(switch, value, shape, default, forced):
    """The switches are read once per process: a fresh child each; without the switch, this process (unless it runs under one)."""
    import os
    import subprocess
    import sys

    from conftest import ROOT

    code = ("from anemoi_models_amd import _lib\n"
            "st, r = _lib.linear_route('linear', dtype=1, out_dtype=1, x=4096, w=8192, y=12288, ldx=%d, ldy=%d, M=%d, N=%d, K=%d)\n"
            "print(st, r.n_launches, r.launch[0].mh, r.launch[0].stagger_phases)\n" % (shape[2], shape[1], *shape))
    env = {k: v for k, v in os.environ.items() if not k.startswith("ANEMOI_AMD_GEMM_")}
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(env, **{switch: value}), capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["0"] + forced.split(), out.stdout
    if len(env) == len(os.environ):
        st, r, _ = library_route(BF16, BF16, *shape, shape[2], shape[1], 0, (FAKE["y"], 0, 0, 0))
        assert [str(v) for v in (st, r.n_launches, r.launch[0].mh, r.launch[0].stagger_phases)] == ["0"] + default.split()


# ------------------------------------------------------------------------------------------------ emulations inside the bounds
@pytest.mark.parametrize("c", R.all_cases(), ids=R.case_id)
def test_emulated_kernels_stay_inside_the_bounds(c):
    o, rt, rows, ref = _setup(c)
    got = emulate(c, o, rt, rows)
    for k, (want, bound) in ref.items():
        if c.data == "exact":
            assert float(bound.max()) == 0.0 and float(want.abs().max()) <= 256 and bool((want == want.round()).all())
        R.check(got[k], want, bound, f"{R.case_id(c)} {k}")
    if c.stats:
        want, bound = _stats_want(c, rt, got["y"], rows)
        R.check(got["stats"], want, bound, f"{R.case_id(c)} stats")
    if c.fold and c.data != "exact" and rows is None:
        z_true, extra = R.fold_true_ref(c, o)
        want = R.act64(z_true, c.act) + (o.res.double() if o.res is not None else 0.0)
        R.check(got["y"], want, ref["y"][1] + R.LIP[c.act] * extra, f"{R.case_id(c)} y against LayerNorm itself")


# ------------------------------------------------------------------------------------------------ wrong kernels
def _find(pred):
    for c in R.all_cases():
        if pred(c, R.case_route(c)):
            return c
    raise AssertionError("the case table has no such case")


def _tail_exact(c, rt):
    return c.kind == "linear" and c.data == "exact" and c.res and not c.fold and rt.tail == "in4" and c.m == 1028 and c.n == 264


def _tail_fold_exact(c, rt):
    return c.kind == "linear" and c.data == "exact" and c.res and c.fold and rt.tail == "in4" and c.m == 1028


MUTANTS = [  # (mutant, case, output it must spoil)
    ("drop_slab", _tail_exact, "y"),
    ("drop_chunk", _tail_exact, "y"),
    ("bias_shift4", _tail_exact, "y"),
    ("bias_shift8", _tail_exact, "y"),
    ("bias_tile_rel", _tail_exact, "y"),
    ("res_next_row", _tail_exact, "y"),
    ("res_prev_row", _tail_exact, "y"),
    ("drop_slab", lambda c, rt: c.data == "spike" and rt.kernel == "w4" and c.act == "GELU" and rt.tail == "in1", "y"),
    ("drop_chunk", lambda c, rt: c.data == "spike" and rt.kernel == "w4" and c.act == "GELU" and rt.tail == "in1", "y"),
    ("acc_bf16", lambda c, rt: c.data == "ordinary" and rt.kernel == "w4" and c.act == "GELU" and c.n == 264 and c.kind == "linear", "y"),
    ("res_before_act", lambda c, rt: c.act == "GELU" and c.res and rt.tail == "skinny" and c.k == 64, "y"),
    ("double_round", lambda c, rt: c.act == "GELU" and c.res and rt.tail == "skinny" and c.n == 260, "y"),
    ("fold_no_shift", _tail_fold_exact, "y"),
    ("stats_tile_rel", _tail_fold_exact, "y"),
    ("tail_stats_0_7", _tail_fold_exact, "y"),
    ("colsum_shift", _tail_fold_exact, "y"),
    ("fold_no_shift", lambda c, rt: c.fold and c.data == "fold_mean" and rt.tail == "in2", "y"),
    ("stats_b_no_offset", lambda c, rt: rt.second and rt.m_a > 0 and c.fold, "y"),
    ("tanh_gelu", lambda c, rt: c.act == "GELU" and c.dtype == F32 and not c.fold and c.data != "exact", "y"),
    ("tanh_gelu", lambda c, rt: c.act == "GELU" and c.dtype == BF16 and c.out == F32 and not c.fold and c.data != "exact", "y"),
    ("tanh_gelu", lambda c, rt: c.data == "ordinary" and rt.kernel == "w4" and c.act == "GELU" and c.n == 264 and c.kind == "linear", "y"),
    ("gelu_q_digit", lambda c, rt: c.data == "ordinary" and rt.kernel == "w4" and c.act == "GELU" and c.n == 264 and c.kind == "linear", "y"),
    ("gelu_q_digit", lambda c, rt: c.kind == "dual" and c.act == "GELU" and rt.kernel == "w4" and rt.tail == "in8", "y"),
    ("dgelu_q_digit", lambda c, rt: c.kind == "actgrad" and c.act == "GELU" and rt.kernel == "w4" and rt.tail == "in8", "y"),
    ("dgelu_no_xphi", lambda c, rt: c.kind == "actgrad" and c.act == "GELU" and rt.kernel == "w4" and rt.tail == "in8", "y"),
    ("dsilu_sigmoid", lambda c, rt: c.kind == "actgrad" and c.act == "SiLU" and rt.kernel == "w4" and rt.tail.startswith("in"), "y"),
    ("pre_activated", lambda c, rt: c.kind == "dual" and c.act == "GELU" and rt.kernel == "w4" and rt.tail == "in8", "pre"),
    ("act_rounded_pre", lambda c, rt: c.kind == "dual" and c.act == "GELU" and rt.kernel == "w4" and rt.tail == "in8", "y"),
    ("w_prev", lambda c, rt: c.kind == "heads" and c.h == 3 and c.data == "exact" and rt.kernel == "w4", "y"),
    ("w_prev", lambda c, rt: c.kind == "heads" and c.h == 3 and c.data == "spike", "y"),
    ("stats_ldy", lambda c, rt: c.stats and rt.rs and c.data == "spike", "stats"),
    ("stats_unrounded", lambda c, rt: c.stats and rt.rs and c.data == "b300", "stats"),
    ("stats_unrounded", lambda c, rt: c.stats and rt.rs and c.data == "spike", "stats"),
]


@pytest.mark.parametrize("mut,pred,output", MUTANTS, ids=[f"{m[0]}-{i}" for i, m in enumerate(MUTANTS)])
def test_wrong_kernels_leave_the_bounds(mut, pred, output):
    c = _find(pred)
    o, rt, rows, ref = _setup(c)
    good, bad = emulate(c, o, rt, rows), emulate(c, o, rt, rows, mut)
    if output == "stats":
        want, bound = _stats_want(c, rt, bad["y"], rows)
        assert not R.fails(good["stats"], *_stats_want(c, rt, good["y"], rows))
    else:
        want, bound = ref[output]
        assert not R.fails(good[output], want, bound)
    assert R.fails(bad[output], want, bound), f"{mut} passes at {R.case_id(c)}"
    if c.data == "exact" and output != "stats":
        assert float(bound.max()) == 0.0


def test_the_mutant_that_no_accuracy_bound_can_reject():
    """One rounding where round / add / round is specified is closer to the truth: inside, and said to be (module docstring)."""
    c = _find(lambda c, rt: c.kind == "linear" and c.act == "SiLU" and c.res and rt.kernel == "w4" and rt.mh == 3 and not c.fold)
    o, rt, rows, ref = _setup(c)
    assert not R.fails(emulate(c, o, rt, rows, "single_round")["y"], *ref["y"])


def _covered(nt, mt, coords):
    """The tiles a launch computes when its tile walk is ``coords`` (tiles outside the grid are dropped by the descriptors)."""
    done = torch.zeros((mt, nt), dtype=torch.bool)
    for t in range(mt * nt):
        i, j = coords(t)
        if 0 <= i < mt and 0 <= j < nt:
            done[i, j] = True
    return done


def test_wrong_tile_walks_leave_tiles_unwritten():
    """Row and column tile swapped, and a last column group of width 8 where the remainder is 9..15 wide: tiles that no workgroup
    computes keep the output buffer's pattern (0x5A5A = 1.5e16 as bf16), far outside every bound of a case with that grid."""
    c = _find(lambda c, rt: rt.kernel == "w4" and rt.nt == 5 and rt.mh == 3 and c.data == "exact")
    rt = R.case_route(c)
    mt = -(-c.m // (32 * rt.mh))
    assert not bool(_covered(rt.nt, mt, lambda t: R.tile_coords(t, rt.nt, mt)[::-1]).all())
    for nt in (17, 18, 23):
        def width8(t, nt=nt, mt=mt):
            groups, per_group = nt // 8, mt * 8
            cg = min(t // per_group, groups - 1)
            r = t - cg * per_group
            return r // 8, cg * 8 + r % 8
        assert not bool(_covered(nt, mt, width8).all())
        assert bool(_covered(nt, mt, lambda t: R.tile_coords(t, nt, mt)).all())
    pattern = torch.tensor([0x5A5A], dtype=torch.int16).view(BF16).double()
    o, rt, rows, ref = _setup(c)
    want, bound = ref["y"]
    assert R.fails(pattern.expand_as(want), want, bound) and bool(((pattern - want).abs() > bound).all())
