"""f64 references, per-element error bounds, the restated dispatch, data sets and the case table of the fused Linear family
(csrc/gemm.hip behind ``ops.linear``, ``ops.linear(ln=)``, ``ops.linear(stats_eps=)``, ``ops.linear_dual``,
``ops.linear_actgrad``, ``ops.linear_heads``).

Pure torch; imports nothing from the library.  Used by tests/test_linear_ref_cpu.py (route coverage, emulations of the kernels'
arithmetic inside the bounds, wrong kernels outside them) and by tests/test_gpu_linear.py (the kernels).

Reference.  f64 from the operands AS STORED (bf16 / f32 values widen exactly):
  plain     z = x W^T + b,  y = act(z) + r
  LN fold   z = rstd_m (x W'^T) + shift_m s_n + b'_n  from the GIVEN f32 (rstd, shift = -mean rstd) and column sums s; a second
            check (``fold_true_ref``) compares with LayerNorm(x) W^T + b itself and widens by the statistics' own bound
  dual      pre = z, y = act(z) (of the unrounded sum);  actgrad  y = (x W^T) act'(pre), pre as stored
  stats     (rstd, -mean rstd) of the STORED y;  batched: one product per problem.

Bounds, per element.  u = 2^-24 (one rounded f32 operation), gamma(n) = n u / (1 - n u) (Higham, lemma 3.1), RB = 2^-8 (one
bf16 store, _gnn_ops_ref), S = |x| |W|^T.
  Accumulation.  E_acc = gamma(K) S.  bf16 x bf16 products are exact in f32 (16 significant bits), so only additions round: K
    terms in ANY order pass through at most K - 1 additions, plus the one into the accumulator (section 4.2 ibid.).  The bf16
    MFMA adds 32 products per instruction in an adder at least as wide as f32 and rounds into the f32 accumulator -- fewer
    roundings than assumed, in an order the tests do not assume; the slab order (64 k per slab) and the wave layout change
    nothing in an any-order bound.  The f32 kernel's 32x32x2 MFMA is the K-ordered fma chain (one rounding per k): gamma(K).
    The skinny passes run a per-lane fmaf chain over K / 64 or fewer terms and a six-step butterfly: again at most K roundings.
  Bias.  z^ = fl(acc^ + b):  E_z = E_acc + u (|acc| + |b| + E_acc).
  Fold.  rstd acc^ and shift s_n are rounded products (an fma removes one of the roundings), two additions follow:
    E_z = |rstd| E_acc + gamma(3) (|rstd acc| + |shift s_n| + |b'|).  The magnitudes enter, not their sum: where rstd acc and
    shift s_n cancel (rows with |mean| >> spread) the bound grows by u |mean| rstd |s_n|, as the arithmetic does.
  Activation.  E_act = L E_z + approximation.  L = max|act'|: GELU 1.13, SiLU 1.10, ReLU / Identity 1.  Approximation:
    erf form (128 x 128 kernel, skinny passes): 2e-7 |z|, the figure csrc/common.hpp documents for fast_erf's GELU, + gamma(3) |act z|
      for evaluating 0.5 x (1 + erf) in f32 (the sum 1 + erf and the two products round once each).  The device meets exactly
      this: test_gpu_linear.py::test_device_activation_figures measures 2.48e-7 |x| in all and 1.63e-7 |x| beside the three u terms;
    SiLU = x * __frcp_rn(1 + __expf(-x)) everywhere: the guides give NO figure for __expf / __frcp_rn, so the device SiLU was
      measured against f64 through ``ops.act_forward`` on 2^20 points of [-24, 24], 2^16 of [-90, 90] and +-VALUE_SET: at most
      SILU_MEASURED = 1.414e-7 |x| (no floor: the error is proportional to |x|; all but 6.9e-9 |x| of it is three f32 roundings of
      the result).  The bound uses SILU_REL = 2 x that: the grid holds 2^20 of the 2^31 arguments of its range and the error is a
      sawtooth of the roundings of exp and rcp, so a denser grid can find a slightly larger tooth, not a different curve; the same
      test asserts the measured figure stays under SILU_REL;
    four-wave GELU polynomial: 5.5e-5 (csrc/gemm.hip::act_apply2) + gamma(12) max(1, |z|) for its Horner evaluation;
    GELU' polynomial: 6.5e-5 inside the clamp |pre| <= 4, 5.5e-4 outside (act_grad2), + gamma(12) max(1, |pre|); SiLU' =
      s (x (1 - s) + 1) from the same sigmoid s: |d/ds| <= 1 + |x| and |s^ - s| <= SILU_REL, four more roundings of terms <= 1 + |x|:
      (SILU_REL + gamma(4)) (1 + |pre|); ReLU': 0.
    Rows that ops.py hands to ``act_forward`` / ``act_backward`` (its fallbacks) are those kernels' results: their bound is the one
      tests/test_gpu_gnn_ops.py holds them to, A max(1, |x|, |result|) with A = 7.48e-7 of _gnn_ops_ref.
  Store.  bf16 without residual: E = E_act + RB (|act z| + E_act).  With a residual the four-wave kernel and the skinny passes
    round, add in f32, round again:  E1 = E_act + RB (|o| + E_act),  E2 = E1 + u (|o + r| + E1),  E = E2 + RB (|o + r| + E2);
    the 128 x 128 kernel adds in f32 and rounds ONCE: E2 = E_act + u (|o + r| + E_act), E = E2 + RB (|o + r| + E2).  The route
    restatement says which rows get which.  f32 output: no store term.
  Dual.  pre: E_z + RB (|z| + E_z).  y: as above from the UNROUNDED z on the kernel; where ops.py falls back to
    ``linear`` + ``act_forward`` (fewer than 1024 tiled rows, ragged rows behind the tiles) the activation sees the stored pre:
    E_z grows by RB (|z| + E_z) first.
  Actgrad.  want = acc g, g = act'(pre):  E32 = |g| E_acc + (|acc| + E_acc) E_g + u |acc g|, then the store; the Python
    fallback rounds acc to bf16 first: E_acc grows by RB (|acc| + E_acc).
  Statistics of the stored y (C = N columns).  Rows the 128 x 128 route hands to ``row_stats``: _row_kernels_ref's two-pass bound.
    Rows of the four-wave tiles: ONE pass, var = ss / C - mean^2 from f32 sums of y and y^2.  The summation is a TREE whose depth
    the source fixes: a lane's 32 stored values of a row through 16 two-term dot products (at most two roundings each), two
    shuffle additions, then the C / 128 slots in sequence: a term passes through at most d = 34 + C / 128 additions, so
    gamma(d + 3) takes the place of the any-order gamma(C + 3), which is too loose to reject the statistics mutants (the kernels
    use a thousandth of it):
    dm = gamma(d) sum|y| / C,  dq = 2 |mu| dm + dm^2 + gamma(d + 3) (E[y^2] + mu^2).  Rows whose variance cancelled
    (var < 1e-3 E[y^2]) are redone in two passes by the fold kernel, a serial loop: the two-pass bound with gamma(C + 3); between
    0.5e-3 and 2e-3 either branch is admitted (the larger bound).  The up to 8 tail rows are summed in one pass WITHOUT that
    fallback (row_sums_finalize_kernel: C / 256 terms per thread, six butterfly steps, four partials: d = C / 256 + 10): the
    one-pass bound, wide when |mean| >> spread -- stated here, not hidden.
  ``exact`` data: every product, sum, bias, residual and result is an integer of magnitude <= 256: bound 0, compared by bits.
No global factor anywhere.
"""

from __future__ import annotations

import math
import types

import torch

from _gnn_ops_ref import A as ACT_A
from _gnn_ops_ref import BF16_STORE, EPS32, act64, dact64
from _mhsa_ref import check, fails  # noqa: F401  (re-exported: the checker of all per-element suites)
from _row_kernels_ref import RSQRT_REL, eps32, gamma, row_stats_ref

U = EPS32 / 2.0
RB = BF16_STORE
F32, BF16 = torch.float32, torch.bfloat16
EPS = 1e-5
LIP = {"Identity": 1.0, "GELU": 1.13, "SiLU": 1.10, "ReLU": 1.0}
GELU_ERF_REL = 2e-7  # csrc/common.hpp: "GELU inherits < 2e-7 * |x|"
SILU_MEASURED = 1.414e-7  # device SiLU, |error| / |x| (test_gpu_linear.py::test_device_activation_figures)
SILU_REL = 2.0 * SILU_MEASURED
GELU_POLY_ERR = 5.5e-5
DGELU_POLY_ERR_IN, DGELU_POLY_ERR_OUT, DGELU_CLAMP = 6.5e-5, 5.5e-4, 4.0
# the polynomials of csrc/gemm.hip as NUMBERS (act_apply2 / act_grad2), highest degree first
GELU_Q = (3.036384685350946e-11, -3.31462968183871e-09, 1.5909856188045524e-07, -4.451706445252057e-06,
          8.142489969031885e-05, -0.0010375895071774721, 0.009585196152329445, -0.06598464399576187, 0.3987126052379608)
DGELU_Q = (9.3872902156732022e-10, -7.9411323687314723e-08, 2.950694481564598e-06, -6.3805510857940873e-05,
           0.00089759489254071564, -0.0086697042593016048, 0.05833774383148245, -0.26469170897426864, 0.79756480213010039)
ERR_UNSUPPORTED = 2


def name(dtype) -> str:
    return "f32" if dtype == F32 else "bf16"


# ================================================================================================ route restatement
BIG, MAX_BLOCKS, SUPER_N = 256, 256, 8
STAGGER_MIN_ROUNDS, STAGGER_MIN_K = 2, 512


def _generic(M, N, ldy, ldr, ptrs, res, fold, tail="none"):
    y, b, r, cs = ptrs
    vec = N % 4 == 0 and ldy % 4 == 0 and y % 16 == 0 and b % 16 == 0 and (not fold or cs % 16 == 0) and \
        (not res or (ldr % 4 == 0 and r % 16 == 0))
    return types.SimpleNamespace(kernel="k128", mh=0, second=False, tail=tail, ragged_m=M % 128 != 0, ragged_n=N % 128 != 0,
                                 nt=-(-N // 128), rem=0, vec_ok=vec, stagger=False, model=False, rs=False, batched=False,
                                 main_rows=0, m_a=0)


def _w4(M, N, K, ldx, ldy, ldr, ptrs, act, res, fold, stats, epi, batch, m_tail):
    """csrc/gemm.hip::plan_w4: None when the persistent kernel refuses the shape."""
    y, b, r, cs = ptrs
    vec = N % 8 == 0 and ldy % 8 == 0 and y % 16 == 0 and b % 16 == 0 and (not res or (ldr % 8 == 0 and r % 16 == 0))
    if not (K >= 128 and max(ldx, ldy, ldr) < 1 << 21 and vec and (M % BIG == 0 or m_tail == 0) and (not fold or cs % 16 == 0)):
        return None
    mt, nt = -(-M // BIG), -(-N // BIG)
    dual_or_gmul = epi != 0
    mt_a, mt_b = mt, 0
    if batch == 0 and nt <= 256 and 256 % nt == 0:
        rem_mt = mt % (256 // nt)
        if rem_mt > 0 and rem_mt * nt <= 128 and ((rem_mt == mt and dual_or_gmul) or (rem_mt != mt and K >= 2048)):
            mt_a, mt_b = mt - rem_mt, rem_mt
    mh, model = 8, False
    split_chosen = mt_b > 0 and not dual_or_gmul
    if batch == 0 and not dual_or_gmul and (mt_b == 0 or split_chosen) and mt * nt < 4 * MAX_BLOCKS:
        model = True
        best_mh, best_cost = 8, 1e30
        for h in (8, 6, 5, 4, 3):
            tiles = -(-M // (32 * h)) * nt
            rounds = -(-tiles // MAX_BLOCKS)
            cost = rounds * (0.8125 * h + (K // 64) * 1.44 * (32 * h + 256) / 512.0)
            if cost < best_cost * 0.97:
                best_cost, best_mh = cost, h
        single = best_mh != 8
        if split_chosen:
            ra, rb_ = -(-mt_a * nt // MAX_BLOCKS), -(-mt_b * 2 * nt // MAX_BLOCKS)
            split_cost = ra * (0.8125 * 8 + (K // 64) * 1.44) + rb_ * (0.8125 * 4 + (K // 64) * 1.44 * 0.75) + 6.0
            single = best_cost < split_cost * 0.97
            if single:
                mt_a, mt_b = mt, 0
        if single and best_mh != 8:
            mh, mt_a = best_mh, 0
    second = mt_b > 0
    if mt_a == 0 and second:
        mh = 4  # launch B alone: half tiles
    problems = batch if batch > 0 else 1
    stagger = mh == 8 and mt_a > 0 and problems * mt_a * nt >= STAGGER_MIN_ROUNDS * MAX_BLOCKS and K >= STAGGER_MIN_K
    tm = 32 * mh
    last_rows = (M - mt_a * BIG) if second else M
    groups = max(nt // SUPER_N, 1)
    tail = "none" if m_tail == 0 else "in%d" % (1 if m_tail == 1 else 2 if m_tail == 2 else 4 if m_tail <= 4 else 8)
    return types.SimpleNamespace(kernel="w4", mh=mh, second=second, tail=tail, ragged_m=last_rows % (128 if second else tm) != 0,
                                 ragged_n=N % BIG != 0, nt=nt, rem=nt - (groups - 1) * SUPER_N, vec_ok=True, stagger=stagger,
                                 model=model, rs=stats and act == "Identity" and N % BIG == 0, batched=batch > 0, main_rows=M,
                                 m_a=min(mt_a * BIG, M) if second else M)


def route(dtype, out_dtype, M, N, K, ldx, ldy, ldr, ptrs=(0, 0, 0, 0), act="Identity", res=False, fold=False, stats=False,
          epi=0, batch=0):
    """What csrc/gemm.hip::linear_plan (and, for dual / actgrad, ops.py in front of it) does with these arguments, restated
    without the library; tests/test_linear_ref_cpu.py holds it against ``anemoi_linear_route``.  ``ptrs`` = (y, bias, residual, colsum) addresses, ``epi`` 1 = dual, 2 = actgrad, ``batch`` =
    problems of ``linear_heads`` (0: not batched).  ``main_rows``: rows computed by the persistent kernel's tiles."""
    if batch > 0:
        if dtype == BF16 and out_dtype == BF16 and K >= 128 and N % 8 == 0 and ldy % 8 == 0 and ptrs[0] % 16 == 0:
            rt = _w4(M, N, K, ldx, ldy, 0, ptrs, act, False, False, False, 0, batch, 0)
            if rt is not None:
                return rt
        rt = _generic(M, N, ldy, 0, ptrs, False, False)
        rt.batched = True
        return rt
    if epi != 0:  # ops.linear_dual / ops.linear_actgrad
        ok = dtype == BF16 and N >= 256 and N % 8 == 0 and K >= 128 and K % 64 == 0 and ldx % 8 == 0 and (epi == 1 or ldr % 8 == 0)
        m_main = M // BIG * BIG if ok else 0
        if m_main < 1024:
            rt = _generic(M, N, ldy, ldr, ptrs, False, False)
            rt.kernel = "py"
            return rt
        m_tail = M - m_main
        rt = _w4(m_main, N, K, ldx, ldy, ldr, ptrs, act, True, False, False, epi, 0, m_tail if m_tail <= 8 else 0)
        assert rt is not None
        if m_tail > 8:
            rt.tail = "py"
        return rt
    if dtype == F32 or out_dtype == F32 or not (M >= 1024 and N >= 256):
        return _generic(M, N, ldy, ldr, ptrs, res, fold)
    m_main = M // BIG * BIG
    m_tail = M - m_main
    args = (N, K, ldx, ldy, ldr, ptrs, act, res, fold, stats, 0, 0)
    if m_tail == 0:
        return _w4(M, *args, 0) or _generic(M, N, ldy, ldr, ptrs, res, fold)
    if m_tail > 8 and K >= 128:
        rt = _w4(M, *args, 0)
        if rt is not None:
            return rt
    rt = _w4(m_main, *args, m_tail if m_tail <= 8 else 0)
    if rt is not None and rt.tail != "none":
        return rt
    tail = "skinny" if (m_tail <= 8 and K % 8 == 0) else "k128"
    if rt is None:
        rt = _generic(m_main, N, ldy, ldr, ptrs, res, fold, tail)
        rt.main_rows = 0
        rt.ragged_m = False
    else:
        rt.tail = tail
    return rt


def route_str(rt) -> str:
    if rt.kernel in ("k128", "py"):
        s = f"{rt.kernel}/vec{int(rt.vec_ok)}" if rt.kernel == "k128" else "py"
        s += ("" if rt.tail == "none" else f"/{rt.tail}") + ("/batched" if rt.batched else "")
        return s
    return f"w4/mh{rt.mh}" + ("/split" if rt.second else "") + ("" if rt.tail == "none" else f"/{rt.tail}") + \
        ("/rm" if rt.ragged_m else "") + ("/rn" if rt.ragged_n else "") + f"/nt{rt.nt}/rem{rt.rem}" + \
        ("/stagger" if rt.stagger else "") + ("" if rt.model or rt.second or rt.batched else "/nomodel") + \
        ("/batched" if rt.batched else "")


def tile_coords(t, nt, mt):
    """csrc/gemm.hip::tile_coords: (row tile, column tile) of list position t."""
    groups = max(nt // SUPER_N, 1)
    per_group = mt * SUPER_N
    cg = min(t // per_group, groups - 1)
    r = t - cg * per_group
    width = nt - cg * SUPER_N if cg == groups - 1 else SUPER_N
    return r // width, cg * SUPER_N + r % width


# ================================================================================================ cases
def Case(kind, m, n, k, expect, act="Identity", res=False, fold=False, stats=False, data="ordinary", dtype=BF16, out=None,
         pads=(0, 0, 0), bias=True, h=0):
    return types.SimpleNamespace(kind=kind, m=m, n=n, k=k, expect=expect, act=act, res=res, fold=fold, stats=stats, data=data,
                                 dtype=dtype, out=out or dtype, pads=pads, bias=bias, h=h)


def case_id(c) -> str:
    s = f"{c.kind}-{name(c.dtype)}{'' if c.out == c.dtype else '>' + name(c.out)}-{c.m}x{c.n}x{c.k}-{c.act}-{c.data}"
    s += ("-res" if c.res else "") + ("-fold" if c.fold else "") + ("-stats" if c.stats else "") + ("" if c.bias else "-nobias")
    s += (f"-h{c.h}" if c.h else "") + ("" if c.pads == (0, 0, 0) else "-pad%d.%d.%d" % c.pads)
    return s


def case_route(c, ptrs=(0, 0, 0, 0)):
    ldx = (c.k * c.h if c.h else c.k) + c.pads[0]
    ldy = (c.n * c.h if c.h else c.n) + c.pads[1]
    ldr = c.n + c.pads[2]
    epi = {"linear": 0, "dual": 1, "actgrad": 2, "heads": 0}[c.kind]
    return route(c.dtype, c.out, c.m, c.n, c.k, ldx, ldy, ldr, ptrs, c.act, c.res or epi == 2, c.fold, c.stats, epi, c.h)


ACTS = ("Identity", "GELU", "SiLU", "ReLU")
EPILOGUES = (dict(res=True, stats=True), dict(act="GELU"), dict(act="SiLU", res=True), dict(fold=True, act="GELU"),
             dict(fold=True, res=True, stats=True))
DATA_CYCLE = ("ordinary", "exact", "cancel", "spike", "ordinary", "exact")


def generic_cases():
    """The 128 x 128 kernel: all three dtype forms, M x N edges, one and three slabs; activation, residual, fold, pitches and data
    kinds cycle over the (M, N) grid so that each value of each meets every dtype form (not the full cross product)."""
    out = []
    i = 0
    for dtype, odt in ((F32, F32), (BF16, BF16), (BF16, F32)):
        slab = 32 if dtype == F32 else 64
        for m in (1, 127, 128, 129, 257):
            for n in (1, 11, 127, 128, 132, 260):
                act = ACTS[i % 4]
                res = (i // 2) % 2 == 1
                fold = (i // 3) % 2 == 1
                pads = ((0, 0, 0), (8, 3, 5), (0, 4, 4), (8, 0, 2))[(i // 5) % 4]
                data = DATA_CYCLE[(i // 4) % 6]
                if data == "exact" and act in ("GELU", "SiLU"):
                    act = "ReLU"
                if fold and data in ("cancel", "spike"):
                    data = "fold_mean"
                vec = n % 4 == 0 and (n + pads[1]) % 4 == 0 and (not res or (n + pads[2]) % 4 == 0)
                out.append(Case("linear", m, n, slab * (1 if (i // 7) % 2 else 3), f"k128/vec{int(vec)}", act, res, fold, False, data,
                                dtype, odt, pads))
                i += 1
    return out


def _epi_cases(m, n, k, expect, datas=("ordinary", "exact", "spike", "fold_mean", "cancel")):
    out = []
    for e, data in zip(EPILOGUES, datas):
        e = dict(e)
        if data == "exact":
            e["act"] = "Identity" if e.get("act", "Identity") == "Identity" else "ReLU"
        if e.get("fold") and data != "exact":
            data = "fold_mean"
        out.append(Case("linear", m, n, k, expect, data=data, **e))
    return out


def w4_cases():
    out = []
    # tile heights, whole and ragged last row tile (N = 256 / 4096, K = 128)
    for m, n, expect in ((1056, 256, "w4/mh3/nt1/rem1"), (1024, 256, "w4/mh3/rm/nt1/rem1"),
                         (1664, 4096, "w4/mh4/nt16/rem8"), (1600, 4096, "w4/mh4/rm/nt16/rem8"),
                         (2080, 4096, "w4/mh5/nt16/rem8"), (2112, 4096, "w4/mh5/rm/nt16/rem8"),
                         (2688, 4096, "w4/mh6/nt16/rem8"), (2592, 4096, "w4/mh6/rm/nt16/rem8"),
                         (3328, 4096, "w4/mh8/nt16/rem8"), (3104, 4096, "w4/mh8/rm/nt16/rem8")):
        out += _epi_cases(m, n, 128, expect)
    # column tiles: ragged last column tile with nt < 8, remainder groups 9 / 10 / 15 wide, three whole groups
    for m, n, expect in ((1056, 264, "w4/mh3/rn/nt2/rem2"), (1024, 1032, "w4/mh3/rm/rn/nt5/rem5"),
                         (1056, 4352, "w4/mh3/nt17/rem9"), (1024, 4360, "w4/mh3/rm/rn/nt18/rem10"),
                         (1056, 5888, "w4/mh3/nt23/rem15"), (1024, 6144, "w4/mh4/nt24/rem8")):
        out.append(Case("linear", m, n, 128, expect, data="exact", res=True))
        out.append(Case("linear", m, n, 128, expect, act="GELU", data="ordinary"))
        out.append(Case("linear", m, n, 128, expect, fold=True, res=True, stats=n % 256 == 0, data="exact"))
    # tails behind whole tiles: every template and every epilogue with a skinny form
    for t, tmpl in ((1, 1), (2, 2), (3, 4), (4, 4), (5, 8), (8, 8)):
        e264 = f"w4/mh3/in{tmpl}/rm/rn/nt2/rem2"
        out.append(Case("linear", 1024 + t, 264, 192, e264, act="GELU", data="spike"))
        out.append(Case("linear", 1024 + t, 264, 192, e264, fold=True, act="SiLU", data="fold_mean"))
        out.append(Case("linear", 1024 + t, 264, 192, e264, res=True, data="exact"))
        out.append(Case("linear", 1024 + t, 264, 192, e264, fold=True, res=True, data="exact", pads=(8, 8, 16)))
        out.append(Case("linear", 1024 + t, 4096, 128, f"w4/mh3/in{tmpl}/rm/nt16/rem8", res=True, stats=True, data="spike"))
        out.append(Case("linear", 1024 + t, 512, 128, f"w4/mh3/in{tmpl}/rm/nt2/rem2", fold=True, stats=True, data="fold_mean"))
        out.append(Case("dual", 1024 + t, 264, 192, f"w4/mh4/split/in{tmpl}/rn/nt2/rem2", act=ACTS[1 + t % 3], data="spike"))
        out.append(Case("actgrad", 1024 + t, 264, 192, f"w4/mh4/split/in{tmpl}/rn/nt2/rem2", act=ACTS[1 + t % 3], data="spike"))
    out.append(Case("linear", 1033, 264, 192, "w4/mh3/rm/rn/nt2/rem2", res=True, data="exact"))  # 9 rows: ragged row tile
    out.append(Case("linear", 1033, 264, 192, "w4/mh3/rm/rn/nt2/rem2", act="GELU", fold=True, data="fold_mean"))
    # shapes the persistent kernel refuses: 128 x 128 main part, stand-alone skinny kernel or 128 x 128 tail
    for (m, n, k, pads) in ((1027, 512, 64, (0, 0, 0)), (1029, 260, 128, (0, 0, 0)), (1032, 512, 128, (0, 4, 0))):
        vec = int(n % 4 == 0)
        for mm, tail in ((m, "skinny"), (1033, "k128")):
            out.append(Case("linear", mm, n, k, f"k128/vec{vec}/{tail}", res=True, data="exact", pads=pads))
            out.append(Case("linear", mm, n, k, f"k128/vec{vec}/{tail}", act="GELU", res=True, data="spike", pads=pads))
            out.append(Case("linear", mm, n, k, f"k128/vec{vec}/{tail}", fold=True, act="SiLU", data="fold_mean", pads=pads,
                            stats=False))
    # statistics: the fallback to row_stats (N = 384), the cancellation rows (bias 300 / 302) with a tail
    out.append(Case("linear", 1056, 384, 128, "w4/mh3/rn/nt2/rem2", stats=True, res=True))
    out.append(Case("linear", 1031, 512, 256, "w4/mh3/in8/rm/nt2/rem2", stats=True, data="b300"))
    out.append(Case("linear", 300, 256, 128, "k128/vec1", stats=True, data="b300"))
    return out


def dual_cases():
    out = []
    i = 0
    for m in (256, 264, 1024, 1031, 2560):
        for n in (256, 264, 1024):
            for kind in ("dual", "actgrad"):
                k = (128, 192)[i % 2]
                act = ACTS[1 + i % 3]
                if m < 1024:
                    expect = "py"
                else:
                    nt = -(-n // 256)
                    expect = "w4/mh4/split" + ("/in8" if m % 256 else "") + ("/rn" if n % 256 else "") + f"/nt{nt}/rem{nt}"
                out.append(Case(kind, m, n, k, expect, act=act, data=("ordinary", "spike", "cancel")[i % 3]))
                i += 1
    # no split (256 % nt != 0): the 256-row tile with the DUAL / GMUL epilogue; ragged rows behind the tiles -> ops.py's fallback
    for kind in ("dual", "actgrad"):
        out.append(Case(kind, 1024, 520, 128, "w4/mh8/rn/nt3/rem3/nomodel", act="GELU"))
        out.append(Case(kind, 1280, 768, 192, "w4/mh8/nt3/rem3/nomodel", act="SiLU", data="spike"))
        out.append(Case(kind, 1033, 264, 128, "w4/mh4/split/py/rn/nt2/rem2", act="GELU"))
        out.append(Case(kind, 1024, 256, 128, "w4/mh4/split/nt1/rem1", act="ReLU", data="exact"))
    return out


def heads_cases():
    out = []
    for h in (1, 3):
        out.append(Case("heads", 300, 264, 128, "w4/mh8/rm/rn/nt2/rem2/batched", h=h, bias=False, data="exact"))
        out.append(Case("heads", 300, 264, 192, "w4/mh8/rm/rn/nt2/rem2/batched", h=h, bias=False, data="spike"))
        out.append(Case("heads", 513, 520, 128, "w4/mh8/rm/rn/nt3/rem3/batched", h=h, bias=False, data="exact", pads=(8, 8, 0)))
        out.append(Case("heads", 300, 264, 64, "k128/vec1/batched", h=h, bias=False, data="exact"))  # K < 128
        out.append(Case("heads", 130, 132, 128, "k128/vec1/batched", h=h, bias=False, data="ordinary"))  # N % 8 != 0
        out.append(Case("heads", 130, 136, 96, "k128/vec1/batched", h=h, bias=False, data="exact", dtype=F32))
        out.append(Case("heads", 130, 136, 128, "k128/vec1/batched", h=h, bias=False, data="ordinary", out=F32))
    return out


def big_cases():
    """Multi-round launches: stagger, the half-tile second launch (residual + fold + statistics), mt nt >= 1024."""
    split = "w4/mh8/split/in4/nt16/rem8/stagger"
    return [Case("linear", 8192, 4096, 512, "w4/mh8/nt16/rem8/stagger", act="GELU", data="spike"),
            Case("linear", 9475, 4096, 2048, split, fold=True, res=True, stats=True, data="exact"),
            Case("linear", 9475, 4096, 2048, split, fold=True, res=True, stats=True, data="ordinary"),
            Case("linear", 16384, 4096, 128, "w4/mh8/nt16/rem8/nomodel", res=True, data="exact"),
            Case("linear", 16384, 4096, 128, "w4/mh8/nt16/rem8/nomodel", act="SiLU", res=True, data="spike")]


def all_cases():
    return generic_cases() + w4_cases() + dual_cases() + heads_cases() + big_cases()


def is_big(c) -> bool:
    return c.m * c.n * c.k * max(c.h, 1) > 4e9


# ================================================================================================ data
def _gen(c) -> torch.Generator:
    return torch.Generator().manual_seed(c.m * 1000003 + c.n * 1009 + c.k * 17 + len(c.act) + 7 * c.h)


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def operands(c):
    """CPU operands of a case, in the case's dtype where the kernel reads that dtype: x [M, Kx], w [N, K] / [H, N, K], bias,
    res / pre [M, N], stats [M, 2] and colsum [N] (fold), plus gamma / beta / w32 / b32 of the fold for the true-LayerNorm check."""
    g = _gen(c)
    m, n, k, h = c.m, c.n, c.k, max(c.h, 1)
    kx = k * h
    o = types.SimpleNamespace(res=None, pre=None, stats=None, colsum=None, bias=None, ln=None)
    if c.data == "exact":
        dens = min(1.0, 96.0 / k)
        x = _ints(g, (m, kx), -1, 1) * (torch.rand((m, kx), generator=g) < dens)
        w = _ints(g, (h * n, k), -2, 2)
        b = _ints(g, (n,), -64, 64)
    else:
        x = torch.randn((m, kx), generator=g, dtype=torch.float64) + 0.3
        w = (torch.randn((h * n, k), generator=g, dtype=torch.float64) + 0.2) / math.sqrt(k)
        b = torch.randn((n,), generator=g, dtype=torch.float64) * 0.5 + 0.1
        if c.data == "cancel":  # the second half of k repeats the first with the opposite weight: sum ~ 0, S large
            half = k // 2
            for j in range(h):
                x[:, j * k + half:(j + 1) * k] = x[:, j * k:j * k + half] * (1.0 + 2.0 ** -6 * torch.randn((m, half), generator=g,
                                                                                                       dtype=torch.float64))
            w = w.to(c.dtype).double()
            w[:, half:] = -w[:, :half]
        elif c.data == "spike":  # one k per row carries the mass
            x = x * 0.05
            rows = torch.arange(m)
            for j in range(h):
                x[rows, j * k + (7 * rows + 3) % k] = 8.0
        elif c.data == "fold_mean":  # |mean| = 100 x spread
            sign = torch.where(torch.arange(m) % 2 == 0, 1.0, -1.0).double()
            x = 5.0 * sign[:, None] + 0.05 * torch.randn((m, kx), generator=g, dtype=torch.float64)
        elif c.data == "b300":  # y = 300 +- 0.05: the one-pass variance cancels
            w = w * 0.05
            b = torch.full((n,), 300.0, dtype=torch.float64)
            b[::2] += 2.0
    o.x = x.to(c.dtype)
    o.bias = b.float() if c.bias else None
    if c.fold:
        if c.data == "exact":  # statistics and column sums that keep the fold exact: powers of two and small integers
            o.w = w.to(c.dtype)
            rows = torch.arange(m)
            o.stats = torch.stack([(1.0 + (rows % 2)).float(), ((rows % 5) - 2.0).float()], dim=1).contiguous()  # period 10: no tile height
            o.colsum = _ints(g, (n,), -8, 8).float()
            o.x = (o.x.double() * (torch.rand((m, kx), generator=g) < 0.5)).to(c.dtype)  # halves |acc|: 2 acc + s + b + r <= 256
        else:  # runtime.fold_layer_norm, restated
            gam = (1.0 + 0.2 * torch.randn(k, generator=g)).float()
            bet = (0.1 * torch.randn(k, generator=g)).float()
            w32 = w.float()
            o.w = (w32 * gam[None, :]).to(c.dtype)
            o.colsum = o.w.float().sum(dim=1).contiguous()
            o.bias = (w32 @ bet + b.float()).contiguous()
            xs = o.x.double()
            mu = xs.mean(dim=1)
            r = ((xs - mu[:, None]).pow(2).mean(dim=1) + eps32(EPS)).rsqrt()
            o.stats = torch.stack([r, -mu * r], dim=1).float().contiguous()
            o.ln = types.SimpleNamespace(gamma=gam, beta=bet, w32=w32, b32=b.float())
    else:
        o.w = w.to(c.dtype)
    if c.h:
        o.w = o.w.reshape(h, n, k).contiguous()
    if c.res:
        o.res = (_ints(g, (m, n), -64, 64) if c.data == "exact" else torch.randn((m, n), generator=g, dtype=torch.float64) * 2.0).to(c.dtype)
    if c.kind == "actgrad":
        o.pre = (_ints(g, (m, n), -3, 3) if c.data == "exact" else torch.randn((m, n), generator=g, dtype=torch.float64) * 2.5).to(c.dtype)
        o.bias = None
    return o


# ================================================================================================ references and bounds
def _row_flags(c, rt):
    """(poly, two) per row: which rows get the four-wave polynomial GELU and which the round / add / round residual."""
    m = c.m
    poly = torch.zeros(m, dtype=torch.bool)
    two = torch.zeros(m, dtype=torch.bool)
    if rt.kernel == "w4":
        poly[:rt.main_rows] = True
        two[:rt.main_rows] = True
        if rt.tail.startswith("in") or rt.tail == "skinny":
            two[rt.main_rows:] = True
    elif rt.tail == "skinny":
        two[m // BIG * BIG:] = True
    return poly, two


def _gnn_act_bound(x, result):
    """The bound of the stand-alone activation kernels (_gnn_ops_ref): rows that ops.py's fallbacks compute."""
    return ACT_A * torch.maximum(torch.maximum(x.abs(), result.abs()), torch.ones_like(x))


def _approx(z, a, act, poly_rows, py_rows=None):
    if act in ("Identity", "ReLU"):
        return torch.zeros_like(z)
    if act == "SiLU":
        own = SILU_REL * z.abs()
    else:
        erf_form = GELU_ERF_REL * z.abs() + gamma(3) * a.abs()
        own = torch.where(poly_rows[:, None].to(z.device), GELU_POLY_ERR + gamma(12) * z.abs().clamp_min(1.0), erf_form)
    return own if py_rows is None else torch.where(py_rows[:, None], _gnn_act_bound(z, a), own)


def _dact_err(pre, g, act, py_rows):
    if act == "ReLU":
        return torch.zeros_like(pre)
    if act == "SiLU":
        own = (SILU_REL + gamma(4)) * (1.0 + pre.abs())
    else:
        own = torch.where(pre.abs() <= DGELU_CLAMP, torch.full_like(pre, DGELU_POLY_ERR_IN), torch.full_like(pre, DGELU_POLY_ERR_OUT)) \
            + gamma(12) * pre.abs().clamp_min(1.0)
    return torch.where(py_rows[:, None], _gnn_act_bound(pre, g), own)


def _store(want, e, out_dtype):
    return e + RB * (want.abs() + e) if out_dtype == BF16 else e


def products(c, o, device="cpu", rows=None):
    """(acc, S) in f64: x W^T and |x| |W|^T, [M, N] (heads: [M, H N], one product per head); ``rows``: only these rows."""
    x, w = (o.x if rows is None else o.x[rows]).to(device).double(), o.w.to(device).double()
    if c.h:
        acc = torch.cat([x[:, j * c.k:(j + 1) * c.k] @ w[j].T for j in range(c.h)], dim=1)
        s = torch.cat([x[:, j * c.k:(j + 1) * c.k].abs() @ w[j].abs().T for j in range(c.h)], dim=1)
        return acc, s
    return x @ w.T, x.abs() @ w.abs().T


def reference(c, o, rt, device="cpu", acc_s=None, rows=None):
    """{output name: (want, bound)} in f64 on ``device``: 'y' always, 'pre' for dual.  (The statistics are referenced from the
    stored y: ``stats_ref``.)  ``rows``: original indices of a row sample; everything is then [len(rows), N]."""
    acc, s = acc_s if acc_s is not None else products(c, o, device, rows)
    dev = acc.device
    ridx = torch.arange(c.m) if rows is None else rows
    if rows is not None:
        o = types.SimpleNamespace(**{k: (v[rows] if k in ("res", "pre", "stats") and v is not None else v)
                                     for k, v in vars(o).items()})
    exact = c.data == "exact"
    e_acc = torch.zeros_like(acc) if exact else gamma(c.k) * s
    b = o.bias.to(dev).double()[None, :] if o.bias is not None else torch.zeros((1, acc.shape[1]), dtype=torch.float64, device=dev)
    poly, two = _row_flags(c, rt)
    poly, two = poly[ridx], two[ridx].to(dev)
    py = torch.zeros(c.m, dtype=torch.bool)
    if rt.kernel == "py":
        py[:] = True
    elif rt.tail == "py":
        py[rt.main_rows:] = True
    py = py[ridx].to(dev)
    if c.kind == "actgrad":
        pre = o.pre.to(dev).double()
        g = dact64(pre, c.act)
        want = acc * g
        ea = torch.where(py[:, None], e_acc + RB * (acc.abs() + e_acc), e_acc)
        e = g.abs() * ea + (acc.abs() + ea) * _dact_err(pre, g, c.act, py) + U * want.abs()
        if exact:
            e = torch.zeros_like(e)
        return {"y": (want, e if exact else _store(want, e, c.out))}
    if c.fold:
        st = o.stats.to(dev).double()
        cs = o.colsum.to(dev).double()[None, :]
        t1, t2 = st[:, :1] * acc, st[:, 1:] * cs
        z = t1 + t2 + b
        e_z = st[:, :1].abs() * e_acc + gamma(3) * (t1.abs() + t2.abs() + b.abs())
    else:
        z = acc + b
        e_z = e_acc + U * (acc.abs() + b.abs() + e_acc)
    if exact:
        e_z = torch.zeros_like(e_z)
    out = {}
    if c.kind == "dual":
        out["pre"] = (z, _store(z, e_z, BF16) if not exact else e_z)
        if not exact:
            e_z = torch.where(py[:, None], e_z + RB * (z.abs() + e_z), e_z)
            poly = poly & ~py.cpu()
    a = act64(z, c.act)
    e_act = torch.zeros_like(z) if exact else LIP[c.act] * e_z + _approx(z, a, c.act, poly, py if c.kind == "dual" else None)
    if o.res is None:
        out["y"] = (a, e_act if exact else _store(a, e_act, c.out))
        return out
    r = o.res.to(dev).double()
    want = a + r
    if exact:
        out["y"] = (want, e_act)
        return out
    e1 = torch.where(two[:, None], e_act + RB * (a.abs() + e_act), e_act) if c.out == BF16 else e_act
    e2 = e1 + U * (want.abs() + e1)
    out["y"] = (want, _store(want, e2, c.out))
    return out


def fold_true_ref(c, o, device="cpu"):
    """(z_true, extra) of the fold against LayerNorm itself: z_true = LayerNorm(x; gamma, beta) W^T + b in f64 from the f32
    parameters, ``extra`` >= |z_fold - z_true|, the distance between the fold's own reference and the truth:
      statistics:  sum_k (|x_k| br + bs) |W'_k|      (br, bs: _row_kernels_ref.row_stats_ref's bound of (rstd, shift); the
                   statistics handed over here are the f64 values rounded to f32, which that bound covers)
      W' = bf16(fl32(W gamma)):  sum_k |r (x_k - mu)| (RB + u) |W_k gamma_k|
      colsum (f32 sum of K terms):  |shift| gamma(K) sum_k |W'_k|;   b' = fl(W beta + b):  gamma(K + 1) (sum_k |W_k beta_k| + |b|)."""
    ln = o.ln
    x = o.x.to(device).double()
    w32, gam, bet = ln.w32.to(device).double(), ln.gamma.to(device).double(), ln.beta.to(device).double()
    wq = o.w.to(device).double()
    (st, sb) = row_stats_ref(o.x, EPS)
    st, sb = st.to(device), sb.to(device)
    mu = x.mean(dim=1, keepdim=True)
    r = st[:, :1]
    xn = (x - mu) * r
    z_true = (xn * gam[None, :] + bet[None, :]) @ w32.T + ln.b32.to(device).double()[None, :]
    wg = (w32 * gam[None, :]).abs()
    extra = (x.abs() * sb[:, :1]) @ wq.abs().T + sb[:, 1:] * wq.abs().sum(dim=1)[None, :] + (RB + U) * (xn.abs() @ wg.T) \
        + st[:, 1:].abs() * gamma(c.k) * wq.abs().sum(dim=1)[None, :] \
        + gamma(c.k + 1) * ((w32 * bet[None, :]).abs().sum(dim=1) + ln.b32.to(device).double().abs())[None, :]
    return z_true, extra


def stats_ref(y_stored, n, rt, m, eps=EPS):
    """(want, bound) [M, 2] of the statistics of the stored y [M, N] (any dtype; widened exactly)."""
    y = y_stored.double().cpu()
    want, two_pass = row_stats_ref(y_stored.cpu(), eps)
    if not rt.rs:
        return want, two_pass
    e32 = eps32(eps)
    mu = y.mean(dim=1)
    ey2 = (y * y).mean(dim=1)
    qc = ((y - mu[:, None]) ** 2).mean(dim=1)
    rows = torch.arange(m)
    tiled = rows < rt.main_rows
    depth = torch.where(tiled, torch.tensor(34.0 + n / 128.0), torch.tensor(n / 256.0 + 10.0)).double()
    dm = gamma(depth) * y.abs().sum(dim=1) / n
    dq = 2.0 * mu.abs() * dm + dm * dm + gamma(depth + 3) * (ey2 + mu * mu)
    big_d = qc + e32
    dd = dq + gamma(2) * (qc + dq + e32)
    r = big_d.rsqrt()
    r_hi = torch.clamp(big_d - dd, min=e32).rsqrt()
    br = torch.maximum(r - (big_d + dd).rsqrt(), r_hi - r) + RSQRT_REL * r_hi
    bs = dm * (r + br) + mu.abs() * br + U * (mu.abs() + dm) * (r + br)
    one_pass = torch.stack([br, bs], dim=1)
    ratio = qc / ey2.clamp_min(1e-300)
    tail = ~tiled & (rt.tail.startswith("in"))
    bound = torch.where((tiled & (ratio > 2e-3))[:, None] | tail[:, None], one_pass,
                        torch.where((tiled & (ratio >= 0.5e-3))[:, None], torch.maximum(one_pass, two_pass), two_pass))
    return want, bound


def sample_rows(c, rt, n=64):
    """Rows of a large case checked against a CPU product: first and last row of every row tile and of launch B, every tail row,
    and ``n`` seeded random rows."""
    tm = 32 * rt.mh if rt.mh else 128
    rows = set()
    main, m_a = rt.main_rows, rt.m_a
    for r0 in range(0, m_a, BIG if rt.second else tm):
        rows |= {r0, min(r0 + (BIG if rt.second else tm), m_a) - 1}
    for r0 in range(m_a, main, 128):
        rows |= {r0, min(r0 + 128, main) - 1}
    rows |= set(range(main, c.m))
    g = torch.Generator().manual_seed(c.m + c.n)
    rows |= set(int(i) for i in torch.randint(0, c.m, (n,), generator=g))
    return torch.tensor(sorted(rows))
