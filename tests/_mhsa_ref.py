"""f64 references, per-element error bounds, data sets, the launcher's route and the case lists for multi-head self
attention (csrc/attention.hip behind ``ops.mhsa`` / ``ops.mhsa_backward`` / ``autograd.mhsa``).

Pure torch on the CPU; imports nothing from the GPU side (``assert_same_plan`` alone reads the library's status text).  Used by tests/test_mhsa_ref_cpu.py (validates the references
against f64 autograd, shows that emulations of the kernels' arithmetic stay inside the bounds and that subtly wrong results do
not) and by tests/test_gpu_mhsa.py (the kernels).

The operation, per batch element b and head h, on the rows of ``qkv = [q | k | v]`` AS STORED (a bf16 operand converts
exactly), c = 1 / sqrt(D):
    s_ij = c q_i . k_j  for the visible keys (all, or |i - j| <= window),   lse_i = log sum_j exp(s_ij),
    P_ij = exp(s_ij - lse_i),   Pt_ij = P_ij keep_ij / (1 - p)  (dropout: the normaliser sees every key),   out_i = sum_j Pt_ij v_j
    dP_ij = do_i . v_j,  delta_i = do_i . out_i,  dS_ij = P_ij (keep_ij / (1 - p) dP_ij - delta_i),
    dv_j = sum_i Pt_ij do_i,   dq_i = c sum_j dS_ij k_j,   dk_j = c sum_i dS_ij q_i.
``keep`` is the kernels' counter-based hash (``keep_mask``: csrc/attention.hip::dropout_keep restated with integer torch ops).

Every bound is per element: |got - want| <= bound and got finite, for each element, nothing exempt.

Notation (as tests/_row_kernels_ref.py): u = 2^-24, gamma(n) = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical
Algorithms, lemma 3.1; a sum of n f32 terms in ANY order errs by at most gamma(n - 1) sum|t_i|, section 4.2), EPS32 = 2 u,
rb = BF16_STORE = 2^-8: one round-to-nearest to bf16's 8 significant bits errs by half a unit of the last place, 2^-8 relative
just above a power of two (e^3.5 = 33.12 -> 33.0 is 0.35 %; the CPU test's fixed-maximum emulation reaches it, an online
maximum hides it because the largest probability is exactly 1).  The final store is the same rounding (the project's
convention, _gnn_ops_ref), applied to |want| + (the bound in front of it) because it is the computed value that is rounded.

Probabilities.  The exponent s_ij - reference is formed in f32: the products of two bf16 numbers are exact, D of them are
summed (gamma(D) sum_d |q_id k_jd|), the f32 scale 1 / sqrtf(D) [times log2 e] is two to four roundings off c (<= 4 u
|s_ij|), the subtraction (or the fma) and the product inside a fast exponential round once each on a number of at most 2 M_i,
M_i = c max_j sum_d |q_id| |k_jd| >= |s_ij| over the visible keys.  An absolute error e of the exponent is a relative error
expm1(e) of the probability; the hardware exponential itself is good to one ulp (CDNA ISA guide, v_exp_f32).  Altogether
    eta_i = gamma(D + 7) M_i + 2 EPS32           (relative, every probability of row i; the row's reference cancels in o / l)
For the gap rows (|s| ~ 100 nats) eta is 4e-4, a fifth of rb; for ordinary rows it is below 1e-5.

bf16 MFMA forward (mhsa_bf16_kernel, mhsa_bf16_w4_kernel; the key-split tail pair computes the same in f32 and is held to the
same bound).  The probabilities are rounded to bf16 (rb) BEFORE the P V product and the normaliser is the sum of the ROUNDED
probabilities, both sums run in f32 on the matrix pipe in an order the tests do not assume (S terms, a rescale per 32-key block
under the online maximum: gamma(S + S / 32 + 4) with the final 1 / l and product):
    eps_i = rb + eta_i + gamma(S + S / 32 + 4)
    num^ = sum_j Pt_ij (1 + e_ij) v_j,  l^ / l = 1 + e'_i,  |e|, |e'| <= eps_i:
    |num^ / (l^ / l) - out| = |num^ - out - out e'| / (1 + e') <= eps_i (A_i + |want|) / (1 - eps_i) =: E32,   A_id = sum_j Pt_ij |v_jd|
    bound = E32 + BF16_STORE (|want| + E32)  [+ 2^-120 max|v|: v_exp_f32 flushes results below 2^-126, l >= 1]
With |want| <= A this is below c 2^-9 (2 A + |want|), c = MFMA_C = 2.25:  2^-8 (A + |want|) + 2^-8 |want| = 2^-9 (2 A + 4 |want|)
<= 2 x 2^-9 (2 A + |want|), and the rest (eta, gamma, 1 / (1 - eps), the store of E32) stays under the remaining 12 % on
every data set of this module -- asserted by the CPU test (``mfma_form``), so the bound in use is never wider than that form.
    lse:  log(l^ / l) <= eps_i / (1 - eps_i);  v_log_f32 (1 ulp) on |log2 l^| <= (|lse| + M_i) / ln 2, the sum m + log2 l and the
    product with ln 2 round once each:  bound = eps_i / (1 - eps_i) + 4 EPS32 (|lse| + M_i).
A kernel whose normaliser sums the UNROUNDED probabilities breaks the cancellation of the common part of e and e' but not the
bound (e' = 0 is allowed).

f32 arithmetic (mhsa_generic_kernel f32 / bf16 storage, and the VALU backward).  The roundoff part is the same expression
without rb:  epsg_i = eta_i + gamma(S + 6),  E = epsg_i (A + |want|) / (1 - epsg_i);  lse: epsg_i / (1 - epsg_i) + 4 EPS32 (|lse| + M_i).
What __expf / __logf (exp2 / log2 around a rounded product with log2 e) add cannot be derived from a published figure, so, as
the GNN file does with its constant A, it is MEASURED on something else than the kernels: torch's own f32 attention on the CPU
(the explicit softmax expression and its autograd) against the f64 reference over F32_MEASURE_CASES, as the worst fraction of
the derived bound (TORCH_F32[...], re-measured by the CPU test, which fails if it moves by more than 1 %).  The kernels get
F32_FACTOR = 4 times that: the factor covers the fast intrinsics and the different summation order.  bf16 storage: one store.

Backward.  The reference is the TRUE gradient (f64, from qkv and dout alone); the kernels recompute P from the stored lse and
form delta from the stored out, so the bound takes what is known about those two operands: ``out_err`` >= |out_stored - out|
per element and ``lse_err`` >= |lse_stored - lse| per row (the forward bounds above, or the actual deviations where the test
hands the backward operands of its own making).  Terms, in the open:
    P^_ij = P_ij (1 + e),  |e| <= relP_i = x / (1 - x),  x = eta_i + lse_err_i            (exponent error, lse error carried in)
    delta^_i:  Ed_i = sum_d |do_id| out_err_id + gamma(D + 1) sum_d |do_id| (|out_id| + out_err_id)     (delta from the stored out)
    dP^_ij:    EdP_ij = gamma(D) sum_d |do_id| |v_jd|                                             (f32 accumulation)
    inner = kk_ij dP_ij - delta_i:   Ein_ij = kk_ij EdP_ij + Ed_i + 2 u (|kk_ij dP_ij| + |delta_i|)
    dS^_ij:    EdS_ij = |dS_ij| (relP_i + u) + P_ij (1 + relP_i) Ein_ij;   MFMA: + rb (|dS_ij| + EdS_ij)   (dS rounded to bf16)
    Pt^_ij:    EPt_ij = Pt_ij (relP_i + 2 u);                                MFMA: + rb (Pt_ij + EPt_ij)   (P rounded to bf16)
    dv_jd:  sum_i EPt_ij |do_id| + gamma(S + S / 32) sum_i (Pt_ij + EPt_ij) |do_id|
    dq_id:  c [sum_j EdS_ij |k_jd| + gamma(S + S / 32 + 2) sum_j (|dS_ij| + EdS_ij) |k_jd|],   dk_jd: the same over i with |q_id|
    then the store (bf16: BF16_STORE (|want| + bound)).
f32 arithmetic: rb = 0, the roundoff part (the expression at out_err = lse_err = 0) times F32_FACTOR TORCH_F32[...], the operand
part (the difference to the full expression) as derived.
A backward that forms delta from the UNROUNDED out is more accurate than this contract: no accuracy bound can reject it, and
the CPU test asserts exactly that instead of pretending otherwise.
"""

from __future__ import annotations

import math
import types

import torch

from _gnn_ops_ref import BF16_STORE, EPS32

U = EPS32 / 2.0
RB = BF16_STORE
F32, BF16 = torch.float32, torch.bfloat16
MFMA_C = 2.25
F32_FACTOR = 4.0
# torch's f32 attention on the CPU against the f64 reference: worst fraction of the DERIVED f32 bound (measure_torch_f32)
TORCH_F32 = {"out": 0.05586, "lse": 0.03851, "dq": 0.07408, "dk": 0.05722, "dv": 0.03910}


def name(dtype) -> str:
    return "f32" if dtype == F32 else "bf16"


def gamma(n):
    n = torch.as_tensor(n, dtype=torch.float64).clamp_min(0.0)
    return n * U / (1.0 - n * U)


# ------------------------------------------------------------------------------------------------ dropout mask
def keep_mask(seed: int, p: float, b: int, h: int, s: int, h0: int = 0, h_total: int = 0) -> torch.Tensor:
    """The kernels' counter-based keep mask (csrc/attention.hip::dropout_keep) restated with torch integer arithmetic:
    [B, H, S, S] of 0 / 1.  One 32-bit hash of (row, key >> 1) -- one multiply, two fold-downs -- decides a key pair, 15 bits
    per key."""
    m32 = 0xFFFFFFFF
    h_total = h_total or h
    bb = torch.arange(b, dtype=torch.int64).view(b, 1, 1, 1)
    hh = torch.arange(h, dtype=torch.int64).view(1, h, 1, 1) + h0
    qq = torch.arange(s, dtype=torch.int64).view(1, 1, s, 1)
    row = (bb * h_total + hh) * s + qq  # (b * H_total + h0 + h) * S + i
    col = torch.arange(s, dtype=torch.int64).view(1, 1, 1, s)
    x = ((row & m32) * 0x9E3779B1) & m32
    x = x ^ (((row >> 32) * 0x85EBCA77) & m32) ^ (seed & m32)
    x = x ^ (((col >> 1) * 0xC2B2AE3D) & m32)
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & m32
    x = x ^ (x >> 15)
    bits = (x >> (16 * (col & 1))) & 0x7FFF
    thr = min(int(p * 32768.0 + 0.5), 32768)
    return (bits >= thr).to(torch.float64) if p < 1.0 else torch.zeros(b, h, s, s, dtype=torch.float64)


def keep_scalar(seed: int, p: float, s: int, h_total: int, b: int, hg: int, i: int, j: int) -> int:
    """One decision of ``keep_mask`` in plain Python integers (an independent restatement, for the CPU test)."""
    m32 = 0xFFFFFFFF
    row = (b * h_total + hg) * s + i
    x = ((row & m32) * 0x9E3779B1 & m32) ^ ((row >> 32) * 0x85EBCA77 & m32) ^ (seed & m32)
    x ^= (j >> 1) * 0xC2B2AE3D & m32
    x ^= x >> 16
    x = x * 0x7FEB352D & m32
    x ^= x >> 15
    thr = min(int(p * 32768.0 + 0.5), 32768)
    return int(p < 1.0 and ((x >> (16 * (j & 1))) & 0x7FFF) >= thr)


def threshold15(p: float) -> int:
    return 0x8000 if p >= 1.0 else min(int(p * 32768.0 + 0.5), 32768) if p > 0.0 else 0


# ------------------------------------------------------------------------------------------------ layout
def heads(x: torch.Tensor, b: int, h: int) -> torch.Tensor:
    """[B S, H D] -> [B, H, S, D] f64."""
    rows, c = x.shape
    return x.double().reshape(b, rows // b, h, c // h).permute(0, 2, 1, 3)


def rows_of(x: torch.Tensor) -> torch.Tensor:
    """[B, H, S, D] -> [B S, H D]."""
    b, h, s, d = x.shape
    return x.permute(0, 2, 1, 3).reshape(b * s, h * d)


def visible(s: int, window: int) -> torch.Tensor:
    i = torch.arange(s)
    if window < 0:
        return torch.ones(s, s, dtype=torch.bool)
    return (i[:, None] - i[None, :]).abs() <= window


# ------------------------------------------------------------------------------------------------ references
def attention_f64(q, k, v, vis, kk=None, c=None, weight=None):
    """(out, lse, P, Pt) of [B, H, S, D] f64 operands; ``vis`` [S, S] bool (or broadcastable), ``kk`` = keep / (1 - p),
    ``weight``: multiplicity of every (query, key) pair (the mutants: 0 = dropped, 2 = counted twice)."""
    c = 1.0 / math.sqrt(q.shape[-1]) if c is None else c
    sc = (q @ k.transpose(-1, -2)) * c
    sc = sc.masked_fill(~vis, float("-inf"))
    if weight is not None:
        sc = sc + torch.log(weight)
    lse = torch.logsumexp(sc, dim=-1)
    prob = torch.exp(sc - lse[..., None])
    pt = prob if kk is None else prob * kk
    return pt @ v, lse, prob, pt


def forward_ref(qkv, b: int, h: int, window: int = -1, keep=None, p: float = 0.0):
    """Everything the forward bounds and the backward share; ``out`` / ``a`` are [B S, C], ``lse`` / ``m`` [B, H, S]."""
    c3 = qkv.shape[1]
    cc = c3 // 3
    q, k, v = (heads(t, b, h) for t in qkv.split(cc, dim=1))
    s, d = q.shape[2], q.shape[3]
    vis = visible(s, window)
    kk = None
    if keep is not None:
        kk = keep * (1.0 / (1.0 - p) if p < 1.0 else 0.0)
    out, lse, prob, pt = attention_f64(q, k, v, vis, kk)
    a = pt @ v.abs()
    m = ((q.abs() @ k.abs().transpose(-1, -2)) / math.sqrt(d)).masked_fill(~vis, 0.0).amax(dim=-1)
    return types.SimpleNamespace(q=q, k=k, v=v, vis=vis, kk=kk, c=1.0 / math.sqrt(d), P=prob, Pt=pt, b=b, h=h, s=s, d=d,
                                 out=rows_of(out), lse=lse, a=rows_of(a), m=m, out4=out)


def backward_ref(ref, dout):
    """The true gradients; ``dq`` / ``dk`` / ``dv`` are [B S, C] (``dqkv`` their concatenation)."""
    do = heads(dout, ref.b, ref.h)
    dp = do @ ref.v.transpose(-1, -2)
    kdp = dp if ref.kk is None else dp * ref.kk
    delta = (do * ref.out4).sum(dim=-1)
    ds = ref.P * (kdp - delta[..., None])
    dq = (ds @ ref.k) * ref.c
    dk = (ds.transpose(-1, -2) @ ref.q) * ref.c
    dv = ref.Pt.transpose(-1, -2) @ do
    return types.SimpleNamespace(do=do, kdp=kdp, delta=delta, dS=ds, dq=rows_of(dq), dk=rows_of(dk), dv=rows_of(dv),
                                 dqkv=torch.cat([rows_of(dq), rows_of(dk), rows_of(dv)], dim=1))


# ------------------------------------------------------------------------------------------------ bounds
def eta(ref) -> torch.Tensor:
    return gamma(ref.d + 7) * ref.m + 2.0 * EPS32


def _store(want, b32, dtype):
    return b32 + BF16_STORE * (want.abs() + b32) if dtype == BF16 else b32


def _per_row(t, ref):
    """[B, H, S] -> [B S, C] (every channel of a head the row's value)."""
    return rows_of(t[..., None].expand(ref.b, ref.h, ref.s, ref.d))


def forward_derived(ref, kind: str):
    """(E32 [B S, C], lse bound [B, H, S]) of the f32 result in front of the store; ``kind`` "mfma" or "f32"."""
    if kind == "mfma":
        eps = RB + eta(ref) + gamma(ref.s + ref.s // 32 + 4)
    else:
        eps = eta(ref) + gamma(ref.s + 6)
    e32 = _per_row(eps / (1.0 - eps), ref) * (ref.a + ref.out.abs())
    if kind == "mfma":
        e32 = e32 + 2.0 ** -120 * rows_of(ref.v.abs().amax(dim=2, keepdim=True).expand_as(ref.v))
    return e32, eps / (1.0 - eps) + 4.0 * EPS32 * (ref.lse.abs() + ref.m)


def forward_bounds(ref, kind: str, dtype):
    """(out bound [B S, C], lse bound [B, H, S]) of a kernel of ``kind`` that stores ``dtype``."""
    e32, el = forward_derived(ref, kind)
    if kind == "f32":
        e32, el = e32 * (F32_FACTOR * TORCH_F32["out"]), el * (F32_FACTOR * TORCH_F32["lse"])
    return _store(ref.out, e32, dtype), el


def mfma_form(ref) -> torch.Tensor:
    """c 2^-9 (2 A + |want|): the first-order form of the bf16 MFMA bound (the CPU test asserts that the bound is below it)."""
    return MFMA_C * RB * (2.0 * ref.a + ref.out.abs())


def _backward_derived(ref, bw, kind: str, out_err, lse_err):
    rb = RB if kind == "mfma" else 0.0
    s, d = ref.s, ref.d
    x = eta(ref) + lse_err
    relp = (x / (1.0 - x))[..., None]
    out_err4 = heads(out_err, ref.b, ref.h)
    ed = (bw.do.abs() * out_err4).sum(-1) + gamma(d + 1) * (bw.do.abs() * (ref.out4.abs() + out_err4)).sum(-1)
    edp = gamma(d) * (bw.do.abs() @ ref.v.abs().transpose(-1, -2))
    if ref.kk is not None:
        edp = edp * ref.kk
    ein = edp + ed[..., None] + 2.0 * U * (bw.kdp.abs() + bw.delta.abs()[..., None])
    eds = bw.dS.abs() * (relp + U) + ref.P * (1.0 + relp) * ein
    eds = eds + rb * (bw.dS.abs() + eds)
    ept = ref.Pt * (relp + 2.0 * U)
    ept = ept + rb * (ref.Pt + ept)
    g1, g2 = gamma(s + s // 32), gamma(s + s // 32 + 2)
    bdv = ept.transpose(-1, -2) @ bw.do.abs() + g1 * ((ref.Pt + ept).transpose(-1, -2) @ bw.do.abs())
    bdq = ref.c * (eds @ ref.k.abs() + g2 * ((bw.dS.abs() + eds) @ ref.k.abs()))
    bdk = ref.c * (eds.transpose(-1, -2) @ ref.q.abs() + g2 * ((bw.dS.abs() + eds).transpose(-1, -2) @ ref.q.abs()))
    return rows_of(bdq), rows_of(bdk), rows_of(bdv)


def backward_bounds(ref, bw, kind: str, dtype, out_err, lse_err):
    """Bounds (dq, dk, dv) [B S, C] each; ``out_err`` [B S, C] and ``lse_err`` [B, H, S] bound the deviation of the stored
    forward results the backward is handed from the true ones."""
    full = _backward_derived(ref, bw, kind, out_err, lse_err)
    if kind == "f32":
        base = _backward_derived(ref, bw, kind, torch.zeros_like(out_err), torch.zeros_like(lse_err))
        full = tuple(b0 * (F32_FACTOR * TORCH_F32[key]) + (b1 - b0) for key, b0, b1 in zip(("dq", "dk", "dv"), base, full))
    return tuple(_store(w, e, dtype) for w, e in zip((bw.dq, bw.dk, bw.dv), full))


# ------------------------------------------------------------------------------------------------ checker
def check(got: torch.Tensor, want: torch.Tensor, bound: torch.Tensor, what: str) -> float:
    """Every element of ``got`` finite and within ``bound`` of ``want``.  Returns the largest fraction of a bound that was
    used (0 / 0 = 0: where the bound is zero the element must be exact).  A failure names the worst element."""
    got = got.detach().cpu()
    assert got.shape == want.shape == bound.shape, f"{what}: shape {tuple(got.shape)}, expected {tuple(want.shape)}"
    if got.numel() == 0:
        return 0.0
    g = got.double()
    finite = torch.isfinite(g)
    if not bool(finite.all()):
        idx = tuple(int(i) for i in torch.nonzero(~finite)[0])
        raise AssertionError(f"{what}: {int((~finite).sum())} non-finite elements, first at {idx}: got {float(g[idx])}, "
                             f"want {float(want[idx]):.9g}")
    diff = (g - want).abs()
    bad = ~(diff <= bound)
    ratio = torch.where(diff == 0, torch.zeros_like(diff), diff / bound)
    worst = float(ratio.max())
    if bool(bad.any()):
        flat = int(torch.argmax(torch.where(bad, ratio, torch.full_like(ratio, -1.0))))
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), got.shape))
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements outside their bound; worst at {idx}: got "
                             f"{float(g[idx]):.9g}, want {float(want[idx]):.9g}, |diff| {float(diff[idx]):.3e} > bound "
                             f"{float(bound[idx]):.3e} (worst ratio {worst:.3g})")
    return worst


def fails(got, want, bound) -> bool:
    """A mutant is rejected: some element is non-finite or outside its bound."""
    g = got.detach().double()
    return not bool((torch.isfinite(g) & ((g - want).abs() <= bound)).all())


# ------------------------------------------------------------------------------------------------ data sets
PAIRS_C = 2.0  # query i = PAIRS_C / 2 (k_pi1(i) + k_pi2(i)): entries -2, 0, 2
COLD_LEVEL = -12.0
INTRUDER_NATS = 20.0
GAP_LOG2 = (40, 100, 121, 123, 126, 140)
GAP_SWEEP = (-1.0, 1.5)  # the rows that see the key are spread over [g - 1, g + 1.5] log2 units
GAP_V = 100.0


def _gen(kind: str, s: int, d: int, window: int, b: int, h: int) -> torch.Generator:
    base = {"pairs": 1, "intruder": 2, "cold": 3, "spread": 4, "gap": 5, "dout": 6}[kind]
    return torch.Generator().manual_seed(((base * 1009 + s) * 1013 + d) * 1019 + max(window, -1) + 2 + 7919 * (b * 64 + h))


def _coprime_step(s: int, start: int) -> int:
    g = max(1, start % max(s, 1))
    while math.gcd(g, s) != 1:
        g += 1
    return g


def pair_targets(s: int, window: int, b: int = 0, h: int = 0):
    """(pi1, pi2): the two designated keys of every query.  Global: two permutations of the key positions (every key is
    designated for some query).  Window: the offset w - (2 i mod (2 w + 1)) takes every value -w ... +w once per 2 w + 1
    queries and i + offset every key position once (2 is coprime to 2 w + 1), the second key is the mirror image i - offset,
    so a query with offset +-w designates BOTH window edges; clipped at the sequence ends."""
    i = torch.arange(s)
    if window < 0 or window >= s - 1:
        g1, g2 = _coprime_step(s, 7 + 2 * h), _coprime_step(s, s // 2 + 3 + 2 * b)
        p1, p2 = (i * g1 + 3 + h) % s, (i * g2 + 11 + b) % s
        if window == s - 1 and s > 1:  # the window's only edges: key S - 1 for query 0, key 0 for query S - 1
            p1[0], p1[s - 1] = s - 1, 0
        return p1, torch.where(p1 == p2, (p2 + 1) % s, p2)  # (two different keys wherever S > 1)
    off = (window - (2 * i) % (2 * window + 1)) * (1 - 2 * ((b + h) % 2))  # (mirrored in every other head)
    return (i + off).clamp(0, s - 1), (i - off).clamp(0, s - 1)


def _pairs_head(s, d, window, b, h):
    g = _gen("pairs", s, d, window, b, h)
    k = torch.randint(0, 2, (s, d), generator=g).double() * 2.0 - 1.0
    p1, p2 = pair_targets(s, window, b, h)
    q = PAIRS_C / 2.0 * (k[p1] + k[p2])
    v = torch.randn(s, d, generator=g, dtype=torch.float64)
    return q, k, v


def intruder_layout(s: int, window: int, b: int = 0, h: int = 0):
    """(target queries, intruder keys): targets every 2 (w + 1) rows, the keys at distance w + 1 between them -- each target
    has an intruder on both sides (where the sequence has room) and sees none."""
    step = 2 * (window + 1)
    t0 = (3 * b + 5 * h) % (window + 1)
    return torch.arange(t0, s, step), torch.arange(t0 + window + 1, s, step)


def _intruder_head(s, d, window, b, h):
    assert 0 <= window and window + 1 < s and d >= 16
    q, k, v = _pairs_head(s, d, window, b, h)
    g = _gen("intruder", s, d, window, b, h)
    u = torch.randint(0, 2, (d,), generator=g).double() * 2.0 - 1.0
    tq, ik = intruder_layout(s, window, b, h)
    q[tq] += 2.0 * u
    vis = visible(s, window)
    amp = 2.0
    while True:
        amp *= 2.0
        assert amp <= 256.0, "intruder: no amplitude separates the keys"
        k[ik] = amp * u
        sc = (q[tq] @ k.T) / math.sqrt(d)
        top_visible = sc.masked_fill(~vis[tq], float("-inf")).amax(dim=1)
        outside = torch.zeros(s, dtype=torch.bool)
        outside[ik] = True
        dist = (tq[:, None] - torch.arange(s)[None, :]).abs()
        intr = sc.masked_fill(~(outside[None, :] & (dist == window + 1)), float("inf")).amin(dim=1)
        if bool((intr - top_visible >= INTRUDER_NATS).all()):
            return q, k, v


def _spread_head(s, d, window, b, h):
    g = _gen("spread", s, d, window, b, h)
    z = torch.randn(s, 3 * d, generator=g, dtype=torch.float64)
    return z[:, :d] * 1.6, z[:, d:2 * d], z[:, 2 * d:]


def _cold_head(s, d, window, b, h, dtype):
    """A common component on the first min(4, D) channels: +a in every query, -a in every key."""
    g = _gen("cold", s, d, window, b, h)
    z = torch.randn(s, 3 * d, generator=g, dtype=torch.float64) * 0.5
    q, k, v = z[:, :d].clone(), z[:, d:2 * d].clone(), z[:, 2 * d:] * 2.0
    n = min(4, d)
    a = 4.0
    while True:
        a *= 2.0
        assert a <= 64.0
        qq, kk = q.clone(), k.clone()
        qq[:, :n] += a
        kk[:, :n] -= a
        sc = (qq.to(dtype).double() @ kk.to(dtype).double().T) / math.sqrt(d)
        if float(sc.max()) <= COLD_LEVEL:
            return qq, kk, v


def gap_key(s: int, g_log2: int) -> int:
    """Position of the one far key: behind the first 32-key block, another 32-key block border / tile border per case."""
    return {40: 32, 100: 63, 121: 64, 123: s - 1, 126: 95, 140: s // 2 + 1}[g_log2]


def _gap_head(s, d, b, h, g_log2):
    """Channels 0, 1 are reserved (zero in every key but the far one, zero in the queries that do not see it).  Rows i with
    i % 2 == 0 see key ``gap_key`` at g + sweep log2 units above the maximum of THEIR first 32-key block; the coarse part of
    the score rides on channel 0 (16 x G), the row's fine part on channel 1."""
    assert d == 64 and s >= 128
    g = _gen("gap", s, d, g_log2, b, h)
    z = torch.randn(s, 3 * d, generator=g, dtype=torch.float64)
    q, k, v = (z[:, :d] * 1.6).bfloat16().double(), z[:, d:2 * d].bfloat16().double(), z[:, 2 * d:].clone()
    q[:, :2] = 0.0
    k[:, :2] = 0.0
    j = gap_key(s, g_log2)
    k[j] = 0.0
    sign = torch.randint(0, 2, (d,), generator=g).double() * 2.0 - 1.0
    v[j] = GAP_V * sign
    block_max = ((q @ k[:32].T) / 8.0).amax(dim=1)  # nats; the far key and channels 0, 1 play no part in it
    rows = torch.arange(0, s, 2)
    sweep = GAP_SWEEP[0] + (GAP_SWEEP[1] - GAP_SWEEP[0]) * torch.arange(len(rows)).double() / max(len(rows) - 1, 1)
    target = (g_log2 + sweep) * math.log(2.0) + block_max[rows]  # score of the far key, nats
    coarse = round(float(target.mean()) * 8.0 / 16.0 * 4.0) / 4.0  # G: a multiple of 1 / 4 below 256 is a bf16 number
    k[j, 0], k[j, 1] = coarse, 1.0
    q[rows, 0] = 16.0
    q[rows, 1] = (8.0 * target - 16.0 * coarse).bfloat16().double()
    return q, k, v


def gap_rows(qkv, h: int, s: int, g_log2: int):
    """(rows that see the far key, their gap in log2 units [H, rows]) of a ``gap`` operand as stored (B = 1)."""
    cc = qkv.shape[1] // 3
    q, k, _ = (heads(t, 1, h)[0] for t in qkv.split(cc, dim=1))
    rows = torch.arange(0, s, 2)
    sc = (q @ k.transpose(-1, -2)) / 8.0
    return rows, (sc[:, rows, gap_key(s, g_log2)] - sc[:, rows, :32].amax(dim=-1)) / math.log(2.0)


def make_qkv(kind: str, dtype, b: int, s: int, h: int, d: int, window: int = -1, g_log2: int = 0) -> torch.Tensor:
    """[B S, 3 H D] in ``dtype``; every (batch element, head) from its own seed."""
    out = torch.empty(b, s, 3, h, d, dtype=torch.float64)
    for bi in range(b):
        for hi in range(h):
            if kind == "pairs":
                parts = _pairs_head(s, d, window, bi, hi)
            elif kind == "intruder":
                parts = _intruder_head(s, d, window, bi, hi)
            elif kind == "spread":
                parts = _spread_head(s, d, window, bi, hi)
            elif kind == "cold":
                parts = _cold_head(s, d, window, bi, hi, dtype)
            elif kind == "gap":
                parts = _gap_head(s, d, bi, hi, g_log2)
            else:
                raise ValueError(kind)
            for t, part in enumerate(parts):
                out[bi, :, t, hi, :] = part
    return out.reshape(b * s, 3 * h * d).to(dtype)


def make_dout(dtype, b: int, s: int, h: int, d: int) -> torch.Tensor:
    g = _gen("dout", s, d, -1, b, h)
    return torch.randn(b * s, h * d, generator=g, dtype=torch.float64).to(dtype)


# ------------------------------------------------------------------------------------------------ the launcher's route
ATT_QBLK = 512


def tail_rows(s: int) -> int:
    """csrc/attention.hip::mhsa_tail_rows."""
    rem = s % ATT_QBLK
    return rem if (s > ATT_QBLK and 0 < rem <= 16) else 0


def tail_splits(b: int, s: int, h: int) -> int:
    """csrc/attention.hip::mhsa_tail_splits."""
    rem = tail_rows(s)
    if rem == 0:
        return 0
    return max(1, min(4096 // (b * rem * h), (s + 255) // 256, 128))


def tail_chunk(b: int, s: int, h: int) -> int:
    n = tail_splits(b, s, h)
    return -(-s // n) if n else 0


def _round256(n: int) -> int:
    return (n + 255) // 256 * 256


def vt_bytes(b: int, s: int, h: int, d: int) -> int:
    return _round256(b * h * d * ((s + 63) // 64 * 64) * 2)


def workspace_bytes(dtype, b: int, s: int, h: int, d: int) -> int:
    """anemoi_mhsa_workspace_bytes: V^T, the tail rows' partial states, the four-wave kernel's flag."""
    if dtype == BF16 and d in (32, 64):
        return vt_bytes(b, s, h, d) + _round256(b * tail_rows(s) * h * tail_splits(b, s, h) * (d + 2) * 4) + 256
    return 0


def backward_workspace_bytes(dtype, b: int, s: int, h: int, d: int) -> int:
    if dtype == BF16 and d in (32, 64):
        return 3 * vt_bytes(b, s, h, d) + 2 * b * h * ((s + 63) // 64 * 64) * 4
    return 0


def _dmax(d: int) -> int:
    return 32 if d <= 32 else 64 if d <= 64 else 128


def _generic_grid(b, s, h):
    return (-(-b * s * h // 4), 1, 1)  # the VALU kernels: a wave per (batch element, row, head), four per workgroup


def route(dtype, b, s, h, d, window, ld, ldo, qkv_ptr=0, out_ptr=0, p=0.0, heads_total=0):
    """The forward launcher's choices (anemoi_mhsa) restated: ``kernel`` "w4" / "w8" / "generic", tail rows and splits, DMAX of
    the generic kernel, the DROP template argument (``drop``: a mask is hashed, 0 < p < 1 after rounding), the main launch's
    ``grid`` and the workspace the route uses (``ws_bytes``: none on the generic route)."""
    drop_all, thr = p >= 1.0, threshold15(p)
    ht = heads_total or h
    mfma = (not drop_all and b * ht * s < 2 ** 32 and dtype == BF16 and d in (32, 64) and qkv_ptr % 16 == 0 and ld % 8 == 0
            and out_ptr % 8 == 0 and ldo % 4 == 0)
    if not mfma:
        return types.SimpleNamespace(kernel="generic", mfma=False, tail=0, n_split=0, chunk=0, dmax=_dmax(d),
                                     drop=thr != 0 and not drop_all, win=False, workgroups=_generic_grid(b, s, h)[0],
                                     grid=_generic_grid(b, s, h), s_pad=0, ws_bytes=0)
    w4 = d == 64 and window < 0 and s * ld * 2 < 2 ** 31
    rem = tail_rows(s)
    wg = -(-(s - rem) // ATT_QBLK)
    return types.SimpleNamespace(kernel="w4" if w4 else "w8", mfma=True, tail=rem, n_split=tail_splits(b, s, h),
                                 chunk=tail_chunk(b, s, h), dmax=0, drop=thr != 0 and not drop_all, win=False, workgroups=wg,
                                 grid=(wg, h, b), s_pad=(s + 63) // 64 * 64, ws_bytes=workspace_bytes(dtype, b, s, h, d))


def route_backward(dtype, b, s, h, d, window, ld, ldo, lddo, lddq, ptrs=(0, 0, 0, 0), p=0.0, heads_total=0, workspace=True):
    """anemoi_mhsa_backward: ``kernel`` "mfma" / "generic", the WIN template argument, DMAX, the grid of the two main kernels.
    ``ptrs``: qkv, out, dout, dqkv.  ``workspace``: its address (True: some aligned one; False / 0: none) -- a call without a
    16-byte aligned workspace takes the VALU kernels, it is not refused."""
    drop_all, thr = p >= 1.0, threshold15(p)
    ht = heads_total or h
    ws = 16 if workspace is True else int(workspace or 0)
    mfma = (not drop_all and b * ht * s < 2 ** 32 and dtype == BF16 and d in (32, 64) and ws != 0 and ws % 16 == 0
            and b * s < 2 ** 31 and ld < 2 ** 31 and lddo < 2 ** 31
            and ptrs[0] % 16 == 0 and ptrs[2] % 16 == 0 and ptrs[1] % 2 == 0 and ptrs[3] % 8 == 0 and ld % 8 == 0
            and lddo % 8 == 0 and lddq % 4 == 0)
    return types.SimpleNamespace(kernel="mfma" if mfma else "generic", mfma=mfma, win=mfma and window >= 0,
                                 dmax=0 if mfma else _dmax(d), drop=thr != 0 and not drop_all, tail=0, n_split=0, chunk=0,
                                 grid=(-(-s // 128), h, b) if mfma else _generic_grid(b, s, h),
                                 s_pad=(s + 63) // 64 * 64 if mfma else 0,
                                 ws_bytes=backward_workspace_bytes(dtype, b, s, h, d) if mfma else 0)


def assert_same_plan(rt, status, lib, what=""):
    """The library's plan (``_lib.mhsa_route``: status and ``MhsaRoute``) equals the restatement ``rt`` field by field."""
    from anemoi_models_amd import _lib

    assert status == 0, f"{what}: anemoi_mhsa_route refuses the call ({status}: {_lib.load().anemoi_last_error()})"
    got = (_lib.MHSA_KERNEL_NAMES[lib.kernel], bool(lib.drop), bool(lib.win), lib.dmax, lib.tail_rows, lib.tail_splits,
           lib.tail_chunk, tuple(lib.grid), lib.S_pad, lib.layout.total)
    want = (rt.kernel, bool(rt.drop), bool(rt.win), rt.dmax, rt.tail, rt.n_split, rt.chunk, tuple(rt.grid), rt.s_pad, rt.ws_bytes)
    assert got == want, f"{what}: the library plans (kernel, drop, win, DMAX, tail rows, splits, chunk, grid, S_pad, workspace) " \
                        f"= {got}, the restatement {want}"


# ------------------------------------------------------------------------------------------------ cases (both test files)
def Case(dtype, b, s, h, d, window, data, expect, g_log2=0, pad=0, opad=0, p=0.0):
    return types.SimpleNamespace(dtype=dtype, b=b, s=s, h=h, d=d, window=window, data=data, expect=expect, g_log2=g_log2,
                                 pad=pad, opad=opad, p=p)


def case_id(c) -> str:
    t = f"{name(c.dtype)}-B{c.b}-S{c.s}-H{c.h}-D{c.d}-w{c.window}-{c.data}"
    t += f"{c.g_log2}" if c.data == "gap" else ""
    t += f"-pad{c.pad}.{c.opad}" if c.pad or c.opad else ""
    return t + (f"-p{c.p}" if c.p else "") + f"-{c.expect}"


def case_qkv(c) -> torch.Tensor:
    return make_qkv(c.data, c.dtype, c.b, c.s, c.h, c.d, c.window, c.g_log2)


def case_kind(c) -> str:
    return "mfma" if c.expect in ("w4", "w8", "mfma") else "f32"


S_EDGES = (1, 31, 32, 33, 64, 65, 127, 129, 512, 513, 528, 529)
WINDOWS = ((65, 0), (65, 1), (130, 31), (130, 32), (130, 63), (130, 64), (200, 199), (200, 200), (200, 5000), (700, 40),
           (514, 40), (1100, 70))
GENERIC_S = (1, 63, 64, 65, 130)
GENERIC_WINDOWS = ((65, 0), (65, 1), (130, 31), (130, 32), (130, 63), (130, 64))
GENERIC_D = {F32: (1, 8, 32, 33, 64, 65, 100, 128), BF16: (16, 48, 128)}


def _ragged(s: int) -> bool:
    return s % 32 != 0


def _has_intruder(s: int, window: int, d: int) -> bool:
    return 0 <= window and window + 1 < s and d >= 16


def forward_mfma_cases():
    out = []
    for d, kern in ((64, "w4"), (32, "w8")):
        for s in S_EDGES:
            for data in ("pairs", "spread") + (("cold",) if _ragged(s) else ()):
                out.append(Case(BF16, 1, s, 2, d, -1, data, kern))
    out += [Case(BF16, 2, 1026, 2, 64, -1, data, "w4") for data in ("pairs", "spread")]
    for d in (64, 32):
        for s, w in WINDOWS:
            datas = ("pairs", "spread") + (("intruder",) if _has_intruder(s, w, d) else ()) + (("cold",) if _ragged(s) else ())
            out += [Case(BF16, 1, s, 2, d, w, data, "w8") for data in datas]
    out += [Case(BF16, 1, s, 2, 64, -1, "gap", "w4", g_log2=g) for s in (200, 700) for g in GAP_LOG2]
    return out


def forward_generic_cases():
    out = []
    for dtype in (F32, BF16):
        for d in GENERIC_D[dtype]:
            for s in GENERIC_S:
                out += [Case(dtype, 1, s, 2, d, -1, data, "generic") for data in ("pairs", "spread")]
            for s, w in GENERIC_WINDOWS:
                out.append(Case(dtype, 1, s, 2, d, w, "intruder" if _has_intruder(s, w, d) else "pairs", "generic"))
    # a pitch that is no multiple of 8 elements takes a bf16 D = 64 call off the MFMA route; + 8 (and an out pitch + 8) keeps it
    out.append(Case(BF16, 1, 130, 2, 64, -1, "pairs", "generic", pad=4))
    out.append(Case(BF16, 1, 130, 2, 64, 31, "pairs", "generic", pad=4))
    out.append(Case(BF16, 1, 130, 2, 64, -1, "pairs", "w4", pad=8, opad=8))
    out.append(Case(BF16, 1, 130, 2, 64, 31, "pairs", "w8", pad=8, opad=8))
    return out


def backward_cases():
    out = []
    for d in (64, 32):
        for s in (1, 31, 32, 33, 127, 128, 129, 300, 514):
            out += [Case(BF16, 1, s, 2, d, -1, data, "mfma") for data in ("pairs", "spread")]
        for w in (0, 1, 31, 32, 100, 300, 5000):
            out.append(Case(BF16, 1, 300, 2, d, w, "pairs", "mfma"))
        out.append(Case(BF16, 1, 300, 2, d, 100, "spread", "mfma"))
        out.append(Case(BF16, 2, 129, 2, d, -1, "pairs", "mfma"))
    for d in (8, 33, 100):
        for s, w in ((1, -1), (65, -1), (130, -1), (130, 31)):
            out.append(Case(F32, 1, s, 2, d, w, "pairs", "generic"))
        out.append(Case(F32, 2, 65, 2, d, -1, "spread", "generic"))
    for d in (64, 16):
        for s, w in ((1, -1), (65, -1), (130, -1), (130, 31)):
            out.append(Case(BF16, 1, s, 2, d, w, "pairs", "generic"))
    return out


def dropout_cases():
    """(forward route, backward route) pairs at one ragged S each."""
    out = []
    for p in (0.25, 0.5):
        out += [Case(BF16, 1, 129, 2, 64, -1, "pairs", "w4", p=p), Case(BF16, 1, 129, 2, 32, -1, "pairs", "w8", p=p),
                Case(BF16, 1, 131, 2, 64, 31, "pairs", "w8", p=p), Case(BF16, 1, 514, 2, 64, -1, "spread", "w4", p=p),
                Case(F32, 1, 65, 2, 33, -1, "pairs", "generic", p=p), Case(BF16, 1, 65, 2, 16, 9, "pairs", "generic", p=p)]
    return out


def backward_expect(c) -> str:
    return "mfma" if c.expect in ("w4", "w8", "mfma") else "generic"


DROPOUT_SEED = 20240611
F32_MEASURE_CASES = [Case(F32, 1, s, 2, d, w, data, "generic") for d in (8, 33, 64, 128) for s, w, data in
                     ((65, -1, "pairs"), (130, -1, "spread"), (130, 31, "pairs"), (130, 32, "intruder"), (65, -1, "cold"))
                     if data != "intruder" or d >= 16]


def torch_f32_attention(qkv, b, h, window, kk=None, dout=None):
    """torch's own f32 attention on the CPU: the explicit softmax expression (and its autograd)."""
    x = qkv.float().clone().requires_grad_(dout is not None)
    cc = x.shape[1] // 3
    q, k, v = (t.reshape(b, x.shape[0] // b, h, cc // h).permute(0, 2, 1, 3) for t in x.split(cc, dim=1))
    sc = (q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(cc // h))
    sc = sc.masked_fill(~visible(sc.shape[-1], window), float("-inf"))
    prob = torch.softmax(sc, dim=-1)
    if kk is not None:
        prob = prob * kk.float()
    out = rows_of(prob @ v)
    lse = torch.logsumexp(sc, dim=-1)
    if dout is None:
        return out.detach(), lse.detach(), None
    out.backward(dout.float())
    return out.detach(), lse.detach(), x.grad


def measure_torch_f32():
    """Worst fraction of the DERIVED f32 bounds that torch's f32 attention uses over F32_MEASURE_CASES (TORCH_F32)."""
    worst = {key: 0.0 for key in TORCH_F32}
    for c in F32_MEASURE_CASES:
        qkv = case_qkv(c)
        dout = make_dout(c.dtype, c.b, c.s, c.h, c.d)
        ref = forward_ref(qkv, c.b, c.h, c.window)
        bw = backward_ref(ref, dout)
        out, lse, grad = torch_f32_attention(qkv, c.b, c.h, c.window, None, dout)
        e32, el = forward_derived(ref, "f32")
        zero_o, zero_l = torch.zeros_like(ref.out), torch.zeros_like(ref.lse)
        bq, bk, bv = _backward_derived(ref, bw, "f32", zero_o, zero_l)
        cc = ref.h * ref.d
        pairs = {"out": (out, ref.out, e32), "lse": (lse, ref.lse, el), "dq": (grad[:, :cc], bw.dq, bq),
                 "dk": (grad[:, cc:2 * cc], bw.dk, bk), "dv": (grad[:, 2 * cc:], bw.dv, bv)}
        for key, (got, want, bound) in pairs.items():
            diff = (got.double() - want).abs()
            frac = torch.where(diff == 0, torch.zeros_like(diff), diff / bound)
            worst[key] = max(worst[key], float(frac.max()))
    return worst
