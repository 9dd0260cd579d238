"""f64 references, per-element error bounds, data sets, shapes and the checker for the LayerNorm family and the row / column
kernels of the dense backward (csrc/elementwise.hip, csrc/backward.hip behind ops.py): ``layer_norm`` (+ residual),
``layer_norm_with_stats``, ``row_stats``, ``layer_norm_backward`` (+ dres), ``col_sum``, ``row_dot``, ``row_scale``, ``add``,
``convert_pad``.

Pure torch on the CPU; imports nothing from the GPU side.  Used by tests/test_row_kernels_ref_cpu.py (validates the backward
reference against torch autograd, shows that correct f32 / bf16 implementations in two summation orders stay inside the bounds
and that subtly wrong ones do not) and by tests/test_gpu_row_kernels.py (the kernels).

Every reference is computed in f64 from the operands AS STORED (a bf16 operand converts exactly; ``eps`` is the f32 value the
library receives; the backward's statistics are the f32 pairs it is handed).  Every bound is per element.

Notation and building blocks
  u = 2^-24 = EPS32 / 2: one rounded f32 operation errs by at most u relative to its result.
  gamma(n) = n u / (1 - n u): n roundings in a row cost at most gamma(n) (Higham, Accuracy and Stability of Numerical
    Algorithms, lemma 3.1).
  Sum of n f32 terms in ANY order (a lane's chain, the wave butterfly, chunk partials, workgroup partials -- the tests assume
    nothing about it):  |s^ - s| <= gamma(n - 1) sum|t_i|  (ibid. section 4.2: every term passes through at most n - 1
    additions).  In the form c n u sum|t_i| the constant is c = 1 / (1 - n u) <= 1.003 for n <= 2^15: nothing but the second
    order terms of the same analysis.  Where the terms themselves are rounded (a product, an fma) n grows by the roundings
    per term, stated at each use.
  EXACT sums: if every term is a multiple of one power of two 2^k and sum|t_i| <= 2^24 2^k, every partial sum in every order
    is a multiple of 2^k below 2^24 2^k, i.e. an f32 number: the sum is exact and its bound is 0 (_exactly_summable).  The
    constant rows (0.75), the zero row and the "exact" row (+-k/4 in cancelling pairs) are of this kind: their mean, their
    centred squares and q = sum d^2 are exact in f32, so that only the division, ``+ eps`` and rsqrtf round.  These rows are
    what resolves C - 1 against C at C >= 4096, where 1 / (2 C) drops below the any-order bound C u / 2 of an ordinary row.
  One bf16 store: 2^-8 relative (BF16_STORE of _gnn_ops_ref: round-to-nearest of 8 significant bits), applied to
    |want| + (the f32 bound), because it is the computed value that is rounded.
  rsqrtf: 2 ulp = 2 EPS32 relative.  ROCm's device library implements the OpenCL accuracy table (rsqrt <= 2 ulp, OpenCL C
    specification, "Relative error as ULPs"); HIP's math API table lists rsqrtf at 1 ulp and the CDNA ISA guide v_rsq_f32 at
    1 ulp.  The larger published figure is used.

Row statistics (C columns, mu = mean, d_i = x_i - mu, q = sum d_i^2, D = q / C + eps, r = D^-1/2, shift = -mu r)
  mean:  m^ = fl(s^ / C), C - 1 additions and a division:  dm = |m^ - mu| <= gamma(C) sum|x_i| / C;  an exact sum leaves the
    correctly rounded quotient, dm = |fl(mu) - mu| (0 when mu is an f32 number).
  centred squares:  d^_i = fl(x_i - m^) = (x_i - m^)(1 + delta), and sum (x_i - m^)^2 = q + C (mu - m^)^2 EXACTLY (the cross
    term sums to zero), so the terms of q^ add up to at most (q + C dm^2)(1 + u)^2 before they are squared, rounded and summed:
    |q^ / C - q / C| <= dm^2 + gamma(C + 3)(q / C + dm^2)   (subtraction counted twice because it is squared, the square or
    fma, C - 1 additions; 0 when the sum is exact, dm = 0 and every d_i and d_i^2 is an f32 number)
  D^ = fl(fl(q^ / C) + eps):  dD = dq + gamma(2)(q / C + dq + eps).   D^ >= eps always (q^ >= 0 and rounding is monotonic).
  rstd:  r^ = rsqrtf(D^) lies between (D + dD)^-1/2 and max(D - dD, eps)^-1/2, each widened by 2 EPS32:
    br = max(r - (D + dD)^-1/2, max(D - dD, eps)^-1/2 - r) + 2 EPS32 max(D - dD, eps)^-1/2.  No linearisation: for a
    near-constant row with a large mean dm^2 can exceed D, and the bound says so.
  shift: fl(-m^ r^):  bs = dm (r + br) + |mu| br + u (|mu| + dm)(r + br).

LayerNorm  y = (x - mu) r gamma + beta = n gamma + beta
  fl(x_i - m^) = d_i + e_i, |e_i| <= dm + u (|d_i| + dm);  times r^:  bn = |e_i| (r + br) + |d_i| br;  then three roundings
  (times r^, times gamma, plus beta; an fma only removes one):
    B32 = |gamma| bn + gamma(3)(|n gamma| + |gamma| bn) + u |beta|;   bf16: B = B32 + 2^-8 (|want| + B32).
  + residual: ``round_to<T>(o) + r`` and then the store -- in bf16 TWO roundings to bf16 with an f32 addition between them:
    E1 = B32 + 2^-8 (|o| + B32);  E = E1 + u (|o + r| + E1);  B = E + 2^-8 (|o + r| + E).   f32: B = B32 + u (|o + r| + B32).
  A result that adds the residual BEFORE the first rounding (one rounding instead of two) is closer to the truth than the
  contract, so no accuracy bound can reject it: that mutant is provably invisible here, and test_row_kernels_ref_cpu.py
  asserts exactly that instead of pretending otherwise.  (tests/test_gpu_parity.py::test_layer_norm pins the contract bit for
  bit against the two separate operations.)

LayerNorm backward, from x, dy, gamma and the f32 statistics (s, t) = (rstd, shift) it is handed (operands):
  xh = x s + t,  g = dy gamma,  sg = mean_c g,  sgx = mean_c g xh,  dx = s (g - sg - xh sgx) (+ dres),
  d gamma = sum_r dy xh,  d beta = sum_r dy.
  xh^ = fl(fl(x s) + t):  Exh = u |x s| + u |xh|.  THE FIRST TERM IS THE CANCELLATION: the statistics carry -mean rstd, so a row
    whose |mean| rstd is large loses u |x| rstd of every xh (1e-3 for mean / spread = 1e4).  The format of the statistics makes
    it unavoidable; it is part of the bound, in the open.
  sg^:   product, C - 1 additions, times fl(1 / C):            Esg  = gamma(C + 2) sum_c |g| / C
  sgx^:  the same with the fma:   Esgx = [sum_c |g| Exh + gamma(C + 3) sum_c |g| (|xh| + Exh)] / C
  inner = g - sg - xh sgx:  A = |g| + |sg| + Esg + (|xh| + Exh)(|sgx| + Esgx) bounds every intermediate, four roundings (g,
    the product, two subtractions):  Ein = Esg + Exh (|sgx| + Esgx) + |xh| Esgx + gamma(4) A
  dx:  B32 = s Ein + u (|s inner| + s Ein) [+ u (|want| + that) for dres];  bf16 store as above.
  d gamma:  sum over R rows of fma(dy, xh, .): sum_r |dy| Exh + gamma(R + 1) sum_r |dy| (|xh| + Exh);  d beta: gamma(R - 1) sum_r |dy|.

col_sum: gamma(R - 1) sum_r |x|.   row_dot: sum_c a (b - shift), the subtraction, the fma, C - 1 more additions:
gamma(C + 1) sum_c |a| |b - shift|.   row_scale: fl(alpha s) then the product: gamma(2) |want| (+ store).   add: u |want|
(+ store).   convert_pad: exact except f32 -> bf16 (2^-8 |want|); the padding is exactly zero.
"""

from __future__ import annotations

import types

import torch

from _gnn_ops_ref import BF16_STORE, EPS32

U = EPS32 / 2.0
RSQRT_REL = 2.0 * EPS32
EPS = 1e-5
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = (F32, BF16)


def vec(dtype) -> int:
    return 4 if dtype == F32 else 8


def name(dtype) -> str:
    return "f32" if dtype == F32 else "bf16"


def gamma(n):
    n = torch.as_tensor(n, dtype=torch.float64).clamp_min(0.0)
    return n * U / (1.0 - n * U)


def eps32(eps: float) -> float:
    return float(torch.tensor(eps, dtype=F32))


def _store(want, b32, dtype):
    return b32 + BF16_STORE * (want.abs() + b32) if dtype == BF16 else b32


def _is_f32(t: torch.Tensor) -> torch.Tensor:
    return t.float().double() == t


def _exactly_summable(t: torch.Tensor) -> torch.Tensor:
    """Per row of ``t`` [R, n] (f64): every term a multiple of one 2^k and sum|t| <= 2^24 2^k (see EXACT sums above)."""
    a = t.abs()
    m, e = torch.frexp(a)  # a = m 2^e, m in [0.5, 1): 53 significant bits
    mi = (m * 2.0 ** 53).to(torch.int64)
    low = (mi & -mi).double()  # the lowest set bit
    lsb = torch.where(a == 0, torch.full_like(a, 4096.0), e.double() - 53.0 + torch.log2(low.clamp_min(1.0)))
    k = lsb.min(dim=1).values
    zero = (a == 0).all(dim=1)
    units = a.sum(dim=1) * torch.exp2(-k.clamp(-1000.0, 1000.0))
    return zero | ((k < 4096.0) & (k > -126.0) & (units <= 2.0 ** 24) & _is_f32(t).all(dim=1))


# ------------------------------------------------------------------------------------------------ row statistics
def row_analysis(x: torch.Tensor, eps: float = EPS):
    """Everything the statistics and the LayerNorm bounds share; fields are [R] or [R, C] f64."""
    x64 = x.double()
    c = x64.shape[1]
    e32 = eps32(eps)
    mu = x64.mean(dim=1)
    exact_s = _exactly_summable(x64)
    dm = torch.where(exact_s, (mu.float().double() - mu).abs(), gamma(c) * x64.abs().sum(dim=1) / c)
    d = x64 - mu[:, None]
    qc = (d * d).mean(dim=1)
    exact_q = exact_s & (dm == 0) & _is_f32(d).all(dim=1) & _exactly_summable(d * d)
    dq = torch.where(exact_q, torch.zeros_like(qc), dm * dm + gamma(c + 3) * (qc + dm * dm))
    big_d = qc + e32
    dd = dq + gamma(2) * (qc + dq + e32)
    r = big_d.rsqrt()
    r_hi = torch.clamp(big_d - dd, min=e32).rsqrt()
    br = torch.maximum(r - (big_d + dd).rsqrt(), r_hi - r) + RSQRT_REL * r_hi
    return types.SimpleNamespace(x=x64, c=c, mu=mu, dm=dm, d=d, r=r, br=br)


def row_stats_ref(x: torch.Tensor, eps: float = EPS):
    """(want, bound) [R, 2] of ``(rstd, -mean rstd)``."""
    a = row_analysis(x, eps)
    bs = a.dm * (a.r + a.br) + a.mu.abs() * a.br + U * (a.mu.abs() + a.dm) * (a.r + a.br)
    return torch.stack([a.r, -a.mu * a.r], dim=1), torch.stack([a.br, bs], dim=1)


def layer_norm_ref(x, weight, bias, eps: float = EPS, residual=None):
    """(want, bound) [R, C] of ``LayerNorm(x) (+ residual)`` stored in x's dtype (weight, bias: f32)."""
    a = row_analysis(x, eps)
    g, b = weight.double()[None, :], bias.double()[None, :]
    e = a.dm[:, None] + U * (a.d.abs() + a.dm[:, None])
    r, br = a.r[:, None], a.br[:, None]
    n = a.d * r
    bn = e * (r + br) + a.d.abs() * br
    o = n * g + b
    b32 = g.abs() * bn + gamma(3) * ((n * g).abs() + g.abs() * bn) + U * b.abs()
    if residual is None:
        return o, _store(o, b32, x.dtype)
    want = o + residual.double()
    if x.dtype == BF16:
        e1 = b32 + BF16_STORE * (o.abs() + b32)
        err = e1 + U * (want.abs() + e1)
        return want, err + BF16_STORE * (want.abs() + err)
    return want, b32 + U * (want.abs() + b32)


# ------------------------------------------------------------------------------------------------ LayerNorm backward
def exact_stats(x: torch.Tensor, eps: float = EPS) -> torch.Tensor:
    """The f64 statistics (for the autograd validation; the kernels and their stand-ins are handed f32 ones)."""
    return row_stats_ref(x, eps)[0]


def layer_norm_backward_ref(x, stats, weight, dy, dres=None):
    """((dx, bound), (d gamma, bound), (d beta, bound)) from the statistics as handed over (``stats`` [R, 2] f32 or f64)."""
    x64, d64, g64 = x.double(), dy.double(), weight.double()[None, :]
    rows, c = x64.shape
    s, t = stats.double()[:, :1], stats.double()[:, 1:]
    xh = x64 * s + t
    exh = U * (x64 * s).abs() + U * xh.abs()
    g = d64 * g64
    sg = g.mean(dim=1, keepdim=True)
    sgx = (g * xh).mean(dim=1, keepdim=True)
    esg = gamma(c + 2) * g.abs().mean(dim=1, keepdim=True)
    esgx = ((g.abs() * exh).sum(dim=1, keepdim=True) + gamma(c + 3) * (g.abs() * (xh.abs() + exh)).sum(dim=1, keepdim=True)) / c
    mag = g.abs() + sg.abs() + esg + (xh.abs() + exh) * (sgx.abs() + esgx)
    ein = esg + exh * (sgx.abs() + esgx) + xh.abs() * esgx + gamma(4) * mag
    ln = s * (g - sg - xh * sgx)
    b32 = s.abs() * ein + U * (ln.abs() + s.abs() * ein)
    want = ln
    if dres is not None:
        want = ln + dres.double()
        b32 = b32 + U * (want.abs() + b32)
    dgamma = (d64 * xh).sum(dim=0)
    bg = (d64.abs() * exh).sum(dim=0) + gamma(rows + 1) * (d64.abs() * (xh.abs() + exh)).sum(dim=0)
    dbeta = d64.sum(dim=0)
    bb = gamma(rows - 1) * d64.abs().sum(dim=0)
    return (want, _store(want, b32, x.dtype)), (dgamma, bg), (dbeta, bb)


# ------------------------------------------------------------------------------------------------ the small kernels
def col_sum_ref(x):
    x64 = x.double()
    return x64.sum(dim=0), gamma(x64.shape[0] - 1) * x64.abs().sum(dim=0)


def row_dot_ref(a, b, shift=None):
    b64 = b.double() if shift is None else b.double() - shift.double()[None, : b.shape[1]]
    terms = a.double() * b64
    return terms.sum(dim=1), gamma(a.shape[1] + 1) * terms.abs().sum(dim=1)


def row_scale_ref(x, s, alpha: float):
    want = float(alpha) * s.double()[:, None] * x.double()
    return want, _store(want, gamma(2) * want.abs(), x.dtype)


def add_ref(a, b):
    want = a.double() + b.double()
    return want, _store(want, U * want.abs(), a.dtype)


def convert_pad_ref(src, dtype, ld_out: int):
    want = torch.zeros((src.shape[0], ld_out), dtype=torch.float64)
    want[:, : src.shape[1]] = src.double()
    lossy = src.dtype == F32 and dtype == BF16
    return want, (BF16_STORE * want.abs() if lossy else torch.zeros_like(want))


# ------------------------------------------------------------------------------------------------ checker
def _where(idx, shape) -> str:
    if len(shape) == 2:
        return f"row {idx[0]}, column {idx[1]}"
    return f"element {idx[0]}" if len(shape) == 1 else f"index {idx}"


def check(got: torch.Tensor, want: torch.Tensor, bound: torch.Tensor, what: str) -> float:
    """Every element of ``got`` finite and within ``bound`` of ``want``.  Returns the largest fraction of a bound that was
    used (0 / 0 = 0: where the bound is zero the element must be exact).  A failure names the worst element's row and column."""
    got = got.detach().cpu()
    assert got.shape == want.shape == bound.shape, f"{what}: shape {tuple(got.shape)}, expected {tuple(want.shape)}"
    if got.numel() == 0:
        return 0.0
    g = got.double()
    finite = torch.isfinite(g)
    if not bool(finite.all()):
        idx = tuple(int(i) for i in torch.nonzero(~finite)[0])
        raise AssertionError(f"{what}: {int((~finite).sum())} non-finite elements, first at {_where(idx, got.shape)}: got "
                             f"{float(g[idx])}, want {float(want[idx]):.9g}")
    diff = (g - want).abs()
    bad = ~(diff <= bound)
    ratio = torch.where(diff == 0, torch.zeros_like(diff), diff / bound)
    worst = float(ratio.max())
    if bool(bad.any()):
        flat = int(torch.argmax(torch.where(bad, ratio, torch.full_like(ratio, -1.0))))
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), got.shape))
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements outside their bound; worst at "
                             f"{_where(idx, got.shape)}: got {float(g[idx]):.9g}, want {float(want[idx]):.9g}, |diff| "
                             f"{float(diff[idx]):.3e} > bound {float(bound[idx]):.3e} (worst ratio {worst:.3g})")
    return worst


# ------------------------------------------------------------------------------------------------ data sets
# Row r of every LayerNorm / backward matrix is of kind ROW_KINDS[r % 9]: one matrix of >= 9 rows runs every data set at its
# width (and fills two full blocks of four waves plus a third with one wave).
ROW_KINDS = ("ordinary", "mean_1e3", "mean_1e4", "constant", "sqrt_eps", "zeros", "huge", "exact", "ordinary")
ALL_KINDS_ROWS = len(ROW_KINDS)
CONSTANT = 0.75  # k * 0.75 is an f32 (and bf16) number for every k <= 2^22: the sum, the mean and d = 0 are exact


def make_rows(rows: int, c: int, dtype, seed: int = 0) -> torch.Tensor:
    """[rows, c] in ``dtype``; see ROW_KINDS.  "ordinary": randn * 2 + 0.5; "mean_1e3" / "mean_1e4": unit spread around 1e3 /
    1e4; "constant": 0.75; "sqrt_eps": spread sqrt(eps) around 0.5, eps is half of the denominator; "zeros"; "huge": 1e18 (1 +
    0.01 randn), its squares overflow f32 unless centred first; "exact": +-k/4, |k| <= 8, in cancelling pairs."""
    g = torch.Generator().manual_seed(9000 + seed + 31 * c + rows)
    z = torch.randn(rows, c, generator=g, dtype=torch.float64)
    k = torch.randint(-8, 9, (rows, c), generator=g).double() / 4.0
    k[:, 1::2] = -k[:, 0:c - (c % 2):2]
    if c % 2:
        k[:, -1] = 0.0
    # (bf16 keeps 8 bits: a spread below one quantum, mean 2^-7, would store a constant row; it gets the narrowest spread the
    #  format can hold, 4 at 1e3 and 64 at 1e4)
    q3, q4 = (1.0, 1.0) if dtype == F32 else (4.0, 64.0)
    forms = {"ordinary": z * 2.0 + 0.5, "mean_1e3": 1e3 + q3 * z, "mean_1e4": 1e4 + q4 * z, "constant": torch.full_like(z, CONSTANT),
             "sqrt_eps": 0.5 + EPS ** 0.5 * z, "zeros": torch.zeros_like(z), "huge": 1e18 * (1.0 + 0.01 * z), "exact": k}
    x = torch.empty_like(z)
    for i, kind in enumerate(ROW_KINDS):
        x[i::ALL_KINDS_ROWS] = forms[kind][i::ALL_KINDS_ROWS]
    return x.to(dtype)


def rows_of(kind: str, rows: int):
    return [r for r in range(rows) if ROW_KINDS[r % ALL_KINDS_ROWS] == kind]


def affine(c: int, seed: int = 0):
    """(gamma, beta) f32 [c]."""
    g = torch.Generator().manual_seed(500 + seed + c)
    return (1.0 + 0.5 * torch.randn(c, generator=g)).float(), torch.randn(c, generator=g).float()


def plain(rows: int, cols: int, dtype, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(100 + seed + 7 * cols + rows)
    return (torch.randn(rows, cols, generator=g, dtype=torch.float64) * 2.0 + 0.5).to(dtype)


def col_data(rows: int, cols: int, dtype) -> torch.Tensor:
    """Columns of mean +-2 and spread 0.5: a chunk of 16 rows sums to about +-32, which stands out of the gamma(R - 1) sum|x| =
    8 that 8192 rows are allowed (a chunk of zero-mean data would not)."""
    g = torch.Generator().manual_seed(300 + 7 * cols + rows)
    sign = 1.0 - 2.0 * (torch.arange(cols) % 2).double()
    return ((torch.randn(rows, cols, generator=g, dtype=torch.float64) * 0.5 + 2.0) * sign).to(dtype)


def backward_rows_per_wg(rows: int) -> int:
    """csrc/backward.hip::layer_norm_backward_launch."""
    return max(32, (rows + 1023) // 1024)


def boundary_rows(rows: int):
    """The last row of the first, the middle and the last workgroup's row range (the rows a short range would lose)."""
    per = backward_rows_per_wg(rows)
    wgs = -(-rows // per)
    return sorted({min(rows, (w + 1) * per) - 1 for w in (0, wgs // 2, wgs - 1)})


def make_dy(rows: int, c: int, dtype, seed: int = 0) -> torch.Tensor:
    """Unit normal; past 1024 rows the boundary rows are 2^10 times larger (exact in both dtypes), so that ONE missing row
    stands out of the gamma(R + 1) sum|dy xh| that R rows are allowed."""
    g = torch.Generator().manual_seed(7000 + seed + 13 * c + rows)
    dy = torch.randn(rows, c, generator=g, dtype=torch.float64)
    if rows > 1024:
        dy[boundary_rows(rows)] *= 1024.0
    return dy.to(dtype)


# ------------------------------------------------------------------------------------------------ shapes (both test files)
def layer_norm_widths(dtype):
    """(C, ITEMS or 0 for the generic kernel, partial last pass?) -- contiguous operands."""
    v = vec(dtype)
    out = [(64 * v * i, i, False) for i in range(1, 9)]
    out += [(64 * v * (i - 1) + v, i, True) for i in range(1, 9)]
    out += [(64 * v * 8 + v, 0, True), (1, 0, True), (v + 1, 0, True), (191, 0, True)]
    return out


def backward_widths(dtype):
    """(C, NC of the kernel form; 0 = the LDS form, wide or unaligned)."""
    v = vec(dtype)
    return [(8, 8), (512, 8), (520, 16), (1024, 16), (1032, 32), (2048, 32), (2048 + v, 0), (5120, 0), (191, 0)]


BACKWARD_MAX_C = 5120  # 8 C floats of LDS = 160 KiB
BACKWARD_ROWS = (1, 3, 32, 33, 65)
BACKWARD_NPART = (1, 15, 16, 17, 48, 49, 63, 64, 65, 113)  # workgroups of 32 rows -> n_part of col_sum_final_kernel
BACKWARD_MANY_ROWS = 32 * 1024 + 5  # rows_per_wg = 33, 994 workgroups, the last one holds 4 rows
COL_SUM_ROWS = (1, 16, 17, 19, 8192, 8193)
COL_SUM_COLS = (1, 255, 256, 257)


def col_sum_chunks(rows: int):
    """(chunk, blocks) of csrc/backward.hip::col_sum_launch."""
    chunk = max(16, (rows + 511) // 512)
    return chunk, -(-rows // chunk)


def row_widths(dtype):
    v = vec(dtype)
    return [(v, True), (64 * v * 4, True), (64 * v * 4 + v, True), (191, False)]
