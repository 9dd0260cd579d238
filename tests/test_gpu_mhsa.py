"""GPU tests of multi-head self attention (csrc/attention.hip behind ``ops.mhsa``, ``ops.mhsa_backward``, ``autograd.mhsa``)
against the f64 references of tests/_mhsa_ref.py: ``out``, ``lse``, ``dq``, ``dk`` and ``dv`` per element, every element
finite and inside a bound derived from the data (``_mhsa_ref``: the derivations).  tests/test_mhsa_ref_cpu.py shows that
emulations of the kernels' arithmetic stay inside these bounds at every shape of this file and that a dropped or doubled key,
an off-by-one window, an admitted pad key, a repeated last key, a missing scale, an lse in the wrong units, a foreign dropout
mask, a missing delta, a missing (query, key) pair and swapped heads do not.

Kernels: ``mhsa_bf16_w4_kernel`` (D = 64, global), ``mhsa_bf16_kernel`` <64 / 32> (windows, D = 32, the four-wave kernel's
fallback), ``mhsa_tail_kernel`` + ``mhsa_tail_merge_kernel`` (S = 513, 514, 528, 1026), ``mhsa_generic_kernel`` <f32 / bf16, DMAX
32 / 64 / 128>, ``mhsa_delta_kernel``, ``mhsa_bwd_dkv_mfma_kernel`` / ``mhsa_bwd_dq_mfma_kernel`` <64 / 32, DROP, WIN>,
``mhsa_bwd_dq_kernel`` / ``mhsa_bwd_dkv_kernel``, ``transpose_v_kernel``.  Every case restates the launcher's dispatch on its own
tensors (``_mhsa_ref.route``), asserts the kernel it reaches, and asserts that the library's own plan for the call's pointers
and pitches (``anemoi_mhsa_route``) equals the restatement: kernel, DROP / WIN, DMAX, tail rows / splits / chunk, workgroups,
workspace size.  ``qkv``, ``out`` (backward: ``out``, ``dout``) sit in buffers with guard rows before and after and guard columns
where the pitch is wider than the data: NaN around the inputs, a bit pattern around the output that must be untouched.

Measured on an MI355X: the largest fraction of its bound that any element used, over all cases of this file (the module
prints the table again at its end, split further by tail rows and dropout):
                                        out      lse
    four-wave forward  (D = 64)         0.471    0.841   (gap rows 0.397 / 0.940; with dropout 0.434 / 0.819)
    eight-wave forward (D = 64)         0.519    0.311   (windows; with dropout 0.397 / 0.044)
    eight-wave forward (D = 32)         0.601    0.375
    ... + key-split tail rows           0.453    0.827   (S = 513, 514, 528, 1026)
    generic forward, f32                0.207    0.646   (of 4 x torch's own f32 fraction of the derived bound)
    generic forward, bf16 storage       0.993    0.599   (out: the bf16 store alone)
                                        dq       dk       dv
    MFMA backward alone (D = 64)        0.635    0.783    0.738   (operands: the rounded reference out and lse)
    MFMA backward alone (D = 32)        0.756    0.753    0.723   (with dropout at most 0.573 / 0.713 / 0.827)
    MFMA backward via autograd          0.186    0.232    0.706   (bounds widened by the forward's own bounds)
    generic backward, f32               0.211    0.127    0.279
    generic backward, bf16 storage      0.806    0.824    0.992
The fixed-maximum rows of the four-wave kernel reach 0.84 -- 0.94 of the lse bound: a probability far from a power of two
loses up to 2^-8 when it is rounded to bf16, which an online maximum hides (its largest probability is exactly 1).  That is
the rounding unit the bound is derived from; a first draft with 2^-9 was refuted by the CPU emulation before any GPU run.
No guard band was written, every repeat of an MFMA call was bit-identical, ``autograd.mhsa`` equalled ``ops.mhsa`` bit for bit.

What the ``gap`` cases showed.  g = 40, 100 (inside the fixed maximum's range) and 123, 126, 140 (row sum >= 1e37: flag,
fallback to the eight-wave kernel) passed on the library as it was.  g = 121 -- rows 120.0 ... 122.5 log2 units above their
first block's maximum, |v| = 100 in the far key -- FAILED at both sizes: from 121.4 on the stored rows were +-inf (5888 of
25 600 elements at S = 200, 20 608 at S = 700) with the flag clear, because the row sum stays below 1e37 while sum x |v|
leaves the f32 range.  Kernel change: the four-wave kernel's epilogue raises the fallback flag also when an accumulator of
a stored row is inf or NaN.  Afterwards all twelve gap cases pass (0.32 / 0.16 of the bounds at g = 121), register
allocation and the tile loop's instructions are unchanged, and 24 ordinary cases (six sizes x two data sets, gap 40 / 100 / 126 /
140 at both sizes, dropout) were bit-identical, forward, lse and backward, between the library before and after.
"""

import pytest
import torch

import _mhsa_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = R.F32, R.BF16
_WORST = {}
_INT = {F32: (torch.int32, 0x5A5A5A5A), BF16: (torch.int16, 0x5A5A)}


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
    """A ``[rows, cols]`` view of pitch ``cols + pad`` inside a larger buffer: two guard rows (a multiple of 64 elements, so
    the view keeps the buffer's 16-byte alignment) before and after, ``pad`` guard columns.  ``data`` given (inputs): the guards
    are NaN, a read outside the operand poisons the result.  Otherwise (outputs) the buffer holds a bit pattern and
    ``assert_clean`` demands that every element outside the view still does."""

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
        idx = margin + torch.arange(rows, device=DEV)[:, None] * ld + torch.arange(cols, device=DEV)[None, :]
        self.outside = torch.ones(n, dtype=torch.bool, device=DEV)
        self.outside[idx.reshape(-1)] = False
        self.ld = ld
        if data is not None:
            self.view.copy_(data)
            assert bool(torch.isnan(flat[self.outside]).all())
        assert self.view.data_ptr() % 16 == 0

    def assert_clean(self, what):
        touched = self.outside & (self.raw != self.pattern)
        assert not bool(touched.any()), f"{what}: {int(touched.sum())} elements outside the result were written, first at " \
                                        f"buffer offset {int(torch.nonzero(touched)[0])}"


def _keep(c, seed=R.DROPOUT_SEED, h0=0, ht=0):
    return R.keep_mask(seed, c.p, c.b, c.h, c.s, h0, ht) if c.p > 0.0 else None


def _forward(c, qkv, p=0.0, seed=0, expect=None):
    """``ops.mhsa`` on guarded buffers; asserts the route, the workspace geometry and the guards.  (out, lse) on the CPU."""
    from anemoi_models_amd import _lib, ops

    rows, cc = c.b * c.s, c.h * c.d
    gin = Guarded(rows, 3 * cc, c.dtype, c.pad, data=qkv.to(DEV))
    gout = Guarded(rows, cc, c.dtype, c.opad)
    rt = R.route(c.dtype, c.b, c.s, c.h, c.d, c.window, gin.ld, gout.ld, gin.view.data_ptr(), gout.view.data_ptr(), p)
    assert rt.kernel == (expect or c.expect), f"{R.case_id(c)}: the launcher takes {rt.kernel}"
    assert _lib.load().anemoi_mhsa_workspace_bytes(ops.dtype_code(c.dtype), c.b, c.s, c.h, c.d) == \
        R.workspace_bytes(c.dtype, c.b, c.s, c.h, c.d)
    # the library's own plan on the pointers and pitches of this call (ops.mhsa brings a workspace wherever one is asked for)
    st, plan = _lib.mhsa_route("forward", dtype=ops.dtype_code(c.dtype), qkv=gin.view.data_ptr(), ld=gin.ld, out=gout.view.data_ptr(),
                               ldo=gout.ld, workspace=256, B=c.b, S=c.s, H=c.h, D=c.d, window=c.window, dropout_p=p,
                               dropout_seed=seed)
    R.assert_same_plan(rt, st, plan, R.case_id(c))
    out, lse = ops.mhsa(gin.view, c.b, c.h, c.window, out=gout.view, return_lse=True, dropout_p=p, dropout_seed=seed)
    assert out.data_ptr() == gout.view.data_ptr() and lse.shape == (c.b, c.h, c.s) and lse.dtype == F32
    torch.cuda.synchronize()
    gout.assert_clean(R.case_id(c))
    return out.cpu().clone(), lse.cpu().clone(), rt


def _check_forward(c, ref, out, lse, tag):
    kind = R.case_kind(c)
    bo, bl = R.forward_bounds(ref, kind, c.dtype)
    f_out = _note(f"forward {tag} out", R.check(out, ref.out, bo, f"{R.case_id(c)} out"))
    f_lse = _note(f"forward {tag} lse", R.check(lse, ref.lse, bl, f"{R.case_id(c)} lse"))
    print(f"{R.case_id(c)}: out {f_out:.3f}, lse {f_lse:.3f} of the bound")
    return bo, bl


def _tag(c, rt=None):
    if c.expect == "generic" or (rt is not None and not rt.mfma):
        return f"generic {R.name(c.dtype)}"
    return f"{c.expect} D={c.d}" + (" gap" if c.data == "gap" else "") + (" +tail" if R.tail_rows(c.s) else "")


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("c", R.forward_mfma_cases() + R.forward_generic_cases(), ids=R.case_id)
def test_forward_and_lse(c):
    qkv = R.case_qkv(c)
    out, lse, rt = _forward(c, qkv)
    ref = R.forward_ref(qkv, c.b, c.h, c.window)
    if c.data == "gap":
        _, gaps = R.gap_rows(qkv, c.h, c.s, c.g_log2)
        print(f"{R.case_id(c)}: far key {float(gaps.min()):.2f} ... {float(gaps.max()):.2f} log2 units above the first block")
    _check_forward(c, ref, out, lse, _tag(c, rt))
    if rt.mfma:
        out2, lse2, _ = _forward(c, qkv)
        assert torch.equal(out2, out) and torch.equal(lse2, lse), "a repeat of the call differs"


def test_head_size_129_is_refused():
    from anemoi_models_amd import ops

    qkv = torch.zeros(4, 3 * 129, device=DEV)
    with pytest.raises(NotImplementedError, match="head size 129 > 128"):
        ops.mhsa(qkv, 1, 1)
    with pytest.raises(NotImplementedError, match="head size 129 > 128"):
        ops.mhsa_backward(qkv, torch.zeros(4, 129, device=DEV), torch.zeros(4, 129, device=DEV), torch.zeros(1, 1, 4, device=DEV), 1, 1)


# ------------------------------------------------------------------------------------------------ backward
def _backward_direct(c, qkv, out_st, dout, lse_st, p=0.0, seed=0):
    """``ops.mhsa_backward`` on guarded operands; asserts the route."""
    from anemoi_models_amd import _lib, ops

    rows, cc = c.b * c.s, c.h * c.d
    gq = Guarded(rows, 3 * cc, c.dtype, data=qkv.to(DEV))
    go = Guarded(rows, cc, c.dtype, data=out_st.to(DEV))
    gd = Guarded(rows, cc, c.dtype, data=dout.to(DEV))
    lse_dev = lse_st.to(DEV)
    use_mfma = R.backward_expect(c) == "mfma"
    rt = R.route_backward(c.dtype, c.b, c.s, c.h, c.d, c.window, gq.ld, go.ld, gd.ld, 3 * cc,
                          (gq.view.data_ptr(), go.view.data_ptr(), gd.view.data_ptr(), 0), p, workspace=use_mfma)
    assert rt.kernel == R.backward_expect(c) and rt.win == (rt.mfma and c.window >= 0)
    # the library's own plan on the operands of this call; dqkv, delta and the workspace are ops.mhsa_backward's own fresh
    # allocations (256-byte aligned), the workspace withheld where the case asks for the VALU kernels
    st, plan = _lib.mhsa_route("backward", dtype=ops.dtype_code(c.dtype), qkv=gq.view.data_ptr(), ld=gq.ld, out=go.view.data_ptr(),
                               ldo=go.ld, dout=gd.view.data_ptr(), lddo=gd.ld, lse=lse_dev.data_ptr(), delta=256, dqkv=256,
                               lddq=3 * cc, workspace=256 if use_mfma else 0, B=c.b, S=c.s, H=c.h, D=c.d, window=c.window,
                               dropout_p=p, dropout_seed=seed)
    R.assert_same_plan(rt, st, plan, R.case_id(c))
    dqkv = ops.mhsa_backward(gq.view, go.view, gd.view, lse_dev, c.b, c.h, c.window, p, seed, use_mfma=use_mfma)
    assert dqkv.data_ptr() % 8 == 0
    return dqkv.cpu(), rt


def _check_backward(c, ref, bw, dqkv, kind, out_err, lse_err, tag, what):
    cc = c.h * c.d
    bounds = R.backward_bounds(ref, bw, kind, c.dtype, out_err, lse_err)
    fr = []
    for i, (name, want) in enumerate((("dq", bw.dq), ("dk", bw.dk), ("dv", bw.dv))):
        fr.append(_note(f"backward {tag} {name}", R.check(dqkv[:, i * cc:(i + 1) * cc], want, bounds[i], f"{R.case_id(c)} {what} {name}")))
    print(f"{R.case_id(c)} {what}: dq {fr[0]:.3f}, dk {fr[1]:.3f}, dv {fr[2]:.3f} of the bound")


def _backward_both(c, qkv, ref, keep_seed=0):
    """The backward kernels alone (operands: the rounded reference out and lse, bounds from their actual deviations) and
    through ``autograd.mhsa`` (operands: the forward kernel's own results, bounds from the forward bounds)."""
    from anemoi_models_amd import autograd, ops

    dout = R.make_dout(c.dtype, c.b, c.s, c.h, c.d)
    bw = R.backward_ref(ref, dout)
    kind = "mfma" if R.backward_expect(c) == "mfma" else "f32"
    out_st, lse_st = ref.out.to(c.dtype), ref.lse.float()
    dqkv, rt = _backward_direct(c, qkv, out_st, dout, lse_st, c.p, keep_seed)
    tag = ("mfma D=%d" % c.d if rt.mfma else f"generic {R.name(c.dtype)}") + (" dropout" if c.p else "")
    _check_backward(c, ref, bw, dqkv, kind, (out_st.double() - ref.out).abs(), (lse_st.double() - ref.lse).abs(), tag, "backward alone")
    if rt.mfma:
        again, _ = _backward_direct(c, qkv, out_st, dout, lse_st, c.p, keep_seed)
        assert torch.equal(again, dqkv), "a repeat of the backward differs"
    # autograd: forward + backward as training runs them (workspace always offered: bf16 D = 64 / 32 take the MFMA kernels)
    cc = c.h * c.d
    x = qkv.to(DEV).requires_grad_()
    rt_f = R.route(c.dtype, c.b, c.s, c.h, c.d, c.window, 3 * cc, cc, x.data_ptr(), 0, c.p)
    rt_b = R.route_backward(c.dtype, c.b, c.s, c.h, c.d, c.window, 3 * cc, cc, cc, 3 * cc, (x.data_ptr(), 0, 0, 0), c.p)
    y = autograd.mhsa(x, c.b, c.h, c.window, c.p, keep_seed)
    plain = ops.mhsa(qkv.to(DEV), c.b, c.h, c.window, dropout_p=c.p, dropout_seed=keep_seed)
    assert torch.equal(y.detach(), plain), "autograd.mhsa forward differs from ops.mhsa"
    y.backward(dout.to(DEV))
    bo, bl = R.forward_bounds(ref, "mfma" if rt_f.mfma else "f32", c.dtype)
    R.check(y.detach(), ref.out, bo, f"{R.case_id(c)} autograd out")
    tag = ("mfma D=%d" % c.d if rt_b.mfma else f"generic {R.name(c.dtype)}") + (" dropout" if c.p else "") + " autograd"
    _check_backward(c, ref, bw, x.grad.cpu(), "mfma" if rt_b.mfma else "f32", bo, bl, tag, "autograd")


@pytest.mark.parametrize("c", R.backward_cases(), ids=R.case_id)
def test_backward(c):
    qkv = R.case_qkv(c)
    _backward_both(c, qkv, R.forward_ref(qkv, c.b, c.h, c.window))


# ------------------------------------------------------------------------------------------------ dropout
@pytest.mark.parametrize("c", R.dropout_cases(), ids=R.case_id)
def test_dropout_forward_and_backward(c):
    qkv = R.case_qkv(c)
    keep = _keep(c)
    assert abs(float(keep.mean()) - (1.0 - c.p)) < 0.02
    ref = R.forward_ref(qkv, c.b, c.h, c.window, keep, c.p)
    out, lse, rt = _forward(c, qkv, c.p, R.DROPOUT_SEED)
    assert rt.drop
    _check_forward(c, ref, out, lse, _tag(c, rt) + " dropout")
    if rt.mfma:
        out2, lse2, _ = _forward(c, qkv, c.p, R.DROPOUT_SEED)
        assert torch.equal(out2, out) and torch.equal(lse2, lse)
    other, _, _ = _forward(c, qkv, c.p, R.DROPOUT_SEED + 1)
    assert not torch.equal(other, out)
    _backward_both(c, qkv, ref, R.DROPOUT_SEED)


@pytest.mark.parametrize("c", [c for c in R.dropout_cases() if c.p == 0.5], ids=R.case_id)
def test_dropout_limits(c):
    """p = 1 drops everything (output and gradients exactly zero); a p whose 15-bit threshold rounds to 0 is no dropout, bit
    for bit."""
    from anemoi_models_amd import autograd, ops

    qkv = R.case_qkv(c).to(DEV)
    dout = R.make_dout(c.dtype, c.b, c.s, c.h, c.d).to(DEV)
    assert R.route(c.dtype, c.b, c.s, c.h, c.d, c.window, qkv.shape[1], dout.shape[1], p=1.0).kernel == "generic"
    x = qkv.clone().requires_grad_()
    y = autograd.mhsa(x, c.b, c.h, c.window, 1.0, 5)
    y.backward(dout)
    assert not bool(y.detach().any()) and not bool(x.grad.any())
    tiny = 1e-6
    assert R.threshold15(tiny) == 0 and not R.route(c.dtype, c.b, c.s, c.h, c.d, c.window, qkv.shape[1], dout.shape[1], p=tiny).drop
    o0, l0 = ops.mhsa(qkv, c.b, c.h, c.window, return_lse=True)
    o1, l1 = ops.mhsa(qkv, c.b, c.h, c.window, return_lse=True, dropout_p=tiny, dropout_seed=77)
    assert torch.equal(o0, o1) and torch.equal(l0, l1)
    g0 = ops.mhsa_backward(qkv, o0, dout, l0, c.b, c.h, c.window)
    g1 = ops.mhsa_backward(qkv, o0, dout, l0, c.b, c.h, c.window, tiny, 77)
    assert torch.equal(g0, g1)


@pytest.mark.parametrize("dtype,d,s,window,p", [(BF16, 64, 129, -1, 0.25), (BF16, 32, 129, 31, 0.5), (F32, 8, 65, -1, 0.25),
                                                (BF16, 64, 514, -1, 0.5)])
def test_head_shard_draws_the_mask_of_the_whole_attention(dtype, d, s, window, p):
    """Heads 2..3 of an H = 4 call, computed alone with ``head_offset=2, heads_total=4`` on their columns: forward, lse and
    backward equal the full call's columns bit for bit; without ``heads_total`` the mask is another one."""
    from anemoi_models_amd import ops

    b, h = 1, 4
    cc = h * d
    qkv = R.make_qkv("spread", dtype, b, s, h, d, window).to(DEV)
    dout = R.make_dout(dtype, b, s, h, d).to(DEV)
    seed = R.DROPOUT_SEED
    cols = slice(2 * d, 4 * d)
    part = torch.cat([qkv[:, t * cc:(t + 1) * cc][:, cols] for t in range(3)], dim=1).contiguous()
    assert R.route(dtype, b, s, h, d, window, 3 * cc, cc, p=p).kernel == R.route(dtype, b, s, 2, d, window, 6 * d, 2 * d, p=p, heads_total=4).kernel
    o_all, l_all = ops.mhsa(qkv, b, h, window, return_lse=True, dropout_p=p, dropout_seed=seed)
    o_part, l_part = ops.mhsa(part, b, 2, window, return_lse=True, dropout_p=p, dropout_seed=seed, head_offset=2, heads_total=4)
    assert torch.equal(o_part, o_all[:, cols]) and torch.equal(l_part, l_all[:, 2:4])
    g_all = ops.mhsa_backward(qkv, o_all, dout, l_all, b, h, window, p, seed)
    g_part = ops.mhsa_backward(part, o_part, dout[:, cols].contiguous(), l_part, b, 2, window, p, seed, head_offset=2, heads_total=4)
    for t in range(3):
        assert torch.equal(g_part[:, t * 2 * d:(t + 1) * 2 * d], g_all[:, t * cc:(t + 1) * cc][:, cols])
    o_wrong, l_wrong = ops.mhsa(part, b, 2, window, return_lse=True, dropout_p=p, dropout_seed=seed)
    assert not torch.equal(o_wrong, o_part) and torch.equal(l_wrong, l_part)  # (the normaliser sees every key: lse has no mask)
    g_wrong = ops.mhsa_backward(part, o_part, dout[:, cols].contiguous(), l_part, b, 2, window, p, seed)
    assert not torch.equal(g_wrong, g_part)
    # against the reference with the restated mask of heads 2..3 of 4
    keep = R.keep_mask(seed, p, b, 2, s, 2, 4)
    ref = R.forward_ref(part.cpu(), b, 2, window, keep, p)
    kind = "mfma" if dtype == BF16 and d in (32, 64) else "f32"
    bo, bl = R.forward_bounds(ref, kind, dtype)
    R.check(o_part, ref.out, bo, "head shard out")
    R.check(l_part, ref.lse, bl, "head shard lse")


# ------------------------------------------------------------------------------------------------ wrapper validation
def test_wrappers_refuse_operands_that_do_not_fit():
    """On device tensors: a bf16 ``dout`` next to an f32 ``qkv`` (which the library would read past its end), another shape,
    rows that are no whole number of sequences, columns that are not 3 x heads x head size -- ValueError before any launch."""
    from anemoi_models_amd import ops

    b, s, h, d = 2, 6, 2, 8
    cc = h * d
    qkv = torch.randn(b * s, 3 * cc, device=DEV)
    out, lse = ops.mhsa(qkv, b, h, return_lse=True)
    dout = torch.randn(b * s, cc, device=DEV)
    ops.mhsa_backward(qkv, out, dout, lse, b, h)
    for bad in (dict(batch_size=5), dict(num_heads=5), dict(qkv=qkv[:, :-1]), dict(out=torch.empty(b * s, cc + 1, device=DEV)),
                dict(out=torch.empty(b * s, cc, device=DEV, dtype=BF16))):
        args = dict(qkv=qkv, batch_size=b, num_heads=h)
        args.update(bad)
        with pytest.raises(ValueError):
            ops.mhsa(**args)
    for bad in (dict(batch_size=5), dict(num_heads=5), dict(qkv=qkv[:, :-1]), dict(dout=dout.bfloat16()), dict(out=out.bfloat16()),
                dict(dout=dout[:-1]), dict(out=torch.empty(b * s, 2 * cc, device=DEV)), dict(lse=lse.reshape(b, s, h)),
                dict(lse=lse.double()), dict(lse=lse[:, :1])):
        args = dict(qkv=qkv, out=out, dout=dout, lse=lse, batch_size=b, num_heads=h)
        args.update(bad)
        with pytest.raises(ValueError):
            ops.mhsa_backward(**args)
