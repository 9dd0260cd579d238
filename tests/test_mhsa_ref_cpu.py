"""CPU checks of tests/_mhsa_ref.py, the yardstick of tests/test_gpu_mhsa.py: the references are right, emulations of the
kernels' arithmetic stay inside the bounds at every shape and data set of the GPU file, and subtly wrong results do not.

Emulations (torch f32 / bf16, two or more orders each):
  * bf16 MFMA forward: key blocks ascending, probabilities rounded to bf16 in front of P V, the normaliser the sum of the
    rounded ones -- with an online maximum over 64-key tiles, and with the FIXED maximum of the first 32-key block (the
    four-wave kernel, global attention) with the launcher's fallback to the online kernel;
  * the key-split-and-merge of the tail pair (f32, exp / log), with 1, 3 and 7 chunks: also the generic kernel's arithmetic in
    three summation orders;
  * the backward with P and dS rounded to bf16 (32-query tiles accumulated / one product), and in plain f32.
Mutants (each computed in f64, rounded to the storage type, and REQUIRED to fail at every shape where it applies): any single
key dropped or counted twice (every designated key position: all keys under global attention), the window compared with <
on either side, a window one too wide (``intruder``), a zero-score pad key admitted (``cold``), the last key repeated for the
clamped positions behind a ragged S, the scale omitted, lse in log2 units, lse without the maximum, the backward's mask drawn
from another seed, delta omitted, one (query, key) pair missing from dk / dv, heads or batch elements swapped.

Cannot be rejected, and said so: a backward whose delta comes from the UNROUNDED out.  It is closer to the true gradient
than the contract (delta from the stored out), so no accuracy bound tells it from a correct kernel; the test asserts that it
passes.  (The zero-score pad key is invisible on ``pairs`` -- it weighs e^-8 next to the designated keys --, which is why
``cold`` exists; a window one too wide is invisible on ``pairs`` for the same reason, which is why ``intruder`` exists.)

The launcher's route: ``anemoi_mhsa_route`` runs the entry points' own validation and plan without a device; its answer is
compared field by field with the restatement (``_mhsa_ref.route`` / ``route_backward``) on every case of the case lists, on a
forward sweep of 359 919 and a backward sweep of 399 134 argument sets (about 11 s together), and on both sides of the
2^31 / 2^32 bounds that no allocation reaches.
"""

import math

import pytest
import torch

import _mhsa_ref as R

F32, BF16 = R.F32, R.BF16
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
_WORST = {}
_MUTANTS = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for key in sorted(_WORST):
        print(f"[emulation, worst fraction of the bound] {key}: {_WORST[key]:.3f}")
    for key in sorted(_MUTANTS):
        print(f"[mutant] {key}: rejected at {_MUTANTS[key]} shapes")


def _note(key, fraction):
    _WORST[key] = max(_WORST.get(key, 0.0), fraction)


def _rejected(key):
    _MUTANTS[key] = _MUTANTS.get(key, 0) + 1


def _kk(c):
    if c.p == 0.0:
        return None, None
    keep = R.keep_mask(R.DROPOUT_SEED, c.p, c.b, c.h, c.s)
    return keep, keep * (1.0 / (1.0 - c.p))


def _f32_heads(x, b, h):
    return R.heads(x, b, h).float()


# ------------------------------------------------------------------------------------------------ emulations
def emu_mfma_forward(qkv, b, h, window, kk, mode, block):
    """bf16 MFMA forward in f32 / bf16 torch; ``mode`` "online" or "fixed" (the first block's maximum for the whole pass)."""
    cc = qkv.shape[1] // 3
    q, k, v = (_f32_heads(t, b, h) for t in qkv.split(cc, dim=1))
    s, d = q.shape[2], q.shape[3]
    vis = R.visible(s, window)
    sl2 = (torch.tensor(1.0) / torch.sqrt(torch.tensor(float(d)))) * torch.tensor(LOG2E, dtype=F32)
    m = torch.full(q.shape[:3], float("-inf"))
    l = torch.zeros(q.shape[:3])
    o = torch.zeros_like(q)
    for j0 in range(0, s, block):
        sc = (q @ k[:, :, j0:j0 + block].transpose(-1, -2)).masked_fill(~vis[:, j0:j0 + block], float("-inf"))
        if mode == "online" or j0 == 0:
            new = torch.maximum(m, sc.amax(dim=-1) * sl2)
            corr = torch.where(new == float("-inf"), torch.ones_like(new), torch.exp2(m - new))
            l, o, m = l * corr, o * corr[..., None], new
        m_neg = torch.where(m == float("-inf"), torch.zeros_like(m), -m)
        pb = torch.exp2(sc * sl2 + m_neg[..., None]).bfloat16().float()
        l = l + pb.sum(dim=-1)
        if kk is not None:
            pb = pb * (kk[..., j0:j0 + block] > 0).float()
        o = o + pb @ v[:, :, j0:j0 + block]
    inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
    if kk is not None:
        inv = inv * float(kk.max())
    return R.rows_of((o * inv[..., None]).bfloat16()), (m + torch.log2(l)) * LN2, l, o


def emu_four_wave(qkv, b, h, flag_on_nonfinite_out):
    """The four-wave kernel with the launcher's fallback: the flag is raised by a row sum that is not below 1e37 and, with
    ``flag_on_nonfinite_out``, also by an accumulator that left the f32 range; a raised flag recomputes the call online."""
    out, lse, l, o = emu_mfma_forward(qkv, b, h, -1, None, "fixed", 32)
    redo = not bool((l < 1e37).all())
    if flag_on_nonfinite_out:
        redo = redo or not bool(torch.isfinite(o).all())
    if redo:
        out, lse, _, _ = emu_mfma_forward(qkv, b, h, -1, None, "online", 64)
    return out, lse, redo


def emu_split_forward(qkv, b, h, window, kk, n_split, dtype):
    """The tail pair / the generic kernel: f32, exp / log, ``n_split`` key chunks merged at the end."""
    cc = qkv.shape[1] // 3
    q, k, v = (_f32_heads(t, b, h) for t in qkv.split(cc, dim=1))
    s, d = q.shape[2], q.shape[3]
    vis = R.visible(s, window)
    qv = q * (torch.tensor(1.0) / torch.sqrt(torch.tensor(float(d))))
    chunk = -(-s // n_split)
    ms, ls, accs = [], [], []
    for j0 in range(0, s, chunk):
        sc = (qv @ k[:, :, j0:j0 + chunk].transpose(-1, -2)).masked_fill(~vis[:, j0:j0 + chunk], float("-inf"))
        mc = sc.amax(dim=-1)
        p = torch.exp(sc - torch.where(mc == float("-inf"), torch.zeros_like(mc), mc)[..., None])
        ls.append(p.sum(dim=-1))
        if kk is not None:
            p = p * kk[..., j0:j0 + chunk].float()
        ms.append(mc)
        accs.append(p @ v[:, :, j0:j0 + chunk])
    mt = torch.stack(ms).amax(dim=0)
    lt, acc = torch.zeros_like(mt), torch.zeros_like(q)
    for mc, lc, ac in zip(ms, ls, accs):
        w = torch.where(mc == float("-inf"), torch.zeros_like(mc), torch.exp(mc - mt))
        lt, acc = lt + lc * w, acc + ac * w[..., None]
    return R.rows_of((acc / lt[..., None]).to(dtype)), mt + torch.log(lt)


def emu_backward(qkv, out, lse, dout, b, h, window, kk, kind, tile, dtype):
    """The backward from the STORED out and lse: ``kind`` "mfma" rounds Pt and dS to bf16 (exp2 on log2-unit operands), "f32"
    does not; ``tile`` > 0 accumulates dk / dv over query tiles of that size."""
    cc = qkv.shape[1] // 3
    q, k, v = (_f32_heads(t, b, h) for t in qkv.split(cc, dim=1))
    do, o = _f32_heads(dout, b, h), _f32_heads(out, b, h)
    s, d = q.shape[2], q.shape[3]
    vis = R.visible(s, window)
    scale = torch.tensor(1.0) / torch.sqrt(torch.tensor(float(d)))
    delta = (do * o).sum(dim=-1)
    if kind == "mfma":
        prob = torch.exp2((q @ k.transpose(-1, -2)) * (scale * torch.tensor(LOG2E, dtype=F32)) - (lse * LOG2E)[..., None])
    else:
        prob = torch.exp((q * scale) @ k.transpose(-1, -2) - lse[..., None])
    prob = prob.masked_fill(~vis, 0.0)
    kf = torch.ones_like(prob) if kk is None else kk.float()
    pt, ds = prob * kf, prob * ((do @ v.transpose(-1, -2)) * kf - delta[..., None])
    if kind == "mfma":
        pt, ds = pt.bfloat16().float(), ds.bfloat16().float()
    dq = (ds @ k) * scale
    step = tile if tile > 0 else s
    dk, dv = torch.zeros_like(k), torch.zeros_like(v)
    for i0 in range(0, s, step):
        dk = dk + ds[:, :, i0:i0 + step].transpose(-1, -2) @ q[:, :, i0:i0 + step]
        dv = dv + pt[:, :, i0:i0 + step].transpose(-1, -2) @ do[:, :, i0:i0 + step]
    return tuple(R.rows_of(t).to(dtype) for t in (dq, dk * scale, dv))


# ------------------------------------------------------------------------------------------------ the references are right
@pytest.mark.parametrize("window,p", [(-1, 0.0), (7, 0.0), (-1, 0.3), (5, 0.5), (0, 0.0)])
def test_backward_reference_agrees_with_f64_autograd(window, p):
    b, s, h, d = 2, 37, 3, 5
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(b * s, 3 * h * d, generator=g, dtype=torch.float64)
    dout = torch.randn(b * s, h * d, generator=g, dtype=torch.float64)
    keep = R.keep_mask(99, p, b, h, s) if p > 0 else None
    ref = R.forward_ref(qkv, b, h, window, keep, p)
    bw = R.backward_ref(ref, dout)
    x = qkv.clone().requires_grad_()
    q, k, v = (t.reshape(b, s, h, d).permute(0, 2, 1, 3) for t in x.split(h * d, dim=1))
    sc = (q @ k.transpose(-1, -2) / d ** 0.5).masked_fill(~R.visible(s, window), float("-inf"))
    prob = torch.softmax(sc, -1)
    if keep is not None:
        prob = prob * keep / (1.0 - p)
    want = (prob @ v).permute(0, 2, 1, 3).reshape(b * s, h * d)
    want.backward(dout)
    assert torch.allclose(ref.out, want.detach(), rtol=1e-12, atol=1e-13)
    assert torch.allclose(ref.lse, torch.logsumexp(sc, -1).detach(), rtol=1e-12, atol=1e-13)
    assert torch.allclose(bw.dqkv, x.grad, rtol=1e-11, atol=1e-12)


def test_keep_mask_restatement_and_the_cpu_mirror():
    """The vectorised mask equals a scalar restatement in Python integers (head shard included); the reference without
    dropout agrees with tests/_cpu_ops.mhsa (which has no dropout of its own) to f32 accuracy."""
    import _cpu_ops

    for seed, p, b, h, s, h0, ht in ((123456789, 0.25, 2, 3, 21, 0, 0), (7, 0.5, 1, 2, 40, 2, 4), (2 ** 32 - 5, 0.9, 2, 2, 9, 1, 5)):
        mask = R.keep_mask(seed, p, b, h, s, h0, ht)
        for bi in range(b):
            for hi in range(h):
                for i in range(0, s, 3):
                    for j in range(s):
                        assert int(mask[bi, hi, i, j]) == R.keep_scalar(seed, p, s, ht or h, bi, h0 + hi, i, j)
    assert not bool(R.keep_mask(1, 1.0, 1, 2, 8).any()) and bool(R.keep_mask(1, 1e-6, 1, 2, 8).all()) and R.threshold15(1e-6) == 0
    qkv = R.make_qkv("spread", F32, 2, 50, 2, 8)
    for window in (-1, 6):
        ref = R.forward_ref(qkv, 2, 2, window)
        out, lse = _cpu_ops.mhsa(qkv, 2, 2, window, return_lse=True)
        assert torch.allclose(out.double(), ref.out, atol=1e-5) and torch.allclose(lse.double(), ref.lse, atol=1e-5)


def test_route_and_workspace_against_the_library():
    from anemoi_models_amd import _lib, ops

    lib = _lib.load()
    for c in R.forward_mfma_cases() + R.forward_generic_cases() + R.backward_cases():
        code = ops.dtype_code(c.dtype)
        assert lib.anemoi_mhsa_workspace_bytes(code, c.b, c.s, c.h, c.d) == R.workspace_bytes(c.dtype, c.b, c.s, c.h, c.d)
        assert lib.anemoi_mhsa_backward_workspace_bytes(code, c.b, c.s, c.h, c.d) == R.backward_workspace_bytes(c.dtype, c.b, c.s, c.h, c.d)
    assert (R.tail_rows(513), R.tail_splits(1, 513, 2), R.tail_rows(528), R.tail_rows(529), R.tail_rows(512)) == (1, 3, 16, 0, 0)
    assert R.route(BF16, 1, 529, 2, 64, -1, 384, 128).workgroups == 2 and R.route(BF16, 1, 513, 2, 64, -1, 384, 128).workgroups == 1
    assert R.route(BF16, 1, 130, 2, 64, -1, 388, 128).kernel == "generic" and R.route(BF16, 1, 130, 2, 64, 5, 392, 136).kernel == "w8"
    assert R.route(BF16, 1, 130, 2, 64, -1, 384, 128, p=1.0).kernel == "generic" and R.route(F32, 1, 9, 2, 64, -1, 384, 128).dmax == 64
    assert R.route_backward(BF16, 1, 9, 2, 32, 3, 192, 64, 64, 192).win and not R.route_backward(BF16, 1, 9, 2, 32, 3, 192, 64, 64, 192, workspace=False).mfma


# ------------------------------------------------------------------------------------------------ the library's plan
# anemoi_mhsa_route runs the entry points' own validation and plan and launches nothing: pointers enter as integers
FAKE = dict(qkv=1 << 20, out=2 << 20, dout=3 << 20, lse=4 << 20, delta=5 << 20, dqkv=6 << 20, workspace=7 << 20)


def _code(dtype):
    from anemoi_models_amd import _lib

    return _lib.F32 if dtype == F32 else _lib.BF16


def _plan_forward(dtype, b, s, h, d, window, ld, ldo, qkv=FAKE["qkv"], out=FAKE["out"], p=0.0, ht=0, workspace=FAKE["workspace"]):
    from anemoi_models_amd import _lib

    return _lib.mhsa_route("forward", dtype=_code(dtype), qkv=qkv, ld=ld, out=out, ldo=ldo, workspace=workspace, B=b, S=s, H=h, D=d,
                           window=window, dropout_p=p, dropout_h_total=ht)


def _plan_backward(dtype, b, s, h, d, window, ld, ldo, lddo, lddq, ptrs=(FAKE["qkv"], FAKE["out"], FAKE["dout"], FAKE["dqkv"]),
                   p=0.0, ht=0, workspace=FAKE["workspace"]):
    from anemoi_models_amd import _lib

    return _lib.mhsa_route("backward", dtype=_code(dtype), qkv=ptrs[0], ld=ld, out=ptrs[1], ldo=ldo, dout=ptrs[2], lddo=lddo,
                           lse=FAKE["lse"], delta=FAKE["delta"], dqkv=ptrs[3], lddq=lddq, workspace=workspace, B=b, S=s, H=h, D=d,
                           window=window, dropout_p=p, dropout_h_total=ht)


def _same_forward(*args, **kw):
    """args: dtype, b, s, h, d, window, ld, ldo; kw: qkv, out, p, ht."""
    rt = R.route(*args, kw.get("qkv", FAKE["qkv"]), kw.get("out", FAKE["out"]), kw.get("p", 0.0), kw.get("ht", 0))
    R.assert_same_plan(rt, *_plan_forward(*args, **kw), what=f"forward {args} {kw}")
    return rt


def _same_backward(*args, **kw):
    """args: dtype, b, s, h, d, window, ld, ldo, lddo, lddq; kw: ptrs, p, ht, workspace."""
    ptrs = kw.get("ptrs", (FAKE["qkv"], FAKE["out"], FAKE["dout"], FAKE["dqkv"]))
    rt = R.route_backward(*args, ptrs, kw.get("p", 0.0), kw.get("ht", 0), kw.get("workspace", FAKE["workspace"]))
    R.assert_same_plan(rt, *_plan_backward(*args, **kw), what=f"backward {args} {kw}")
    return rt


def test_the_library_plans_every_case_as_restated():
    """Forward and backward plan of every case of the three case lists (and the dropout cases), the kernel the case names, the
    two workspace functions against the plan's layout, and the layout's offsets."""
    from anemoi_models_amd import _lib

    lib = _lib.load()
    forward = R.forward_mfma_cases() + R.forward_generic_cases() + R.dropout_cases()
    # (the backward list names the backward's route; its bf16 "generic" cases are run without a workspace)
    for i, c in enumerate(forward + R.backward_cases()):
        cc = c.h * c.d
        rt = _same_forward(c.dtype, c.b, c.s, c.h, c.d, c.window, 3 * cc + c.pad, cc + c.opad, p=c.p)
        assert i >= len(forward) or rt.kernel == c.expect, R.case_id(c)
        if not c.pad:
            ws = FAKE["workspace"] if R.backward_expect(c) == "mfma" else 0
            rb = _same_backward(c.dtype, c.b, c.s, c.h, c.d, c.window, 3 * cc, cc, cc, 3 * cc, p=c.p, workspace=ws)
            assert rb.kernel == R.backward_expect(c), R.case_id(c)
            assert _same_backward(c.dtype, c.b, c.s, c.h, c.d, c.window, 3 * cc, cc, cc, 3 * cc, p=c.p, workspace=0).kernel == "generic"
        if rt.mfma:
            _, plan = _plan_forward(c.dtype, c.b, c.s, c.h, c.d, c.window, 3 * cc + c.pad, cc + c.opad, p=c.p)
            _, planb = _plan_backward(c.dtype, c.b, c.s, c.h, c.d, c.window, 3 * cc + c.pad, cc, cc, 3 * cc, p=c.p)
            vt, lo, lb = R.vt_bytes(c.b, c.s, c.h, c.d), plan.layout, planb.layout
            assert lo.total == lib.anemoi_mhsa_workspace_bytes(_lib.BF16, c.b, c.s, c.h, c.d)
            assert (lo.vt, lo.tail, lo.flag) == (0, vt, lo.total - 256) and lo.flag - lo.tail >= c.b * rt.tail * c.h * rt.n_split * (c.d + 2) * 4
            assert lb.total == lib.anemoi_mhsa_backward_workspace_bytes(_lib.BF16, c.b, c.s, c.h, c.d)
            rows = c.b * c.h * planb.S_pad * 4
            assert (lb.qt, lb.kt, lb.dot, lb.lse2p, lb.deltap, lb.total) == (0, vt, 2 * vt, 3 * vt, 3 * vt + rows, 3 * vt + 2 * rows)


SWEEP_SHAPES = [(dtype, b, s, h, d, w) for dtype in (F32, BF16) for b in (1, 2, 3)
                for s in (1, 9, 63, 64, 65, 130, 511, 512, 513, 528, 529, 1040) for h in (1, 2, 16) for d in (8, 32, 33, 64, 65, 128)
                for w in (-1, 0, 5)]
SWEEP_P = (0.0, 1e-6, 0.1, 1.0)
FORWARD_STRIDE, BACKWARD_STRIDE = 7, 101  # coprime to the number of combinations (648, 10 368): every one meets many shapes


def test_the_library_plans_a_forward_sweep_as_restated():
    """3888 shapes (dtype x B {1, 2, 3} x S {1 ... 1040, the 512 / 513 / 528 / 529 tail edges} x H {1, 2, 16} x D {8 ... 128} x
    window {-1, 0, 5}) times every 7th of the 648 combinations of qkv pitch + {0, 4, 8}, out pitch + {0, 2, 4}, qkv pointer +
    {0, 8, 16} bytes, out pointer + {0, 4, 8}, p {0, 1e-6, 0.1, 1} and heads_total {0, 2 H}, the first combination moving with
    the shape: 359 919 argument sets."""
    combos = [(lp, op, qo, oo, p, t) for lp in (0, 4, 8) for op in (0, 2, 4) for qo in (0, 8, 16) for oo in (0, 4, 8)
              for p in SWEEP_P for t in (0, 2)]
    n, kernels = 0, set()
    for i, (dtype, b, s, h, d, w) in enumerate(SWEEP_SHAPES):
        cc = h * d
        for lp, op, qo, oo, p, t in combos[i % FORWARD_STRIDE::FORWARD_STRIDE]:
            rt = _same_forward(dtype, b, s, h, d, w, 3 * cc + lp, cc + op, qkv=FAKE["qkv"] + qo, out=FAKE["out"] + oo, p=p, ht=t * h)
            kernels.add((rt.kernel, rt.drop, rt.tail > 0))
            n += 1
    assert n == 359919 and len(combos) == 648
    assert kernels == {(k, dr, tl) for k in ("w4", "w8") for dr in (False, True) for tl in (False, True)} | {("generic", False, False), ("generic", True, False)}


def test_the_library_plans_a_backward_sweep_as_restated():
    """The 3888 shapes of the forward sweep times every 101st of the 10 368 combinations of qkv pitch + {0, 4, 8}, qkv pointer +
    {0, 8, 16} bytes, out pointer + {0, 1, 4}, dout pointer + {0, 8}, dqkv pointer + {0, 4}, dout pitch + {0, 4}, dqkv pitch +
    {0, 2}, workspace null / off by 8 bytes / aligned, p {0, 1e-6, 0.1, 1} and heads_total {0, 2 H}: 399 134 argument sets."""
    combos = [(lp, qo, oo, do, gq, dp, gp, ws, p, t) for lp in (0, 4, 8) for qo in (0, 8, 16) for oo in (0, 1, 4) for do in (0, 8)
              for gq in (0, 4) for dp in (0, 4) for gp in (0, 2) for ws in (0, FAKE["workspace"] + 8, FAKE["workspace"])
              for p in SWEEP_P for t in (0, 2)]
    n, kernels = 0, set()
    for i, (dtype, b, s, h, d, w) in enumerate(SWEEP_SHAPES):
        cc = h * d
        for lp, qo, oo, do, gq, dp, gp, ws, p, t in combos[i % BACKWARD_STRIDE::BACKWARD_STRIDE]:
            ptrs = (FAKE["qkv"] + qo, FAKE["out"] + oo, FAKE["dout"] + do, FAKE["dqkv"] + gq)
            rt = _same_backward(dtype, b, s, h, d, w, 3 * cc + lp, cc, cc + dp, 3 * cc + gp, ptrs=ptrs, p=p, ht=t * h, workspace=ws)
            kernels.add((rt.kernel, rt.drop, rt.win))
            n += 1
    assert n == 399134 and len(combos) == 10368
    assert kernels == {("mfma", dr, wn) for dr in (False, True) for wn in (False, True)} | {("generic", False, False), ("generic", True, False)}


def test_the_32_bit_bounds_of_the_routes():
    """Shapes no allocation reaches: B x heads x S on either side of 2^32 (the dropout hash's row index), S x ld x 2 on either
    side of 2^31 (four-wave -> eight-wave kernel), and the backward's B x S, ld and lddo on either side of 2^31."""
    assert _same_forward(BF16, 65536, 4095, 1, 64, -1, 192, 64, ht=16).kernel == "w4"  # 2^32 - 2^20 rows
    assert _same_forward(BF16, 65536, 4096, 1, 64, -1, 192, 64, ht=16).kernel == "generic"  # 2^32
    assert _same_backward(BF16, 65536, 4095, 1, 64, -1, 192, 64, 64, 192, ht=16).kernel == "mfma"
    assert _same_backward(BF16, 65536, 4096, 1, 64, -1, 192, 64, 64, 192, ht=16).kernel == "generic"
    assert _same_forward(BF16, 1, (1 << 20) - 512, 1, 64, -1, 1024, 64).kernel == "w4"  # S ld 2 = 2^31 - 2^20
    assert _same_forward(BF16, 1, 1 << 20, 1, 64, -1, 1024, 64).kernel == "w8"  # = 2^31
    assert _same_forward(BF16, 1, 1 << 20, 1, 64, -1, 1016, 64).kernel == "w4"
    assert _same_backward(BF16, 65536, 32767, 1, 64, -1, 192, 64, 64, 192).kernel == "mfma"  # B S = 2^31 - 2^16
    assert _same_backward(BF16, 65536, 32768, 1, 64, -1, 192, 64, 64, 192).kernel == "generic"  # = 2^31
    for ld, lddo, kernel in (((1 << 31) - 8, 64, "mfma"), (1 << 31, 64, "generic"), (192, (1 << 31) - 8, "mfma"), (192, 1 << 31, "generic")):
        assert _same_backward(BF16, 1, 130, 1, 64, -1, ld, 64, lddo, 192).kernel == kernel


def test_what_the_route_query_refuses():
    """The query answers with the entry point's own status and text: the forward refuses an MFMA call without a workspace, the
    backward takes the VALU kernels instead; D = 129; the backward's seed message names the backward."""
    import ctypes

    from anemoi_models_amd import _lib

    err = _lib.load().anemoi_last_error
    st, _ = _plan_forward(BF16, 1, 130, 2, 64, -1, 384, 128, workspace=0)
    assert st == _lib.ANEMOI_ERR_INVALID and err() == b"anemoi_mhsa: workspace of %d bytes required" % R.workspace_bytes(BF16, 1, 130, 2, 64)
    st, plan = _plan_forward(BF16, 1, 130, 2, 64, -1, 388, 128, workspace=0)  # off the MFMA route: none needed
    assert st == 0 and plan.kernel == _lib.MHSA_KERNEL_GENERIC and plan.layout.total == 0
    st, plan = _plan_backward(BF16, 1, 130, 2, 64, -1, 384, 128, 128, 384, workspace=0)
    assert st == 0 and plan.kernel == _lib.MHSA_KERNEL_GENERIC
    st, _ = _plan_forward(F32, 1, 4, 1, 129, -1, 387, 129)
    assert st == _lib.ANEMOI_ERR_UNSUPPORTED and err() == b"anemoi_mhsa: head size 129 > 128"
    st, _ = _plan_backward(F32, 1, 4, 1, 129, -1, 387, 129, 129, 387, p=2.0)  # the backward tests the head size first
    assert st == _lib.ANEMOI_ERR_UNSUPPORTED and err() == b"anemoi_mhsa_backward: head size 129 > 128"
    st, _ = _plan_forward(F32, 1, 4, 1, 129, -1, 387, 129, p=2.0)  # the forward the dropout rate
    assert st == _lib.ANEMOI_ERR_INVALID and b"dropout_p 2 outside [0, 1]" in err()
    st, _ = _lib.mhsa_route("backward", dtype=_lib.F32, qkv=64, out=64, dout=64, lse=64, delta=64, dqkv=64, ld=24, ldo=8, lddo=8,
                            lddq=24, B=1, S=4, H=1, D=8, dropout_seed_dev=66)
    assert st == _lib.ANEMOI_ERR_INVALID and err() == b"anemoi_mhsa_backward: dropout_seed_dev must be 4-byte aligned"
    st, _ = _lib.mhsa_route("forward", dtype=2, qkv=64, out=64, ld=24, ldo=8, B=1, S=4, H=1, D=8)
    assert st == _lib.ANEMOI_ERR_UNSUPPORTED and err() == b"anemoi_mhsa: dtype 2"
    args, route = _lib.MhsaArgs(), _lib.MhsaRoute()
    args.struct_bytes, route.struct_bytes = ctypes.sizeof(_lib.MhsaArgs), ctypes.sizeof(_lib.MhsaRoute) - 8
    assert _lib.load().anemoi_mhsa_route(ctypes.byref(args), ctypes.byref(route)) == _lib.ANEMOI_ERR_INVALID and b"out of sync" in err()


def test_wrappers_refuse_operands_that_do_not_fit_before_any_launch():
    """ops.mhsa / ops.mhsa_backward raise ValueError on shapes and dtypes that contradict qkv (the checks come first: CPU
    tensors get that far, a fitting CPU call is refused as every CPU call is -- RuntimeError, no fallback)."""
    from anemoi_models_amd import ops

    b, s, h, d = 2, 6, 2, 8
    c = h * d
    qkv, out, dout, lse = torch.zeros(b * s, 3 * c), torch.zeros(b * s, c), torch.zeros(b * s, c), torch.zeros(b, h, s)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mhsa(qkv, b, h)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mhsa_backward(qkv, out, dout, lse, b, h)
    for bad in (dict(batch_size=5), dict(num_heads=5), dict(qkv=torch.zeros(b * s, 3 * c + 1)), dict(qkv=torch.zeros(b * s, 3 * c + 3)),
                dict(out=torch.zeros(b * s, c + 1)), dict(out=torch.zeros(b * s + 1, c)), dict(out=out.bfloat16()), dict(out=out.double())):
        args = dict(qkv=qkv, batch_size=b, num_heads=h, out=out)
        args.update(bad)
        with pytest.raises(ValueError):
            ops.mhsa(**args)
    for bad in (dict(batch_size=5), dict(num_heads=5), dict(qkv=torch.zeros(b * s, 3 * c + 1)), dict(out=torch.zeros(b * s, c + 2)),
                dict(out=out.bfloat16()), dict(dout=dout.bfloat16()), dict(dout=torch.zeros(b * s - 1, c)), dict(dout=torch.zeros(b * s, 2 * c)),
                dict(lse=torch.zeros(b, s, h)), dict(lse=torch.zeros(b * h * s)), dict(lse=lse.double()),
                dict(qkv=qkv.bfloat16())):
        args = dict(qkv=qkv, out=out, dout=dout, lse=lse, batch_size=b, num_heads=h)
        args.update(bad)
        with pytest.raises(ValueError):
            ops.mhsa_backward(**args)


def test_torch_f32_constants_are_what_was_measured():
    got = R.measure_torch_f32()
    for key, value in R.TORCH_F32.items():
        print(f"torch f32 attention, worst fraction of the derived bound, {key}: measured {got[key]:.5f}, constant {value:.5f}")
    for key, value in R.TORCH_F32.items():
        assert abs(got[key] / value - 1.0) <= 0.01, (key, got[key], value)


# ------------------------------------------------------------------------------------------------ every GPU case
def _all_cases():
    seen, out = set(), []
    for c in R.forward_mfma_cases() + R.forward_generic_cases() + R.backward_cases() + R.dropout_cases():
        if R.case_id(c) not in seen:
            seen.add(R.case_id(c))
            out.append(c)
    return out


_BACKWARD_IDS = {R.case_id(c) for c in R.backward_cases() + R.dropout_cases()}
_STATE = {}


def _state(c):
    key = R.case_id(c)
    if _STATE.get("key") != key:
        qkv = R.case_qkv(c)
        keep, kk = _kk(c)
        ref = R.forward_ref(qkv, c.b, c.h, c.window, keep, c.p)
        kind = R.case_kind(c)
        _STATE.clear()
        _STATE.update(key=key, qkv=qkv, keep=keep, kk=kk, ref=ref, kind=kind, bounds=R.forward_bounds(ref, kind, c.dtype))
        if key in _BACKWARD_IDS:
            dout = R.make_dout(c.dtype, c.b, c.s, c.h, c.d)
            _STATE.update(dout=dout, bw=R.backward_ref(ref, dout))
    return types_ns(_STATE)


def types_ns(d):
    import types

    return types.SimpleNamespace(**d)


@pytest.mark.parametrize("c", _all_cases(), ids=R.case_id)
def test_emulations_stay_inside_the_bounds(c):
    st = _state(c)
    ref, (bo, bl) = st.ref, st.bounds
    tag = f"{st.kind} {R.name(c.dtype)}"
    if st.kind == "mfma":
        assert bool((bo <= R.mfma_form(ref) + 2.0 ** -119 * 1e3).all()), "the bound left c 2^-9 (2 A + |want|)"
        runs = [("online/64", emu_mfma_forward(st.qkv, c.b, c.h, c.window, st.kk, "online", 64)[:2]),
                ("online/32", emu_mfma_forward(st.qkv, c.b, c.h, c.window, st.kk, "online", 32)[:2])]
        if c.window < 0 and c.d == 64 and st.kk is None:
            out, lse, redo = emu_four_wave(st.qkv, c.b, c.h, True)
            runs.append(("fixed/32" + ("+fallback" if redo else ""), (out, lse)))
        elif c.window < 0 and c.data != "gap":
            runs.append(("fixed/32", emu_mfma_forward(st.qkv, c.b, c.h, c.window, st.kk, "fixed", 32)[:2]))
        runs += [(f"split/{n}", emu_split_forward(st.qkv, c.b, c.h, c.window, st.kk, n, BF16)) for n in (3, 7)]
    else:
        runs = [(f"split/{n}", emu_split_forward(st.qkv, c.b, c.h, c.window, st.kk, n, c.dtype)) for n in (1, 3, 7)]
    for label, (out, lse) in runs:
        f_out = R.check(out, ref.out, bo, f"{label} out")
        f_lse = R.check(lse, ref.lse, bl, f"{label} lse")
        _note(f"forward {tag} {label.split('+')[0]} out", f_out)
        _note(f"forward {tag} {label.split('+')[0]} lse", f_lse)
    if not hasattr(st, "bw"):
        return
    out, lse = runs[0][1]
    bounds = R.backward_bounds(ref, st.bw, st.kind, c.dtype, bo, bl)
    for tile in (32, 0):
        grads = emu_backward(st.qkv, out, lse.float(), st.dout, c.b, c.h, c.window, st.kk, st.kind, tile, c.dtype)
        for what, got, want, bound in zip(("dq", "dk", "dv"), grads, (st.bw.dq, st.bw.dk, st.bw.dv), bounds):
            _note(f"backward {tag} {what}", R.check(got, want, bound, f"backward tile {tile} {what}"))
    # delta from the UNROUNDED out: more accurate than the contract, cannot be rejected -- and is not
    grads = emu_backward(st.qkv, ref.out.float(), lse.float(), st.dout, c.b, c.h, c.window, st.kk, st.kind, 0, c.dtype)
    for what, got, want, bound in zip(("dq", "dk", "dv"), grads, (st.bw.dq, st.bw.dk, st.bw.dv), bounds):
        R.check(got, want, bound, f"backward with delta from the unrounded out, {what}")


def test_four_wave_fallback_flag_and_the_gap_band():
    """The fixed-maximum emulation with the flag on the row sum ALONE stores non-finite rows in the band between 2^128 /
    GAP_V and 1e37 (the g = 121 case sweeps it); with the flag also raised by a non-finite accumulator it does not."""
    c = [c for c in R.forward_mfma_cases() if c.data == "gap" and c.s == 200 and c.g_log2 == 121][0]
    qkv = R.case_qkv(c)
    _, gaps = R.gap_rows(qkv, c.h, c.s, c.g_log2)
    assert float(gaps.min()) < 121.0 and 121.5 < float(gaps.max()) < 122.8
    out, _, redo = emu_four_wave(qkv, c.b, c.h, False)
    assert not redo and not bool(torch.isfinite(out.float()).all())
    out, _, redo = emu_four_wave(qkv, c.b, c.h, True)
    assert redo and bool(torch.isfinite(out.float()).all())


# ------------------------------------------------------------------------------------------------ mutants
def _cast(x, dtype):
    return x.to(dtype)


def _must_include(c):
    """Key positions the single-key mutants have to cover at this shape."""
    keys = {0, c.s - 1, 31, 32, 63, 64}
    n = R.tail_splits(c.b, c.s, c.h)
    if n:
        chunk = R.tail_chunk(c.b, c.s, c.h)
        keys |= {j for t in range(1, n) for j in (t * chunk - 1, t * chunk)}
    return {j for j in keys if 0 <= j < c.s}


def _single_key_mutants(c, st):
    """Key j dropped / counted twice, in the row where it weighs most: out' = (out -+ Pt_ij v_j) / (1 -+ P_ij)."""
    ref, (bo, bl) = st.ref, st.bounds
    rows3 = ref.out4  # [B, H, S, D]
    glob = c.window < 0 or c.window >= c.s - 1
    for bi in range(c.b):
        for hi in range(c.h):
            prob, pt = ref.P[bi, hi], ref.Pt[bi, hi]
            if glob:
                keys = torch.arange(c.s)
            else:
                p1, p2 = R.pair_targets(c.s, c.window, bi, hi)
                keys = torch.unique(torch.cat([p1, p2]))
                i = torch.arange(c.s)  # both window edges are among the designated keys
                assert bool(((p1 - i == c.window) | (p2 - i == c.window)).any()) and bool(((i - p1 == c.window) | (i - p2 == c.window)).any())
            if c.data == "pairs":
                assert _must_include(c) <= set(keys.tolist()), sorted(_must_include(c) - set(keys.tolist()))
            i_of = prob[:, keys].argmax(dim=0)
            pij, ptij = prob[i_of, keys], pt[i_of, keys]
            keep_rows = pij < 1.0  # (S = 1: dropping the only key leaves nothing to compare)
            bo_h, bl_h = R.heads(bo, c.b, c.h)[bi, hi], bl[bi, hi]
            for sign, label in ((-1.0, "key dropped"), (1.0, "key counted twice")):
                o2 = (rows3[bi, hi][i_of] + sign * ptij[:, None] * ref.v[bi, hi][keys]) / (1.0 + sign * pij)[:, None]
                l2 = ref.lse[bi, hi][i_of] + torch.log1p(sign * pij)
                got = _cast(o2, c.dtype).double()
                bad_o = ((got - rows3[bi, hi][i_of]).abs() > bo_h[i_of]).any(dim=1) | ~torch.isfinite(got).all(dim=1)
                bad_l = (l2.float().double() - ref.lse[bi, hi][i_of]).abs() > bl_h[i_of]
                # (a key that holds its row alone -- offset 0 under a window -- leaves out unchanged when it is counted twice:
                #  that row shows it in lse only)
                ok = ((bad_o | ((sign > 0) & (pij > 0.6))) & bad_l) | ~keep_rows
                assert bool(ok.all()), f"{label}: key {int(keys[~ok][0])} of head {hi} passes (row {int(i_of[~ok][0])})"
    if c.s > 1:
        _rejected("a single key dropped (out and lse)")
        _rejected("a single key counted twice (out and lse)")


def _forward_mutant(c, st, label, **kw):
    ref = st.ref
    vis = kw.get("vis", ref.vis)
    out, lse, _, _ = R.attention_f64(ref.q, ref.k, ref.v, vis, ref.kk, kw.get("scale"), kw.get("weight"))
    if "extra" in kw:  # n keys of score 0 and v = 0 join the normaliser
        big = torch.logaddexp(lse, torch.full_like(lse, math.log(kw["extra"])))
        out, lse = out * torch.exp(lse - big)[..., None], big
    return _cast(R.rows_of(out), c.dtype), lse.float()


def _expect_out_fails(c, st, label, got):
    assert R.fails(got, st.ref.out, st.bounds[0]), f"{label}: passes the out bound"
    _rejected(label)


@pytest.mark.parametrize("c", _all_cases(), ids=R.case_id)
def test_mutants_fail_the_bounds(c):
    st = _state(c)
    ref, (bo, bl) = st.ref, st.bounds
    s, w = c.s, c.window
    i = torch.arange(s)
    diff = i[None, :] - i[:, None]  # key - query
    if c.data == "pairs" and c.p == 0.0:
        _single_key_mutants(c, st)
    if c.data == "pairs" and 0 <= w < s:
        if w >= 1 or s > 1:
            for label, vis in (("window: key - query < w", ref.vis & (diff != w)), ("window: query - key < w", ref.vis & (diff != -w))):
                if w == 0:
                    continue  # (the row would be empty: a kernel like that returns NaN or 0, rejected by the scale mutant's kin)
                _expect_out_fails(c, st, label, _forward_mutant(c, st, label, vis=vis)[0])
    if c.data == "intruder":
        for label, vis in (("window one too wide (both sides)", diff.abs() <= w + 1), ("window one too wide (right)", (diff <= w + 1) & (-diff <= w)),
                           ("window one too wide (left)", (diff <= w) & (-diff <= w + 1))):
            _expect_out_fails(c, st, label, _forward_mutant(c, st, label, vis=vis)[0])
    if c.data == "cold":
        pad = (-s) % 64
        assert pad > 0
        for n, label in ((1, "one zero-score pad key admitted"), (pad, "every zero-score pad key admitted")):
            got, lse = _forward_mutant(c, st, label, extra=float(n))
            _expect_out_fails(c, st, label, got)
            assert R.fails(lse, ref.lse, bl), label
    if c.data == "pairs" and s % 64 != 0 and s > 1 and c.p == 0.0 and (w < 0 or w >= s):
        # (global attention: under a window the copies lie at positions >= S, which the intruder mutants cover)
        weight = torch.ones(s, s, dtype=torch.float64)
        weight[:, s - 1] = 1.0 + (-s) % 64
        label = "the last key repeated for the clamped positions"
        _expect_out_fails(c, st, label, _forward_mutant(c, st, label, weight=weight)[0])
    if s > 1 and c.d > 1:
        label = "scale 1 / sqrt(D) omitted"  # (a row that sees one key -- window 0 -- shows it in lse only)
        got, lse = _forward_mutant(c, st, label, scale=1.0)
        assert R.fails(lse, ref.lse, bl) and (w == 0 or R.fails(got, ref.out, bo)), label
        _rejected(label)
    for label, lse in (("lse in log2 units", ref.lse / LN2), ("lse without the maximum", ref.lse - (ref.q @ ref.k.transpose(-1, -2) * ref.c).masked_fill(~ref.vis, float("-inf")).amax(-1))):
        if bool(((lse - ref.lse).abs() > 2.0 * bl).any()):  # (a row whose lse or maximum is 0 says nothing)
            assert R.fails(lse.float(), ref.lse, bl), label
            _rejected(label)
        else:
            assert c.s == 1 or c.d == 1, f"{label}: no row of this data set can show it"
    if c.h > 1:
        label = "heads swapped"
        _expect_out_fails(c, st, label, _cast(R.rows_of(ref.out4.flip(1)), c.dtype))
    if c.b > 1:
        label = "batch elements swapped"
        _expect_out_fails(c, st, label, _cast(R.rows_of(ref.out4.flip(0)), c.dtype))
    if not hasattr(st, "bw"):
        return
    bw = st.bw
    # exact operands: the tightest bounds a test of the backward alone uses
    out_st, lse_st = _cast(ref.out, c.dtype), ref.lse.float()
    bounds = R.backward_bounds(ref, bw, st.kind, c.dtype, (out_st.double() - ref.out).abs(), (lse_st.double() - ref.lse).abs())
    wants = (bw.dq, bw.dk, bw.dv)

    def grads_with(kk=None, delta=None, prob=None):
        kk_ = ref.kk if kk is None else kk
        pr = ref.P if prob is None else prob
        kdp = (bw.do @ ref.v.transpose(-1, -2)) * (1.0 if kk_ is None else kk_)
        dl = bw.delta if delta is None else delta
        ds = pr * (kdp - dl[..., None])
        pt = pr if kk_ is None else pr * kk_
        return [(ds @ ref.k) * ref.c, (ds.transpose(-1, -2) @ ref.q) * ref.c, pt.transpose(-1, -2) @ bw.do], ds

    def expect(label, grads, which):
        for idx in which:
            assert R.fails(_cast(R.rows_of(grads[idx]), c.dtype), wants[idx], bounds[idx]), f"{label}: {('dq', 'dk', 'dv')[idx]} passes"
        _rejected(label)

    true_grads, ds = grads_with()
    for got, want, bound in zip(true_grads, wants, bounds):
        R.check(_cast(R.rows_of(got), c.dtype), want, bound, "the rounded true gradient")
    expect("delta omitted", grads_with(delta=torch.zeros_like(bw.delta))[0], (0, 1))
    if c.p > 0.0:
        other = R.keep_mask(R.DROPOUT_SEED + 1, c.p, c.b, c.h, c.s) * (1.0 / (1.0 - c.p))
        expect("the backward's mask drawn with another seed", grads_with(kk=other)[0], (0, 1, 2))
    if c.data == "pairs" and s > 1:
        flat = int((ref.Pt[0, 0]).argmax())
        qi, kj = flat // s, flat % s
        dv2 = true_grads[2].clone()
        dv2[0, 0, kj] -= ref.Pt[0, 0, qi, kj] * bw.do[0, 0, qi]
        flat = int((ds[0, 0].abs() * ref.q[0, 0].abs().amax(dim=1, keepdim=True)).argmax())
        qi, kj = flat // s, flat % s
        dk2 = true_grads[1].clone()
        dk2[0, 0, kj] -= ref.c * ds[0, 0, qi, kj] * ref.q[0, 0, qi]
        # (window 0: every row sees one key, dS is identically zero and dk has nothing to lose)
        expect("one (query, key) pair missing from dk / dv", [None, dk2, dv2], (2,) if w == 0 else (1, 2))
    if c.h > 1 and s > 1:
        expect("heads swapped (backward)", [t.flip(1) for t in true_grads], (2,) if w == 0 else (0, 1, 2))
