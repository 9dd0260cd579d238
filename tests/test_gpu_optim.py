"""``anemoi_models_amd.optim`` on the MI355X (``-m gpu``): the multi-tensor kernels per element against the f64 restatement
(tests/_optim_ref.py, which derives the two bounds), the semantics of ``FusedAdamW`` and ``clip_grad_norm_``, determinism,
torch.optim.AdamW as the yardstick at model level, the stale-derived-weight guard, HIP-graph capture and checkpoint resume
in both directions."""

import copy

import pytest
import torch

import _optim_ref as R
from anemoi_models_amd import _lib
from anemoi_models_amd import optim
from conftest import split_prefix

pytestmark = pytest.mark.gpu

DEV = "cuda"
C, M = _lib.OPT_CHUNK, _lib.OPT_MAX_TENSORS
HYPER = dict(lr=1e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1)


def rel_err(got, want):
    got, want = got.float().cpu(), want.float().cpu()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def _params(lengths, seed=0, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(n, generator=gen).to(DEV)) for n in lengths]
    for p in ps:
        p.grad = (scale * torch.randn(p.shape, generator=gen)).to(DEV)
    return ps


def _new_grads(ps, seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    for p in ps:
        if p.grad is not None:
            p.grad = (scale * torch.randn(p.shape, generator=gen)).to(DEV)


def _within(got, ref, bound):
    return bool(((got.detach().double().cpu() - ref).abs() <= bound).all())


def _step_and_check(opt):
    """One ``opt.step()``, then: the sum of squares within the norm bound, the constants block against f64, and m, v, p of
    every updated tensor per element within the update bounds (scalars as the device rounded them)."""
    groups = opt.param_groups
    before, versions = {}, {}
    for group in groups:
        for p in group["params"]:
            st = opt.state.get(p, {})
            before[p] = (p.detach().clone(), st["exp_avg"].clone() if "exp_avg" in st else torch.zeros_like(p),
                         st["exp_avg_sq"].clone() if "exp_avg_sq" in st else torch.zeros_like(p),
                         None if p.grad is None else p.grad.clone())
            versions[p] = p._version
    steps_before = [float(opt._steps[gi]) if gi < len(opt._steps) and opt._steps[gi] is not None else 0.0
                    for gi in range(len(groups))]
    opt.step()
    torch.cuda.synchronize()
    active = [gi for gi, g in enumerate(groups) if any(p.grad is not None for p in g["params"])]
    want_norm = opt.max_grad_norm is not None or opt.skip_nonfinite
    consts = opt._consts.view(-1, _lib.OPT_CONSTS).cpu().double()
    sumsq32 = None
    if want_norm:
        grads = [p.grad for g in groups for p in g["params"] if p.grad is not None]
        ref, sumsq32 = R.sumsq(grads), float(opt._sumsq)
        assert abs(sumsq32 - ref) <= R.sumsq_bound(ref, C, R.n_chunks([g.numel() for g in grads], C)), (sumsq32, ref)
        assert opt.grad_norm is not None and abs(float(opt.grad_norm) - sumsq32 ** 0.5) <= 1.01 * R.U * sumsq32 ** 0.5
    else:
        assert opt.grad_norm is None
    for k, gi in enumerate(active):
        group, blk = groups[gi], consts[1 + k]
        c = R.constants(sumsq32, steps_before[gi], float(group["lr"]), group["betas"], group["weight_decay"],
                        opt.max_grad_norm, opt.skip_nonfinite)
        assert not c["skip"] and float(blk[4]) == 0.0 and float(blk[6]) == c["t"] == float(opt._steps[gi])
        clip, decay, step_size, bc2s = (float(blk[i]) for i in range(4))
        assert abs(clip - c["clip"]) <= 1.01 * 3 * R.U * c["clip"]        # sqrtf, the add, the division
        for got, want in ((decay, c["decay"]), (step_size, c["step_size"]), (bc2s, c["bc2s"])):
            assert abs(got - want) <= 1.01 * R.U * abs(want), (got, want)  # f64, rounded once
        for p in group["params"]:
            p0, m0, v0, g = before[p]
            if g is None:
                assert torch.equal(p.detach(), p0) and p._version == versions[p] and "exp_avg" not in opt.state.get(p, {})
                continue
            assert torch.equal(p.grad, g)  # .grad is only read
            assert p._version > versions[p] or p.numel() == 0
            m1, v1 = opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]
            m_ref, m_bound, v_ref, v_bound = R.moments_ref(g, m0, v0, clip, *group["betas"])
            assert _within(m1, m_ref, m_bound) and _within(v1, v_ref, v_bound)
            p_ref, p_bound = R.param_ref(p0, m1, v1, decay, step_size, bc2s, group["eps"])
            assert _within(p, p_ref, p_bound)
    return consts


# ---------------------------------------------------------------- kernel edges
def test_tensor_lengths_around_the_chunk_with_an_empty_tensor_and_a_missing_gradient():
    lengths = [1, 3, 4, C - 1, 0, C, C + 1, 2 * C + 5, 7]
    ps = _params(lengths, scale=30.0)
    ps[-1].grad = None
    opt = optim.FusedAdamW(ps, max_grad_norm=1.0, **HYPER)
    c = _step_and_check(opt)
    assert float(c[0, 1]) < 1.0  # clipped
    _new_grads(ps, 1, scale=30.0)
    _step_and_check(opt)  # with moments that are not zero
    assert float(opt.step_count) == 2.0 and ps[-1] not in opt.state


@pytest.mark.parametrize("which", ["p", "g", "m", "v"])
def test_a_view_at_element_offset_one(which):
    """A tensor whose base is only 4-byte aligned, for each operand in turn; the elements around the view keep their bits."""
    n = C + 3
    ps = _params([5, n, 9], seed=3)
    gen = torch.Generator().manual_seed(4)
    buf = torch.randn(n + 6, generator=gen).to(DEV)
    guard = buf.clone()
    view = buf[1: n + 1]
    assert view.data_ptr() % 16 == 4
    if which == "p":
        ps[1] = torch.nn.Parameter(view)
        ps[1].grad = torch.randn(n, generator=gen).to(DEV)
    elif which == "g":
        ps[1].grad = view
    opt = optim.FusedAdamW(ps, max_grad_norm=1.0, **HYPER)
    opt.init_state()
    if which in ("m", "v"):
        view.abs_().mul_(1e-3)  # a plausible moment (v >= 0)
        guard = buf.clone()
        opt.state[ps[1]]["exp_avg" if which == "m" else "exp_avg_sq"] = view
    _step_and_check(opt)
    assert torch.equal(buf[:1], guard[:1]) and torch.equal(buf[n + 1:], guard[n + 1:])
    if which == "g":
        assert torch.equal(buf, guard)


@pytest.mark.parametrize("count", [M - 1, M, M + 1, 2 * M + 3])
def test_list_lengths_around_the_launch_limit(count):
    ps = _params([5] * count, seed=count)
    opt = optim.FusedAdamW(ps, max_grad_norm=1.0, **HYPER)
    _step_and_check(opt)
    _new_grads(ps, 2)
    _step_and_check(opt)


# ---------------------------------------------------------------- semantics
def test_clip_inactive_and_no_norm_without_a_reason():
    ps = _params([C + 1, 33], seed=5, scale=1e-4)
    opt = optim.FusedAdamW(ps, max_grad_norm=1.0, **HYPER)
    c = _step_and_check(opt)
    assert float(c[0, 1]) == 1.0  # not clipped
    opt = optim.FusedAdamW(ps, **HYPER)
    _step_and_check(opt)  # asserts grad_norm is None: no norm launch
    assert opt._workspace.numel() == 1


def test_two_groups_share_one_norm_and_a_device_lr_is_honoured():
    ps = _params([C + 7, 40, 3], seed=6, scale=5.0)
    lr_dev = torch.tensor(2e-3, device=DEV)
    opt = optim.FusedAdamW([dict(params=ps[:2]), dict(params=ps[2:], lr=lr_dev, weight_decay=0.0)], max_grad_norm=1.0, **HYPER)
    c = _step_and_check(opt)
    assert float(c[1, 0]) == float(c[2, 0]) == float(c[0, 1]) < 1.0  # one clip coefficient
    assert float(c[1, 5]) == R.f32(1e-3) and float(c[2, 5]) == R.f32(2e-3) and float(c[2, 1]) == 1.0
    lr_dev.fill_(5e-4)  # what a scheduler does between two steps
    _new_grads(ps, 7, scale=5.0)
    c = _step_and_check(opt)
    assert float(c[2, 5]) == R.f32(5e-4) and float(c[2, 6]) == 2.0


def test_zero_gradient_and_zero_moments_leave_only_the_decay():
    ps = _params([C + 2], seed=8)
    ps[0].grad.zero_()
    p0 = ps[0].detach().clone()
    opt = optim.FusedAdamW(ps, **HYPER)
    opt.step()
    decay = float(opt._consts.view(-1, _lib.OPT_CONSTS)[1, 1])
    assert torch.equal(ps[0].detach(), p0 * decay)
    assert not opt.state[ps[0]]["exp_avg"].any() and not opt.state[ps[0]]["exp_avg_sq"].any()


def test_a_nonfinite_gradient_is_skipped_on_the_device_or_propagates():
    ps = _params([C + 2, 17], seed=9)
    opt = optim.FusedAdamW(ps, max_grad_norm=1.0, skip_nonfinite=True, **HYPER)
    _step_and_check(opt)
    _new_grads(ps, 10)
    ps[0].grad[5] = float("inf")
    snap = [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in ps]
    opt.step()
    for p, (p0, m0, v0) in zip(ps, snap):
        assert torch.equal(p.detach(), p0) and torch.equal(opt.state[p]["exp_avg"], m0)
        assert torch.equal(opt.state[p]["exp_avg_sq"], v0)
    assert float(opt.step_count) == 1.0 and int(opt.skipped_steps) == 1 and not torch.isfinite(opt.grad_norm)
    _new_grads(ps, 11)
    _step_and_check(opt)  # and the next good step is step 2
    assert float(opt.step_count) == 2.0 and int(opt.skipped_steps) == 1
    # without the switch: as clip_grad_norm_ + torch.optim.AdamW (clip = 1 / inf = 0, 0 * inf = NaN in that element)
    ps = _params([40, 17], seed=9)
    ps[0].grad[5] = float("inf")
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    for q, p in zip(qs, ps):
        q.grad = p.grad.clone()
    optim.FusedAdamW(ps, max_grad_norm=1.0, **HYPER).step()
    torch.nn.utils.clip_grad_norm_(qs, 1.0)
    torch.optim.AdamW(qs, **HYPER).step()
    for p, q in zip(ps, qs):
        assert torch.equal(torch.isnan(p), torch.isnan(q))
        assert torch.allclose(p.detach().nan_to_num(0.0), q.detach().nan_to_num(0.0), rtol=1e-6, atol=0)
    assert torch.isnan(ps[0][5]) and int(torch.isnan(ps[0]).sum()) == 1


def test_the_launch_trail_records_the_scalars_and_the_updated_tensors():
    """While a trail is armed: ``sumsq``, the constants block and params / exp_avg / exp_avg_sq of every non-empty tensor, with
    digests that are those of the tensors as they stand after the step; the stand-alone clip records the scaled gradients."""
    from anemoi_models_amd import trail

    ps = _params([C + 1, 0, 6], seed=16, scale=3.0)
    opt = optim.FusedAdamW(ps, max_grad_norm=1.0, **HYPER)
    with trail.record() as t:
        opt.step()
    want = ["anemoi_multi_sumsq:sumsq", "anemoi_adamw_constants:consts"] + \
        [f"anemoi_multi_adamw:{what}[{i}]" for what in ("params", "exp_avg", "exp_avg_sq") for i in (0, 2)]
    assert t.names() == want and t.dropped == 0 and t.first_nonfinite() is None
    by_name = {e.name: e for e in t.entries}
    assert (by_name["anemoi_adamw_constants:consts"].rows, by_name["anemoi_adamw_constants:consts"].cols) == (2, _lib.OPT_CONSTS)
    for i in (0, 2):
        for what, tensor in (("params", ps[i].detach()), ("exp_avg", opt.state[ps[i]]["exp_avg"])):
            e = by_name[f"anemoi_multi_adamw:{what}[{i}]"]
            assert (e.rows, e.cols) == (1, ps[i].numel()) and e.digest == trail.digest(tensor.view(1, -1)).digest
    with trail.record() as t:
        optim.clip_grad_norm_(ps, 1.0)
    assert t.names() == ["anemoi_multi_sumsq:sumsq", "anemoi_adamw_constants:consts", "anemoi_multi_scale:grads[0]",
                         "anemoi_multi_scale:grads[2]"]


# ---------------------------------------------------------------- determinism
def test_two_runs_from_the_same_state_have_the_same_bits():
    lengths = [3 * C + 11, 5, C, 129]
    runs = []
    for _ in range(2):
        ps = _params(lengths, seed=12, scale=3.0)
        opt = optim.FusedAdamW(ps, max_grad_norm=1.0, **HYPER)
        opt.step()
        _new_grads(ps, 13, scale=3.0)
        opt.step()
        runs.append(([p.detach().clone() for p in ps], [opt.state[p]["exp_avg"] for p in ps],
                     [opt.state[p]["exp_avg_sq"] for p in ps], opt.grad_norm.clone()))
    for a, b in zip(runs[0][:3], runs[1][:3]):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert torch.equal(runs[0][3], runs[1][3])


def test_the_norm_depends_on_values_and_lengths_not_on_addresses():
    """The rule DESIGN.md 8f-10 states: the sum of squares is a function of the values and the ordered list of lengths --
    the same gradients as odd-offset views of other buffers give the same bits.  (It is NOT claimed for a list that is
    part of a longer one: stage 2 deals the partials to its threads by their position in the whole list.)"""
    from anemoi_models_amd import ops

    gen = torch.Generator().manual_seed(14)
    lengths = [2 * C + 5, 3, C - 1] + [5] * (M + 2)
    grads = [torch.randn(n, generator=gen).to(DEV) for n in lengths]
    want = ops.multi_sumsq(grads)
    moved = []
    for k, g in enumerate(grads):
        buf = torch.zeros(g.numel() + 4, device=DEV)
        buf[1 + k % 3: 1 + k % 3 + g.numel()] = g
        moved.append(buf[1 + k % 3: 1 + k % 3 + g.numel()])
    assert torch.equal(ops.multi_sumsq(moved), want)
    ref = R.sumsq(grads)
    assert abs(float(want) - ref) <= R.sumsq_bound(ref, C, R.n_chunks(lengths, C))


# ---------------------------------------------------------------- the stand-alone clip
def test_clip_grad_norm_against_f64_and_a_coefficient_of_one():
    ps = _params([C + 1, 1, 2 * C + 5, 64], seed=15, scale=2.0)
    ps.append(torch.nn.Parameter(torch.zeros(3, device=DEV)))  # no gradient
    g0 = [p.grad.clone() for p in ps[:-1]]
    norm = optim.clip_grad_norm_(ps, 1.0)
    ref_sq = R.sumsq(g0)
    ref_norm = ref_sq ** 0.5
    assert norm.dim() == 0 and norm.is_cuda
    assert abs(float(norm) - ref_norm) <= (0.5 * 1.01 * (R.sumsq_depth(C, 1) + 2) + 1.01) * R.U * ref_norm  # sqrt halves it
    coef = 1.0 / (float(norm) + 1e-6)
    for p, g in zip(ps, g0):
        # coefficient: 2 roundings (the add, the division) from the device's norm; the product: 1
        assert _within(p.grad, coef * g.double().cpu(), 1.01 * 3 * R.U * (coef * g.double().cpu()).abs())
    for p in ps[:-1]:  # the clipped norm is ~ 1; a quarter of it is well below the threshold
        p.grad.mul_(0.25)
    small = [p.grad.clone() for p in ps[:-1]]
    optim.clip_grad_norm_(ps, 1.0)
    assert all(torch.equal(p.grad, g) for p, g in zip(ps, small))  # multiplied by exactly 1
    assert ps[-1].grad is None


# ---------------------------------------------------------------- model level
def _cfg1(graph_o32, gold, heads=None):
    from test_gpu_parity import _build

    model, _ = _build(graph_o32, 64, 4) if heads is None else _build(graph_o32, 64, 4, heads=heads)
    model.load_state_dict(split_prefix(gold, "sd."))
    return model.to(DEV).train()


def _batches(gold, n, seed=5):
    gen = torch.Generator().manual_seed(seed)
    xs = [(gold["x"] + (0.1 * torch.randn(gold["x"].shape, generator=gen) if k else 0.0)).to(DEV) for k in range(n)]
    ts = [torch.randn(gold["y"].shape, generator=gen).to(DEV) for _ in xs]
    return xs, ts


def _loss(y, t):
    return ((y - t) ** 2).mean()


TORCH_DISTANCE = 3.044e-5  # torch fused=True against torch foreach on these inputs, measured (docstring below)


def test_three_steps_against_torch_adamw_on_the_config1_model(graph_o32, golden_cfg1_gt):
    """FusedAdamW(max_grad_norm=1) against clip_grad_norm_ + torch.optim.AdamW (foreach): rel_err per parameter after three
    steps below 1e-5, the figure the captured-SGD test of tests/test_gpu_training.py holds an optimizer step to -- except for
    the attention key biases (``*.lin_key.bias``).  Their gradient is exactly zero in real arithmetic (the softmax over the
    edges of a destination does not change when every key moves by the same vector), so what reaches the optimizer is
    rounding noise of the backward, which Adam normalises to full-size steps: from the second step on, any two optimizers
    whose parameters differ in the last bit draw different noise there.  torch's own two routes show it: measured on these
    inputs, torch fused=True against torch foreach is 3.044e-5 (encoder.proc.lin_key.bias; the six key biases are the only
    parameters beyond 1e-5, everything else is below), FusedAdamW against torch foreach is 3.966e-5
    (processor.proc.0.blocks.0.lin_key.bias; five key biases beyond 1e-5, everything else below).  The key biases are
    therefore held to four times torch's own distance, 4 x 3.044e-5 = 1.22e-4.  Every run prints both figures."""
    models = {name: _cfg1(graph_o32, golden_cfg1_gt) for name in ("ours", "foreach", "fused")}
    opts = {"ours": optim.FusedAdamW(models["ours"].parameters(), max_grad_norm=1.0, **HYPER),
            "foreach": torch.optim.AdamW(models["foreach"].parameters(), foreach=True, **HYPER),
            "fused": torch.optim.AdamW(models["fused"].parameters(), fused=True, **HYPER)}
    xs, ts = _batches(golden_cfg1_gt, 3)
    for x, t in zip(xs, ts):
        norms = {}
        for name, model in models.items():
            opts[name].zero_grad(set_to_none=True)
            _loss(model(x), t).backward()
            if name != "ours":
                norms[name] = torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
            opts[name].step()
        assert rel_err(opts["ours"].grad_norm, norms["foreach"]) < 1e-5
    named = {name: dict(model.named_parameters()) for name, model in models.items()}
    d_ours = {k: rel_err(named["ours"][k].detach(), p.detach()) for k, p in named["foreach"].items()}
    d_torch = {k: rel_err(named["fused"][k].detach(), p.detach()) for k, p in named["foreach"].items()}
    k_ours, k_torch = max(d_ours, key=d_ours.get), max(d_torch, key=d_torch.get)
    print(f"after three steps, worst parameter rel_err: FusedAdamW vs torch foreach {d_ours[k_ours]:.3e} ({k_ours}); "
          f"torch fused vs torch foreach {d_torch[k_torch]:.3e} ({k_torch}); "
          f"parameters beyond 1e-5: ours {sorted(k for k, v in d_ours.items() if v >= 1e-5)}, "
          f"torch {sorted(k for k, v in d_torch.items() if v >= 1e-5)}")
    for k, v in d_ours.items():
        assert v < (4 * TORCH_DISTANCE if k.endswith("lin_key.bias") else 1e-5), (k, v)


@pytest.mark.parametrize("route", ["f32", "bf16-autocast", "bf16x3"])
def test_derived_weights_are_not_stale_after_a_step(graph_o32, golden_cfg1_gt, monkeypatch, route):
    """INTEGRATION.md's hole (an optimizer that writes parameters without bumping their version leaves packed weights,
    split-bf16 planes and folds stale) does not apply: after one eager step the model's output is bit-equal to that of a fresh
    model loaded with the updated state_dict, and differs from the output before the step."""
    import contextlib

    monkeypatch.delenv("ANEMOI_AMD_DTYPE", raising=False)
    monkeypatch.delenv("ANEMOI_AMD_F32_TRAIN_LINEAR", raising=False)
    if route == "bf16x3":
        monkeypatch.setenv("ANEMOI_AMD_DTYPE", "fp32")
        monkeypatch.setenv("ANEMOI_AMD_F32_TRAIN_LINEAR", "bf16x3")
    heads = 4 if route == "bf16-autocast" else None
    ctx = (lambda: torch.autocast("cuda", dtype=torch.bfloat16)) if route == "bf16-autocast" else contextlib.nullcontext
    model = _cfg1(graph_o32, golden_cfg1_gt, heads)
    (x,), (t,) = _batches(golden_cfg1_gt, 1)
    opt = optim.FusedAdamW(model.parameters(), max_grad_norm=1.0, **dict(HYPER, lr=1e-2))
    with ctx():
        y0 = model(x)
    _loss(y0.float(), t).backward()
    opt.step()
    with ctx():
        y1 = model(x)
    fresh = _cfg1(graph_o32, golden_cfg1_gt, heads)
    fresh.load_state_dict(model.state_dict())
    with ctx():
        y2 = fresh(x)
    assert torch.equal(y1.detach(), y2.detach())
    assert not torch.equal(y1.detach(), y0.detach())


def test_captured_in_a_hip_graph(graph_o32, golden_cfg1_gt):
    """GraphedTrainStep(..., optimizer=FusedAdamW(max_grad_norm=1), warmup=1), two replays against two eager steps from the
    same state: parameters, both moments, step_count and grad_norm bit-equal."""
    from anemoi_models_amd.runtime import GraphedTrainStep

    xs, ts = _batches(golden_cfg1_gt, 2)
    eager, captured = _cfg1(graph_o32, golden_cfg1_gt), _cfg1(graph_o32, golden_cfg1_gt)
    opt_e = optim.FusedAdamW(eager.parameters(), max_grad_norm=1.0, **HYPER)
    opt_c = optim.FusedAdamW(captured.parameters(), max_grad_norm=1.0, **HYPER)
    graphed = GraphedTrainStep(captured, _loss, xs[0], ts[0], optimizer=opt_c, warmup=1)

    def eager_step(x, t):
        opt_e.zero_grad(set_to_none=True)
        loss = _loss(eager(x), t)
        loss.backward()
        opt_e.step()
        return loss.detach()

    eager_step(xs[0], ts[0])  # the warm-up step is a real step on the example
    for x, t in zip(xs, ts):
        le = eager_step(x, t)
        lc = graphed(x, t)
        assert torch.equal(lc, le)
        assert torch.equal(opt_c.grad_norm, opt_e.grad_norm)
    assert float(opt_c.step_count) == float(opt_e.step_count) == 3.0
    for (k, pe), (_, pc) in zip(eager.named_parameters(), captured.named_parameters()):
        assert torch.equal(pc.detach(), pe.detach()), k
        if pe in opt_e.state:
            for name in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(opt_c.state[pc][name], opt_e.state[pe][name]), (k, name)


def _pair(seed):
    a = _params([C + 9, 50, 7], seed=seed)
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    return a, b


def _torch_step(opt, ps, max_norm=1.0):
    torch.nn.utils.clip_grad_norm_(ps, max_norm)
    opt.step()


def test_resume_from_a_torch_checkpoint_and_back():
    kw = dict(max_grad_norm=1.0, **HYPER)
    # torch -> FusedAdamW
    a, b = _pair(20)
    opt_t = torch.optim.AdamW(a, **HYPER)
    for k in range(2):
        _new_grads(a, 21 + k, scale=4.0)
        _torch_step(opt_t, a)
    for q, p in zip(b, a):
        q.data.copy_(p.detach())
    opt_o = optim.FusedAdamW(b, **kw)
    opt_o.load_state_dict(copy.deepcopy(opt_t.state_dict()))  # (as a checkpoint: load_state_dict keeps tensors it need not cast)
    assert float(opt_o.step_count) == 2.0
    _new_grads(a, 23, scale=4.0)
    for q, p in zip(b, a):
        q.grad = p.grad.clone()
    _torch_step(opt_t, a)
    opt_o.step()
    assert float(opt_o.step_count) == 3.0
    for q, p in zip(b, a):
        assert rel_err(q.detach(), p.detach()) < 1e-5
    # FusedAdamW -> torch
    a, b = _pair(30)
    opt_o = optim.FusedAdamW(a, **kw)
    for k in range(2):
        _new_grads(a, 31 + k, scale=4.0)
        opt_o.step()
    for q, p in zip(b, a):
        q.data.copy_(p.detach())
    opt_t = torch.optim.AdamW(b, **HYPER)
    opt_t.load_state_dict(copy.deepcopy(opt_o.state_dict()))
    _new_grads(a, 33, scale=4.0)
    for q, p in zip(b, a):
        q.grad = p.grad.clone()
    opt_o.step()
    _torch_step(opt_t, b)
    for q, p in zip(b, a):
        assert rel_err(q.detach(), p.detach()) < 1e-5
        assert float(opt_t.state[q]["step"]) == 3.0
