"""``optim.WeightAverager`` / ``optim.DeviceLRSchedule`` and their kernels on the MI355X (``-m gpu``): the update per element
against the f64 restatement (tests/_average_ref.py, which derives the bounds), the exact copy and swap, the inactive steps,
determinism, HIP-graph capture with the optimizer step, the schedule kernel against its closed form, ``AveragedModel`` as the
yardstick, checkpoint resume and the refusals."""

import contextlib
import copy

import pytest
import torch

import _average_ref as R
from anemoi_models_amd import _lib
from anemoi_models_amd import ops
from anemoi_models_amd import optim

pytestmark = pytest.mark.gpu

DEV = "cuda"
C, M = _lib.OPT_CHUNK, _lib.OPT_MAX_TENSORS
HYPER = dict(lr=1e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1)
LENGTHS = [1, 3, 5, C - 1, C, C + 1, 2 * C + 7]


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def _tensors(lengths, seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return [(scale * torch.randn(n, generator=gen)).to(DEV) for n in lengths]


def _odd_views(tensors):
    """The same values as views at element offsets 1, 2, 3 of fresh buffers (4-byte alignment only), with the buffers."""
    bufs, views = [], []
    for k, t in enumerate(tensors):
        off = 1 + k % 3
        buf = torch.full((t.numel() + 5,), 7.0, device=DEV)
        buf[off: off + t.numel()] = t
        bufs.append((buf, off, t.numel()))
        views.append(buf[off: off + t.numel()])
    assert any(v.data_ptr() % 16 for v in views)
    return bufs, views


def _consts(n, **kw):
    """The block of ``anemoi_average_constants`` for a counter that stands at ``n``: (avg on the host, counter tensor, avg)."""
    avg = torch.full((_lib.AVG_CONSTS,), -1.0, device=DEV)
    counter = torch.tensor(float(n), device=DEV)
    for name in ("step", "skip"):
        if kw.get(name) is not None:
            kw[name] = torch.tensor(float(kw[name]), device=DEV)
    ops.average_constants(avg, counter, **kw)
    return avg.cpu().tolist(), counter, avg


WEIGHTS = [("ema", 0.999, False, 0), ("ema", 0.999, False, 3), ("ema", 0.0, False, 3), ("ema", 0.999, True, 1),
           ("ema", 0.999, True, 5), ("ema", 0.999, True, 200), ("swa", 0.999, False, 1), ("swa", 0.999, False, 2),
           ("swa", 0.999, False, 1000)]


# ---------------------------------------------------------------- 1. per element against f64
@pytest.mark.parametrize("kind,decay,warmup,n", WEIGHTS)
def test_update_per_element_against_f64(kind, decay, warmup, n):
    """Lengths around the chunk, a list of M + 1 tensors (a second launch) and both again as odd-offset views: the scalars
    against f64 rounded once, every element within ``1.01 u (w |p - s| + |ref|)`` with w as the device rounded it, parameters
    and the floats around the views untouched."""
    got, counter, avg = _consts(n, kind=kind, decay=decay, warmup=warmup)
    want = R.constants(float(n), kind, decay, warmup)
    w = got[0]
    print(f"{kind} decay {decay} warmup {warmup} n {n}: w = {w!r}, f64 rounded once {R.f32(want['w'])!r}")
    if R.weight_is_exact(kind, float(n), warmup):
        assert w == R.f32(want["w"])
    else:
        assert abs(w - R.f32(want["w"])) <= R.ulp32(want["w"])
    assert got[1:] == [1.0, 1.0 if want["copy"] else 0.0, want["n_after"]] and float(counter) == want["n_after"] == n + 1.0
    for lengths, seed in ((LENGTHS, 1), ([7] * (M + 1), 2)):
        ps, ss = _tensors(lengths, seed), _tensors(lengths, seed + 10, scale=0.5)
        for moved in (False, True):
            p_in, s_in, bufs = ps, [s.clone() for s in ss], []
            if moved:
                (_, p_in), (bufs, s_in) = _odd_views(ps), _odd_views(ss)
            ops.multi_average(p_in, s_in, avg)
            for p, p0, s, s0 in zip(p_in, ps, s_in, ss):
                assert same_bits(p, p0)  # params are only read
                ref, bound = R.update(p0, s0, w, copy=want["copy"])
                assert bool(((s.double().cpu() - ref).abs() <= bound).all()), (lengths[0], moved)
                if want["copy"]:
                    assert same_bits(s, p0)
            for buf, off, numel in bufs:
                assert bool((buf[:off] == 7.0).all()) and bool((buf[off + numel:] == 7.0).all())


# ---------------------------------------------------------------- 2. the copy
def test_the_first_update_is_a_bit_copy():
    ps = _tensors([5, C + 1, 9], 3)
    ps[0][0], ps[0][1], ps[1][C], ps[2][3] = -0.0, float("inf"), -0.0, float("nan")
    bits(ps[1])[7] = 0x7FC12345   # a NaN with a payload
    bits(ps[2])[8] = -4194305     # 0xFFBFFFFF: a negative signalling NaN
    _, (ps[2],) = _odd_views([ps[2]])
    av = optim.WeightAverager(ps, kind="ema", decay=0.9)
    for s in av.averaged:
        s.fill_(float("nan"))     # whatever the shadows held is not read
    av.update()
    assert float(av.n_averaged) == 1.0
    for p, s in zip(ps, av.averaged):
        assert same_bits(s, p) and s.data_ptr() != p.data_ptr()
    assert int(bits(av.averaged[1])[7]) == 0x7FC12345 and int(bits(av.averaged[2])[8]) == -4194305


# ---------------------------------------------------------------- 3. inactive steps
def test_inactive_steps_leave_the_shadow_and_the_counter_alone():
    ps, ss = _tensors([C + 3, 6], 4), _tensors([C + 3, 6], 5)
    ss[1][2] = float("nan")
    snap = [s.clone() for s in ss]
    for kw, active in ((dict(step=2, start_step=3), False), (dict(step=3, start_step=3), True),
                       (dict(step=4, start_step=3, every=2), False), (dict(step=5, start_step=3, every=2), True),
                       (dict(step=5, start_step=3, every=2, skip=1), False), (dict(step=5, start_step=3, every=2, skip=0), True),
                       (dict(skip=1), False)):
        got, counter, avg = _consts(4, kind="ema", decay=0.9, **kw)
        assert got == ([R.f32(1.0 - 0.9), 1.0, 0.0, 5.0] if active else [0.0, 0.0, 0.0, 4.0]), kw
        assert float(counter) == (5.0 if active else 4.0)
        if not active:
            ops.multi_average(ps, ss, avg)
            assert all(same_bits(s, s0) for s, s0 in zip(ss, snap)), kw


def test_a_skipped_optimizer_step_does_not_enter_the_average():
    gen = torch.Generator().manual_seed(6)
    ps = [torch.nn.Parameter(t) for t in _tensors([C + 2, 17], 6)]
    opt = optim.FusedAdamW(ps, max_grad_norm=1.0, skip_nonfinite=True, **HYPER)
    av = optim.WeightAverager(opt, kind="ema", decay=0.5)

    def step(bad=False):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=gen).to(DEV)
        if bad:
            ps[0].grad[5] = float("inf")
        opt.step()

    step()
    assert float(av.n_averaged) == 1.0 and all(same_bits(s, p) for s, p in zip(av.averaged, ps))
    step()
    assert float(av.n_averaged) == 2.0
    snap = [s.clone() for s in av.averaged]
    step(bad=True)
    assert int(opt.skipped_steps) == 1 and float(opt.step_count) == 2.0 and float(opt.skip_flag) == 1.0
    assert float(av.n_averaged) == 2.0 and all(same_bits(s, s0) for s, s0 in zip(av.averaged, snap))
    assert av._avg.cpu().tolist() == [0.0, 0.0, 0.0, 2.0]
    step()
    assert float(av.n_averaged) == 3.0 and not any(same_bits(s, s0) for s, s0 in zip(av.averaged, snap))
    av.detach()
    step()
    assert float(av.n_averaged) == 3.0 and float(opt.step_count) == 4.0


def test_start_step_and_every_count_optimizer_steps():
    ps = [torch.nn.Parameter(t) for t in _tensors([33], 7)]
    opt = optim.FusedAdamW(ps, **HYPER)
    av = optim.WeightAverager(opt, kind="swa", start_step=2, every=2)
    counts = []
    for _ in range(6):
        ps[0].grad = torch.ones_like(ps[0])
        opt.step()
        counts.append(float(av.n_averaged))
    assert counts == [0.0, 1.0, 1.0, 2.0, 2.0, 3.0]  # after steps 2, 4 and 6


# ---------------------------------------------------------------- 4. swap
def test_swap_is_exact_and_bumps_the_versions():
    lengths = LENGTHS + [7] * (M + 1)
    ps = [torch.nn.Parameter(t) for t in _tensors(lengths, 8)]
    av = optim.WeightAverager(ps, kind="swa")
    for k, s in enumerate(av.averaged):
        s.copy_(torch.randn(s.shape, generator=torch.Generator().manual_seed(100 + k)))
    with torch.no_grad():
        ps[3][0], ps[3][1] = -0.0, float("nan")
    bits(av.averaged[4])[2] = 0x7FC00001
    p0, s0 = [p.detach().clone() for p in ps], [s.clone() for s in av.averaged]
    versions = [p._version for p in ps]
    av.swap()
    assert all(same_bits(p, s) for p, s in zip(ps, s0)) and all(same_bits(s, p) for s, p in zip(av.averaged, p0))
    assert all(p._version > v for p, v in zip(ps, versions))
    versions = [p._version for p in ps]
    av.swap()
    assert all(same_bits(p, q) for p, q in zip(ps, p0)) and all(same_bits(s, q) for s, q in zip(av.averaged, s0))
    assert all(p._version > v for p, v in zip(ps, versions))
    with av.applied():
        assert all(same_bits(p, s) for p, s in zip(ps, s0))
    assert all(same_bits(p, q) for p, q in zip(ps, p0))
    # odd-offset views on either side
    (_, a), (_, b) = _odd_views(_tensors([C + 5, 3], 9)), _odd_views(_tensors([C + 5, 3], 10))
    a0, b0 = [t.clone() for t in a], [t.clone() for t in b]
    ops.multi_swap(a, b)
    assert all(same_bits(x, y) for x, y in zip(a, b0)) and all(same_bits(x, y) for x, y in zip(b, a0))
    av.copy_to()
    assert all(same_bits(p, s) for p, s in zip(ps, s0))


@pytest.mark.parametrize("route", ["f32", "bf16-autocast"])
def test_derived_weights_are_not_stale_after_a_swap(graph_o32, golden_cfg1_gt, monkeypatch, route):
    """INTEGRATION.md's hole (a writer of parameter storage that does not bump versions leaves packed weights, split planes
    and folds stale) does not apply to ``swap()``: on the config-1 model, in validation mode (eval, no_grad) and in training
    mode, the forward after ``swap()`` is bit-equal to that of a fresh model loaded with the averaged values, and after the
    second swap bit-equal to the original forward."""
    from test_gpu_optim import _batches, _cfg1

    monkeypatch.delenv("ANEMOI_AMD_DTYPE", raising=False)
    monkeypatch.delenv("ANEMOI_AMD_F32_TRAIN_LINEAR", raising=False)
    heads = 4 if route == "bf16-autocast" else None
    ctx = (lambda: torch.autocast("cuda", dtype=torch.bfloat16)) if route == "bf16-autocast" else contextlib.nullcontext
    model = _cfg1(graph_o32, golden_cfg1_gt, heads)
    (x,), _ = _batches(golden_cfg1_gt, 1)
    av = optim.WeightAverager(model.parameters(), kind="ema", decay=0.5)
    av.update()
    gen = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for p in model.parameters():
            p.add_((0.05 * torch.randn(p.shape, generator=gen)).to(DEV))
    av.update()
    assert float(av.n_averaged) == 2.0
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    for (name, _), s in zip(model.named_parameters(), av.averaged):
        sd[name] = s.clone()
    fresh = _cfg1(graph_o32, golden_cfg1_gt, heads)
    fresh.load_state_dict(sd)

    def forward(m, training):
        m.train(training)
        with ctx(), (contextlib.nullcontext() if training else torch.no_grad()):
            return m(x).detach().clone()

    for training in (False, True):
        y0 = forward(model, training)  # (fills whatever the route derives from the parameters)
        av.swap()
        y1 = forward(model, training)
        y2 = forward(fresh, training)
        assert torch.equal(y1, y2) and not torch.equal(y1, y0), training
        av.swap()
        assert torch.equal(forward(model, training), y0), training


# ---------------------------------------------------------------- 5. determinism
def test_the_same_updates_twice_and_a_split_list_have_the_same_bits():
    lengths = [3 * C + 11, 5, C, 129] + [7] * M
    runs = []
    for split in (False, False, True):
        ps = _tensors(lengths, 12)
        av = optim.WeightAverager(ps, kind="ema", decay=0.99, warmup=True)
        for k in range(3):
            for p, d in zip(ps, _tensors(lengths, 20 + k, scale=0.1)):
                p.add_(d)
            if split:  # the list cut at the launch limit, two calls under the same scalars
                ops.average_constants(av._avg, av.n_averaged, kind="ema", decay=0.99, warmup=True)
                ops.multi_average(ps[:M], av.averaged[:M], av._avg)
                ops.multi_average(ps[M:], av.averaged[M:], av._avg)
            else:
                av.update()
        runs.append(([s.clone() for s in av.averaged], av.n_averaged.clone()))
    for other in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0][0], other[0])) and torch.equal(runs[0][1], other[1])


# ---------------------------------------------------------------- 6. capture
def test_captured_with_the_optimizer_step_and_the_schedule_advances(graph_o32, golden_cfg1_gt):
    """``GraphedTrainStep(model, loss, x, y, FusedAdamW)`` with an averager and a schedule attached, four replays against an
    eager loop from the same state: parameters, moments, shadows, ``n_averaged`` and the ``lr`` tensor bit-equal; the ``lr``
    of replay i is the closed form at the steps completed before it; and the parameters differ from those of a captured run
    whose float ``lr`` a host scheduler assigns (frozen at capture: the documented pitfall)."""
    from anemoi_models_amd.runtime import GraphedTrainStep
    from test_gpu_optim import _batches, _cfg1, _loss

    k, sched = 4, dict(warmup_steps=2, total_steps=6, lr_min=1e-5, warmup_start=1e-4)
    xs, ts = _batches(golden_cfg1_gt, k)
    models = {name: _cfg1(graph_o32, golden_cfg1_gt) for name in ("eager", "captured", "frozen")}
    opts = {name: optim.FusedAdamW(m.parameters(), max_grad_norm=1.0, **HYPER) for name, m in models.items()}
    scheds = {name: optim.DeviceLRSchedule(opts[name], **sched) for name in ("eager", "captured")}
    avs = {name: optim.WeightAverager(opts[name], kind="ema", decay=0.9, start_step=2) for name in ("eager", "captured")}
    assert float(scheds["eager"].get_last_lr()[0]) == R.f32(R.lr(0, HYPER["lr"], **sched))
    opts["frozen"].param_groups[0]["lr"] = R.lr(0, HYPER["lr"], **sched)
    graphed = GraphedTrainStep(models["captured"], _loss, xs[0], ts[0], optimizer=opts["captured"], warmup=1)
    frozen = GraphedTrainStep(models["frozen"], _loss, xs[0], ts[0], optimizer=opts["frozen"], warmup=1)

    def eager_step(x, t):
        opts["eager"].zero_grad(set_to_none=True)
        loss = _loss(models["eager"](x), t)
        loss.backward()
        opts["eager"].step()
        return loss.detach()

    eager_step(xs[0], ts[0])  # the warm-up step is a real step on the example
    for i, (x, t) in enumerate(zip(xs, ts)):
        le, lc = eager_step(x, t), graphed(x, t)
        opts["frozen"].param_groups[0]["lr"] = R.lr(1 + i, HYPER["lr"], **sched)  # what a host scheduler does: not seen
        frozen(x, t)
        assert torch.equal(lc, le)
        lr_e, lr_c = scheds["eager"].get_last_lr()[0], scheds["captured"].get_last_lr()[0]
        want = R.lr(1 + i, HYPER["lr"], **sched)
        assert torch.equal(lr_c, lr_e) and abs(float(lr_c) - R.f32(want)) <= R.ulp32(want), (i, float(lr_c), want)
        assert lr_c is opts["captured"].param_groups[0]["lr"]
    assert float(opts["captured"].step_count) == float(opts["eager"].step_count) == 1.0 + k
    assert float(avs["captured"].n_averaged) == float(avs["eager"].n_averaged) == k  # after steps 2 .. 5
    differs = False
    for (name, pe), (_, pc), (_, pf), se, sc in zip(models["eager"].named_parameters(), models["captured"].named_parameters(),
                                                    models["frozen"].named_parameters(), avs["eager"].averaged,
                                                    avs["captured"].averaged):
        assert torch.equal(pc.detach(), pe.detach()), name
        assert torch.equal(sc, se), name
        differs = differs or not torch.equal(pf.detach(), pc.detach())
        if pe in opts["eager"].state:
            for what in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(opts["captured"].state[pc][what], opts["eager"].state[pe][what]), (name, what)
    assert differs
    assert not any(torch.equal(s, p.detach()) for s, p in zip(avs["captured"].averaged, models["captured"].parameters())
                   if p.numel() > 16)


# ---------------------------------------------------------------- 7. the schedule kernel
@pytest.mark.parametrize("prefix", [False, True])
@pytest.mark.parametrize("warmup", [0, 5])
def test_schedule_kernel_against_the_closed_form(prefix, warmup):
    total, bases, lr_min, start = 40, (1e-3, 6.25e-5), 1e-6, 1e-5
    steps = [torch.zeros((), device=DEV) for _ in bases]
    lrs = [torch.full((), -1.0, device=DEV) for _ in bases]
    n = len(bases)
    points = {0, 1, max(warmup - 1, 0), warmup, warmup + 1, total - 1, total, total + 5, total + warmup - 1, total + warmup,
              total + warmup + 1}
    for t in sorted(points):
        steps[0].fill_(t)
        steps[1].fill_(t + 1)  # the groups' counters are their own
        ops.lr_schedule(lrs, steps, bases, warmup_steps=[warmup] * n, total_steps=[total] * n, lr_min=[lr_min, 0.0],
                        warmup_start=[start, 0.0], warmup_prefix=[prefix] * n)
        for g, (tg, lo, ws) in enumerate(((t, lr_min, start), (t + 1, 0.0, 0.0))):
            want = R.lr(tg, bases[g], warmup, total, lo, ws, prefix)
            got = float(lrs[g])
            assert abs(got - R.f32(want)) <= R.ulp32(want), (g, tg, got, want)
        assert float(steps[0]) == t  # the counters are only read


def test_schedule_on_the_optimizer_follows_its_counter():
    """A float and a tensor ``lr`` as bases of two groups; the step that moves the counter from t to t + 1 uses lr(t) (read
    from the optimizer's constants block); ``detach()`` leaves the tensors."""
    ps = [torch.nn.Parameter(t) for t in _tensors([C + 1, 9], 13)]
    lr1 = torch.tensor(4e-3, device=DEV)
    opt = optim.FusedAdamW([dict(params=ps[:1]), dict(params=ps[1:], lr=lr1)], **HYPER)
    sched = optim.DeviceLRSchedule(opt, warmup_steps=2, total_steps=3, warmup_prefix=True)
    assert sched.base_lrs == [1e-3, R.f32(4e-3)] and opt.param_groups[1]["lr"] is lr1
    assert isinstance(opt.param_groups[0]["lr"], torch.Tensor) and opt.param_groups[0]["lr"].dim() == 0
    for t in range(7):
        for p in ps:
            p.grad = torch.ones_like(p)
        opt.step()
        consts = opt._consts.view(-1, _lib.OPT_CONSTS).cpu()
        for g, base in enumerate(sched.base_lrs):
            want = R.lr(t, base, 2, 3, warmup_prefix=True)
            assert abs(float(consts[1 + g, 5]) - R.f32(want)) <= R.ulp32(want) and float(consts[1 + g, 6]) == t + 1.0
            assert float(sched.get_last_lr()[g]) == float(consts[1 + g, 5])
    assert float(lr1) == 0.0  # t = 6 is behind the warm-up and the period: lr_min
    sched.detach()
    lr1.fill_(2e-3)
    opt.step()
    assert float(lr1) == R.f32(2e-3) and float(opt._consts.view(-1, _lib.OPT_CONSTS)[2, 5]) == R.f32(2e-3)


# ---------------------------------------------------------------- 8. the yardstick
def test_five_updates_against_averaged_model():
    """``AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(0.9))`` and ``WeightAverager(decay=0.9)`` over five updates of a
    small module on the GPU, both against the f64 chain: ours within the chained bound (``E' = |1 - w| E + bound``); torch's
    distance is printed."""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

    torch.manual_seed(14)
    model = torch.nn.Sequential(torch.nn.Linear(67, 129), torch.nn.Linear(129, 33)).to(DEV)
    theirs = AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(0.9))
    ours = optim.WeightAverager(model.parameters(), kind="ema", decay=0.9)
    gen = torch.Generator().manual_seed(15)
    history = [[] for _ in model.parameters()]
    for _ in range(5):
        with torch.no_grad():
            for p in model.parameters():
                p.add_(torch.randn(p.shape, generator=gen).to(DEV))
        theirs.update_parameters(model)
        ours.update()
        for h, p in zip(history, model.parameters()):
            h.append(p.detach().clone())
    assert float(ours.n_averaged) == float(theirs.n_averaged) == 5.0
    worst_ours = worst_theirs = 0.0
    for h, s, a in zip(history, ours.averaged, theirs.module.parameters()):
        ref, bound = R.chain(h, "ema", 0.9)
        d = (s.double().cpu() - ref).abs()
        assert bool((d <= bound).all())
        scale = float(ref.abs().max())
        worst_ours = max(worst_ours, float(d.max()) / scale)
        worst_theirs = max(worst_theirs, float((a.detach().double().cpu() - ref).abs().max()) / scale)
    print(f"five EMA updates against the f64 chain, worst |d| / max|ref|: WeightAverager {worst_ours:.3e}, "
          f"AveragedModel {worst_theirs:.3e}")


# ---------------------------------------------------------------- 9. checkpoint
def test_resume_from_a_state_dict_continues_bit_for_bit():
    lengths = [C + 9, 50, 7]
    deltas = [_tensors(lengths, 30 + k, scale=0.1) for k in range(4)]

    def advance(av, ps, ks):
        for k in ks:
            for p, d in zip(ps, deltas[k]):
                p.add_(d)
            av.update()

    a = _tensors(lengths, 16)
    whole = optim.WeightAverager(a, kind="ema", decay=0.95, warmup=True)
    advance(whole, a, range(4))
    b = _tensors(lengths, 16)
    first = optim.WeightAverager(b, kind="ema", decay=0.95, warmup=True)
    advance(first, b, range(2))
    sd = copy.deepcopy(first.state_dict())
    assert sorted(sd["averaged"]) == [0, 1, 2] and float(sd["n_averaged"]) == 2.0
    c = [t.clone() for t in b]
    second = optim.WeightAverager(c, kind="ema", decay=0.95, warmup=True)
    where = [s.data_ptr() for s in second.averaged] + [second.n_averaged.data_ptr()]
    second.load_state_dict(sd)
    assert [s.data_ptr() for s in second.averaged] + [second.n_averaged.data_ptr()] == where
    advance(second, c, range(2, 4))
    assert torch.equal(second.n_averaged, whole.n_averaged) and float(whole.n_averaged) == 4.0
    assert all(torch.equal(s, w) for s, w in zip(second.averaged, whole.averaged))
    with pytest.raises(ValueError, match="decay"):
        optim.WeightAverager(c, kind="ema", decay=0.5).load_state_dict(sd)


# ---------------------------------------------------------------- 10. refusals, the trail
def test_refusals():
    good = torch.nn.Parameter(torch.zeros(8, device=DEV))
    for bad in (torch.nn.Parameter(torch.zeros(8, device=DEV, dtype=torch.bfloat16)), torch.nn.Parameter(torch.zeros(8)),
                torch.zeros(4, 6, device=DEV).t()):
        with pytest.raises(NotImplementedError, match="parameter 1 is"):
            optim.WeightAverager([good, bad])
    for kw in (dict(decay=1.0), dict(decay=-0.5), dict(every=0), dict(start_step=-2)):
        with pytest.raises(ValueError):
            optim.WeightAverager([good], **kw)
    avg, n = torch.zeros(_lib.AVG_CONSTS, device=DEV), torch.zeros((), device=DEV)
    for kw in (dict(decay=1.0), dict(every=0), dict(start_step=-1)):  # and through the C ABI
        with pytest.raises(ValueError, match="anemoi_average_constants"):
            ops.average_constants(avg, n, **kw)
    with pytest.raises(NotImplementedError, match="FusedAdamW"):
        optim.DeviceLRSchedule(torch.optim.AdamW([good]), warmup_steps=1, total_steps=2)
    opt = optim.FusedAdamW([good])
    for kw in (dict(warmup_steps=-1, total_steps=5), dict(warmup_steps=1, total_steps=0)):
        with pytest.raises(ValueError):
            optim.DeviceLRSchedule(opt, **kw)
    with pytest.raises(ValueError, match="has 4 elements"):
        ops.multi_swap([good.detach()], [torch.zeros(4, device=DEV)])


def test_the_launch_trail_records_what_was_written():
    from anemoi_models_amd import trail

    ps = [torch.nn.Parameter(t) for t in _tensors([C + 1, 0, 6], 17)]
    av = optim.WeightAverager(ps)
    with trail.record() as t:
        av.update()
        av.swap()
    want = ["anemoi_average_constants:avg"] + [f"anemoi_multi_average:shadow[{i}]" for i in (0, 2)] + \
        [f"anemoi_multi_swap:{side}[{i}]" for side in ("a", "b") for i in (0, 2)]
    assert t.names() == want and t.dropped == 0
    by_name = {e.name: e for e in t.entries}
    assert by_name["anemoi_multi_swap:b[0]"].digest == trail.digest(av.averaged[0].view(1, -1)).digest
    assert (by_name["anemoi_average_constants:avg"].rows, by_name["anemoi_average_constants:avg"].cols) == (1, _lib.AVG_CONSTS)
    opt = optim.FusedAdamW([dict(params=ps[:1]), dict(params=ps[2:])], **HYPER)
    with trail.record() as t:
        optim.DeviceLRSchedule(opt, warmup_steps=1, total_steps=2)
    assert t.names() == ["anemoi_lr_schedule:lr[0]", "anemoi_lr_schedule:lr[1]"]
