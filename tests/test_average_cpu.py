"""Weight averaging and the device LR schedule without a GPU: the f64 restatement (tests/_average_ref.py) against
``torch.optim.swa_utils`` and ``SequentialLR(LinearLR, CosineAnnealingLR)``, the argument checks of the four entry points
through the C ABI (the library validates before it launches) and the refusals of ``optim.WeightAverager`` /
``optim.DeviceLRSchedule``."""

import ctypes

import pytest
import torch

import _average_ref as R
from anemoi_models_amd import _lib
from anemoi_models_amd import optim


# ---------------------------------------------------------------- the restatement
def _module(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.Linear(7, 3)).double()


@pytest.mark.parametrize("kind", [R.EMA, R.SWA])
def test_restatement_against_torch_swa_utils_in_f64(kind):
    """Five updates of ``AveragedModel`` (``get_ema_multi_avg_fn(0.9)`` / its default, the SWA form) on f64 CPU parameters
    against ``chain`` with unrounded weights: the first update is a copy, ``n_averaged`` counts, and the values agree to a few
    f64 roundings per update (|d| <= 1e-14 (|s| + 1e-300))."""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

    model = _module(3)
    avg = AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(0.9)) if kind == R.EMA else AveragedModel(model)
    gen = torch.Generator().manual_seed(4)
    history = [[] for _ in model.parameters()]
    for k in range(5):
        with torch.no_grad():
            for p in model.parameters():
                p.add_(torch.randn(p.shape, generator=gen, dtype=torch.float64))
        avg.update_parameters(model)
        for h, p in zip(history, model.parameters()):
            h.append(p.detach().clone())
        assert int(avg.n_averaged) == k + 1 == int(R.constants(float(k), kind, 0.9)["n_after"])
        if k == 0:
            assert all(torch.equal(a.detach(), p.detach()) for a, p in zip(avg.module.parameters(), model.parameters()))
            assert R.constants(0.0, kind, 0.9)["copy"] and not R.constants(1.0, kind, 0.9)["copy"]
    for h, a in zip(history, avg.module.parameters()):
        ref, _ = R.chain(h, kind, 0.9, rounded=False)
        assert bool(((ref - a.detach()).abs() <= 1e-14 * (a.detach().abs() + 1e-300)).all())


def test_weights_gating_and_the_update_form():
    assert R.weight(R.EMA, 0.0, 0.999) == 1.0 and R.weight(R.EMA, 7.0, 0.999) == 1.0 - 0.999
    assert R.weight(R.EMA, 5.0, 0.999, warmup=True) == 1.0 - 6.0 / 15.0   # the ramp is below the decay
    assert R.weight(R.EMA, 10 ** 6, 0.999, warmup=True) == 1.0 - 0.999     # and above it
    assert R.weight(R.SWA, 3.0) == 0.25
    assert R.weight_is_exact(R.EMA, 5.0, False) and R.weight_is_exact(R.SWA, 0.0, False)
    assert not R.weight_is_exact(R.EMA, 5.0, True) and not R.weight_is_exact(R.SWA, 5.0, False)
    # start_step / every count completed optimizer steps; a skipped step is inactive; inactive keeps n and has w = 0
    act = [R.constants(2.0, start_step=3, every=2, t=t)["active"] for t in range(1, 9)]
    assert act == [False, False, True, False, True, False, True, False]
    assert R.constants(2.0, t=5, skip=True) == dict(w=0.0, active=False, copy=False, n_after=2.0)
    assert R.constants(2.0)["active"] and R.constants(2.0)["n_after"] == 3.0
    # the update: torch.lerp on f32 CPU tensors stays inside the two-rounding bound
    gen = torch.Generator().manual_seed(5)
    p, s = torch.randn(4099, generator=gen), torch.randn(4099, generator=gen)
    for w in (R.f32(1e-3), 1.0, R.f32(1.0 / 3.0)):
        ref, bound = R.update(p, s, w)
        assert bool(((torch.lerp(s, p, w).double() - ref).abs() <= bound).all())
    ref, bound = R.update(p, s, 0.5, copy=True)
    assert torch.equal(ref, p.double()) and not bound.any()


def test_schedule_restatement_against_torch_sequential_lr():
    """``warmup_prefix=True`` against ``SequentialLR(LinearLR, CosineAnnealingLR)`` at every step of the warm-up and of one
    cosine period (torch does not clamp behind it), two groups with different bases: |d| <= 1.1e-16."""
    from torch.optim.lr_scheduler import CosineAnnealingLR, LinearLR, SequentialLR

    bases, warmup, total, lr_min, factor = (1e-3, 2.5e-4), 5, 20, 1e-5, 0.1
    opt = torch.optim.SGD([dict(params=[torch.nn.Parameter(torch.zeros(1))], lr=b) for b in bases], lr=1.0)
    sched = SequentialLR(opt, [LinearLR(opt, start_factor=factor, end_factor=1.0, total_iters=warmup),
                               CosineAnnealingLR(opt, T_max=total, eta_min=lr_min)], milestones=[warmup])
    worst = 0.0
    for t in range(warmup + total + 1):
        for group, base in zip(opt.param_groups, bases):
            want = R.lr(t, base, warmup, total, lr_min, warmup_start=factor * base, warmup_prefix=True)
            worst = max(worst, abs(group["lr"] - want))
        opt.step()
        sched.step()
    print(f"closed form against SequentialLR: worst |d| = {worst:.3e}")
    assert worst <= 1.1e-16
    # behind the period the closed form stays at lr_min; without the prefix the cosine runs on t itself
    assert R.lr(warmup + total, 1e-3, warmup, total, lr_min, 0.0, True) == lr_min == R.lr(10 ** 6, 1e-3, warmup, total, lr_min)
    assert R.lr(0, 1e-3, warmup, total) == 0.0 and R.lr(0, 1e-3, 0, total) == 1e-3
    assert R.lr(warmup, 1e-3, warmup, total, 0.0, 0.0, False) == 0.5e-3 * (1.0 + R.math.cos(R.math.pi * warmup / total))
    assert R.lr(total, 1e-3, warmup, total, lr_min) == lr_min and R.lr(total, 1e-3, warmup, total, lr_min, 0.0, True) > lr_min


# ---------------------------------------------------------------- the C ABI
def _refused(fn, a, *needles):
    lib = _lib.load()
    st = fn(ctypes.byref(a) if a is not None else None, None)
    msg = lib.anemoi_last_error()
    assert st == _lib.ANEMOI_ERR_INVALID, (st, msg)
    for needle in needles:
        assert needle in msg, (needle, msg)


def _arr(ctype, values):
    return (ctype * len(values))(*values)


def _set(block, keep, fields):
    for k, v in fields.items():
        if isinstance(v, ctypes.Array):
            keep.append(v)
            v = ctypes.cast(v, ctypes.c_void_p)
        setattr(block, k, v)
    block._keep = keep
    return block


def _const_args(**fields):
    """Well-formed blocks over fake device pointers (never dereferenced: every refusal comes before any launch)."""
    c = _lib.AverageConstantsArgs()
    c.struct_bytes = ctypes.sizeof(_lib.AverageConstantsArgs)
    c.n_averaged, c.step, c.skip, c.avg = 4096, 4160, 4224, 4288
    c.decay, c.start_step, c.every, c.kind = 0.999, 0, 1, _lib.AVERAGE_EMA
    return _set(c, [], fields)


def _list_args(cls, names, **fields):
    a = cls()
    a.struct_bytes, a.n_tensors = ctypes.sizeof(cls), 2
    keep = [_arr(ctypes.c_int64, [5, 7])]
    a.numel = ctypes.cast(keep[0], ctypes.c_void_p)
    for name in names:
        keep.append(_arr(ctypes.c_void_p, [4096, 8192]))
        setattr(a, name, ctypes.cast(keep[-1], ctypes.c_void_p))
    if cls is _lib.MultiAverageArgs:
        a.avg = 4096
    return _set(a, keep, fields)


def _lr_args(n=2, **fields):
    s = _lib.LrScheduleArgs()
    s.struct_bytes, s.n_groups = ctypes.sizeof(_lib.LrScheduleArgs), n
    m = max(n, 2)
    base = dict(step=_arr(ctypes.c_void_p, [4096 + 64 * i for i in range(m)]),
                lr=_arr(ctypes.c_void_p, [8192 + 64 * i for i in range(m)]),
                base=_arr(ctypes.c_double, [1e-3] * m), lr_min=_arr(ctypes.c_double, [0.0] * m),
                warmup_start=_arr(ctypes.c_double, [0.0] * m), warmup_steps=_arr(ctypes.c_int64, [5] * m),
                total_steps=_arr(ctypes.c_int64, [20] * m), warmup_prefix=_arr(ctypes.c_int32, [0] * m))
    base.update(fields)
    return _set(s, [], base)


def test_abi_version_and_struct_sizes():
    lib = _lib.load()
    assert lib.anemoi_abi_version() == _lib.ABI_VERSION == 55
    assert ctypes.sizeof(_lib.AverageConstantsArgs) == 72 and ctypes.sizeof(_lib.MultiAverageArgs) == 48
    assert ctypes.sizeof(_lib.MultiSwapArgs) == 40 and ctypes.sizeof(_lib.LrScheduleArgs) == 80
    # the v54 blocks keep their layout
    assert ctypes.sizeof(_lib.MultiTensorArgs) == 120 and ctypes.sizeof(_lib.AdamwConstantsArgs) == 104


def test_average_constants_refuses_bad_arguments_before_any_launch():
    fn = _lib.load().anemoi_average_constants
    _refused(fn, None, b"anemoi_average_constants", b"null argument block")
    _refused(fn, _const_args(struct_bytes=8), b"out of sync")
    _refused(fn, _const_args(n_averaged=None), b"null pointer (n_averaged)")
    _refused(fn, _const_args(avg=None), b"null pointer (avg)")
    _refused(fn, _const_args(kind=2), b"kind 2")
    for bad in (1.0, -0.1, 1.5, float("nan")):
        _refused(fn, _const_args(decay=bad), b"decay")
    _refused(fn, _const_args(every=0), b"every = 0 < 1")
    _refused(fn, _const_args(start_step=-1), b"start_step = -1 < 0")


def test_list_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    for name, cls, fields in (("anemoi_multi_average", _lib.MultiAverageArgs, ("params", "shadow")),
                              ("anemoi_multi_swap", _lib.MultiSwapArgs, ("a", "b"))):
        fn, who = getattr(lib, name), name.encode()
        _refused(fn, None, who, b"null argument block")
        _refused(fn, _list_args(cls, fields, struct_bytes=ctypes.sizeof(cls) - 8), who, b"out of sync")
        _refused(fn, _list_args(cls, fields, n_tensors=-1), who, b"negative n_tensors")
        _refused(fn, _list_args(cls, fields, numel=None), who, b"null pointer (numel)")
        _refused(fn, _list_args(cls, fields, numel=_arr(ctypes.c_int64, [5, -7])), who, b"negative numel[1]")
        for field in fields:
            _refused(fn, _list_args(cls, fields, **{field: None}), who, b"null pointer (" + field.encode() + b")")
            _refused(fn, _list_args(cls, fields, **{field: _arr(ctypes.c_void_p, [4096, None])}), who,
                     b"null pointer (" + field.encode() + b"[1])")
        # an empty list, and a list of empty tensors with null pointers, launch nothing (no GPU needed)
        assert fn(ctypes.byref(_list_args(cls, fields, n_tensors=0)), None) == _lib.ANEMOI_OK
        empty = {f: _arr(ctypes.c_void_p, [None, None]) for f in fields}
        assert fn(ctypes.byref(_list_args(cls, fields, numel=_arr(ctypes.c_int64, [0, 0]), **empty)), None) == _lib.ANEMOI_OK
    _refused(lib.anemoi_multi_average, _list_args(_lib.MultiAverageArgs, ("params", "shadow"), avg=None), b"null pointer (avg)")


def test_lr_schedule_refuses_bad_arguments_before_any_launch():
    fn = _lib.load().anemoi_lr_schedule
    _refused(fn, None, b"anemoi_lr_schedule", b"null argument block")
    _refused(fn, _lr_args(struct_bytes=8), b"out of sync")
    _refused(fn, _lr_args(n_groups=-1), b"negative n_groups")
    _refused(fn, _lr_args(n=_lib.LR_MAX_GROUPS + 1), b"n_groups = 33, at most 32")
    for field in ("step", "lr", "base", "lr_min", "warmup_start", "warmup_steps", "total_steps", "warmup_prefix"):
        _refused(fn, _lr_args(**{field: None}), b"null pointer (step / lr / base")
    _refused(fn, _lr_args(step=_arr(ctypes.c_void_p, [4096, None])), b"null pointer (step[1])")
    _refused(fn, _lr_args(lr=_arr(ctypes.c_void_p, [None, 4096])), b"null pointer (lr[0])")
    _refused(fn, _lr_args(base=_arr(ctypes.c_double, [1e-3, -1e-3])), b"base[1]")
    _refused(fn, _lr_args(lr_min=_arr(ctypes.c_double, [-1e-9, 0.0])), b"lr_min[0]")
    _refused(fn, _lr_args(warmup_start=_arr(ctypes.c_double, [0.0, -1.0])), b"warmup_start[1]")
    _refused(fn, _lr_args(warmup_steps=_arr(ctypes.c_int64, [-1, 5])), b"warmup_steps[0] = -1 < 0")
    _refused(fn, _lr_args(total_steps=_arr(ctypes.c_int64, [20, 0])), b"total_steps[1] = 0 < 1")
    assert fn(ctypes.byref(_lr_args(n=0)), None) == _lib.ANEMOI_OK  # no group: nothing is launched


# ---------------------------------------------------------------- the classes
def test_weight_averager_refusals():
    w = torch.nn.Parameter(torch.zeros(4))
    for kw in (dict(decay=1.0), dict(decay=-0.1), dict(every=0), dict(every=1.5), dict(start_step=-1), dict(kind="mean")):
        with pytest.raises(ValueError):
            optim.WeightAverager([w], **kw)
    with pytest.raises(ValueError, match="no parameters"):
        optim.WeightAverager([])
    with pytest.raises(NotImplementedError, match="parameter 0 is torch.float32 on cpu"):
        optim.WeightAverager([w])
    with pytest.raises(NotImplementedError, match="parameter 0 is torch.bfloat16"):
        optim.WeightAverager([torch.nn.Parameter(torch.zeros(4, dtype=torch.bfloat16))])
    with pytest.raises(NotImplementedError, match=r"parameter 0 is torch.float32 on cpu \(not contiguous\)"):
        optim.WeightAverager([torch.zeros(4, 6).t()])
    with pytest.raises(NotImplementedError, match="parameter 0 is torch.float32 on cpu"):
        optim.WeightAverager(optim.FusedAdamW([w]))  # through the optimizer's groups
    with pytest.raises(NotImplementedError, match="device step counter"):
        optim.WeightAverager(torch.optim.AdamW([w]))


def test_device_lr_schedule_refusals():
    w = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(NotImplementedError, match="FusedAdamW"):
        optim.DeviceLRSchedule(torch.optim.AdamW([w]), warmup_steps=1, total_steps=2)
    opt = optim.FusedAdamW([w])
    for kw in (dict(warmup_steps=-1, total_steps=2), dict(warmup_steps=1, total_steps=0), dict(warmup_steps=1.5, total_steps=2),
               dict(warmup_steps=1, total_steps=2, lr_min=-1e-6), dict(warmup_steps=1, total_steps=2, warmup_start=-1.0)):
        with pytest.raises(ValueError):
            optim.DeviceLRSchedule(opt, **kw)
    many = optim.FusedAdamW([dict(params=[torch.nn.Parameter(torch.zeros(1))]) for _ in range(_lib.LR_MAX_GROUPS + 1)])
    with pytest.raises(ValueError, match="at most 32"):
        optim.DeviceLRSchedule(many, warmup_steps=1, total_steps=2)
    assert opt.param_groups[0]["lr"] == 1e-3 and isinstance(opt.param_groups[0]["lr"], float)  # a refusal changes nothing
    assert opt.skip_flag is None
