"""The optimizer step without a GPU: the f64 restatement (tests/_optim_ref.py) against torch.optim.AdamW +
torch.nn.utils.clip_grad_norm_, the argument checks of the multi-tensor entry points through the C ABI, the workspace query
against the chunking rule, the struct_bytes handshake and the state_dict layout of ``optim.FusedAdamW``."""

import ctypes

import pytest
import torch

import _optim_ref as R
from anemoi_models_amd import _lib
from anemoi_models_amd import optim


def test_restatement_against_torch_adamw_in_f64():
    """Five steps, weight decay 0.1, betas (0.9, 0.95), gradients alternating between a clipped and an unclipped scale, one
    empty tensor: |dp| <= 1e-12 (|p| + lr), norms equal to rounding."""
    shapes, lr, betas, eps, wd, max_norm = [(1,), (3,), (7, 5), (4097,), (0,)], 1e-3, (0.9, 0.95), 1e-8, 0.1, 1.0
    gen = torch.Generator().manual_seed(11)
    init = [torch.randn(s, generator=gen, dtype=torch.float64) for s in shapes]
    tp = [torch.nn.Parameter(t.clone()) for t in init]
    opt = torch.optim.AdamW(tp, lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
    p = [t.clone() for t in init]
    m, v, steps = [torch.zeros_like(t) for t in p], [torch.zeros_like(t) for t in p], [0]
    groups = [(list(range(len(p))), dict(lr=lr, betas=betas, eps=eps, weight_decay=wd))]
    clipped = []
    for k in range(5):
        scale = 10.0 if k % 2 == 0 else 1e-3  # norm ~ 640 (clipped) / 0.064 (not)
        grads = [scale * torch.randn(s, generator=gen, dtype=torch.float64) for s in shapes]
        for t, g in zip(tp, grads):
            t.grad = g.clone()
        want_norm = torch.nn.utils.clip_grad_norm_(tp, max_norm)
        opt.step()
        c = R.step_f64(p, grads, m, v, steps, groups, max_norm=max_norm)
        clipped.append(c["clip"] < 1.0)
        assert abs(c["norm"] - float(want_norm)) <= 4 * 2.0 ** -53 * float(want_norm)
        for a, b in zip(p, tp):
            assert bool(((a - b.detach()).abs() <= 1e-12 * (b.detach().abs() + lr)).all())
    assert clipped == [True, False, True, False, True] and steps == [5]


def test_constants_and_depth_match_the_library():
    lib = _lib.load()
    assert _lib.ABI_VERSION >= 54
    assert lib.anemoi_multi_tensor_max_tensors() == _lib.OPT_MAX_TENSORS
    assert lib.anemoi_multi_tensor_chunk() == _lib.OPT_CHUNK and _lib.OPT_CHUNK % 1024 == 0
    assert R.sumsq_depth(_lib.OPT_CHUNK, 1) == R.sumsq_depth(_lib.OPT_CHUNK, 10 ** 6) == _lib.OPT_SUMSQ_DEPTH
    assert max(R.N_M, R.N_V, R.N_P) <= 8


def _numel(values):
    return (ctypes.c_int64 * len(values))(*values)


def test_workspace_query_follows_the_chunking_rule():
    """One float per (tensor, chunk): a function of the list of lengths alone; empty tensors have no chunk."""
    lib, c = _lib.load(), _lib.OPT_CHUNK
    numels = [1, 3, 4, c - 1, c, c + 1, 2 * c + 5, 0, 10 * c]
    want = [1, 1, 1, 1, 1, 2, 3, 0, 10]
    for n, w in zip(numels, want):
        assert lib.anemoi_multi_sumsq_workspace_floats(ctypes.cast(_numel([n]), ctypes.c_void_p), 1) == w
    arr = _numel(numels)
    assert lib.anemoi_multi_sumsq_workspace_floats(ctypes.cast(arr, ctypes.c_void_p), len(numels)) == sum(want)
    assert sum(want) == R.n_chunks(numels, c)
    assert lib.anemoi_multi_sumsq_workspace_floats(None, 3) == 0
    assert lib.anemoi_multi_sumsq_workspace_floats(ctypes.cast(arr, ctypes.c_void_p), 0) == 0
    from anemoi_models_amd import ops

    assert ops.multi_tensor_chunks(numels) == sum(want)


def _list_args(n=2, lengths=(5, 7), **fields):
    """A well-formed block over fake (never dereferenced: every refusal comes before any launch) device pointers."""
    a = _lib.MultiTensorArgs()
    a.struct_bytes, a.n_tensors = ctypes.sizeof(_lib.MultiTensorArgs), n
    keep = [_numel(list(lengths))]
    a.numel = ctypes.cast(keep[0], ctypes.c_void_p)
    for name in ("params", "grads", "exp_avg", "exp_avg_sq"):
        keep.append((ctypes.c_void_p * len(lengths))(*[4096 + 64 * i for i in range(len(lengths))]))
        setattr(a, name, ctypes.cast(keep[-1], ctypes.c_void_p))
    a.workspace, a.workspace_floats, a.sumsq, a.consts, a.coef = 4096, 16, 4096, 4096, 4096
    a.beta1, a.beta2, a.eps = 0.9, 0.95, 1e-8
    for k, val in fields.items():
        if isinstance(val, ctypes.Array):
            keep.append(val)
            val = ctypes.cast(val, ctypes.c_void_p)
        setattr(a, k, val)
    a._keep = keep
    return a


def _refused(fn, a, *needles):
    lib = _lib.load()
    st = fn(ctypes.byref(a) if a is not None else None, None)
    msg = lib.anemoi_last_error()
    assert st == _lib.ANEMOI_ERR_INVALID, (st, msg)
    for needle in needles:
        assert needle in msg, (needle, msg)


def test_list_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    entries = {"anemoi_multi_sumsq": lib.anemoi_multi_sumsq, "anemoi_multi_adamw": lib.anemoi_multi_adamw,
               "anemoi_multi_scale": lib.anemoi_multi_scale}
    for name, fn in entries.items():
        who = name.encode()
        _refused(fn, None, who, b"null argument block")
        _refused(fn, _list_args(struct_bytes=ctypes.sizeof(_lib.MultiTensorArgs) - 8), who, b"out of sync")  # the handshake
        _refused(fn, _list_args(n_tensors=-1), who, b"negative n_tensors")
        _refused(fn, _list_args(numel=None), who, b"null pointer (numel)")
        _refused(fn, _list_args(numel=_numel([5, -7])), who, b"negative numel[1]")
        _refused(fn, _list_args(grads=None), who, b"null pointer (grads)")
        _refused(fn, _list_args(grads=(ctypes.c_void_p * 2)(4096, None)), who, b"null pointer (grads[1])")
    for field in ("params", "exp_avg", "exp_avg_sq"):
        _refused(lib.anemoi_multi_adamw, _list_args(**{field: None}), b"null pointer (" + field.encode() + b")")
        _refused(lib.anemoi_multi_adamw, _list_args(**{field: (ctypes.c_void_p * 2)(None, 4096)}),
                 b"null pointer (" + field.encode() + b"[0])")
    _refused(lib.anemoi_multi_sumsq, _list_args(sumsq=None), b"null pointer (sumsq)")
    _refused(lib.anemoi_multi_sumsq, _list_args(workspace_floats=1), b"workspace of 1 floats, 2 needed")
    _refused(lib.anemoi_multi_sumsq, _list_args(workspace=None), b"workspace")
    _refused(lib.anemoi_multi_adamw, _list_args(consts=None), b"null pointer (consts)")
    _refused(lib.anemoi_multi_adamw, _list_args(beta1=1.0), b"beta1")
    _refused(lib.anemoi_multi_adamw, _list_args(beta1=-0.1), b"beta1")
    _refused(lib.anemoi_multi_adamw, _list_args(beta2=1.5), b"beta2")
    _refused(lib.anemoi_multi_adamw, _list_args(eps=-1e-8), b"eps")
    _refused(lib.anemoi_multi_scale, _list_args(coef=None), b"null pointer (coef)")
    # a tensor of numel 0 may have null pointers; an empty list launches nothing (the update and the scale: no GPU needed)
    assert lib.anemoi_multi_adamw(ctypes.byref(_list_args(n_tensors=0)), None) == _lib.ANEMOI_OK
    assert lib.anemoi_multi_scale(ctypes.byref(_list_args(n_tensors=0)), None) == _lib.ANEMOI_OK


def _const_args(n=2, **fields):
    c = _lib.AdamwConstantsArgs()
    c.struct_bytes, c.n_groups = ctypes.sizeof(_lib.AdamwConstantsArgs), n
    fa = ctypes.c_double * 2
    keep = dict(step=(ctypes.c_void_p * 2)(4096, 4160), lr_dev=(ctypes.c_void_p * 2)(None, None), lr=fa(1e-3, 1e-3),
                beta1=fa(0.9, 0.9), beta2=fa(0.95, 0.95), weight_decay=fa(0.1, 0.0))
    keep.update({k: v for k, v in fields.items() if isinstance(v, ctypes.Array)})
    for k, v in keep.items():
        setattr(c, k, ctypes.cast(v, ctypes.c_void_p))
    c.sumsq, c.skipped, c.consts, c.max_norm, c.has_max_norm = 4096, 4096, 4096, 1.0, 1
    for k, v in fields.items():
        if not isinstance(v, ctypes.Array):
            setattr(c, k, v)
    c._keep = keep
    return c


def test_constants_entry_point_refuses_bad_arguments_before_any_launch():
    fn, fa = _lib.load().anemoi_adamw_constants, ctypes.c_double * 2
    _refused(fn, None, b"anemoi_adamw_constants", b"null argument block")
    _refused(fn, _const_args(struct_bytes=8), b"out of sync")
    _refused(fn, _const_args(n_groups=-2), b"negative n_groups")
    _refused(fn, _const_args(consts=None), b"null pointer (consts)")
    _refused(fn, _const_args(sumsq=None), b"max_norm without sumsq")
    _refused(fn, _const_args(sumsq=None, has_max_norm=0, skip_nonfinite=1), b"skip_nonfinite without sumsq")
    _refused(fn, _const_args(max_norm=-1.0), b"max_norm")
    _refused(fn, _const_args(step=None), b"null pointer (step")
    _refused(fn, _const_args(step=(ctypes.c_void_p * 2)(4096, None)), b"null pointer (step[1])")
    _refused(fn, _const_args(beta1=fa(0.9, 1.0)), b"beta1[1]")
    _refused(fn, _const_args(beta2=fa(-0.5, 0.9)), b"beta2[0]")
    _refused(fn, _const_args(lr=fa(1e-3, -1e-3)), b"lr[1]")
    _refused(fn, _const_args(weight_decay=fa(-0.1, 0.0)), b"weight_decay[0]")


def test_python_wrappers_refuse_what_the_kernels_do_not_take():
    w = torch.nn.Parameter(torch.zeros(4))
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(differentiable=True)):
        with pytest.raises(NotImplementedError):
            optim.FusedAdamW([w], **kw)
    for kw in (dict(lr=-1.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1)), dict(eps=-1.0), dict(weight_decay=-1.0),
               dict(max_grad_norm=-1.0)):
        with pytest.raises(ValueError):
            optim.FusedAdamW([w], **kw)
    optim.FusedAdamW([w], foreach=True, fused=True, capturable=True)  # accepted and ignored
    w.grad = torch.ones(4)
    with pytest.raises(NotImplementedError, match="parameter 0 is torch.float32 on cpu"):
        optim.FusedAdamW([w]).step()
    with pytest.raises(NotImplementedError, match="2-norm"):
        optim.clip_grad_norm_([w], 1.0, norm_type=1.0)
    with pytest.raises(NotImplementedError, match="error_if_nonfinite"):
        optim.clip_grad_norm_([w], 1.0, error_if_nonfinite=True)
    with pytest.raises(NotImplementedError, match="gradient 0"):
        optim.clip_grad_norm_([w], 1.0)


def test_state_dict_layout_is_torch_adamws():
    """Keys and shapes only (``FusedAdamW.step`` has no CPU form): group keys, per-parameter state keys and shapes against a
    torch.optim.AdamW that has stepped once on the same CPU parameters; and the refusal of a dict whose parameters of one
    group disagree on ``step``."""
    ps = [torch.nn.Parameter(torch.randn(3, 4)), torch.nn.Parameter(torch.randn(5))]
    kw = dict(lr=2e-3, betas=(0.9, 0.95), eps=1e-7, weight_decay=0.1)
    ref = torch.optim.AdamW([dict(params=[ps[0]]), dict(params=[ps[1]], lr=1e-4)], **kw)
    for p in ps:
        p.grad = torch.ones_like(p)
    ref.step()
    ours = optim.FusedAdamW([dict(params=[ps[0]]), dict(params=[ps[1]], lr=1e-4)], max_grad_norm=1.0, **kw)
    ours.init_state()
    a, b = ours.state_dict(), ref.state_dict()
    assert a.keys() == b.keys() and len(a["param_groups"]) == len(b["param_groups"]) == 2
    for ga, gb in zip(a["param_groups"], b["param_groups"]):
        assert ga.keys() == gb.keys() and ga["params"] == gb["params"]
        assert (ga["lr"], ga["betas"], ga["eps"], ga["weight_decay"]) == (gb["lr"], gb["betas"], gb["eps"], gb["weight_decay"])
    assert a["state"].keys() == b["state"].keys()
    for k in b["state"]:
        assert a["state"][k].keys() == b["state"][k].keys() == {"step", "exp_avg", "exp_avg_sq"}
        for name in b["state"][k]:
            assert a["state"][k][name].shape == b["state"][k][name].shape and a["state"][k][name].dtype == torch.float32
    assert a["state"][0]["step"] is not ours.state[ps[0]]["step"]  # a copy per parameter, as torch writes them
    # torch's dict loads; state[p]["step"] then reads the group's counter
    ours.load_state_dict(b)
    assert float(ours.state[ps[0]]["step"]) == 1.0 and ours.state[ps[0]]["step"] is ours.step_count
    assert torch.equal(ours.state[ps[1]]["exp_avg"], ref.state[ps[1]]["exp_avg"])
    ref.load_state_dict(ours.state_dict())  # and the reverse
    # parameters of one group that disagree on `step`
    both = optim.FusedAdamW(ps, **kw)
    other = torch.optim.AdamW(ps, **kw)
    other.step()
    ps[1].grad = None
    other.step()  # ps[0] has stepped twice, ps[1] once
    with pytest.raises(ValueError, match="disagree on `step`"):
        both.load_state_dict(other.state_dict())
