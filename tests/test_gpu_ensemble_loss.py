"""The ensemble scores on the HIP kernels (csrc/ensemble.hip): anemoi_ensemble_score / _backward, autograd.ensemble_score,
AlmostFairKernelCRPS / KernelCRPS and EnsembleMetrics against the plain-torch restatement of tests/_ensemble_ref.py in float64,
at the smallest shapes at which the column layout of the reduction and the member stride can go wrong.

Bounds (those of tests/test_gpu_loss_family.py, per output element): forward -- relative error against the f64 restatement at
most 4 x that of the restatement evaluated in f32 on the CPU, or 2e-6 if that is larger; where the reference is exactly 0 the
result is exactly 0; gradient -- at most 1e-6 of max |dpred|.  The f64 reference is given the f32 inputs cast up, so every sgn
of the gradient agrees exactly."""

import functools
import warnings

import numpy as np
import pytest
import torch

import _ensemble_ref as er
import _rollout_ref as rr
from conftest import split_prefix

pytestmark = pytest.mark.gpu

DEV = "cuda"
# (G, V, B, n_groups, E); points per group = B * G.  E is a template argument of the kernels from 2 to 16: there is no seam
# between a small-E and a generic route, every E is its own instantiation -- 2, 3, 4, 5, 8, 9 and 16 are launched here.
SHAPES = [
    (1, 1, 1, 1, 2),       # the smallest case
    (257, 5, 2, 3, 3),     # an idle lane (51 row lanes x 5 < 256); row weights wrap inside a group; a chunk tail; B > 1
    (2062, 80, 1, 2, 4),   # three row lanes, 41 workgroups per group
    (33, 257, 1, 1, 9),    # crosses the column tile of 256
    (1031, 256, 1, 1, 8),  # exactly one row per pass
    (5000, 3, 1, 4, 16),   # the largest E; several workgroups per group
    (257, 5, 1, 1, 5),     # a middle E
]
IDS = [f"G{g}-V{v}-B{b}-L{n}-E{e}" for g, v, b, n, e in SHAPES]
KIND_ALPHA = [("afcrps", 1.0), ("afcrps", 0.95), ("afcrps", 0.0), ("mean_se", 1.0), ("variance", 1.0)]
KA_IDS = ["afcrps-a1", "afcrps-a095", "afcrps-a0", "mean_se", "variance"]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def _case(shape, masked, scaled):
    """Inputs on the CPU (never modified).  Members = target + N(0, 0.7^2) per member with one element in eight uniform in
    [-100, 100]; 3 % of the member-target pairs and 3 % of the pairs of neighbouring members are exactly equal; with a mask, at
    most 10 % of [G, V] is masked, the target is NaN there and member 0 Inf at half of those positions."""
    g, v, b, n_groups, e = shape
    gen = _gen(1000 * g + 10 * v + 100 * e + 2 * masked + scaled)
    full = (n_groups, b, e, g, v)
    target = torch.randn((n_groups, b, g, v), generator=gen)
    d = 0.7 * torch.randn(full, generator=gen)
    d = torch.where(torch.rand(full, generator=gen) < 0.125, 200.0 * torch.rand(full, generator=gen) - 100.0, d)
    pred = torch.where(torch.rand(full, generator=gen) < 0.03, target.unsqueeze(2).expand(full), target.unsqueeze(2) + d)
    same = torch.rand(full, generator=gen) < 0.03
    for j in range(1, e):
        pred[:, :, j] = torch.where(same[:, :, j], pred[:, :, j - 1], pred[:, :, j])
    if g * v == 1:  # one point: no ties, the target outside the members (the fair CRPS of a target between two members is 0)
        pred = target.unsqueeze(2) + 1.75 + 0.5 * torch.arange(e, dtype=torch.float32).reshape(1, 1, e, 1, 1)
    else:
        assert bool((pred == target.unsqueeze(2)).any()) and bool((pred[:, :, 1:] == pred[:, :, :-1]).any())
    row_w = torch.rand(g, generator=gen) + 0.1
    col_w = torch.rand(v, generator=gen) + 0.5
    c = (0.1 + 9.9 * torch.rand(v, generator=gen)) if scaled else None
    mask = None
    if masked:
        mask = (torch.rand((g, v), generator=gen) > 0.08).float()
        if g * v == 1:
            mask[:] = 1.0
        target = torch.where(mask != 0, target, torch.full((), float("nan")))
        pred = pred.clone()
        pred[:, :, 0] = torch.where((mask == 0) & (torch.rand((g, v), generator=gen) < 0.5), torch.full((), float("inf")),
                                    pred[:, :, 0])
    upstream = torch.randn((n_groups, v), generator=gen)
    return dict(pred=pred, target=target, row_w=row_w, col_w=col_w, c=c, mask=mask, upstream=upstream, n_groups=n_groups,
                scale=1.0 / b)


def _d64(t):
    return None if t is None else t.double()


@functools.lru_cache(maxsize=None)
def _reference(shape, masked, scaled, kind, alpha):
    """(out f64, out of the f32 CPU evaluation) of the restatement."""
    cs = _case(shape, masked, scaled)
    with torch.no_grad():
        out = er.ensemble_score(cs["pred"].double(), cs["target"].double(), cs["row_w"].double(), kind, alpha,
                                _d64(cs["col_w"]), cs["mask"], _d64(cs["c"]), cs["n_groups"], cs["scale"])
        cpu32 = er.ensemble_score(cs["pred"], cs["target"], cs["row_w"], kind, alpha, cs["col_w"], cs["mask"], cs["c"],
                                  cs["n_groups"], cs["scale"])
    return out, cpu32


@functools.lru_cache(maxsize=None)
def _reference_grad(shape, masked, scaled, alpha):
    """dpred f64 for the case's upstream: autograd of the restatement."""
    cs = _case(shape, masked, scaled)
    p64 = cs["pred"].double().requires_grad_()
    out = er.ensemble_score(p64, cs["target"].double(), cs["row_w"].double(), "afcrps", alpha, _d64(cs["col_w"]), cs["mask"],
                            _d64(cs["c"]), cs["n_groups"], cs["scale"])
    (out * cs["upstream"].double()).sum().backward()
    return p64.grad


def _dev(cs):
    return {k: (t.to(DEV) if isinstance(t, torch.Tensor) else t) for k, t in cs.items()}


def _kernel_kwargs(cs, alpha):
    return dict(alpha=alpha, col_w=cs["col_w"], mask=cs["mask"], diff_scale=cs["c"], n_groups=cs["n_groups"], scale=cs["scale"])


def _forward_errors(got, ref64, cpu32):
    """Per output element: (error of the kernel, its bound), both relative to |ref|; where ref is 0 the kernel gives 0."""
    got, cpu32 = got.double().cpu(), cpu32.double()
    zero = ref64 == 0
    assert bool((got[zero] == 0).all())
    den = torch.where(zero, torch.ones_like(ref64), ref64.abs())
    err, err_cpu = (got - ref64).abs() / den, (cpu32 - ref64).abs() / den
    return err, torch.clamp(4 * err_cpu, min=2e-6)


@pytest.mark.parametrize("scaled", [False, True], ids=["c1", "c"])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("kind,alpha", KIND_ALPHA, ids=KA_IDS)
def test_ensemble_score_forward_vs_f64(kind, alpha, shape, masked, scaled):
    from anemoi_models_amd import autograd, ops

    cs, (ref64, cpu32) = _case(shape, masked, scaled), _reference(shape, masked, scaled, kind, alpha)
    d = _dev(cs)
    got = autograd.ensemble_score(d["pred"], d["target"], d["row_w"], kind, **_kernel_kwargs(d, alpha))
    assert got.dtype == torch.float32 and tuple(got.shape) == (cs["n_groups"], shape[1]) and bool(torch.isfinite(got).all())
    err, bound = _forward_errors(got, ref64, cpu32)
    print(f"ensemble_score {kind} alpha={alpha} G={shape[0]} V={shape[1]} B={shape[2]} groups={shape[3]} E={shape[4]} "
          f"masked={masked} scaled={scaled}: worst rel err {float(err.max()):.3e} (f32 CPU "
          f"{float(((cpu32.double() - ref64).abs() / ref64.abs().clamp(min=1e-300)).max()):.3e}), "
          f"worst err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    # the op underneath, on the flattened rows, is the same call
    v = shape[1]
    flat = ops.ensemble_score(d["pred"].view(-1, v), d["target"].view(-1, v), d["row_w"], kind, n_members=shape[4],
                              **_kernel_kwargs(d, alpha))
    assert torch.equal(flat, got)


def _check_backward(shape, masked, scaled, alpha):
    from anemoi_models_amd import autograd

    cs, want = _case(shape, masked, scaled), _reference_grad(shape, masked, scaled, alpha)
    d = _dev(cs)
    pd = d["pred"].clone().requires_grad_()
    out = autograd.ensemble_score(pd, d["target"], d["row_w"], "afcrps", **_kernel_kwargs(d, alpha))
    out.backward(d["upstream"])
    got = pd.grad.cpu()
    assert got.shape == want.shape and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    top = float(want.abs().max())
    gerr = float((got.double() - want).abs().max()) / top
    print(f"ensemble_score_backward alpha={alpha} G={shape[0]} V={shape[1]} groups={shape[3]} E={shape[4]} masked={masked} "
          f"scaled={scaled}: gradient err {gerr:.3e} of max |dpred|")
    assert gerr <= 1e-6
    if masked:
        assert bool((got[..., cs["mask"] == 0] == 0).all())
        assert shape[0] * shape[1] == 1 or bool((got[..., cs["mask"] != 0] != 0).any())
    # a member that equals the target: its target term is exactly absent -- the closed form without that term
    same = cs["pred"] == cs["target"].unsqueeze(2)
    if shape[0] * shape[1] > 1:
        assert int(same.sum()) > 0
        no_y = er.closed_form_grad(cs["pred"].double(), cs["target"].double(), cs["row_w"].double(), cs["upstream"].double(),
                                   alpha, _d64(cs["col_w"]), cs["mask"], _d64(cs["c"]), cs["n_groups"], cs["scale"],
                                   target_term=False)
        assert float((got.double()[same] - no_y[same]).abs().max()) <= 1e-6 * top
        # two members that are equal and differ from the target receive the same gradient, bit for bit
        twin = (cs["pred"][:, :, 1:] == cs["pred"][:, :, :-1])
        assert torch.equal(got[:, :, 1:][twin], got[:, :, :-1][twin])


@pytest.mark.parametrize("scaled", [False, True], ids=["c1", "c"])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_ensemble_score_backward_vs_f64(shape, masked, scaled):
    """dpred (alpha = 0.95) for a random upstream [n_groups, V] against f64 autograd of the restatement; exactly 0 under the
    mask (NaN targets, Inf members there); where a member equals the target, the closed form without its target term."""
    _check_backward(shape, masked, scaled, 0.95)


@pytest.mark.parametrize("alpha", [1.0, 0.0])
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=[IDS[1], IDS[3]])
def test_ensemble_score_backward_at_the_ends_of_alpha(shape, alpha):
    _check_backward(shape, True, True, alpha)


def test_ensemble_score_is_deterministic_and_groups_are_independent():
    """Forward and backward twice: equal bits.  n_groups = 3 over a stacked tensor: group by group the bits of three
    n_groups = 1 calls on the slices -- a workgroup never straddles two groups.  A bf16 pred gives the bits of its .float()
    copy.  No rows: zeros.  CPU tensors, E = 1 and E = 17: refused."""
    from anemoi_models_amd import autograd, ops

    shape = SHAPES[1]
    v, e = shape[1], shape[4]
    for kind, alpha in KIND_ALPHA[1:]:
        for masked in (False, True):
            d = _dev(_case(shape, masked, True))
            kw = dict(_kernel_kwargs(d, alpha), n_members=e)
            p2, t2 = d["pred"].view(-1, v), d["target"].view(-1, v)
            out = ops.ensemble_score(p2, t2, d["row_w"], kind, **kw)
            assert torch.equal(ops.ensemble_score(p2, t2, d["row_w"], kind, **kw), out)
            grad = None
            if kind == "afcrps":
                grad = ops.ensemble_score_backward(p2, t2, d["row_w"], kind, upstream=d["upstream"], **kw)
                assert torch.equal(ops.ensemble_score_backward(p2, t2, d["row_w"], kind, upstream=d["upstream"], **kw), grad)
            else:
                with pytest.raises(NotImplementedError, match="only ANEMOI_ENS_AFCRPS has a gradient"):
                    ops.ensemble_score_backward(p2, t2, d["row_w"], kind, upstream=d["upstream"], **kw)
            kw1 = dict(kw, n_groups=1)
            rt, rp = t2.shape[0] // 3, p2.shape[0] // 3
            for l in range(3):
                ps, ts = p2[l * rp:(l + 1) * rp], t2[l * rt:(l + 1) * rt]
                assert torch.equal(ops.ensemble_score(ps, ts, d["row_w"], kind, **kw1), out[l:l + 1]), (kind, l)
                if grad is not None:
                    gs = ops.ensemble_score_backward(ps, ts, d["row_w"], kind, upstream=d["upstream"][l:l + 1].contiguous(),
                                                     **kw1)
                    assert torch.equal(gs, grad[l * rp:(l + 1) * rp]), (kind, l)
            # any float dtype is taken to f32
            pb = d["pred"].bfloat16()
            akw = _kernel_kwargs(d, alpha)
            assert torch.equal(autograd.ensemble_score(pb, d["target"], d["row_w"], kind, **akw),
                               autograd.ensemble_score(pb.float(), d["target"], d["row_w"], kind, **akw))
    w = torch.ones(4, device=DEV)
    for kind in er.KINDS:
        assert ops.ensemble_score(torch.zeros((0, 3), device=DEV), torch.zeros((0, 3), device=DEV), w, kind, n_members=3,
                                  n_groups=2).tolist() == [[0.0] * 3] * 2
        with pytest.raises(RuntimeError, match="CPU tensor"):
            ops.ensemble_score(torch.zeros(8, 3), torch.zeros(4, 3), torch.ones(4), kind, n_members=2)
        with pytest.raises(ValueError, match="at least 2 members"):
            ops.ensemble_score(torch.zeros((4, 3), device=DEV), torch.zeros((4, 3), device=DEV), w, kind, n_members=1)
        with pytest.raises(NotImplementedError, match="at most 16"):
            ops.ensemble_score(torch.zeros((68, 3), device=DEV), torch.zeros((4, 3), device=DEV), w, kind, n_members=17)
    with pytest.raises(ValueError, match="at least 2 members"):
        autograd.ensemble_score(torch.zeros((1, 4, 3), device=DEV), torch.zeros((4, 3), device=DEV), w)
    with pytest.raises(NotImplementedError, match="at most 16"):
        autograd.ensemble_score(torch.zeros((17, 4, 3), device=DEV), torch.zeros((4, 3), device=DEV), w)


# --------------------------------------------------------------------------------------------------- the modules
@pytest.mark.parametrize("lead_dims", [0, 1])
@pytest.mark.parametrize("squash", [True, False])
@pytest.mark.parametrize("name,kw,alpha", [("AlmostFairKernelCRPS", dict(alpha=0.95), 0.95), ("KernelCRPS", dict(fair=False), 0.0)],
                         ids=["afcrps", "kernel-crps-unfair"])
def test_ensemble_loss_classes_vs_restatement(name, kw, alpha, squash, lead_dims):
    """Both classes on a [3, 2, 3, 257, 5] rollout result with a mask over NaN targets: value (forward bound, per element) and
    gradient (1e-6 of max |dpred|) against the f64 restatement."""
    import anemoi_models_amd

    cs = _case(SHAPES[1], True, False)
    pred, target = cs["pred"], cs["target"]
    assert tuple(pred.shape) == (3, 2, 3, 257, 5) and tuple(target.shape) == (3, 2, 257, 5)
    loss_fn = getattr(anemoi_models_amd, name)(cs["row_w"], cs["col_w"], **kw).to(DEV)
    pd = pred.to(DEV).requires_grad_()
    got = loss_fn(pd, target.to(DEV), cs["mask"].to(DEV), squash=squash, lead_dims=lead_dims)
    assert tuple(got.shape) == ((3,) if lead_dims else ()) + (() if squash else (5,)) and got.dtype == torch.float32
    weights = torch.randn(got.shape, generator=_gen(5))
    (got * weights.to(DEV)).sum().backward()
    p64 = pred.double().requires_grad_()
    ref64 = er.loss(p64, target.double(), cs["row_w"].double(), cs["col_w"].double(), cs["mask"], alpha, squash, lead_dims)
    (ref64 * weights.double()).sum().backward()
    with torch.no_grad():
        cpu32 = er.loss(pred, target, cs["row_w"], cs["col_w"], cs["mask"], alpha, squash, lead_dims)
    err, bound = _forward_errors(got.detach(), ref64.detach(), cpu32)
    gerr = float((pd.grad.cpu().double() - p64.grad).abs().max() / p64.grad.abs().max())
    print(f"{name} squash={squash} lead_dims={lead_dims}: worst err / bound {float((err / bound).max()):.3f}, gradient err {gerr:.3e}")
    assert bool((err <= bound).all()) and gerr <= 1e-6
    assert bool((pd.grad.cpu()[..., cs["mask"] == 0] == 0).all()) and bool(torch.isfinite(pd.grad).all())


def test_ensemble_metrics_vs_the_explicit_route():
    """EnsembleMetrics with a mean-std InputNormalizer and two variable groups: the documented keys and shapes, and the numbers
    of the explicit route -- de-normalise both operands, then the restatement -- within the forward bound."""
    from anemoi_models_amd import EnsembleMetrics
    from anemoi_models_amd.preprocessing.normalizer import InputNormalizer
    from anemoi_models_amd.utils.indices import SimpleDataIndices

    cs = _case(SHAPES[1], True, False)
    n_steps, b, e, g, v = 3, 2, 3, 257, 5
    idx = SimpleDataIndices(n_prognostic=3, n_forcing=2, n_diagnostic=2)  # 5 output variables of 7
    gen = np.random.default_rng(3)
    stats = {"minimum": np.zeros(7), "maximum": np.ones(7), "mean": gen.normal(size=7) * 50.0,
             "stdev": gen.uniform(0.5, 20.0, size=7)}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        norm = InputNormalizer(config={"default": "mean-std"}, data_indices=idx, statistics=stats)
    groups = {"sfc": [0, 3], "pl": [1, 2, 4]}
    keys = ("crps", "ens_rmse", "spread", "spread_skill")
    em = EnsembleMetrics(cs["row_w"], norm, groups=groups, alpha=0.95).to(DEV)
    pred, target = cs["pred"], cs["target"]
    pd = pred.to(DEV).requires_grad_()  # (the metrics run without autograd whatever comes in)
    got = em(pd, target.to(DEV), cs["mask"].to(DEV))
    assert sorted(got) == sorted(list(keys) + [f"{k}/{n}" for k in keys for n in groups])
    out_idx = norm._output_idx.long()

    def explicit(dt):
        mul, add = norm._norm_mul[out_idx].to(dt), norm._norm_add[out_idx].to(dt)
        with torch.no_grad():
            return er.metrics((pred.to(dt) - add) / mul, (target.to(dt) - add) / mul, cs["row_w"].to(dt), None, cs["mask"],
                              0.95, groups)

    ref64, cpu32 = explicit(torch.float64), explicit(torch.float32)
    for key, val in got.items():
        assert not val.requires_grad and val.dtype == torch.float32
        assert tuple(val.shape) == ((n_steps,) if "/" in key else (n_steps, v)), key
        err, bound = _forward_errors(val, ref64[key], cpu32[key])
        print(f"EnsembleMetrics {key}: worst rel err {float(err.max()):.3e}, worst err / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), key
    one = em(pred[0].to(DEV), target[0].to(DEV), cs["mask"].to(DEV))  # without the step axis: one step
    for key in keys:
        assert tuple(one[key].shape) == (1, v) and torch.equal(one[key][0], got[key][0]), key
    assert tuple(one["crps/sfc"].shape) == (1,)


# --------------------------------------------------------------------------------------------------- training
N_STEPS, N_MEMBERS, ALPHA = 2, 3, 0.95


@pytest.fixture(scope="module")
def crps_rollout_case(golden_cfg1_gt, graph_o32):
    """A three-member input and the f64 CPU autograd reference (loss, parameter gradients) of a 2-step rollout of config 1's
    model under the restated almost-fair CRPS.  The oracle's model_forward takes one member, and the model treats members
    independently: the reference is one rollout per member, concatenated on the ensemble axis."""
    from test_gpu_rollout_train import KW
    from test_oracle_golden import graph_tensors

    from anemoi_models_amd.utils.indices import SimpleDataIndices, advance_colmap

    gold = golden_cfg1_gt
    sd = split_prefix(gold, "sd.")
    graph = {k: (v.double() if v.is_floating_point() else v) for k, v in graph_tensors(graph_o32).items()}
    colmap = advance_colmap(SimpleDataIndices(n_prognostic=10, n_forcing=2, n_diagnostic=1)).tolist()
    gen = _gen(21)
    x = gold["x"]
    assert x.shape[2] == 1
    x = x.repeat(1, 1, N_MEMBERS, 1, 1)
    x = x + 0.1 * torch.randn(x.shape, generator=gen)
    g, v_out = gold["y"].shape[-2], gold["y"].shape[-1]
    rsd = {k: (v.double().requires_grad_() if v.is_floating_point() else v) for k, v in sd.items()}
    y = torch.cat([rr.rollout(rsd, graph, x[:, :, m:m + 1].double(), N_STEPS, colmap, **KW) for m in range(N_MEMBERS)], dim=2)
    assert tuple(y.shape[:3]) == (N_STEPS, x.shape[0], N_MEMBERS)
    targets = y.detach().mean(2).float() + 0.05 * torch.randn(y.shape[:2] + y.shape[3:], generator=gen)
    case = {"x": x, "targets": targets, "node_w": torch.rand(g, generator=gen) + 0.1,
            "var_w": torch.rand(v_out, generator=gen) + 0.5}
    # sgn is discontinuous: the share of near-ties, where the f32 run may take the other side, is capped
    yd = y.detach()
    mm = torch.stack([(yd[:, :, j] - yd[:, :, k]).abs() for j in range(N_MEMBERS) for k in range(j + 1, N_MEMBERS)])
    mt = (yd - targets.double().unsqueeze(2)).abs()
    case["near"] = (int((mm < 1e-4).sum()), mm.numel(), int((mt < 1e-4).sum()), mt.numel())
    loss = er.loss(y, targets.double(), case["node_w"].double(), case["var_w"].double(), None, ALPHA)
    loss.backward()
    case["loss"] = float(loss.detach())
    case["grads"] = {k: t.grad.float() for k, t in rsd.items() if t.is_floating_point() and t.grad is not None
                     and float(t.grad.abs().max()) > 0}
    return case


def test_rollout_training_step_with_crps_vs_oracle_autograd(crps_rollout_case, golden_cfg1_gt, graph_o32, monkeypatch):
    """Loss and every used parameter gradient of a 2-step RolloutModel on a three-member input under
    AlmostFairKernelCRPS(alpha=0.95) against f64 CPU autograd of the oracle rollouts plus the restated loss: the tolerance of
    test_rollout_training_step_vs_oracle_autograd (5e-3 per step).  The gradient of the CRPS is a sum of signs: a gap smaller
    than the f32 forward error (1.6e-6 here) can take the other side in the f32 run, and one such element moves the gradient of
    its node by a few per cent.  The fixture counts the gaps below 1e-4 and the test asserts the cap on their share (0.5 %) and
    prints the counts; what a flip costs is inside the tolerance that the test asserts, nothing else is relied on."""
    from test_gpu_rollout_train import _check_grads, _fresh

    from anemoi_models_amd import AlmostFairKernelCRPS
    from anemoi_models_amd.training import RolloutModel

    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "fp32")
    case, n = crps_rollout_case, N_STEPS
    tol = 5e-3 * n
    near_mm, n_mm, near_mt, n_mt = case["near"]
    print(f"crps rollout: {near_mm} of {n_mm} member-member and {near_mt} of {n_mt} member-target gaps below 1e-4")
    assert near_mm <= 0.005 * n_mm and near_mt <= 0.005 * n_mt
    model, idx = _fresh(graph_o32, golden_cfg1_gt)
    loss_fn = AlmostFairKernelCRPS(case["node_w"], case["var_w"], alpha=ALPHA).to(DEV)
    pred = RolloutModel(model, idx, n)(case["x"].to(DEV))
    assert tuple(pred.shape) == (n, case["x"].shape[0], N_MEMBERS) + tuple(case["targets"].shape[-2:])
    loss = loss_fn(pred, case["targets"].to(DEV))
    loss.backward()
    grads = {k: p.grad.float().clone() for k, p in model.named_parameters() if p.grad is not None}
    loss = float(loss.detach())
    print(f"crps rollout n_steps={n} E={N_MEMBERS} f32: loss {loss:.6f} (f64 oracle {case['loss']:.6f}, rel err "
          f"{abs(loss - case['loss']) / abs(case['loss']):.2e}); {len(case['grads'])} reference gradients")
    assert abs(loss - case["loss"]) <= tol * abs(case["loss"])
    assert len([k for k in case["grads"] if k in grads]) > 50
    _check_grads(grads, case["grads"], tol, 0.02, f"crps rollout n_steps={n} E={N_MEMBERS} f32 vs f64 oracle")


def test_graphed_crps_rollout_train_step_equals_eager(crps_rollout_case, golden_cfg1_gt, graph_o32, monkeypatch):
    """The same step under runtime.GraphedTrainStep: a replay is bit-equal to the eager step, two replays are bit-equal --
    the upstream gradient is read on the device, nothing in the loss synchronises."""
    from test_gpu_rollout_train import _fresh

    from anemoi_models_amd import AlmostFairKernelCRPS
    from anemoi_models_amd.runtime import GraphedTrainStep
    from anemoi_models_amd.training import RolloutModel

    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "fp32")
    case = crps_rollout_case
    model, idx = _fresh(graph_o32, golden_cfg1_gt)
    roll = RolloutModel(model, idx, N_STEPS)
    loss_fn = AlmostFairKernelCRPS(case["node_w"], case["var_w"], alpha=ALPHA).to(DEV)
    x, targets = case["x"].to(DEV), case["targets"].to(DEV)

    def eager_step():  # (in a function: no autograd graph of it may be alive at the capture, see GraphedTrainStep)
        for p in model.parameters():
            p.grad = None
        loss = loss_fn(roll(x), targets)
        loss.backward()
        return loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}

    want_loss, want = eager_step()
    graphed = GraphedTrainStep(roll, loss_fn, torch.zeros_like(x), torch.zeros_like(targets))
    runs = []
    for _ in range(2):
        loss = graphed(x, targets)
        runs.append((loss, {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}))
    assert torch.equal(runs[0][0], want_loss) and torch.equal(runs[1][0], want_loss)
    assert set(runs[0][1]) == set(want) and len(want) > 20
    for k, g in want.items():
        assert torch.equal(runs[0][1][k], g), k
        assert torch.equal(runs[1][1][k], g), k
