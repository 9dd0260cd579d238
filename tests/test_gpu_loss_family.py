"""The loss family on the HIP kernels (csrc/losses.hip): anemoi_weighted_error / _backward, autograd.weighted_error, the loss
classes and ValidationMetrics against the plain-torch restatement of tests/_loss_family_ref.py in float64, at the smallest
shapes at which the column layout of the reduction can go wrong.

Bounds (those of test_weighted_mse_loss_and_gradient_vs_f64, per output element): forward -- relative error against the f64
restatement at most 4 x that of the restatement evaluated in f32 on the CPU, or 2e-6 if that is larger; gradient -- at most
1e-6 of max |dpred|."""

import functools
import warnings

import numpy as np
import pytest
import torch

import _loss_family_ref as lf
import _rollout_ref as rr
from conftest import split_prefix

pytestmark = pytest.mark.gpu

DEV = "cuda"
DELTA = 1.0
# (G, V, B, n_groups); rows_per_group = B * G
SHAPES = [
    (1, 1, 1, 1),      # degenerate
    (257, 5, 2, 3),    # an idle lane (51 row lanes x 5 < 256); row weights wrap inside a group; a chunk tail
    (2062, 80, 1, 2),  # three row lanes, 41 workgroups per group
    (33, 257, 1, 1),   # crosses the column tile of 256
    (1031, 256, 1, 1),  # exactly one row per pass
    (5000, 3, 1, 4),   # several workgroups per group
]
IDS = [f"G{g}-V{v}-B{b}-L{n}" for g, v, b, n in SHAPES]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def _case(shape, masked, scaled):
    """Inputs on the CPU (never modified).  pred - target is N(0, 0.7^2) with one element in eight uniform in [-100, 100]: Huber
    (delta = 1) sees both branches, log-cosh sees |d| up to 100; 3 % of the elements have pred == target; with a mask, at most
    10 % of [G, V] is masked, the target is NaN there and the prediction Inf at half of those positions."""
    g, v, b, n_groups = shape
    gen = _gen(1000 * g + 10 * v + 2 * masked + scaled)
    full = (n_groups, b, g, v)
    target = torch.randn(full, generator=gen)
    d = 0.7 * torch.randn(full, generator=gen)
    d = torch.where(torch.rand(full, generator=gen) < 0.125, 200.0 * torch.rand(full, generator=gen) - 100.0, d)
    pred = torch.where(torch.rand(full, generator=gen) < 0.03, target, target + d)
    if g * v == 1:
        pred = target + 1.75
    row_w = torch.rand(g, generator=gen) + 0.1
    col_w = torch.rand(v, generator=gen) + 0.5
    c = (0.1 + 9.9 * torch.rand(v, generator=gen)) if scaled else None
    mask = None
    if masked:
        mask = (torch.rand((g, v), generator=gen) > 0.08).float()
        if g * v == 1:
            mask[:] = 1.0
        target = torch.where(mask != 0, target, torch.full((), float("nan")))
        pred = torch.where((mask == 0) & (torch.rand((g, v), generator=gen) < 0.5), torch.full((), float("inf")), pred)
    upstream = torch.randn((n_groups, v), generator=gen)
    return dict(pred=pred, target=target, row_w=row_w, col_w=col_w, c=c, mask=mask, upstream=upstream, n_groups=n_groups,
                scale=1.0 / b)


@functools.lru_cache(maxsize=None)
def _reference(shape, masked, scaled, kind):
    """(out f64, dpred f64 for the case's upstream, out of the f32 CPU evaluation) of the restatement."""
    cs = _case(shape, masked, scaled)
    d64 = lambda t: None if t is None else t.double()  # noqa: E731
    p64 = cs["pred"].double().requires_grad_()
    out = lf.weighted_error(p64, cs["target"].double(), cs["row_w"].double(), kind, DELTA, d64(cs["col_w"]), cs["mask"],
                            d64(cs["c"]), cs["n_groups"], cs["scale"])
    (out * cs["upstream"].double()).sum().backward()
    cpu32 = lf.weighted_error(cs["pred"], cs["target"], cs["row_w"], kind, DELTA, cs["col_w"], cs["mask"], cs["c"],
                              cs["n_groups"], cs["scale"])
    return out.detach(), p64.grad, cpu32


def _dev(cs):
    return {k: (t.to(DEV) if isinstance(t, torch.Tensor) else t) for k, t in cs.items()}


def _kernel_kwargs(cs, kind):
    return dict(delta=DELTA, col_w=cs["col_w"], mask=cs["mask"], diff_scale=cs["c"], n_groups=cs["n_groups"], scale=cs["scale"])


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
@pytest.mark.parametrize("kind", lf.KINDS)
def test_weighted_error_forward_vs_f64(kind, shape, masked, scaled):
    from anemoi_models_amd import autograd, ops

    cs, (ref64, _, cpu32) = _case(shape, masked, scaled), _reference(shape, masked, scaled, kind)
    d = _dev(cs)
    got = autograd.weighted_error(d["pred"], d["target"], d["row_w"], kind, **_kernel_kwargs(d, kind))
    assert got.dtype == torch.float32 and tuple(got.shape) == (cs["n_groups"], shape[1]) and bool(torch.isfinite(got).all())
    err, bound = _forward_errors(got, ref64, cpu32)
    print(f"weighted_error {kind} G={shape[0]} V={shape[1]} B={shape[2]} groups={shape[3]} masked={masked} scaled={scaled}: "
          f"worst rel err {float(err.max()):.3e} (f32 CPU {float(((cpu32.double() - ref64).abs() / ref64.abs().clamp(min=1e-300)).max()):.3e}), "
          f"worst err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    # the op underneath, on the flattened rows, is the same call
    v = shape[1]
    flat = ops.weighted_error(d["pred"].view(-1, v), d["target"].view(-1, v), d["row_w"], kind, **_kernel_kwargs(d, kind))
    assert torch.equal(flat, got)


@pytest.mark.parametrize("scaled", [False, True], ids=["c1", "c"])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("kind", lf.KINDS)
def test_weighted_error_backward_vs_f64(kind, shape, masked, scaled):
    """dpred for a random upstream [n_groups, V] against f64 autograd of the restatement; exactly 0 under the mask (NaN targets
    there) and, for MAE, exactly 0 where pred == target."""
    from anemoi_models_amd import autograd

    cs, (_, want, _) = _case(shape, masked, scaled), _reference(shape, masked, scaled, kind)
    d = _dev(cs)
    pd = d["pred"].clone().requires_grad_()
    out = autograd.weighted_error(pd, d["target"], d["row_w"], kind, **_kernel_kwargs(d, kind))
    out.backward(d["upstream"])
    got = pd.grad.cpu()
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    gerr = float((got.double() - want).abs().max() / want.abs().max())
    print(f"weighted_error_backward {kind} G={shape[0]} V={shape[1]} groups={shape[3]} masked={masked} scaled={scaled}: "
          f"gradient err {gerr:.3e} of max |dpred|")
    assert gerr <= 1e-6
    if masked:
        assert bool((got[..., cs["mask"] == 0] == 0).all())
        assert shape[0] * shape[1] == 1 or bool((got[..., cs["mask"] != 0] != 0).any())
    if kind == "mae":
        same = cs["pred"] == cs["target"]
        assert shape[0] * shape[1] == 1 or int(same.sum()) > 0
        assert bool((got[same] == 0).all())
    # dtarget = -dpred, only where the target asks for a gradient
    if not masked:
        p2, t2 = d["pred"].clone().requires_grad_(), d["target"].clone().requires_grad_()
        autograd.weighted_error(p2, t2, d["row_w"], kind, **_kernel_kwargs(d, kind)).backward(d["upstream"])
        assert torch.equal(p2.grad, pd.grad) and torch.equal(t2.grad, -pd.grad)


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_mse_through_the_new_kernel_agrees_with_the_scalar_kernel(shape, masked):
    """The squashed MSE through anemoi_weighted_error against WeightedMSELoss (anemoi_weighted_mse) within the forward bound;
    WeightedMSELoss with its default keywords is still autograd.weighted_mse, bit for bit."""
    from anemoi_models_amd import WeightedMSELoss, autograd

    cs = _case(shape, masked, False)
    g, v = shape[0], shape[1]
    d = _dev(cs)
    loss_fn = WeightedMSELoss(cs["row_w"], cs["col_w"]).to(DEV)
    pd = d["pred"].clone().requires_grad_()
    old = loss_fn(pd, d["target"], d["mask"])
    old.backward()
    new = loss_fn.per_variable(d["pred"], d["target"], d["mask"]).mean(-1)
    assert old.dim() == 0 and new.dim() == 0
    old = old.detach()
    ref64 = lf.loss("mse", cs["pred"].double(), cs["target"].double(), cs["row_w"].double(), cs["col_w"].double(), cs["mask"])
    cpu32 = lf.loss("mse", cs["pred"], cs["target"], cs["row_w"], cs["col_w"], cs["mask"])
    bound = max(4 * abs(float(cpu32) - float(ref64)) / abs(float(ref64)), 2e-6)
    gap = abs(float(new) - float(old)) / abs(float(old))
    err = abs(float(new) - float(ref64)) / abs(float(ref64))
    print(f"mse G={g} V={v} masked={masked}: new vs scalar kernel {gap:.3e}, new vs f64 {err:.3e}, bound {bound:.3e}")
    assert gap <= bound and err <= bound
    p2 = d["pred"].clone().requires_grad_()
    n_lead = cs["pred"].numel() // (g * v)
    direct = autograd.weighted_mse(p2, d["target"], loss_fn.node_weights, loss_fn.variable_weights, d["mask"], 1.0 / (n_lead * v))
    direct.backward()
    assert torch.equal(direct.detach(), old.detach()) and torch.equal(p2.grad, pd.grad)


@pytest.mark.parametrize("kind", lf.KINDS)
def test_weighted_error_is_deterministic_and_groups_are_independent(kind):
    """Forward and backward twice: equal bits.  n_groups = 3 over a stacked tensor: group by group the bits of three
    n_groups = 1 calls on the slices -- a workgroup never straddles two groups."""
    from anemoi_models_amd import ops

    shape = SHAPES[1]
    for masked in (False, True):
        d = _dev(_case(shape, masked, True))
        v = shape[1]
        kw = _kernel_kwargs(d, kind)
        p2, t2 = d["pred"].view(-1, v), d["target"].view(-1, v)
        out = ops.weighted_error(p2, t2, d["row_w"], kind, **kw)
        grad = ops.weighted_error_backward(p2, t2, d["row_w"], kind, upstream=d["upstream"], **kw)
        assert torch.equal(ops.weighted_error(p2, t2, d["row_w"], kind, **kw), out)
        assert torch.equal(ops.weighted_error_backward(p2, t2, d["row_w"], kind, upstream=d["upstream"], **kw), grad)
        kw1 = dict(kw, n_groups=1)
        rpg = p2.shape[0] // 3
        for l in range(3):
            ps, ts = p2[l * rpg:(l + 1) * rpg], t2[l * rpg:(l + 1) * rpg]
            assert torch.equal(ops.weighted_error(ps, ts, d["row_w"], kind, **kw1), out[l:l + 1]), (kind, l)
            gs = ops.weighted_error_backward(ps, ts, d["row_w"], kind, upstream=d["upstream"][l:l + 1].contiguous(), **kw1)
            assert torch.equal(gs, grad[l * rpg:(l + 1) * rpg]), (kind, l)
    # no rows at all: zeros; CPU tensors: refused
    w = torch.ones(4, device=DEV)
    empty = torch.zeros((0, 3), device=DEV)
    assert ops.weighted_error(empty, empty, w, kind, n_groups=2).tolist() == [[0.0] * 3] * 2
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.weighted_error(torch.zeros(4, 3), torch.zeros(4, 3), torch.ones(4), kind)


# --------------------------------------------------------------------------------------------------- the modules
LOSSES = [("mse", "WeightedMSELoss"), ("mae", "WeightedMAELoss"), ("huber", "WeightedHuberLoss"),
          ("logcosh", "WeightedLogCoshLoss"), ("rmse", "WeightedRMSELoss")]


@pytest.mark.parametrize("lead_dims", [0, 1])
@pytest.mark.parametrize("squash", [True, False])
@pytest.mark.parametrize("kind,name", LOSSES)
def test_loss_classes_vs_restatement(kind, name, squash, lead_dims):
    """Every loss class on a [3, 2, 1, 257, 5] rollout result with a mask over NaN targets: value (forward bound, per element)
    and gradient (1e-6 of max |dpred|; for RMSE it passes through torch's sqrt into the kernel) against the f64 restatement."""
    import anemoi_models_amd

    cs = _case(SHAPES[1], True, False)
    pred, target = cs["pred"].reshape(3, 2, 1, 257, 5), cs["target"].reshape(3, 2, 1, 257, 5)
    kw = dict(delta=1.5) if kind == "huber" else {}
    loss_fn = getattr(anemoi_models_amd, name)(cs["row_w"], cs["col_w"], **kw).to(DEV)
    pd = pred.to(DEV).requires_grad_()
    got = loss_fn(pd, target.to(DEV), cs["mask"].to(DEV), squash=squash, lead_dims=lead_dims)
    assert tuple(got.shape) == ((3,) if lead_dims else ()) + (() if squash else (5,)) and got.dtype == torch.float32
    weights = torch.randn(got.shape, generator=_gen(5))
    (got * weights.to(DEV)).sum().backward()
    p64 = pred.double().requires_grad_()
    args = (cs["row_w"].double(), cs["col_w"].double(), cs["mask"], kw.get("delta", 1.0), squash, lead_dims)
    ref64 = lf.loss(kind, p64, target.double(), *args)
    (ref64 * weights.double()).sum().backward()
    cpu32 = lf.loss(kind, pred, target, cs["row_w"], cs["col_w"], *args[2:])
    err, bound = _forward_errors(got.detach(), ref64.detach(), cpu32)
    gerr = float((pd.grad.cpu().double() - p64.grad).abs().max() / p64.grad.abs().max())
    print(f"{name} squash={squash} lead_dims={lead_dims}: worst err / bound {float((err / bound).max()):.3f}, gradient err {gerr:.3e}")
    assert bool((err <= bound).all()) and gerr <= 1e-6
    assert bool((pd.grad.cpu()[..., cs["mask"] == 0] == 0).all()) and bool(torch.isfinite(pd.grad).all())


def test_validation_metrics_vs_the_explicit_route():
    """ValidationMetrics with a mean-std InputNormalizer and two variable groups: the documented keys and shapes, and the
    numbers of the explicit route -- de-normalise both operands, then the restatement -- within the forward bound."""
    from anemoi_models_amd import ValidationMetrics
    from anemoi_models_amd.preprocessing.normalizer import InputNormalizer
    from anemoi_models_amd.utils.indices import SimpleDataIndices

    cs = _case(SHAPES[1], True, False)
    n_steps, b, g, v = 3, 2, 257, 5
    idx = SimpleDataIndices(n_prognostic=3, n_forcing=2, n_diagnostic=2)  # 5 output variables of 7
    gen = np.random.default_rng(3)
    stats = {"minimum": np.zeros(7), "maximum": np.ones(7), "mean": gen.normal(size=7) * 50.0,
             "stdev": gen.uniform(0.5, 20.0, size=7)}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        norm = InputNormalizer(config={"default": "mean-std"}, data_indices=idx, statistics=stats)
    groups = {"sfc": [0, 3], "pl": [1, 2, 4]}
    kinds = ("mse", "mae", "huber", "logcosh", "rmse")
    vm = ValidationMetrics(cs["row_w"], norm, groups=groups, kinds=kinds, delta=2.0).to(DEV)
    pred, target = cs["pred"].reshape(n_steps, b, 1, g, v), cs["target"].reshape(n_steps, b, 1, g, v)
    pd = pred.to(DEV).requires_grad_()  # (the metrics run without autograd whatever comes in)
    got = vm(pd, target.to(DEV), cs["mask"].to(DEV))
    assert sorted(got) == sorted(list(kinds) + [f"{k}/{n}" for k in kinds for n in groups])
    out_idx = norm._output_idx.long()
    w = cs["row_w"] / cs["row_w"].sum()

    def explicit(dt):
        mul, add = norm._norm_mul[out_idx].to(dt), norm._norm_add[out_idx].to(dt)
        pp, tp = (pred.to(dt) - add) / mul, (target.to(dt) - add) / mul
        res = {}
        for kind in kinds:
            res[kind] = lf.weighted_error(pp, tp, w.to(dt), "mse" if kind == "rmse" else kind, 2.0, None, cs["mask"], None,
                                          n_steps, 1.0 / b)
            if kind == "rmse":
                res[kind] = res[kind].sqrt()
            for name, cols in groups.items():
                res[f"{kind}/{name}"] = res[kind][:, cols].mean(-1)
        return res

    ref64, cpu32 = explicit(torch.float64), explicit(torch.float32)
    for key, val in got.items():
        assert not val.requires_grad and val.dtype == torch.float32
        assert tuple(val.shape) == ((n_steps,) if "/" in key else (n_steps, v)), key
        err, bound = _forward_errors(val, ref64[key], cpu32[key])
        print(f"ValidationMetrics {key}: worst rel err {float(err.max()):.3e}, worst err / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), key
    one = vm(pred[0].to(DEV), target[0].to(DEV), cs["mask"].to(DEV))  # without the step axis: one step
    assert tuple(one["mse"].shape) == (1, v) and torch.equal(one["mse"][0], got["mse"][0])


# --------------------------------------------------------------------------------------------------- training
@pytest.fixture(scope="module")
def huber_rollout_case(golden_cfg1_gt, graph_o32):
    """Inputs and the f64 CPU autograd reference (loss, parameter gradients) of a 2-step rollout of config 1's model under the
    restated Huber loss."""
    from test_gpu_rollout_train import KW
    from test_oracle_golden import graph_tensors

    from anemoi_models_amd.utils.indices import SimpleDataIndices, advance_colmap

    gold = golden_cfg1_gt
    sd = split_prefix(gold, "sd.")
    graph = {k: (v.double() if v.is_floating_point() else v) for k, v in graph_tensors(graph_o32).items()}
    colmap = advance_colmap(SimpleDataIndices(n_prognostic=10, n_forcing=2, n_diagnostic=1)).tolist()
    gen = _gen(12)
    g, v_out = gold["y"].shape[-2], gold["y"].shape[-1]
    case = {"x": gold["x"], "targets": torch.randn((2,) + tuple(gold["y"].shape), generator=gen),
            "node_w": torch.rand(g, generator=gen) + 0.1, "var_w": torch.rand(v_out, generator=gen) + 0.5}
    rsd = {k: (v.double().requires_grad_() if v.is_floating_point() else v) for k, v in sd.items()}
    y = rr.rollout(rsd, graph, gold["x"].double(), 2, colmap, **KW)
    d = (y - case["targets"].double()).abs()
    case["branches"] = (int((d <= DELTA).sum()), int((d > DELTA).sum()))
    loss = lf.loss("huber", y, case["targets"].double(), case["node_w"].double(), case["var_w"].double(), None, DELTA)
    loss.backward()
    case["loss"] = float(loss.detach())
    case["grads"] = {k: t.grad.float() for k, t in rsd.items() if t.is_floating_point() and t.grad is not None
                     and float(t.grad.abs().max()) > 0}
    return case


def test_rollout_training_step_with_huber_vs_oracle_autograd(huber_rollout_case, golden_cfg1_gt, graph_o32, monkeypatch):
    """Loss and every used parameter gradient of a 2-step RolloutModel under WeightedHuberLoss against f64 CPU autograd of the
    oracle rollout plus the restated loss: the tolerance of test_rollout_training_step_vs_oracle_autograd (5e-3 per step)."""
    from test_gpu_rollout_train import _check_grads, _fresh

    from anemoi_models_amd import WeightedHuberLoss
    from anemoi_models_amd.training import RolloutModel

    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "fp32")
    case, n = huber_rollout_case, 2
    tol = 5e-3 * n
    assert min(case["branches"]) > 100  # both branches of the Huber function are in the loss
    model, idx = _fresh(graph_o32, golden_cfg1_gt)
    loss_fn = WeightedHuberLoss(case["node_w"], case["var_w"], delta=DELTA).to(DEV)
    loss = loss_fn(RolloutModel(model, idx, n)(case["x"].to(DEV)), case["targets"].to(DEV))
    loss.backward()
    grads = {k: p.grad.float().clone() for k, p in model.named_parameters() if p.grad is not None}
    loss = float(loss.detach())
    print(f"huber rollout n_steps={n} f32: loss {loss:.6f} (f64 oracle {case['loss']:.6f}, rel err "
          f"{abs(loss - case['loss']) / abs(case['loss']):.2e})")
    assert abs(loss - case["loss"]) <= tol * abs(case["loss"])
    assert len([k for k in case["grads"] if k in grads]) > 50
    _check_grads(grads, case["grads"], tol, 0.02, f"huber rollout n_steps={n} f32 vs f64 oracle")


def test_graphed_huber_rollout_train_step_equals_eager(huber_rollout_case, golden_cfg1_gt, graph_o32, monkeypatch):
    """The same step under runtime.GraphedTrainStep: a replay is bit-equal to the eager step, two replays are bit-equal --
    the upstream gradient is read on the device, nothing in the loss synchronises."""
    from test_gpu_rollout_train import _fresh

    from anemoi_models_amd import WeightedHuberLoss
    from anemoi_models_amd.runtime import GraphedTrainStep
    from anemoi_models_amd.training import RolloutModel

    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "fp32")
    case = huber_rollout_case
    model, idx = _fresh(graph_o32, golden_cfg1_gt)
    roll = RolloutModel(model, idx, 2)
    loss_fn = WeightedHuberLoss(case["node_w"], case["var_w"], delta=DELTA).to(DEV)
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
