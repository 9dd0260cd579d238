"""The bounding family on the GPU: ``anemoi_bound_output_leaky`` (csrc/elementwise.hip, LEAKY) and the training pair
``anemoi_bound_output_train`` / ``anemoi_bound_output_backward`` (csrc/bounding.hip) per element against the f64 module chain with
the propagated bounds of tests/_bounding_ref.py, their ownership / determinism properties, and the routes that use them: the
training forward of the models (``training._finish``), ``RolloutModel``, ``GraphedTrainStep`` and ``predict_step``."""

import os
import subprocess
import sys

import pytest
import torch

import _bounding_ref as br
import _impute_ref as ir
from conftest import ROOT
from conftest import split_prefix

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = torch.finfo(torch.float32).eps
# the project's bound on the parameter gradients of its f32 backward (tests/test_gpu_truncation.py, tests/test_gpu_cond_ln.py)
GRAD_TOL_F32 = 1e-4


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from anemoi_models_amd import _lib

    _lib.load()  # the native library must be present: no fallback
    assert torch.cuda.is_available()


_REF = {}


def _ref(rows, v_out):
    """One case per shape, computed once and shared: inputs, the chain, and the f64 contracts of both directions."""
    if (rows, v_out) not in _REF:
        modules = br.chain(v_out)
        x, g = br.inputs(rows, v_out)
        _REF[(rows, v_out)] = {"modules": modules, "x": x, "g": g, "fwd": br.forward_ref(x, modules),
                               "bwd": br.backward_ref(x, g, modules)[:2], "left_out": br.guarded_rows(x, modules)}
    return _REF[(rows, v_out)]


def _train_pair(x, g, lists, slope, n_tape):
    """``autograd.bound_output`` on a fresh non-leaf copy of ``x`` and its backward: ``(y, dx)``."""
    from anemoi_models_amd import autograd

    leaf = x.to(DEV).requires_grad_()
    y = autograd.bound_output(leaf.clone(), lists, slope, n_tape)
    y.backward(g)
    return y.detach(), leaf.grad


@pytest.mark.parametrize("v_out", br.WIDTHS)
@pytest.mark.parametrize("rows", br.ROWS)
def test_leaky_kernel_and_training_forward_vs_f64(rows, v_out):
    """Every element of both forwards within its propagated bound of the f64 module chain (no exclusions: every op is
    continuous); a NaN in a touched column stays a NaN and stays in its row."""
    from anemoi_models_amd import ops

    case = _ref(rows, v_out)
    lists, slope, n_tape = br.op_tensors(case["modules"], DEV)
    want, bound = case["fwd"]
    x = case["x"]
    got = ops.bound_output(x.to(DEV).clone(), *lists, slope=slope)
    used = br.check(got, want, bound, "anemoi_bound_output_leaky")
    y, _ = _train_pair(x, case["g"].to(DEV), lists, slope, n_tape)
    used_t = br.check(y, want, bound, "anemoi_bound_output_train")
    print(f"rows={rows} V_out={v_out}: largest fraction of a bound used: leaky {used:.3f}, training forward {used_t:.3f}")
    x_nan = x.clone()
    x_nan[rows // 2, v_out // 2] = float("nan")  # column b: leaky relu, normalised relu, leaky fraction
    want_n, bound_n = br.forward_ref(x_nan, case["modules"])
    assert int(torch.isnan(want_n).sum()) == 1
    br.check(ops.bound_output(x_nan.to(DEV), *lists, slope=slope), want_n, bound_n, "leaky, NaN")
    br.check(_train_pair(x_nan, case["g"].to(DEV), lists, slope, n_tape)[0], want_n, bound_n, "training forward, NaN")


@pytest.mark.parametrize("v_out", br.WIDTHS)
@pytest.mark.parametrize("rows", br.ROWS)
def test_training_backward_vs_f64_autograd(rows, v_out):
    """dx per element within its propagated bound of f64 autograd over the module chain, on every row but those with an op
    input within the guard of a threshold (at most 1 %); the incoming gradient keeps its bits; two calls give the same bits."""
    from anemoi_models_amd import ops

    case = _ref(rows, v_out)
    lists, slope, n_tape = br.op_tensors(case["modules"], DEV)
    want, bound = case["bwd"]
    left_out = case["left_out"]
    share = float(left_out.double().mean())
    g = case["g"].to(DEV)
    g_bits = g.clone()
    y, dx = _train_pair(case["x"], g, lists, slope, n_tape)
    used = br.check(dx, want, bound, "anemoi_bound_output_backward", ~left_out)
    print(f"rows={rows} V_out={v_out}: largest fraction of a bound used {used:.3f}; rows left out {100 * share:.2f} %")
    assert share <= 0.01
    assert torch.equal(g.view(torch.int32), g_bits.view(torch.int32)) and dx.data_ptr() != g.data_ptr()
    y2, dx2 = _train_pair(case["x"], g, lists, slope, n_tape)
    assert torch.equal(y.view(torch.int32), y2.view(torch.int32)) and torch.equal(dx.view(torch.int32), dx2.view(torch.int32))
    # the two entry points alone: the tape has the stated size, untouched columns are copies
    yy = case["x"].to(DEV).clone()
    tape = ops.bound_output_train(yy, *lists, slope, n_tape)
    assert tuple(tape.shape) == (13, rows) and torch.equal(yy, y)
    direct = ops.bound_output_backward(g, tape, *lists, slope)
    assert torch.equal(direct.view(torch.int32), dx.view(torch.int32))
    untouched = [c for c in range(v_out) if c not in (0, v_out // 2, v_out - 1)]
    assert torch.equal(direct[:, untouched], g[:, untouched])


@pytest.mark.parametrize("v_out", br.WIDTHS)
def test_old_classes_give_the_module_route_bits(v_out):
    """Lists of the three classes of the reference checkout: selections and one f32 multiply -- the plain kernel, the leaky
    kernel with zero slopes and the training forward equal the module route on the device, +-inf included."""
    from anemoi_models_amd import ops

    modules = br.old_chain(v_out)
    x, g = br.inputs(1000, v_out, seed=1)
    x[5, 0], x[6, v_out - 1] = -float("inf"), float("inf")
    lists, slope, n_tape = br.op_tensors(modules, DEV)
    assert not bool(slope.any())
    want = br.module_chain(modules, x.to(DEV))
    assert not bool(torch.isnan(want).any())
    assert torch.equal(ops.bound_output(x.to(DEV).clone(), *lists), want)
    assert torch.equal(ops.bound_output(x.to(DEV).clone(), *lists, slope=slope), want)
    assert torch.equal(_train_pair(x, g.to(DEV), lists, slope, n_tape)[0], want)


def test_leaky_kernel_with_the_imputed_variant():
    """80 rows on a grid of 40 (two batch entries share the map): the 11-op chain, then the de-normalisation of the bounded
    columns, then the NaNs of the map in column c -- the total of the leaky fraction on column b, which stays finite: NaNs are
    restored only after the ops."""
    from anemoi_models_amd import ops
    from anemoi_models_amd.preprocessing.imputer import Imputation

    v_out, n = 7, 40
    modules = br.chain(v_out)
    gen = torch.Generator().manual_seed(8)
    y = torch.randn(2, 1, n, v_out, generator=gen) * 1.5
    nan_map = torch.rand(n, 5, generator=gen) < 0.3
    nan_map[1, :], nan_map[2, :] = True, False
    lists, slope, _ = br.op_tensors(modules, DEV)
    cols = [0, v_out // 2, v_out - 1]
    fin = (torch.tensor(cols, dtype=torch.int32), torch.rand(3, generator=gen) + 0.5, torch.randn(3, generator=gen))
    obj = Imputation(torch.zeros(4), [-1] * 4, nan_map, [-1, -1, 4])  # fin_nan_src: only column c gets NaNs back
    dev = Imputation(obj.fill_val.to(DEV), obj.fill_src.tolist(), nan_map.to(DEV), obj.out_nan_src.tolist())
    fin_dev = tuple(t.to(DEV) for t in fin)
    got = ops.bound_output(y.to(DEV).clone(), *lists, fin=fin_dev, impute=dev, slope=slope)
    again = ops.bound_output(y.to(DEV).clone(), *lists, fin=fin_dev, impute=dev, slope=slope)
    assert torch.equal(torch.nan_to_num(got, nan=7.0), torch.nan_to_num(again, nan=7.0))
    want, bound = br.forward_ref(y, modules)
    mul, add = fin[1].double(), fin[2].double()
    # z = (w - add) / mul: the subtraction rounds once, the f32 division is within 2.5 ulp (tests/_remap_ref.py)
    z = (want[..., cols] - add) / mul
    bz = (bound[..., cols] + br.U * (want[..., cols] - add).abs()) / mul.abs() + 2.5 * EPS * (z.abs() + bound[..., cols] / mul.abs())
    want[..., cols], bound[..., cols] = z, bz
    want[..., v_out - 1] = torch.where(nan_map[:, 4].expand(2, 1, n), torch.full_like(want[..., 0], float("nan")), want[..., v_out - 1])
    assert bool(nan_map[:, 4].any()) and not bool(torch.isnan(want[..., :v_out - 1]).any())
    print(f"leaky + imputed: largest fraction of a bound used {br.check(got, want, bound, 'anemoi_bound_output_leaky, imputed'):.3f}")
    none = Imputation(torch.zeros(4, device=DEV), [-1] * 4, nan_map.to(DEV), [-1, -1, -1])
    plain = ops.bound_output(y.to(DEV).clone(), *lists, fin=fin_dev, slope=slope)
    assert torch.equal(ops.bound_output(y.to(DEV).clone(), *lists, fin=fin_dev, impute=none, slope=slope), plain)


# ------------------------------------------------------------------------------------------------------------ models
A = "anemoi.models.layers.bounding."
ONE_OF_EACH = [
    {"_target_": A + "ReluBounding", "variables": ["prog_0", "diag_0"]},
    {"_target_": A + "LeakyReluBounding", "variables": ["prog_1"]},
    {"_target_": A + "HardtanhBounding", "variables": ["prog_2"], "min_val": -0.5, "max_val": 0.75},
    {"_target_": A + "LeakyHardtanhBounding", "variables": ["prog_3", "prog_0"], "min_val": -0.25, "max_val": 0.5},
    {"_target_": A + "NormalizedReluBounding", "variables": ["prog_5", "prog_4"], "min_val": [5.0, 0.0],
     "normalizer": ["mean-std", "max"]},
    {"_target_": A + "LeakyNormalizedReluBounding", "variables": ["prog_6"], "min_val": [1.0], "normalizer": ["min-max"]},
    {"_target_": A + "FractionBounding", "variables": ["prog_7"], "min_val": 0.0, "max_val": 1.0, "total_var": "prog_2"},
    {"_target_": A + "LeakyFractionBounding", "variables": ["prog_8", "prog_9"], "min_val": 0.0, "max_val": 1.0,
     "total_var": "prog_9"},
]
# (prog_2 is the column whose NaNs the imputer of the predict_step test restores: here the bounding kernel de-normalises it)
LEAKY_LIST = [{"_target_": A + "LeakyReluBounding", "variables": ["prog_1", "prog_2"]}, ONE_OF_EACH[3], ONE_OF_EACH[4],
              ONE_OF_EACH[7]]


def _stats(gold):
    return {k: v.numpy() for k, v in split_prefix(gold, "stat.").items()}


def _flat_model(graph, stats, boundings, seed=3):
    from anemoi_models_amd.models import AnemoiModelEncProcDec
    from anemoi_models_amd.utils.indices import SimpleDataIndices
    from anemoi_models_amd.utils.presets import model_config

    torch.manual_seed(seed)
    cfg = model_config("GraphTransformer", 64, 2, 16)
    cfg["model"]["bounding"] = [dict(b) for b in boundings]
    idx = SimpleDataIndices(n_prognostic=10, n_forcing=2, n_diagnostic=1)
    return AnemoiModelEncProcDec(model_config=type(cfg)(cfg), data_indices=idx, graph_data=graph, statistics=stats).to(DEV), idx


def _training_results(graph, stats):
    """One training step of the flat model and one of a two-step ``RolloutModel`` over it (the same weights and data in every
    process): outputs, losses, parameter gradients, the launch names of each step."""
    from anemoi_models_amd import WeightedMSELoss, trail
    from anemoi_models_amd.training import RolloutModel

    model, idx = _flat_model(graph, stats, ONE_OF_EACH)
    model.train()
    g = graph["data"].num_nodes
    gen = torch.Generator().manual_seed(4)
    x = (torch.randn(1, 2, 1, g, idx.num_input, generator=gen)).to(DEV)
    dy = torch.randn(1, 1, g, model.num_output_channels, generator=gen).to(DEV)
    targets = torch.randn(2, 1, 1, g, model.num_output_channels, generator=gen).to(DEV)
    loss_fn = WeightedMSELoss(torch.rand(g, generator=gen) + 0.1, torch.rand(model.num_output_channels, generator=gen) + 0.5).to(DEV)
    grads = lambda: {k: p.grad.clone().cpu() for k, p in model.named_parameters() if p.grad is not None}  # noqa: E731
    with trail.record(capacity=16384) as flat_trail:
        y = model(x)
        y.backward(dy)
    out = {"y": y.detach().cpu(), "grads": grads(), "names": sorted({n.split(":")[0] for n in flat_trail.names()})}
    for p in model.parameters():
        p.grad = None
    with trail.record(capacity=16384) as roll_trail:
        loss = loss_fn(RolloutModel(model, idx, 2)(x), targets)
        loss.backward()
    out.update(roll_loss=loss.detach().cpu(), roll_grads=grads(), roll_names=list(roll_trail.names()))
    assert flat_trail.dropped == 0 and roll_trail.dropped == 0
    # the output of the residual the boundings saw: the same weights without a bounding list (every kernel is deterministic)
    bare, _ = _flat_model(graph, stats, [])
    bare.load_state_dict(model.state_dict())
    bare.train()
    out["y_pre"], out["dy"] = bare(x).detach().cpu(), dy.cpu()
    return out


def _child(path):
    """Entry of the child process (``ANEMOI_AMD_TRAIN_FUSED_BOUND=0`` in its environment): the same step on the module route."""
    from anemoi_models_amd.graphs.synthetic import build_graph
    from conftest import load_npz

    torch.save(_training_results(build_graph("o32_ico2"), _stats(load_npz("interface_gt.npz"))), path)


def _rel(got, want):
    return float((got.double() - want.double()).abs().max() / want.double().abs().max().clamp_min(1e-30))


def _worst_gradient_error(got: dict, want: dict) -> float:
    """Largest error of a parameter gradient relative to the largest entry among the gradients of ITS LAYER (weight and bias of
    one Linear / LayerNorm share a prefix): the bias gradient of an attention key projection is analytically zero -- a softmax
    does not see a shift of its keys -- so what is computed there is the rounding residue of the sums that also form the weight
    gradient, and only their magnitude gives it a scale."""
    scale = {}
    for k, v in want.items():
        layer = k.rsplit(".", 1)[0]
        scale[layer] = max(scale.get(layer, 0.0), float(v.abs().max()))
    return max(float((got[k].double() - v.double()).abs().max()) / max(scale[k.rsplit(".", 1)[0]], 1e-30) for k, v in want.items())


def test_training_step_fused_pair_vs_module_route(graph_o32, golden_interface, monkeypatch, tmp_path):
    """``graph_o32``, 64 channels, 2 layers, one bounding of each class.  The fused pair against the module route
    (``ANEMOI_AMD_TRAIN_FUSED_BOUND=0`` in a fresh child process), flat model and two-step rollout.

    Tolerances, from the bounds of tests/_bounding_ref.py and fixed before any run: both outputs lie within their propagated
    per-element bound of the f64 module chain on the residual output ``y_pre`` -- the kernel's bound for the fused route, the
    modules' own (two more roundings in the normalised classes) for the other.  The two routes hand the decoder gradients dx
    that differ by at most r = 2 |bound_dx| / |dx| in the 2-norm; the parameter gradients are a linear map of dx evaluated by the
    same deterministic f32 backward, whose own error the suite bounds by GRAD_TOL_F32 relative to the largest entry, so the two
    sets may differ by that bound plus r and no more is asked (the scale of an entry: ``_worst_gradient_error``)."""
    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "fp32")
    stats = _stats(golden_interface)
    fused = _training_results(graph_o32, stats)
    assert "anemoi_bound_output_train" in fused["names"] and "anemoi_bound_output_backward" in fused["names"]
    assert fused["roll_names"].count("anemoi_bound_output_train:out") == 2  # one launch per step, each way
    assert fused["roll_names"].count("anemoi_bound_output_backward:dx") == 2
    path = str(tmp_path / "module_route.pt")
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; import test_gpu_bounding_family as t; t._child({path!r})"
    subprocess.run([sys.executable, "-c", code], check=True, timeout=600,
                   env=dict(os.environ, ANEMOI_AMD_TRAIN_FUSED_BOUND="0", ANEMOI_AMD_DTYPE="fp32"))
    module = torch.load(path)
    assert "anemoi_bound_output_train" not in module["names"] and "anemoi_bound_output_train:out" not in module["roll_names"]
    assert torch.equal(fused["y_pre"], module["y_pre"])
    model, _ = _flat_model(graph_o32, stats, ONE_OF_EACH)
    chain = [b.cpu() for b in model.boundings]
    y_pre = fused["y_pre"]
    want, bound = br.forward_ref(y_pre, chain)
    used = br.check(fused["y"], want, bound, "training forward, fused pair")
    want_m, bound_m = br.forward_ref(y_pre, chain, module_route=True)
    used_m = br.check(module["y"], want_m, bound_m, "training forward, module route")
    dx, bound_dx, _ = br.backward_ref(y_pre, fused["dy"], chain)
    r = 2.0 * float(bound_dx.norm() / dx.norm())
    tol = GRAD_TOL_F32 + r
    worst = _worst_gradient_error(fused["grads"], module["grads"])
    worst_roll = _worst_gradient_error(fused["roll_grads"], module["roll_grads"])
    loss_err = abs(float(fused["roll_loss"]) - float(module["roll_loss"])) / abs(float(module["roll_loss"]))
    print(f"fused pair vs module route: forward {used:.3f} / {used_m:.3f} of a bound; r = {r:.2e}; parameter gradients: worst rel "
          f"err {worst:.2e} (flat), {worst_roll:.2e} (rollout); rollout loss rel err {loss_err:.2e}")
    assert set(fused["grads"]) == set(module["grads"]) and len(fused["grads"]) > 20
    assert set(fused["roll_grads"]) == set(module["roll_grads"])
    assert worst <= tol and worst_roll <= tol and loss_err <= tol


def test_graphed_train_step_replays_the_eager_bits(graph_o32, golden_interface, monkeypatch):
    """One ``GraphedTrainStep`` capture of the two-step rollout with the fused pair: the replay equals, bit for bit, the eager step
    of the same model and inputs (both launches are capturable: nothing is read back, no workspace)."""
    from anemoi_models_amd import WeightedMSELoss
    from anemoi_models_amd.runtime import GraphedTrainStep
    from anemoi_models_amd.training import RolloutModel

    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "fp32")
    model, idx = _flat_model(graph_o32, _stats(golden_interface), ONE_OF_EACH)
    model.train()
    g = graph_o32["data"].num_nodes
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(1, 2, 1, g, idx.num_input, generator=gen).to(DEV)
    targets = torch.randn(2, 1, 1, g, model.num_output_channels, generator=gen).to(DEV)
    loss_fn = WeightedMSELoss(torch.rand(g, generator=gen) + 0.1, torch.rand(model.num_output_channels, generator=gen) + 0.5).to(DEV)
    roll = RolloutModel(model, idx, 2)

    def eager_step():  # (in a function: no autograd graph of it may be alive at the capture)
        for p in model.parameters():
            p.grad = None
        loss = loss_fn(roll(x), targets)
        loss.backward()
        return loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}

    want_loss, want = eager_step()
    graphed = GraphedTrainStep(roll, loss_fn, torch.zeros_like(x), torch.zeros_like(targets))
    loss = graphed(x, targets)
    assert torch.equal(loss, want_loss)
    for k, gr in want.items():
        assert torch.equal(model.get_parameter(k).grad, gr), k


NORMALIZER = ("normalizer", "anemoi.models.preprocessing.normalizer.InputNormalizer", None)


@pytest.mark.parametrize("with_imputer", [False, True])
def test_predict_step_with_a_leaky_list_stays_fused(graph_o32, golden_interface, monkeypatch, with_imputer):
    """Normaliser (+ imputer) and a bounding list with leaky and normalised classes: the fused route is kept -- the trail shows
    ``anemoi_bound_output_leaky`` -- and agrees with the generic route (``ANEMOI_AMD_FUSE_NORMALIZER=0``) as the fused routes of
    the hard classes do (tests/test_gpu_impute_io.py: 1e-5 of the largest entry, NaN maps identical)."""
    from anemoi_models_amd import trail
    from anemoi_models_amd.utils.presets import model_config

    gold = golden_interface
    cfg = model_config("GraphTransformer", 64, 4, 16)
    cfg["model"]["bounding"] = [dict(b) for b in LEAKY_LIST]
    iface = ir.build_case_interface(graph_o32, gold, 1, config=cfg, processors=None if with_imputer else [NORMALIZER])
    iface.load_state_dict(split_prefix(gold, "sd."))
    iface = iface.to(DEV).eval()
    fix = ir.fixture.load()
    batch1 = (ir.batch1_of(gold, fix, 1) if with_imputer else gold["batch"]).to(DEV)
    batch2 = (fix["batch2"] if with_imputer else gold["batch"] * 1.25).to(DEV)
    iface.predict_step(batch1)  # (the first call is generic: it fixes the NaN map / checks the first batch)
    assert iface._fused_route(batch2) is not None
    with trail.record() as launches:
        fused = iface.predict_step(batch2)
    names = {n.split(":")[0] for n in launches.names()}
    assert "anemoi_bound_output_leaky" in names and "anemoi_bound_output" not in names
    assert ("anemoi_finalize_output_imputed" in names) == with_imputer
    monkeypatch.setenv("ANEMOI_AMD_FUSE_NORMALIZER", "0")
    assert iface._fused_route(batch2) is None
    generic = iface.predict_step(batch2)

    def routes_agree(a, b):
        err = _rel(a, b)
        print(f"predict_step, leaky list, imputer={with_imputer}: fused against generic {err:.3e}")
        assert err < 1e-5

    ir.assert_matches(fused, generic.cpu(), routes_agree)
    assert bool(torch.isnan(generic).any()) == with_imputer
