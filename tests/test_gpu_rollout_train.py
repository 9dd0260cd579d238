"""Rollout training on the HIP kernels: the differentiable state advance, the input gradients of the one-pass I/O kernels, the
weighted MSE and ``training.RolloutModel`` -- against the plain-torch restatements of tests/_rollout_ref.py (f32 for the pure
copies: exact; f64 CPU autograd for the arithmetic) on the golden weights of config 1."""

import pytest
import torch

import _rollout_ref as rr
from conftest import split_prefix

pytestmark = pytest.mark.gpu

DEV = "cuda"
KW = dict(num_heads=16, num_layers=4, num_chunks=2, prognostic_in=list(range(10)), prognostic_out=list(range(10)))
COLMAP = [3, -1, 0, -2, 4, -3, -1]  # V_in = 7, V_out = 5, F = 2: prognostic, persisting and forcing columns interleaved


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# --------------------------------------------------------------------------------------------------- the state advance
@pytest.mark.parametrize("forcing", [True, False])
@pytest.mark.parametrize("g", [1031, 1032])  # Ens * G * V_in odd (element-wise time shift) / a multiple of 4 (16-byte pieces)
@pytest.mark.parametrize("t", [1, 2, 3])
def test_advance_input_forward_and_backward_are_exact(t, g, forcing):
    from anemoi_models_amd import autograd, ops

    gen = _gen(t * 10 + forcing)
    x = torch.randn((2, t, 1, g, 7), generator=gen)
    y = torch.randn((2, 1, g, 5), generator=gen)
    f = torch.randn((2, 1, g, 2), generator=gen) if forcing else None
    dz = torch.randn(x.shape, generator=gen)
    cmap = torch.tensor(COLMAP, dtype=torch.int32, device=DEV)
    xd, yd = x.to(DEV).requires_grad_(), y.to(DEV).requires_grad_()
    fd = None if f is None else f.to(DEV)
    out = autograd.advance_input(xd, yd, cmap, fd)
    assert out.data_ptr() != xd.data_ptr() and torch.equal(xd.detach().cpu(), x)  # out of place
    assert torch.equal(out.detach(), ops.advance_input(x.to(DEV).clone(), y.to(DEV), cmap, fd))
    with torch.no_grad():
        assert torch.equal(autograd.advance_input(xd, yd, cmap, fd), out.detach())
    out.backward(dz.to(DEV))
    xr, yr = x.clone().requires_grad_(), y.clone().requires_grad_()
    want = rr.advance(xr, yr, COLMAP, f)
    assert torch.equal(out.detach().cpu(), want.detach())
    want.backward(dz)
    assert torch.equal(xd.grad.cpu(), xr.grad)
    assert torch.equal(yd.grad.cpu(), yr.grad)


def test_advance_input_refuses_a_colmap_with_a_repeated_output_column():
    from anemoi_models_amd import autograd

    x = torch.zeros((1, 2, 1, 8, 3), device=DEV, requires_grad=True)
    y = torch.zeros((1, 1, 8, 2), device=DEV)
    with pytest.raises(ValueError, match="feeds input columns"):
        autograd.advance_input(x, y, torch.tensor([1, 1, -1], dtype=torch.int32, device=DEV))


# --------------------------------------------------------------------------- input gradients of the one-pass I/O kernels
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("v", [7, 8])  # element-wise / four columns per thread
def test_assemble_nodes_backward_is_the_slice_and_cast(dtype, v):
    from anemoi_models_amd import ops

    b, t, ens, g = 2, 2, 1, 1031
    full = torch.randn((b * ens * g, 24), generator=_gen(v)).to(dtype).to(DEV)
    for grad in (full, full[:, :20]):  # the whole buffer / a slice of it: leading dimension 24 > the used width
        dx = ops.assemble_nodes_backward(grad, (b, t, ens, g, v))
        want = grad[:, : t * v].float().reshape(b, ens, g, t, v).permute(0, 3, 1, 2, 4)
        assert dx.dtype == torch.float32 and dx.is_contiguous() and torch.equal(dx, want)
    with pytest.raises(ValueError):
        ops.assemble_nodes_backward(full[:, :10], (b, t, ens, g, v))


@pytest.mark.parametrize("t", [1, 2])
@pytest.mark.parametrize("g", [1031, 1032])
def test_prognostic_residual_backward_is_the_scatter_into_the_last_slice(t, g):
    from anemoi_models_amd import ops

    b, v_in = 2, 7
    dy = torch.randn((b, 1, g, 5), generator=_gen(g + t)).to(DEV)
    for src in ([2, -1, 0, 6, -1], [2, 2, -1, 0, 2]):  # a bijection / one input column feeding several output columns
        dx = ops.prognostic_residual_backward(dy, torch.tensor(src, dtype=torch.int32, device=DEV), (b, t, 1, g, v_in))
        want = torch.zeros((b, t, 1, g, v_in), device=DEV)
        for c, s in enumerate(src):  # (in output-column order, as the kernel sums)
            if s >= 0:
                want[:, -1, :, :, s] += dy[..., c]
        assert torch.equal(dx, want), src


def test_fused_io_functions_return_the_input_gradient():
    """training._AssembleNodes / _PrognosticResidual with an input that requires a gradient: dx is the un-permuted slice of the
    incoming gradient / the prognostic columns of it, the other gradients as before."""
    from anemoi_models_amd import training

    b, t, g, v = 2, 2, 1031, 6
    gen = _gen(3)
    x = torch.randn((b, t, 1, g, v), generator=gen).to(DEV).requires_grad_()
    latlons = torch.randn((g, 4), generator=gen).to(DEV)
    tr = torch.randn((g, 3), generator=gen).to(DEV).requires_grad_()
    out = training._AssembleNodes.apply(x, latlons, tr, torch.bfloat16, 64)
    grad = torch.randn(out.shape, generator=gen).to(torch.bfloat16).to(DEV)
    out.backward(grad)
    assert torch.equal(x.grad, grad[:, : t * v].float().reshape(b, 1, g, t, v).permute(0, 3, 1, 2, 4))
    assert torch.equal(tr.grad, grad[:, t * v + 4 : t * v + 7].float().reshape(b, g, 3).sum(0))
    src = torch.tensor([1, -1, 4, 0], dtype=torch.int32, device=DEV)
    o = torch.randn((b * g, 4), generator=gen).to(DEV).requires_grad_()
    x.grad = None
    y = training._PrognosticResidual.apply(o, x, src, (b, 1, g, 4))
    want_y = o.detach().reshape(b, 1, g, 4).clone()
    want_y[..., [0, 2, 3]] += x.detach()[:, -1][..., [1, 4, 0]]
    assert torch.equal(y.detach(), want_y)
    gy = torch.randn(y.shape, generator=gen).to(DEV)
    y.backward(gy)
    want = torch.zeros_like(x)
    want[:, -1][..., [1, 4, 0]] = gy[..., [0, 2, 3]]
    assert torch.equal(x.grad, want) and torch.equal(o.grad, gy.reshape(b * g, 4))


# --------------------------------------------------------------------------------------------------- the loss
def _loss_case(rows, g, v, masked, seed=0):
    gen = _gen(seed + rows + v)
    pred = torch.randn((rows // g, g, v), generator=gen)
    target = torch.randn((rows // g, g, v), generator=gen)
    node_w = torch.rand(g, generator=gen) + 0.1
    var_w = torch.rand(v, generator=gen) + 0.5
    mask = None
    if masked:
        mask = (torch.rand((g, v), generator=gen) > 0.08).float()  # at most 10 % masked (exactly: see the assertion below)
        if g * v == 1:
            mask[:] = 1.0
    return pred, target, node_w, var_w, mask


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("rows,g,v", [(2 * 1031, 1031, 5), (257, 257, 80), (1, 1, 1)])
def test_weighted_mse_loss_and_gradient_vs_f64(rows, g, v, masked):
    """Loss: relative error against the f64 restatement at most 4 x that of torch's own f32 evaluation of the same formula on
    the CPU (or 2e-6 if that is smaller).  Gradient: at most 1e-6 of max |dpred| (a handful of f32 roundings, 2^-24 each)."""
    from anemoi_models_amd import WeightedMSELoss

    pred, target, node_w, var_w, mask = _loss_case(rows, g, v, masked)
    p64 = pred.double().requires_grad_()
    ref64 = rr.weighted_mse(p64, target.double(), node_w.double(), var_w.double(), mask)
    ref64.backward()
    cpu32 = rr.weighted_mse(pred, target, node_w, var_w, mask)
    loss_fn = WeightedMSELoss(node_w, var_w).to(DEV)
    pd = pred.to(DEV).requires_grad_()
    md = None if mask is None else mask.to(DEV)
    loss = loss_fn(pd, target.to(DEV), md)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    loss.backward()
    err = abs(float(loss.detach()) - float(ref64.detach())) / abs(float(ref64.detach()))
    err_cpu = abs(float(cpu32) - float(ref64.detach())) / abs(float(ref64.detach()))
    gerr = float((pd.grad.cpu().double() - p64.grad).abs().max() / p64.grad.abs().max())
    print(f"weighted_mse rows={rows} V={v} masked={masked}: loss rel err kernel {err:.3e}, torch f32 CPU {err_cpu:.3e}; "
          f"gradient rel err {gerr:.3e}")
    assert err <= max(4 * err_cpu, 2e-6)
    assert gerr <= 1e-6
    if mask is not None:
        assert bool((pd.grad.cpu()[:, mask == 0] == 0).all())
    # the same inputs give the same bits
    pd2 = pred.to(DEV).requires_grad_()
    loss2 = loss_fn(pd2, target.to(DEV), md)
    loss2.backward()
    assert torch.equal(loss2.detach(), loss.detach()) and torch.equal(pd2.grad, pd.grad)


def test_weighted_mse_mask_is_a_select():
    """target = NaN exactly where the mask is 0 (an imputer's case): finite loss, gradient exactly 0 there; one unmasked NaN
    makes the loss NaN.  A leading rollout axis is part of the mean."""
    from anemoi_models_amd import WeightedMSELoss
    from anemoi_models_amd import autograd

    g, v = 1031, 5
    pred, target, node_w, var_w, mask = _loss_case(3 * g, g, v, True, seed=1)
    assert 0 < int((mask == 0).sum()) <= 0.1 * mask.numel()
    pred, target = pred.reshape(3, 1, 1, g, v), target.reshape(3, 1, 1, g, v)
    clean = float(rr.weighted_mse(pred.double(), target.double(), node_w.double(), var_w.double(), mask))
    err_cpu = abs(float(rr.weighted_mse(pred, target, node_w, var_w, mask)) - clean) / abs(clean)
    target = torch.where(mask != 0, target, torch.full((), float("nan")))
    loss_fn = WeightedMSELoss(node_w, var_w).to(DEV)
    pd = pred.to(DEV).requires_grad_()
    loss = loss_fn(pd, target.to(DEV), mask.to(DEV))
    loss.backward()
    assert bool(torch.isfinite(loss)) and abs(float(loss.detach()) - clean) / abs(clean) <= max(4 * err_cpu, 2e-6)  # (the bound of the test above)
    assert bool(torch.isfinite(pd.grad).all()) and bool((pd.grad.cpu()[..., mask == 0] == 0).all())
    assert bool((pd.grad.cpu()[..., mask != 0] != 0).any())
    assert bool(torch.isnan(loss_fn(pd.detach(), target.to(DEV))))  # without the mask the NaNs are in
    one = torch.ones_like(mask).to(DEV)
    t2 = torch.where(torch.isnan(target), torch.zeros(()), target).to(DEV)
    t2[2, 0, 0, 1030, 4] = float("nan")  # the very last element
    assert bool(torch.isnan(loss_fn(pd.detach(), t2, one)))
    # the functional form: no rows at all is a loss of 0
    w = torch.ones(g, device=DEV)
    empty = torch.zeros((0, g, v), device=DEV)
    assert float(autograd.weighted_mse(empty, empty, w, torch.ones(v, device=DEV))) == 0.0
    with pytest.raises(RuntimeError, match="CPU tensor"):
        autograd.weighted_mse(pred, target, node_w, var_w)


# --------------------------------------------------------------------------------------------------- the whole model
def _fresh(graph, gold, idx_out=None):
    from test_gpu_parity import _build

    model, idx = _build(graph, 64, 4)
    model.load_state_dict(split_prefix(gold, "sd."))
    return model.to(DEV).train(), idx


@pytest.fixture(scope="module")
def rollout_case(golden_cfg1_gt, graph_o32):
    """Inputs, loss weights and the f64 CPU autograd reference (loss, parameter and input gradients) of 1 and 3 steps."""
    from test_oracle_golden import graph_tensors

    from anemoi_models_amd.utils.indices import SimpleDataIndices, advance_colmap

    gold = golden_cfg1_gt
    sd = split_prefix(gold, "sd.")
    graph = {k: (v.double() if v.is_floating_point() else v) for k, v in graph_tensors(graph_o32).items()}
    colmap = advance_colmap(SimpleDataIndices(n_prognostic=10, n_forcing=2, n_diagnostic=1)).tolist()
    gen = _gen(11)
    g, v_out = gold["y"].shape[-2], gold["y"].shape[-1]
    case = {"x": gold["x"], "targets": torch.randn((3,) + tuple(gold["y"].shape), generator=gen),
            "node_w": torch.rand(g, generator=gen) + 0.1, "var_w": torch.rand(v_out, generator=gen) + 0.5, "ref": {}}
    for n in (1, 3):
        rsd = {k: (v.double().requires_grad_() if v.is_floating_point() else v) for k, v in sd.items()}
        x64 = gold["x"].double().requires_grad_()
        y = rr.rollout(rsd, graph, x64, n, colmap, **KW)
        loss = rr.weighted_mse(y, case["targets"][:n].double(), case["node_w"].double(), case["var_w"].double())
        loss.backward()
        grads = {k: t.grad.float() for k, t in rsd.items() if t.is_floating_point() and t.grad is not None
                 and float(t.grad.abs().max()) > 0}
        case["ref"][n] = (float(loss.detach()), grads, x64.grad.float(), y.detach().float())
    return case


def _rollout_step(graph, gold, case, n, x_grad=False):
    """One training step of RolloutModel on a fresh model: (loss, parameter gradients, input gradient, output)."""
    from anemoi_models_amd import WeightedMSELoss
    from anemoi_models_amd.training import RolloutModel

    model, idx = _fresh(graph, gold)
    loss_fn = WeightedMSELoss(case["node_w"], case["var_w"]).to(DEV)
    x = case["x"].to(DEV)
    if x_grad:
        x.requires_grad_()
    y = RolloutModel(model, idx, n)(x)
    loss = loss_fn(y, case["targets"][:n].to(DEV))
    loss.backward()
    grads = {k: p.grad.float().clone() for k, p in model.named_parameters() if p.grad is not None}
    return float(loss.detach()), grads, (x.grad.clone() if x_grad else None), y.detach().float()


def _check_grads(got, want, tol, floor, what):
    scale_all = max(float(g.abs().max()) for g in want.values())
    worst = 0.0
    for k, g in want.items():
        if k not in got:
            continue  # (buffers of the module -- the sin / cos coordinates -- carry no .grad)
        err = float((got[k].cpu() - g.cpu()).abs().max())
        bound = tol * max(float(g.abs().max()), floor * scale_all)
        worst = max(worst, err / bound)
        assert err <= bound, (what, k, err, float(g.abs().max()))
    print(f"{what}: worst parameter-gradient error {worst:.3f} of its bound (tol {tol:g})")
    return worst


@pytest.mark.parametrize("n", [1, 3])
def test_rollout_training_step_vs_oracle_autograd(rollout_case, golden_cfg1_gt, graph_o32, monkeypatch, n):
    """Loss, every used parameter gradient and the input gradient of an n-step rollout against f64 CPU autograd of the
    restated rollout, in the bound form of test_whole_model_training_step_vs_oracle_autograd: 5e-3 for one step, 3 x that
    for three (the per-step errors add to first order)."""
    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "fp32")
    tol = 5e-3 * n
    loss, grads, dx, y = _rollout_step(graph_o32, golden_cfg1_gt, rollout_case, n, x_grad=True)
    want_loss, want, want_dx, want_y = rollout_case["ref"][n]
    assert y.shape == want_y.shape == (n,) + tuple(golden_cfg1_gt["y"].shape)
    used = [k for k in want if k in grads]
    assert len(used) > 50
    print(f"rollout n_steps={n} f32: loss {loss:.6f} (f64 oracle {want_loss:.6f}, rel err {abs(loss - want_loss) / abs(want_loss):.2e})")
    assert abs(loss - want_loss) <= tol * abs(want_loss)
    assert float((y.cpu() - want_y).abs().max()) <= tol * float(want_y.abs().max())
    _check_grads(grads, want, tol, 0.02, f"rollout n_steps={n} f32 vs f64 oracle")
    derr = float((dx.cpu() - want_dx).abs().max())
    print(f"rollout n_steps={n} f32: input-gradient error {derr / float(want_dx.abs().max()):.2e} of max |dx|")
    assert derr <= tol * float(want_dx.abs().max())


def test_rollout_training_step_bf16_vs_f32(rollout_case, golden_cfg1_gt, graph_o32, monkeypatch):
    """The 3-step rollout in bf16 (input assembled by anemoi_assemble_nodes from step 2 on, its gradient from
    anemoi_assemble_nodes_backward) against the f32 run: the bound form of the bf16-vs-fp32 training test (8e-2, floor 0.05),
    times the three steps."""
    res = {}
    for mode in ("fp32", "bf16"):
        monkeypatch.setenv("ANEMOI_AMD_DTYPE", mode)
        res[mode] = _rollout_step(graph_o32, golden_cfg1_gt, rollout_case, 3, x_grad=True)
    tol = 8e-2 * 3
    (l32, g32, dx32, _), (l16, g16, dx16, _) = res["fp32"], res["bf16"]
    print(f"rollout n_steps=3: loss bf16 {l16:.6f}, f32 {l32:.6f}")
    assert abs(l16 - l32) <= tol * abs(l32)
    assert set(g16) == set(g32)
    _check_grads(g16, g32, tol, 0.05, "rollout n_steps=3 bf16 vs f32")
    assert float((dx16 - dx32).abs().max()) <= tol * float(dx32.abs().max())


def test_one_step_rollout_is_the_single_step(rollout_case, golden_cfg1_gt, graph_o32, monkeypatch):
    """n_steps = 1: output and every gradient bit-equal to model(x) followed by autograd.weighted_mse -- the rollout adds
    nothing to a single step."""
    from anemoi_models_amd import WeightedMSELoss, autograd
    from anemoi_models_amd.training import RolloutModel

    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "fp32")
    case = rollout_case
    model, idx = _fresh(graph_o32, golden_cfg1_gt)
    loss_fn = WeightedMSELoss(case["node_w"], case["var_w"]).to(DEV)
    x, target = case["x"].to(DEV), case["targets"][0].to(DEV)
    y1 = RolloutModel(model, idx, 1)(x)
    l1 = loss_fn(y1, target[None])
    l1.backward()
    g1 = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    for p in model.parameters():
        p.grad = None
    y0 = model(x)
    l0 = autograd.weighted_mse(y0, target, loss_fn.node_weights, loss_fn.variable_weights, None, 1.0 / y0.shape[-1])
    l0.backward()
    assert y1.shape == (1,) + tuple(y0.shape) and torch.equal(y1[0].detach(), y0.detach()) and torch.equal(l1.detach(), l0.detach())
    g0 = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    assert set(g0) == set(g1) and len(g0) > 20
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    with torch.no_grad():  # and without a graph the same loop gives the same numbers
        y3 = RolloutModel(model, idx, 3)(x)
    assert not y3.requires_grad and y3.shape[0] == 3
    with pytest.raises(NotImplementedError):
        RolloutModel(model, idx, 2)(x, model_comm_group=object())


def test_gradient_crosses_the_seam_and_both_routes_agree(rollout_case, golden_cfg1_gt, graph_o32, monkeypatch):
    """The 3-step gradients differ from those of a run whose state is detached between the steps; the fused input-gradient
    route and ANEMOI_AMD_ROLLOUT_FUSED=0 (the generic torch route) agree within 1e-5 in f32; a direct model(x) with an
    input that requires a gradient keeps the generic route bit for bit."""
    from anemoi_models_amd import WeightedMSELoss, autograd, training
    from anemoi_models_amd.utils.indices import advance_colmap

    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "fp32")
    case = rollout_case
    loss_f, g_fused, dx_fused, y_fused = _rollout_step(graph_o32, golden_cfg1_gt, case, 3, x_grad=True)
    monkeypatch.setenv("ANEMOI_AMD_ROLLOUT_FUSED", "0")
    loss_g, g_generic, dx_generic, y_generic = _rollout_step(graph_o32, golden_cfg1_gt, case, 3, x_grad=True)
    monkeypatch.delenv("ANEMOI_AMD_ROLLOUT_FUSED")
    # (the forward arithmetic is the same on both routes: f32 rounding noise at the most)
    assert float((y_fused - y_generic).abs().max()) <= 1e-6 * float(y_generic.abs().max()) and abs(loss_f - loss_g) <= 1e-6 * abs(loss_g)
    _check_grads(g_fused, g_generic, 1e-5, 0.02, "fused vs generic input-gradient route")
    assert float((dx_fused - dx_generic).abs().max()) <= 1e-5 * float(dx_generic.abs().max())
    # the state detached between the steps
    model, idx = _fresh(graph_o32, golden_cfg1_gt)
    loss_fn = WeightedMSELoss(case["node_w"], case["var_w"]).to(DEV)
    cmap = advance_colmap(idx).to(DEV)
    x, outs = case["x"].to(DEV), []
    for s in range(3):
        outs.append(model(x))
        x = autograd.advance_input(x, outs[-1].detach(), cmap)
    loss_fn(torch.stack(outs), case["targets"].to(DEV)).backward()
    scale_all = max(float(g.abs().max()) for g in g_fused.values())
    gap = max(float((p.grad - g_fused[k]).abs().max()) for k, p in model.named_parameters() if p.grad is not None)
    print(f"seam: largest parameter-gradient difference to the detached run {gap / scale_all:.3e} of the largest gradient")
    assert gap > 1e-3 * scale_all
    # a direct call with an input gradient: the generic route, with and without the switch
    dy = torch.randn(golden_cfg1_gt["y"].shape, generator=_gen(2)).to(DEV)
    res = []
    for env in (None, "0"):
        if env is not None:
            monkeypatch.setenv("ANEMOI_AMD_ROLLOUT_FUSED", env)
        for p in model.parameters():
            p.grad = None
        xg = case["x"].to(DEV).requires_grad_()
        assert not training._fused_io(xg)
        model(xg).backward(dy)
        res.append((xg.grad.clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}))
    assert torch.equal(res[0][0], res[1][0]) and all(torch.equal(res[0][1][k], res[1][1][k]) for k in res[0][1])


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_whole_model_input_gradient_on_the_fused_route(rollout_case, golden_cfg1_gt, graph_o32, monkeypatch, mode):
    """d loss / d x of ONE step with the one-pass I/O kernels kept (training.rollout_input_grad): f32 against the f64 oracle
    (5e-3 of max |dx|), bf16 -- where the input is assembled by anemoi_assemble_nodes -- against the f32 run (8e-2)."""
    from anemoi_models_amd import WeightedMSELoss, training

    case = rollout_case
    loss_fn = WeightedMSELoss(case["node_w"], case["var_w"]).to(DEV)

    def run(m):
        monkeypatch.setenv("ANEMOI_AMD_DTYPE", m)
        model, _ = _fresh(graph_o32, golden_cfg1_gt)
        x = case["x"].to(DEV).requires_grad_()
        with training.rollout_input_grad():
            assert training._fused_io(x)
            y = model(x)
        assert not training._fused_io(x)
        loss_fn(y[None], case["targets"][:1].to(DEV)).backward()
        return x.grad.cpu()

    want = rollout_case["ref"][1][2] if mode == "fp32" else run("fp32")
    tol = 5e-3 if mode == "fp32" else 8e-2
    got = run(mode)
    err = float((got - want).abs().max()) / float(want.abs().max())
    print(f"one-step input gradient on the fused route, {mode}: error {err:.3e} of max |dx|")
    assert err <= tol


def test_graphed_rollout_train_step_equals_eager(rollout_case, golden_cfg1_gt, graph_o32, monkeypatch):
    """runtime.GraphedTrainStep(RolloutModel(...), loss, x, targets): a replay is bit-equal to the eager step, two replays are
    bit-equal."""
    from anemoi_models_amd import WeightedMSELoss
    from anemoi_models_amd.runtime import GraphedTrainStep
    from anemoi_models_amd.training import RolloutModel

    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "fp32")
    case = rollout_case
    model, idx = _fresh(graph_o32, golden_cfg1_gt)
    roll = RolloutModel(model, idx, 3)
    loss_fn = WeightedMSELoss(case["node_w"], case["var_w"]).to(DEV)
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
