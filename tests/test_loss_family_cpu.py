"""The loss family, the parts that need no GPU: the plain-torch restatement (tests/_loss_family_ref.py) against hand-computed
values, the argument checks of anemoi_weighted_error / _backward through the C ABI, the workspace size as a function of the
shape alone, and what ValidationMetrics refuses."""

import math
import warnings

import numpy as np
import pytest
import torch

import _loss_family_ref as lf


def _f64(*vals):
    return torch.tensor(vals, dtype=torch.float64)


def test_restated_pointwise_functions_on_hand_computed_values():
    """f and (through autograd) f' of every kind at d = 0, at the Huber corner |d| = delta, on both Huber branches, and at
    |d| = 100 for log-cosh: finite and equal to 100 - ln 2 to f64 rounding."""
    d = _f64(0.0, 3.0, -2.0, 0.5, 1.5, -1.5, 100.0, -100.0).requires_grad_()
    cases = {
        "mse": ([0.0, 9.0, 4.0, 0.25, 2.25, 2.25, 1e4, 1e4], [0.0, 6.0, -4.0, 1.0, 3.0, -3.0, 200.0, -200.0]),
        "mae": ([0.0, 3.0, 2.0, 0.5, 1.5, 1.5, 100.0, 100.0], [0.0, 1.0, -1.0, 1.0, 1.0, -1.0, 1.0, -1.0]),  # sign(0) = 0
        # delta = 1.5: 0.5 d^2 up to and at the corner (1.125 on either branch), 1.5 (|d| - 0.75) beyond
        "huber": ([0.0, 3.375, 1.875, 0.125, 1.125, 1.125, 148.875, 148.875], [0.0, 1.5, -1.5, 0.5, 1.5, -1.5, 1.5, -1.5]),
        "logcosh": ([0.0] + [math.log(math.cosh(x)) for x in (3.0, 2.0, 0.5, 1.5, 1.5)] + [100.0 - math.log(2.0)] * 2,
                    [math.tanh(x) for x in (0.0, 3.0, -2.0, 0.5, 1.5, -1.5, 100.0, -100.0)]),
    }
    assert sorted(cases) == sorted(lf.KINDS)
    for kind, (want, want_grad) in cases.items():
        got = lf.pointwise(kind, d, 1.5)
        (grad,) = torch.autograd.grad(got.sum(), d)
        assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(grad).all()), kind
        torch.testing.assert_close(got.detach(), _f64(*want), rtol=1e-14, atol=1e-15, msg=kind)
        torch.testing.assert_close(grad, _f64(*want_grad), rtol=1e-14, atol=1e-15, msg=kind)
    assert float(lf.pointwise("logcosh", _f64(0.0))) == 0.0
    assert abs(float(lf.pointwise("logcosh", _f64(100.0))) - (100.0 - math.log(2.0))) <= 2 ** -52 * 100.0
    assert bool(torch.isfinite(lf.pointwise("logcosh", torch.tensor([100.0, 1e4]))).all())  # f32 too: no overflow
    with pytest.raises(ValueError):
        lf.pointwise("l3", d)


def test_restated_weighted_error_on_a_hand_written_case():
    """[2 groups x (B = 2) x (G = 2), V = 2]: row weights wrap inside a group, column weights, the scale of the difference,
    the scale of the result and a mask over a NaN target -- group by group, variable by variable."""
    pred = _f64(1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0).reshape(2, 2, 2, 2)
    target = torch.zeros_like(pred)
    target[1, 1] = _f64(3.0, float("nan"), 1.0, 5.0).reshape(2, 2)
    row_w, col_w, c = _f64(1.0, 10.0), _f64(1.0, 0.5), _f64(2.0, 1.0)
    mask = _f64(1.0, 0.0, 1.0, 1.0).reshape(2, 2)  # (g = 0, v = 1) is masked: the NaN sits there in group 1
    p = pred.clone().requires_grad_()
    got = lf.weighted_error(p, target, row_w, "mae", col_w=col_w, mask=mask, diff_scale=c, n_groups=2, scale=0.25)
    # group 0, v = 0: rows (g0, g1, g0, g1) = |2 * (1, 3, 5, 7)| weighted (1, 10, 1, 10) -> 2 + 60 + 10 + 140 = 212
    # group 0, v = 1: g = 0 masked -> 10 * 0.5 * (4 + 8) = 60
    # group 1, v = 0: rows 0, 0 then |2 * (1 - 3)| = 4 and |2 * (1 - 1)| = 0 -> 4;  v = 1: only g = 1 of the last row: 10 * 0.5 * 4
    torch.testing.assert_close(got.detach(), 0.25 * _f64(212.0, 60.0, 4.0, 20.0).reshape(2, 2), rtol=1e-15, atol=0)
    up = _f64(1.0, 2.0, 3.0, 4.0).reshape(2, 2)
    (grad,) = torch.autograd.grad((got * up).sum(), p)
    assert bool(torch.isfinite(grad).all()) and bool((grad[:, :, 0, 1] == 0).all())  # masked: exactly 0, NaN or not
    assert float(grad[1, 1, 1, 0]) == 0.0 and float(grad[1, 0, 1, 0]) == 0.0  # pred == target: sign(0) = 0
    assert float(grad[0, 0, 1, 0]) == 0.25 * 1.0 * 10.0 * 1.0 * 2.0  # scale * upstream * row_w * col_w * c * sign
    assert float(grad[1, 1, 0, 0]) == -(0.25 * 3.0 * 1.0 * 1.0 * 2.0)
    # the module contract: w^ = w / sum(w), the mean over the leading axes that are not kept, RMSE per variable / squashed
    per_var = lf.loss("mse", pred, torch.zeros_like(pred), row_w, squash=False, lead_dims=1)
    want00 = (1.0 * (1.0 + 25.0) + 10.0 * (9.0 + 49.0)) / 11.0 / 2.0
    assert per_var.shape == (2, 2) and abs(float(per_var[0, 0]) - want00) <= 1e-14 * want00
    torch.testing.assert_close(lf.loss("rmse", pred, torch.zeros_like(pred), row_w, squash=False, lead_dims=1), per_var.sqrt())
    torch.testing.assert_close(lf.loss("rmse", pred, torch.zeros_like(pred), row_w), per_var.mean().sqrt())
    torch.testing.assert_close(lf.loss("mse", pred, torch.zeros_like(pred), row_w), per_var.mean())


def test_loss_family_entry_points_validate_without_gpu():
    """Null pointers, rows that are no multiple of n_groups * G, G * V >= 2^31, an unknown kind, a Huber delta <= 0 and a short
    workspace come back as status codes with a message before anything is launched."""
    from anemoi_models_amd import _lib

    lib = _lib.load()
    bad, p = _lib.ANEMOI_ERR_INVALID, 4096  # p: a non-null pointer value that is never dereferenced by the checks
    mse, huber = _lib.LOSS_KINDS["mse"], _lib.LOSS_KINDS["huber"]
    assert sorted(_lib.LOSS_KINDS.values()) == [0, 1, 2, 3]
    fwd, bwd = lib.anemoi_weighted_error, lib.anemoi_weighted_error_backward
    ws = lib.anemoi_weighted_error_workspace_floats(2, 8, 3)
    assert ws > 0
    assert fwd(mse, 1.0, None, None, 16, 3, 4, 2, None, None, None, None, 1.0, None, None, 0, None) == bad
    assert b"anemoi_weighted_error: null pointer" in lib.anemoi_last_error()
    assert fwd(mse, 1.0, p, p, 16, 3, 4, 2, p, None, None, None, 1.0, None, p, ws, None) == bad  # out
    assert b"null pointer (out)" in lib.anemoi_last_error()
    assert fwd(mse, 1.0, p, p, 12, 3, 4, 2, p, None, None, None, 1.0, p, p, ws, None) == bad  # 12 rows: not 2 groups of k * 4
    assert b"rows 12 is not a multiple of n_groups * G = 2 * 4" in lib.anemoi_last_error()
    assert fwd(mse, 1.0, p, p, 18, 3, 3, 4, p, None, None, None, 1.0, p, p, ws, None) == bad
    assert fwd(mse, 1.0, p, p, -8, 3, 4, 2, p, None, None, None, 1.0, p, p, ws, None) == bad
    assert fwd(mse, 1.0, p, p, 16, 3, 4, 0, p, None, None, None, 1.0, p, p, ws, None) == bad
    assert fwd(mse, 1.0, p, p, 1 << 24, 256, 1 << 23, 2, p, None, None, None, 1.0, p, p, 1 << 40, None) == _lib.ANEMOI_ERR_UNSUPPORTED
    assert b"G * V does not fit 31 bits" in lib.anemoi_last_error()
    assert fwd(7, 1.0, p, p, 16, 3, 4, 2, p, None, None, None, 1.0, p, p, ws, None) == bad
    assert b"unknown kind 7" in lib.anemoi_last_error()
    assert fwd(-1, 1.0, p, p, 16, 3, 4, 2, p, None, None, None, 1.0, p, p, ws, None) == bad
    for delta in (0.0, -1.0, float("nan")):
        assert fwd(huber, delta, p, p, 16, 3, 4, 2, p, None, None, None, 1.0, p, p, ws, None) == bad
        assert b"delta must be positive" in lib.anemoi_last_error()
    assert fwd(mse, 1.0, p, p, 16, 3, 4, 2, p, None, None, None, 1.0, p, p, ws - 1, None) == bad
    assert b"workspace" in lib.anemoi_last_error()
    assert fwd(mse, 1.0, p, p, 16, 3, 4, 2, p, None, None, None, 1.0, p, None, ws, None) == bad
    assert bwd(mse, 1.0, None, None, 16, 3, 4, 2, None, None, None, None, 1.0, None, None, None) == bad
    assert b"anemoi_weighted_error_backward: null pointer" in lib.anemoi_last_error()
    assert bwd(mse, 1.0, p, p, 16, 3, 4, 2, p, None, None, None, 1.0, None, p, None) == bad  # upstream
    assert b"upstream / dpred" in lib.anemoi_last_error()
    assert bwd(mse, 1.0, p, p, 16, 3, 4, 2, p, None, None, None, 1.0, p, None, None) == bad
    assert bwd(mse, 1.0, p, p, 12, 3, 4, 2, p, None, None, None, 1.0, p, p, None) == bad
    assert b"not a multiple" in lib.anemoi_last_error()
    assert bwd(9, 1.0, p, p, 16, 3, 4, 2, p, None, None, None, 1.0, p, p, None) == bad
    assert bwd(huber, 0.0, p, p, 16, 3, 4, 2, p, None, None, None, 1.0, p, p, None) == bad
    assert bwd(mse, 1.0, p, p, 1 << 24, 256, 1 << 23, 2, p, None, None, None, 1.0, p, p, None) == _lib.ANEMOI_ERR_UNSUPPORTED
    assert bwd(mse, 1.0, p, p, 0, 3, 4, 2, p, None, None, None, 1.0, p, p, None) == _lib.ANEMOI_OK  # no rows: nothing to do


def test_weighted_error_workspace_is_a_function_of_its_three_arguments():
    """One [V] partial per workgroup; the workgroup count of a group depends on (rows_per_group, V) alone and every group has
    the same: the reduction order cannot change with the device, the occupancy or the number of groups."""
    from anemoi_models_amd import _lib

    ws = _lib.load().anemoi_weighted_error_workspace_floats
    assert ws(0, 8, 3) == 0 and ws(1, 0, 3) == 0 and ws(1, 8, 0) == 0
    assert ws(1, 1, 1) == 1
    for rpg, v in [(1, 1), (514, 5), (2062, 80), (33, 257), (1031, 256), (5000, 3), (542080, 90)]:
        one = ws(1, rpg, v)
        assert one % v == 0 and 1 <= one // v <= rpg, (rpg, v)
        assert [ws(n, rpg, v) for n in (2, 3, 4, 7)] == [n * one for n in (2, 3, 4, 7)]
        assert ws(1, rpg, v) == one  # the same call, the same answer
    assert ws(1, 5000, 3) // 3 > 1  # several workgroups per group at the smallest test shape that asks for them
    counts = [ws(1, r, 80) // 80 for r in (1, 52, 1031, 542080, 4 * 542080, 64 * 542080)]
    # grows with the size up to 1024 workgroups per group (chunks are whole passes, so the last few may not be needed)
    assert counts == sorted(counts) and counts[0] == 1 and 1000 < counts[-3] <= 1024 and counts[-2:] == [1024, 1024]


def _normalizer(stdev):
    from anemoi_models_amd.preprocessing.normalizer import InputNormalizer
    from anemoi_models_amd.utils.indices import SimpleDataIndices

    idx = SimpleDataIndices(n_prognostic=2, n_forcing=2, n_diagnostic=1, names=["x", "y", "z", "q", "other"])
    n = 5
    stats = {"minimum": np.zeros(n), "maximum": np.ones(n), "mean": np.arange(n, dtype=np.float64),
             "stdev": np.asarray(stdev, dtype=np.float64)}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return InputNormalizer(config={"default": "mean-std"}, data_indices=idx, statistics=stats), idx, stats


def test_validation_metrics_takes_an_affine_normalizer_only():
    from anemoi_models_amd import ValidationMetrics
    from anemoi_models_amd.preprocessing import Processors
    from anemoi_models_amd.preprocessing.imputer import ConstantImputer

    norm, idx, stats = _normalizer([1.0, 2.0, 4.0, 8.0, 16.0])
    w = torch.ones(4)
    vm = ValidationMetrics(w, norm, groups={"sfc": [0, 2], "pl": [1]}, kinds=("mse", "rmse"))
    # the output variables are x, y (prognostic) and `other` (diagnostic): 1 / _norm_mul = their stdev
    assert vm.diff_scale.tolist() == [1.0, 2.0, 16.0] and vm.node_weights.tolist() == [0.25] * 4
    assert ValidationMetrics(w, Processors([["normalizer", norm]]), kinds=("mae",)).diff_scale.tolist() == [1.0, 2.0, 16.0]
    assert ValidationMetrics(w).diff_scale is None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        imp = ConstantImputer(config={"default": "none", 0: ["x"]}, data_indices=idx, statistics=None)
    with pytest.raises(NotImplementedError, match="not affine"):
        ValidationMetrics(w, imp)
    with pytest.raises(NotImplementedError, match="ConstantImputer"):
        ValidationMetrics(w, Processors([["normalizer", norm], ["imputer", imp]]))
    zero, _, _ = _normalizer([1.0, 2.0, 4.0, 8.0, 16.0])
    zero._norm_mul[1] = 0.0
    with pytest.raises(ValueError, match="zero or non-finite _norm_mul"):
        ValidationMetrics(w, zero)
    with pytest.raises(ValueError, match="unknown kinds"):
        ValidationMetrics(w, norm, kinds=("mse", "crps"))
    with pytest.raises(ValueError, match="node_weights"):
        ValidationMetrics(torch.zeros(4), norm)
    with pytest.raises(RuntimeError, match="CPU tensor"):  # no CPU fallback behind the metrics either
        vm(torch.zeros(2, 1, 1, 4, 3), torch.zeros(2, 1, 1, 4, 3))
    with pytest.raises(ValueError, match="must be"):
        vm(torch.zeros(2, 1, 1, 5, 3), torch.zeros(2, 1, 1, 5, 3))


def test_loss_classes_check_their_arguments_without_gpu():
    from anemoi_models_amd import WeightedHuberLoss, WeightedMAELoss, WeightedMSELoss, WeightedRMSELoss

    w = torch.tensor([1.0, 3.0])
    assert WeightedMAELoss(w).node_weights.tolist() == [0.25, 0.75] and WeightedRMSELoss(w).kind == "mse"
    assert WeightedHuberLoss(w, delta=2.5).delta == 2.5
    with pytest.raises(ValueError, match="delta must be positive"):
        WeightedHuberLoss(w, delta=0.0)
    x = torch.zeros(3, 2, 4)
    with pytest.raises(ValueError, match="lead_dims"):
        WeightedMAELoss(w)(x, x, lead_dims=2)
    with pytest.raises(ValueError, match="mask must be"):
        WeightedMSELoss(w)(x, x, torch.ones(2, 3), squash=False)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        WeightedMSELoss(w)(x, x, squash=False)
