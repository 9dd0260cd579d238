"""The ensemble scores, the parts that need no GPU: the plain-torch restatement (tests/_ensemble_ref.py) against hand values,
against the sorted identity and against the closed-form gradient, the argument checks of anemoi_ensemble_score / _backward
through the C ABI, the workspace size as a function of the shape alone, and what the classes refuse."""

import warnings

import pytest
import torch

import _ensemble_ref as er


def _f64(*vals):
    return torch.tensor(vals, dtype=torch.float64)


def test_restated_scores_on_hand_computed_values():
    """E = 2, members {0, 2}, target 1: |x_j - y| = 1 each, |x_1 - x_2| = 2, so the fair CRPS (alpha = 1) is 1 - 2 / 2 = 0 and
    the ensemble CRPS (alpha = 0, coefficient 1 / (2 E^2) on sum_{j != k} = 4) is 1 - 4 / 8 = 0.5; in between eps = (1 - alpha)
    / 2.  E = 3, members {0, 1, 5}, target 2: mean 2 -> mean_se 0; variance (4 + 1 + 9) / 2 = 7; sum_j |x_j - y| = 6, sum_{j<k}
    = 1 + 5 + 4 = 10 -> fair CRPS 6 / 3 - 10 / 6."""
    x, y = _f64(0.0, 2.0).reshape(2, 1, 1), _f64(1.0).reshape(1, 1)
    assert float(er.point_score("afcrps", x, y, 1.0)) == 0.0
    assert float(er.point_score("afcrps", x, y, 0.0)) == 0.5
    assert abs(float(er.point_score("afcrps", x, y, 0.9)) - (1.0 - (1.0 - 0.05) * 4.0 / 4.0)) <= 1e-15
    assert float(er.point_score("mean_se", x, y)) == 0.0 and float(er.point_score("variance", x, y)) == 2.0
    x, y = _f64(0.0, 1.0, 5.0).reshape(3, 1, 1), _f64(2.0).reshape(1, 1)
    assert float(er.point_score("mean_se", x, y)) == 0.0 and float(er.point_score("variance", x, y)) == 7.0
    assert abs(float(er.point_score("afcrps", x, y, 1.0)) - (2.0 - 10.0 / 6.0)) <= 1e-15
    assert abs(float(er.point_score("afcrps", x, y, 0.0)) - (2.0 - 20.0 / 18.0)) <= 1e-15
    with pytest.raises(ValueError):
        er.point_score("energy", x, y)
    # the kernel contract on [2 groups, B = 1, E = 2, G = 2, V = 2]: row / column weights, the scale c inside S (|c| for the CRPS,
    # c^2 for the squares), the result scale, and a mask over a NaN target and an Inf member
    pred = _f64(0.0, 0.0, 0.0, 0.0, 2.0, 4.0, 6.0, 8.0, 1.0, 1.0, 1.0, 1.0, 1.0, 3.0, 1.0, 1.0).reshape(2, 1, 2, 2, 2)
    target = _f64(1.0, 1.0, 1.0, 1.0, 0.0, float("nan"), 0.0, 2.0).reshape(2, 1, 2, 2)
    pred[1, 0, 0, 0, 1] = float("inf")
    row_w, col_w, c, mask = _f64(1.0, 10.0), _f64(1.0, 0.5), _f64(2.0, -1.0), _f64(1.0, 0.0, 1.0, 1.0).reshape(2, 2)
    p = pred.clone().requires_grad_()
    got = er.ensemble_score(p, target, row_w, "afcrps", 0.0, col_w, mask, c, 2, 0.25)
    # group 0: members (0, x2), target 1 -> S = (1 + |x2 - 1|) / 2 - x2 / 4: v = 0: g0 x2 = 2 -> 0.5, g1 x2 = 6 -> 1.5;
    # v = 1: g0 masked, g1 x2 = 8 -> 2.  With c: v = 0 doubles, v = 1 keeps |.|
    # group 1: v = 0: members (1, 1), target 0 -> S = 1 at both nodes; v = 1: g0 masked, g1 members (1, 1), target 2 -> 1
    want = 0.25 * _f64(2.0 * (0.5 + 10.0 * 1.5), 0.5 * 10.0 * 2.0, 2.0 * (1.0 + 10.0), 0.5 * 10.0 * 1.0).reshape(2, 2)
    torch.testing.assert_close(got.detach(), want, rtol=1e-15, atol=0)
    up = _f64(1.0, 2.0, 3.0, 4.0).reshape(2, 2)
    (grad,) = torch.autograd.grad((got * up).sum(), p)
    assert bool(torch.isfinite(grad).all()) and bool((grad[..., 0, 1] == 0).all())  # masked: exactly 0, NaN / Inf or not
    # member 2 of (l = 0, g = 1, v = 0): scale * upstream * row_w * col_w * |c| * (1 / 2 - 1 / 4)
    assert float(grad[0, 0, 1, 1, 0]) == 0.25 * 1.0 * 10.0 * 1.0 * 2.0 * 0.25
    assert bool((grad[1, 0, :, 1, 1] == 4.0 * 0.25 * 10.0 * 0.5 * 1.0 * -0.5).all())  # tied members below the target
    v = er.ensemble_score(pred, target, row_w, "variance", 1.0, None, mask, c, 2, 1.0)
    assert float(v[0, 0]) == 4.0 * (2.0 + 10.0 * 18.0) and float(v[1, 0]) == 0.0 and float(v[1, 1]) == 0.0


@pytest.mark.parametrize("e", [2, 3, 5, 8, 9, 16])
def test_restated_crps_against_the_sorted_identity(e):
    """sum_{j < k} |x_j - x_k| = sum_i (2 i - E - 1) x_(i) over the sorted members (i = 1 .. E): an evaluation of the pair term
    that shares nothing with the restatement's, in f64.  Against it: the restatement for three alphas, and its two ends against
    the textbook forms (fair: 1 / (2 E (E - 1)), ensemble: 1 / (2 E^2))."""
    gen = torch.Generator().manual_seed(40 + e)
    x = torch.randn((4, e, 7, 3), generator=gen, dtype=torch.float64) * 3.0
    y = torch.randn((4, 7, 3), generator=gen, dtype=torch.float64)
    x[0, 1] = x[0, 0]  # ties
    srt = torch.sort(x, dim=-3).values
    coef = (2.0 * torch.arange(1, e + 1, dtype=torch.float64) - e - 1).reshape(e, 1, 1)
    pair = (coef * srt).sum(-3)  # sum_{j < k}
    mae = (x - y.unsqueeze(-3)).abs().mean(-3)
    for alpha, pair_coef in [(1.0, 1.0 / (e * (e - 1))), (0.0, 1.0 / (e * e)), (0.95, (1.0 - 0.05 / e) / (e * (e - 1)))]:
        got = er.point_score("afcrps", x, y, alpha)
        want = mae - pair_coef * pair
        assert float((got - want).abs().max()) <= 1e-13 * float(mae.abs().max()), (e, alpha)


@pytest.mark.parametrize("e", [2, 3, 9, 16])
def test_restated_crps_against_the_form_the_kernel_evaluates(e):
    """csrc/ensemble.hip sums, per pair, 2 |med3(e_j, e_k, 0)| + eps |e_j - e_k| with e_j = c (x_j - y) -- anemoi-training's
    pair term |e_j| + |e_k| - (1 - eps) |e_j - e_k| with the cancellation taken out (equal signs: the two moduli less their
    difference is twice the smaller; opposite signs: it is 0).  The same number as the restatement, ties, zeros and a member far
    from the others included."""
    gen = torch.Generator().manual_seed(80 + e)
    x = torch.randn((3, e, 11, 2), generator=gen, dtype=torch.float64)
    y = torch.randn((3, 11, 2), generator=gen, dtype=torch.float64)
    x[0, 0] = y[0]  # e_0 = 0
    x[1, 1] = x[1, 0]  # a tie
    x[2, 0] += 100.0
    c = -1.5
    ej = c * (x - y.unsqueeze(1))
    for alpha in (1.0, 0.95, 0.0):
        eps = (1.0 - alpha) / e
        p = torch.zeros_like(y)
        q = torch.zeros_like(y)
        for j in range(e):
            for k in range(j + 1, e):
                med = torch.stack([ej[:, j], ej[:, k], torch.zeros_like(y)]).median(0).values
                p = p + med.abs()
                q = q + (ej[:, j] - ej[:, k]).abs()
        want = (2.0 * p + eps * q) / (e * (e - 1))
        got = er.point_score("afcrps", c * x, c * y, alpha)
        assert float((got - want).abs().max()) <= 1e-13 * float(got.abs().max()), (e, alpha)


@pytest.mark.parametrize("e", [2, 3, 8, 16])
def test_restated_crps_gradient_against_the_closed_form(e):
    """Autograd of the restatement against the gradient written out (the contract of anemoi_ensemble_score_backward), with
    exact member-member and member-target ties (sgn(0) = 0), a mask over NaN targets, a negative scale of the difference."""
    gen = torch.Generator().manual_seed(60 + e)
    n_groups, b, g, v = 2, 2, 6, 3
    y = torch.randn((n_groups, b, g, v), generator=gen, dtype=torch.float64)
    x = y.unsqueeze(-3) + torch.randn((n_groups, b, e, g, v), generator=gen, dtype=torch.float64)
    x[:, :, 0, :2] = y[:, :, :2]  # member 0 equals the target at two nodes
    x[:, :, 1, 1:4] = x[:, :, 0, 1:4]  # members 0 and 1 are equal at three nodes (one of them also the target's)
    mask = torch.ones(g, v, dtype=torch.float64)
    mask[5, 1] = 0.0
    y[..., 5, 1] = float("nan")
    x[:, :, 0, 5, 1] = float("inf")
    row_w = torch.rand(g, generator=gen, dtype=torch.float64) + 0.1
    col_w = torch.rand(v, generator=gen, dtype=torch.float64) + 0.5
    c = _f64(2.0, -0.5, 1.0)
    up = torch.randn((n_groups, v), generator=gen, dtype=torch.float64)
    for alpha in (1.0, 0.95, 0.0):
        p = x.clone().requires_grad_()
        out = er.ensemble_score(p, y, row_w, "afcrps", alpha, col_w, mask, c, n_groups, 0.5)
        (grad,) = torch.autograd.grad((out * up).sum(), p)
        want = er.closed_form_grad(x, y, row_w, up, alpha, col_w, mask, c, n_groups, 0.5)
        assert bool(torch.isfinite(grad).all()) and bool((grad[..., 5, 1] == 0).all())
        assert float((grad - want).abs().max()) <= 1e-14 * float(want.abs().max()), (e, alpha)
        # where member 0 equals the target its target term is exactly absent
        no_y = er.closed_form_grad(x, y, row_w, up, alpha, col_w, mask, c, n_groups, 0.5, target_term=False)
        assert float((grad[:, :, 0, :2] - no_y[:, :, 0, :2]).abs().max()) <= 1e-14 * float(want.abs().max())
        assert float((want[:, :, -1, 4] - no_y[:, :, -1, 4]).abs().min()) > 0  # (and present elsewhere)


def test_ensemble_entry_points_validate_without_gpu():
    """Null pointers, E = 1 and E = 17, alpha outside [0, 1] or NaN, rows that are no multiple of n_groups * G, an unknown
    kind, a short workspace and the backward of a kind without a gradient come back as status codes with a message before
    anything is launched."""
    from anemoi_models_amd import _lib

    lib = _lib.load()
    bad, unsup, p = _lib.ANEMOI_ERR_INVALID, _lib.ANEMOI_ERR_UNSUPPORTED, 4096  # p: non-null, never dereferenced by the checks
    assert _lib.ENS_KINDS == {"afcrps": 0, "mean_se": 1, "variance": 2} and _lib.ABI_VERSION >= 49
    crps, mse, var = (_lib.ENS_KINDS[k] for k in ("afcrps", "mean_se", "variance"))
    fwd, bwd = lib.anemoi_ensemble_score, lib.anemoi_ensemble_score_backward
    ws = lib.anemoi_ensemble_score_workspace_floats(2, 8, 3, 4)
    assert ws > 0
    #            kind alpha pred target rows V G E groups row_w col_w mask c scale out ws ws_floats stream
    assert fwd(crps, 1.0, None, None, 16, 3, 4, 4, 2, None, None, None, None, 1.0, None, None, 0, None) == bad
    assert b"anemoi_ensemble_score: null pointer" in lib.anemoi_last_error()
    assert fwd(crps, 1.0, p, p, 16, 3, 4, 4, 2, p, None, None, None, 1.0, None, p, ws, None) == bad
    assert b"null pointer (out)" in lib.anemoi_last_error()
    for e in (1, 0, -3):
        assert fwd(crps, 1.0, p, p, 16, 3, 4, e, 2, p, None, None, None, 1.0, p, p, ws, None) == bad
        assert b"at least 2 members" in lib.anemoi_last_error()
    assert fwd(crps, 1.0, p, p, 16, 3, 4, 17, 2, p, None, None, None, 1.0, p, p, ws, None) == unsup
    assert b"E = 17 members, at most 16" in lib.anemoi_last_error()
    for alpha in (-0.1, 1.5, float("nan")):
        for kind in (crps, mse):
            assert fwd(kind, alpha, p, p, 16, 3, 4, 4, 2, p, None, None, None, 1.0, p, p, ws, None) == bad
            assert b"alpha must lie in [0, 1]" in lib.anemoi_last_error()
        assert bwd(crps, alpha, p, p, 16, 3, 4, 4, 2, p, None, None, None, 1.0, p, p, None) == bad
    assert fwd(crps, 1.0, p, p, 12, 3, 4, 4, 2, p, None, None, None, 1.0, p, p, ws, None) == bad  # 12 rows: not 2 groups of k * 4
    assert b"rows 12 is not a multiple of n_groups * G = 2 * 4" in lib.anemoi_last_error()
    assert fwd(crps, 1.0, p, p, -8, 3, 4, 4, 2, p, None, None, None, 1.0, p, p, ws, None) == bad
    assert fwd(crps, 1.0, p, p, 16, 3, 4, 4, 0, p, None, None, None, 1.0, p, p, ws, None) == bad
    assert fwd(crps, 1.0, p, p, 1 << 24, 256, 1 << 23, 2, 2, p, None, None, None, 1.0, p, p, 1 << 40, None) == unsup
    assert b"G * V does not fit 31 bits" in lib.anemoi_last_error()
    assert fwd(3, 1.0, p, p, 16, 3, 4, 4, 2, p, None, None, None, 1.0, p, p, ws, None) == bad
    assert b"unknown kind 3" in lib.anemoi_last_error()
    assert fwd(-1, 1.0, p, p, 16, 3, 4, 4, 2, p, None, None, None, 1.0, p, p, ws, None) == bad
    assert fwd(var, 1.0, p, p, 16, 3, 4, 4, 2, p, None, None, None, 1.0, p, p, ws - 1, None) == bad
    assert b"workspace" in lib.anemoi_last_error()
    assert fwd(var, 1.0, p, p, 16, 3, 4, 4, 2, p, None, None, None, 1.0, p, None, ws, None) == bad
    #            kind alpha pred target rows V G E groups row_w col_w mask c scale upstream dpred stream
    assert bwd(crps, 1.0, None, None, 16, 3, 4, 4, 2, None, None, None, None, 1.0, None, None, None) == bad
    assert b"anemoi_ensemble_score_backward: null pointer" in lib.anemoi_last_error()
    assert bwd(crps, 1.0, p, p, 16, 3, 4, 4, 2, p, None, None, None, 1.0, None, p, None) == bad
    assert b"upstream / dpred" in lib.anemoi_last_error()
    assert bwd(crps, 1.0, p, p, 16, 3, 4, 4, 2, p, None, None, None, 1.0, p, None, None) == bad
    assert bwd(crps, 1.0, p, p, 12, 3, 4, 4, 2, p, None, None, None, 1.0, p, p, None) == bad
    assert b"not a multiple" in lib.anemoi_last_error()
    assert bwd(crps, 1.0, p, p, 16, 3, 4, 1, 2, p, None, None, None, 1.0, p, p, None) == bad
    assert bwd(crps, 1.0, p, p, 16, 3, 4, 17, 2, p, None, None, None, 1.0, p, p, None) == unsup
    for kind in (mse, var):
        assert bwd(kind, 1.0, p, p, 16, 3, 4, 4, 2, p, None, None, None, 1.0, p, p, None) == unsup
        assert b"only ANEMOI_ENS_AFCRPS has a gradient" in lib.anemoi_last_error()
    assert bwd(crps, 1.0, p, p, 0, 3, 4, 4, 2, p, None, None, None, 1.0, p, p, None) == _lib.ANEMOI_OK  # no rows: nothing to do


def test_ensemble_score_workspace_is_a_function_of_its_four_arguments():
    """One [V] partial per workgroup; the workgroup count of a group depends on (points_per_group, V, E) alone and every group
    has the same: the reduction order cannot change with the device, the occupancy or the number of groups."""
    from anemoi_models_amd import _lib

    ws = _lib.load().anemoi_ensemble_score_workspace_floats
    assert ws(0, 8, 3, 2) == 0 and ws(1, 0, 3, 2) == 0 and ws(1, 8, 0, 2) == 0 and ws(1, 8, 3, 1) == 0 and ws(1, 8, 3, 17) == 0
    assert ws(1, 1, 1, 2) == 1
    assert ws(1, 514, 5, 3) == 5 and ws(3, 514, 5, 3) == 15  # 2570 (point, column) pairs: one workgroup per group
    assert ws(2, 2062, 80, 4) == 2 * 41 * 80  # three row lanes, chunks of 51 points: 41 workgroups per group
    for ppg, v, e in [(1, 1, 2), (514, 5, 3), (2062, 80, 4), (33, 257, 9), (1031, 256, 8), (5000, 3, 16), (542080, 90, 16)]:
        one = ws(1, ppg, v, e)
        assert one % v == 0 and 1 <= one // v <= ppg, (ppg, v, e)
        assert [ws(n, ppg, v, e) for n in (2, 3, 4, 7)] == [n * one for n in (2, 3, 4, 7)]
        assert ws(1, ppg, v, e) == one  # the same call, the same answer
    assert ws(1, 5000, 3, 16) // 3 > 1  # several workgroups per group at the smallest test shape that asks for them
    counts = [ws(1, r, 80, 8) // 80 for r in (1, 52, 1031, 542080, 4 * 542080, 64 * 542080)]
    assert counts == sorted(counts) and counts[0] == 1 and 1000 < counts[-3] <= 2048 and counts[-1] <= 2048


def test_ensemble_classes_check_their_arguments_without_gpu():
    import anemoi_models_amd
    from anemoi_models_amd import AlmostFairKernelCRPS, EnsembleMetrics, KernelCRPS, autograd

    assert {"AlmostFairKernelCRPS", "KernelCRPS", "EnsembleMetrics"} <= set(anemoi_models_amd.__all__)
    w = torch.tensor([1.0, 3.0])
    loss_fn = AlmostFairKernelCRPS(w, alpha=0.95)
    assert loss_fn.node_weights.tolist() == [0.25, 0.75] and loss_fn.alpha == 0.95 and AlmostFairKernelCRPS(w).alpha == 1.0
    assert KernelCRPS(w).alpha == 1.0 and KernelCRPS(w, fair=False).alpha == 0.0
    for alpha in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            AlmostFairKernelCRPS(w, alpha=alpha)
        with pytest.raises(ValueError, match="alpha"):
            EnsembleMetrics(w, alpha=alpha)
    x, y = torch.zeros(3, 4, 2, 5), torch.zeros(3, 2, 5)  # [lead, E, G, V] / [lead, G, V]
    with pytest.raises(ValueError, match="lead_dims"):  # one leading axis: lead_dims = 2 would keep the ensemble axis
        loss_fn(x, y, lead_dims=2)
    with pytest.raises(ValueError, match="lead_dims"):
        loss_fn(x, y, lead_dims=-1)
    with pytest.raises(ValueError, match="without the ensemble axis"):
        loss_fn(x, x)
    with pytest.raises(ValueError, match="without the ensemble axis"):
        loss_fn(x, torch.zeros(2, 2, 5))
    with pytest.raises(ValueError, match="does not end in"):
        loss_fn(torch.zeros(3, 4, 3, 5), torch.zeros(3, 3, 5))
    with pytest.raises(ValueError, match="mask must be"):
        loss_fn(x, y, torch.ones(2, 4))
    with pytest.raises(ValueError, match="target requires a gradient"):
        loss_fn(x, y.clone().requires_grad_())
    with pytest.raises(ValueError, match="target requires a gradient"):
        autograd.ensemble_score(x, y.clone().requires_grad_(), w)
    with pytest.raises(ValueError, match="has none"):
        autograd.ensemble_score(x.clone().requires_grad_(), y, w, "variance")
    with pytest.raises(ValueError, match="without the ensemble axis"):
        autograd.ensemble_score(x, x, w)
    with pytest.raises(RuntimeError, match="CPU tensor"):  # no CPU fallback
        loss_fn(x, y)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        KernelCRPS(w, fair=False)(x, y, squash=False, lead_dims=1)
    em = EnsembleMetrics(w, groups={"a": [0, 1]})
    assert em.diff_scale is None and em.KEYS == ("crps", "ens_rmse", "spread", "spread_skill")
    with pytest.raises(ValueError, match="empty variable group"):
        EnsembleMetrics(w, groups={"a": []})
    with pytest.raises(ValueError, match="node_weights"):
        EnsembleMetrics(torch.zeros(2))
    with pytest.raises(ValueError, match="must be"):
        em(torch.zeros(2, 1, 4, 2, 5), torch.zeros(2, 1, 4, 2, 5))  # the target carries an ensemble axis
    with pytest.raises(ValueError, match="group index"):
        EnsembleMetrics(w, groups={"a": [7]})(torch.zeros(2, 1, 4, 2, 5), torch.zeros(2, 1, 2, 5))
    with pytest.raises(RuntimeError, match="CPU tensor"):
        em(torch.zeros(1, 4, 2, 5), torch.zeros(1, 2, 5))  # without the step axis


def test_ensemble_metrics_take_an_affine_normalizer_only():
    from test_loss_family_cpu import _normalizer

    from anemoi_models_amd import EnsembleMetrics
    from anemoi_models_amd.preprocessing import Processors
    from anemoi_models_amd.preprocessing.imputer import ConstantImputer

    norm, idx, _ = _normalizer([1.0, 2.0, 4.0, 8.0, 16.0])
    w = torch.ones(4)
    assert EnsembleMetrics(w, norm).diff_scale.tolist() == [1.0, 2.0, 16.0]
    assert EnsembleMetrics(w, Processors([["normalizer", norm]])).diff_scale.tolist() == [1.0, 2.0, 16.0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        imp = ConstantImputer(config={"default": "none", 0: ["x"]}, data_indices=idx, statistics=None)
    with pytest.raises(NotImplementedError, match="not affine"):
        EnsembleMetrics(w, imp)
    zero, _, _ = _normalizer([1.0, 2.0, 4.0, 8.0, 16.0])
    zero._norm_mul[1] = 0.0
    with pytest.raises(ValueError, match="zero or non-finite _norm_mul"):
        EnsembleMetrics(w, zero)
    with pytest.raises(ValueError, match="output variables"):
        EnsembleMetrics(w, norm)(torch.zeros(1, 4, 4, 5), torch.zeros(1, 4, 5))
