"""NaN imputation inside the assemble / finish kernels on the MI355X: the three ``*_imputed`` entry points against the
plain-torch restatement of their contracts (tests/_impute_ref.py), the imputer modules on device tensors against the vectors of
the reference imputers, and ``AnemoiModelInterface.predict_step`` with an imputer in the processor chain against the reference
interface (tests/golden/make_golden_interface_imputers.py)."""

import os
import warnings

import numpy as np
import pytest
import torch

import _impute_ref as ir
from conftest import GOLDEN
from conftest import split_prefix
from test_host_logic import IMPUTER_CASES

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
EPS = torch.finfo(torch.float32).eps


def rel_err(got, want):  # the helper of tests/test_gpu_parity.py
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def on(obj, device=DEV):
    """The same Imputation on another device."""
    from anemoi_models_amd.preprocessing.imputer import Imputation

    out = Imputation(obj.fill_val.to(device), obj.fill_src.tolist(), None if obj.nan_map is None else obj.nan_map.to(device),
                     None if obj.out_nan_src is None else obj.out_nan_src.tolist())
    return out


def same_with_nans(got, want):
    got = got.cpu()
    return torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.nan_to_num(got), torch.nan_to_num(want))


def close_with_nans(got, want, rtol, atol):
    got = got.cpu().float()
    want = want.float()
    return torch.equal(torch.isnan(got), torch.isnan(want)) and torch.allclose(torch.nan_to_num(got), torch.nan_to_num(want),
                                                                                rtol=rtol, atol=atol)


def make_case(g, b, t, e, n, v, v_out=None):
    """State with NaNs inside and outside the map; a map of width W = v + 3 with a grid point set in every column (1) and one
    set in none (2); fill_src with -1 entries and two input columns on the same map column."""
    from anemoi_models_amd.preprocessing.imputer import Imputation

    w = v + 3
    x = torch.randn(b, t, e, n, v, generator=g)
    x[torch.rand(x.shape, generator=g) < 0.15] = NAN
    nan_map = torch.rand(n, w, generator=g) < 0.3
    nan_map[1, :] = True
    nan_map[2, :] = False
    fill_src = [-1] * v
    fill_src[0], fill_src[1], fill_src[v - 1] = w - 1, w - 1, 1  # (W > V: the last map column; columns 0 and 1 share it)
    if v > 6:
        fill_src[4] = 3
    fill_val = torch.randn(v, generator=g) * 3.0
    out_src = None
    if v_out is not None:
        out_src = [-1] * v_out
        out_src[0], out_src[v_out - 1], out_src[2] = w - 1, 0, 1
    static = Imputation(fill_val, fill_src, nan_map, out_src)
    dynamic = Imputation(fill_val, fill_src, None)
    return x, static, dynamic


@pytest.mark.parametrize("shape", [(2, 2, 2, 37, 6, 24), (1, 2, 1, 65, 7, 24), (1, 2, 1, 65, 7, 21), (1, 1, 1, 300, 12, 32)])
def test_assemble_nodes_imputed(shape):
    from anemoi_models_amd import ops

    b, t, e, n, v, ld = shape
    g = torch.Generator().manual_seed(n + v + ld)
    x, static, dynamic = make_case(g, b, t, e, n, v)
    ll, tr = torch.randn(n, 4, generator=g), torch.randn(n, 3, generator=g)
    aff = (torch.rand(v, generator=g) + 0.5, torch.randn(v, generator=g))
    xd, lld, trd = x.to(DEV), ll.to(DEV), tr.to(DEV)
    w = t * v + 7
    for obj in (static, dynamic):
        od = on(obj)
        for dtype in (torch.float32, torch.bfloat16):
            for affine in (None, aff):
                ad = None if affine is None else tuple(a.to(DEV) for a in affine)
                got = ops.assemble_nodes(xd, lld, trd, b, dtype, ld_out=ld, in_affine=ad, impute=od)
                again = ops.assemble_nodes(xd, lld, trd, b, dtype, ld_out=ld, in_affine=ad, impute=od)
                assert same_with_nans(again.float(), got.float().cpu())  # run to run: the same bits
                want = ir.assemble_nodes(x, ll, tr, b, dtype, ld_out=ld, in_affine=affine, impute=obj)
                assert got.shape == want.shape == (b * e * n, ld) and got.dtype == dtype
                assert int(torch.isnan(want[:, :t * v]).sum()) > 0 and int((~torch.isnan(want[:, :t * v])).sum()) > 0
                if affine is None:
                    assert same_with_nans(got[:, :w].float(), want[:, :w].float())
                else:
                    assert close_with_nans(got[:, :w], want[:, :w], 1e-2 if dtype == torch.bfloat16 else 1e-6, 1e-6)
                assert torch.all(got[:, w:] == 0)
    # nothing imputed (all fill_src = -1): the bits of the existing entry point
    from anemoi_models_amd.preprocessing.imputer import Imputation

    none = Imputation(static.fill_val.to(DEV), [-1] * v, static.nan_map.to(DEV))
    for dtype in (torch.float32, torch.bfloat16):
        ad = tuple(a.to(DEV) for a in aff)
        plain = ops.assemble_nodes(xd, lld, trd, b, dtype, ld_out=ld, in_affine=ad)
        got = ops.assemble_nodes(xd, lld, trd, b, dtype, ld_out=ld, in_affine=ad, impute=none)
        bits = torch.int32 if dtype == torch.float32 else torch.int16
        assert torch.equal(got.view(bits), plain.view(bits))


@pytest.mark.parametrize("shape", [(2, 2, 2, 37, 6, 5), (1, 2, 1, 300, 12, 11)])
def test_finalize_output_imputed(shape):
    from anemoi_models_amd import ops
    from anemoi_models_amd.preprocessing.imputer import Imputation

    b, t, e, n, v, v_out = shape
    g = torch.Generator().manual_seed(n + v)
    x, static, dynamic = make_case(g, b, t, e, n, v, v_out)
    # residual columns: output 0 <- input 0 (imputed, restored), 1 <- 2 (neither), 2 <- v - 1 (imputed, restored), 3 <- 1 (imputed,
    # not restored); the last output column is restored without being a residual column
    src = torch.full((v_out,), -1, dtype=torch.int32)
    src[0], src[1], src[2], src[3] = 0, 2, v - 1, 1
    # (outside the map a static imputer leaves a raw NaN alone: it reaches the result through the residual, on both sides)
    y = torch.randn(b, e, n, v_out, generator=g)
    in_aff = (torch.rand(v, generator=g) + 0.5, torch.randn(v, generator=g))
    out_aff = (torch.rand(v_out, generator=g) + 0.5, torch.randn(v_out, generator=g))
    xd, srcd = x.to(DEV), src.to(DEV)
    for obj in (static, dynamic):
        od = on(obj)
        for ia, oa in ((None, None), (in_aff, None), (in_aff, out_aff), (None, out_aff)):
            iad = None if ia is None else tuple(a.to(DEV) for a in ia)
            oad = None if oa is None else tuple(a.to(DEV) for a in oa)
            got = ops.finalize_output(y.clone().to(DEV), xd, srcd, iad, oad, impute=od)
            again = ops.finalize_output(y.clone().to(DEV), xd, srcd, iad, oad, impute=od)
            assert same_with_nans(again, got.cpu())
            want = ir.finalize_output(y.clone(), x, src, ia, oa, impute=obj)
            if obj is dynamic:  # restores nothing; the residual added imputed values, so only NaNs outside fill_src remain
                assert torch.equal(torch.isnan(want[..., 0]), torch.zeros_like(want[..., 0], dtype=torch.bool))
            else:
                assert bool(torch.isnan(want[:, :, 1, [0, 2, v_out - 1]]).all())  # grid point 1 is set in every map column
            if ia is None and oa is None:
                assert same_with_nans(got, want)
            else:
                # absolute: one rounding of difference in the normalised residual term (the kernel may contract x * mul + add
                # into one fused multiply-add) and one in the sum, each at most eps of the largest term, over the smallest
                # divisor.  relative: the f32 division, 2.5 ulp at the worst where it is not correctly rounded, plus the
                # final rounding -- 4 eps
                big = float((x[~torch.isnan(x)].abs().max() * in_aff[0].max() + in_aff[1].abs().max()) + y.abs().max()
                            + out_aff[1].abs().max())
                atol = 2 * EPS * big / (float(out_aff[0].min()) if oa is not None else 1.0)
                assert close_with_nans(got, want, 4 * EPS, atol)
    none = Imputation(static.fill_val.to(DEV), [-1] * v, static.nan_map.to(DEV), [-1] * v_out)
    iad, oad = tuple(a.to(DEV) for a in in_aff), tuple(a.to(DEV) for a in out_aff)
    plain = ops.finalize_output(y.clone().to(DEV), xd, srcd, iad, oad)
    got = ops.finalize_output(y.clone().to(DEV), xd, srcd, iad, oad, impute=none)
    assert torch.equal(got.view(torch.int32), plain.view(torch.int32))


def test_bound_output_imputed():
    """300 rows on a grid of 150 (two batch entries share the map): a relu / hardtanh / fraction op list whose total column is
    restored -- after the ops, so the fraction column that multiplied by it stays finite."""
    from anemoi_models_amd import ops
    from anemoi_models_amd.preprocessing.imputer import Imputation

    g = torch.Generator().manual_seed(8)
    n, v_out, w = 150, 6, 9
    y = torch.randn(2, 1, n, v_out, generator=g)
    nan_map = torch.rand(n, w, generator=g) < 0.3
    nan_map[1, :], nan_map[2, :] = True, False
    inf = float("inf")
    # relu on 0; hardtanh [0, 1] on 4 (the total); fraction: 3 = clamp(3, 0, 1) * column 4
    lists = (torch.tensor([0, 4, 3, 3], dtype=torch.int32), torch.tensor([0.0, 0.0, 0.0, -inf]),
             torch.tensor([inf, 1.0, 1.0, inf]), torch.tensor([-1, -1, -1, 4], dtype=torch.int32))
    fin = (torch.tensor([0, 3, 4], dtype=torch.int32), torch.rand(3, generator=g) + 0.5, torch.randn(3, generator=g))
    obj = Imputation(torch.zeros(4), [-1] * 4, nan_map, [-1, -1, 8])  # fin_nan_src: only the total (column 4) is restored
    od = on(obj)
    got = ops.bound_output(y.clone().to(DEV), *(t.to(DEV) for t in lists), fin=tuple(t.to(DEV) for t in fin), impute=od)
    again = ops.bound_output(y.clone().to(DEV), *(t.to(DEV) for t in lists), fin=tuple(t.to(DEV) for t in fin), impute=od)
    assert same_with_nans(again, got.cpu())
    want = ir.bound_output(y.clone(), *lists, fin=fin, impute=obj)
    assert torch.equal(torch.isnan(want[..., 4]), nan_map[:, 8].expand(2, 1, n)) and not bool(torch.isnan(want[..., :4]).any())
    # the same clamp, product and subtraction on both sides (one rounding each, no contraction possible); the f32 division is
    # 2.5 ulp at the worst where it is not correctly rounded: 4 eps relative, nothing absolute beyond the smallest normal
    assert close_with_nans(got, want, 4 * EPS, 1e-30)
    plain = ops.bound_output(y.clone().to(DEV), *(t.to(DEV) for t in lists), fin=tuple(t.to(DEV) for t in fin))
    none = Imputation(torch.zeros(4, device=DEV), [-1] * 4, nan_map.to(DEV), [-1, -1, -1])
    got = ops.bound_output(y.clone().to(DEV), *(t.to(DEV) for t in lists), fin=tuple(t.to(DEV) for t in fin), impute=none)
    assert torch.equal(got, plain)


@pytest.mark.parametrize("case", sorted(IMPUTER_CASES))
def test_imputer_modules_on_the_device(case):
    """The five cases of imputers.npz with every tensor on the device, against the file."""
    from anemoi_models_amd.preprocessing import imputer
    from anemoi_models_amd.utils.indices import SimpleDataIndices

    with np.load(os.path.join(GOLDEN, "imputers.npz")) as z:
        gold = {k: torch.from_numpy(z[k]) for k in z.files}
    g = split_prefix(gold, case + ".")
    stats = None if "Constant" in case else {k: v.numpy() for k, v in split_prefix(gold, "stat.").items()}
    idx = SimpleDataIndices(n_prognostic=2, n_forcing=2, n_diagnostic=1, names=["x", "y", "z", "q", "other"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        imp = getattr(imputer, case.replace("Default", ""))(config=dict(IMPUTER_CASES[case]), data_indices=idx, statistics=stats)
    for name, fn in (("t_train", lambda: imp.transform(g["x_train"].to(DEV), in_place=False)),
                     ("t_infer", lambda: imp.transform(g["x_infer"].to(DEV), in_place=False)),
                     ("inv_train", lambda: imp.inverse_transform(g["y_train"].to(DEV), in_place=False)),
                     ("inv_infer", lambda: imp.inverse_transform(g["y_infer"].to(DEV), in_place=False))):
        got = fn()
        assert got.is_cuda
        torch.testing.assert_close(got.cpu(), g[name], rtol=0, atol=0, equal_nan=True)
    torch.testing.assert_close(imp.loss_mask_training.cpu(), g["loss_mask"], rtol=0, atol=0)
    # ... and the kernel on the same vectors: the select of anemoi_assemble_nodes_imputed is the module's transform
    from anemoi_models_amd import ops

    obj = imp.imputation(DEV)
    x = g["x_infer"][:, :, None].to(DEV)
    n, v = x.shape[-2], x.shape[-1]
    out = ops.assemble_nodes(x, torch.zeros(n, 0, device=DEV), None, x.shape[0], torch.float32, impute=obj)
    want = g["t_infer"].permute(0, 2, 1, 3).reshape(-1, 2 * v)
    torch.testing.assert_close(out.cpu(), want, rtol=0, atol=0, equal_nan=True)


@pytest.fixture(scope="module")
def fix():
    return ir.fixture.load()


@pytest.mark.parametrize("case", [1, 2, 3, 4])
def test_interface_predict_step_with_an_imputer_vs_reference(graph_o32, golden_interface, fix, case, monkeypatch):
    from anemoi_models_amd import trail

    gold = golden_interface
    iface = ir.build_case_interface(graph_o32, gold, case)
    iface.load_state_dict(split_prefix(gold, "sd."))
    iface = iface.to(DEV).eval()
    batch1, batch2 = ir.batch1_of(gold, fix, case).to(DEV), fix["batch2"].to(DEV)

    def within(got, want):
        err = rel_err(got, want)
        print(f"case {case}: max rel err over the finite entries {err:.3e}")
        assert err < 1e-4

    assert iface._fused_route(batch1) is None
    y1 = iface.predict_step(batch1)
    assert y1.dtype == torch.float32
    ir.assert_matches(y1, fix[f"case{case}.y1"], within)
    assert iface._fused_route(batch2) is not None  # the second call is fused ...
    with trail.record() as launches:
        y2 = iface.predict_step(batch2)
    names = {n.split(":")[0] for n in launches.names()}  # ("<entry point>:<operand>")
    assert "anemoi_assemble_nodes_imputed" in names and "anemoi_finalize_output_imputed" in names  # ... on the new kernels
    if case == 4:
        assert "anemoi_bound_output_imputed" in names
    ir.assert_matches(y2, fix[f"case{case}.y2"], within)
    monkeypatch.setenv("ANEMOI_AMD_FUSE_NORMALIZER", "0")
    assert iface._fused_route(batch2) is None
    y3 = iface.predict_step(batch2)  # the generic route
    ir.assert_matches(y3, fix[f"case{case}.y2"], within)

    def routes_agree(a, b):
        err = rel_err(a, b)
        print(f"case {case}: fused against generic {err:.3e}")
        assert err < 1e-5

    ir.assert_matches(y2, y3.cpu(), routes_agree)


def test_ensemble_model_passes_the_imputation_through(graph_o32, golden_interface, fix, monkeypatch):
    """Case 1 on AnemoiEnsModelEncProcDec with inject_noise: false and two equal members: each member is the one-member result."""
    from anemoi_models_amd.utils.presets import model_config

    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "fp32")
    noise = {"noise_std": 1.0, "noise_channels_dim": 8, "noise_mlp_hidden_dim": 16, "inject_noise": False}
    torch.manual_seed(5)
    try:
        iface = ir.build_case_interface(graph_o32, golden_interface, 1, config=model_config("Transformer", 64, 2, noise_injector=noise),
                                        model_target="anemoi.models.models.ensemble.AnemoiEnsModelEncProcDec")
    except (NotImplementedError, ValueError) as e:
        pytest.skip(f"AnemoiEnsModelEncProcDec refuses the configuration: {e}")
    iface = iface.to(DEV).eval()
    batch1, batch2 = ir.batch1_of(golden_interface, fix, 1).to(DEV), fix["batch2"].to(DEV)
    iface.predict_step(batch1)
    route = iface._fused_route(batch2)
    assert route is not None
    one = iface.predict_step(batch2)
    with torch.no_grad():
        two = iface.model(batch2[:, 0:2, None].repeat(1, 1, 2, 1, 1), input_affine=route[0], output_affine=route[1])
    assert tuple(two.shape) == (1, 2) + tuple(one.shape[2:]) and int(torch.isnan(one).sum()) > 0

    def same_member(a, b):
        err = rel_err(a, b)
        print(f"member against the one-member call {err:.3e}")
        assert err < 1e-5  # (two rows of members may take another GEMM tile than one: the bound between two routes)

    for m in range(2):
        ir.assert_matches(two[:, m:m + 1], one.cpu(), same_member)
