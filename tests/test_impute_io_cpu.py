"""NaN imputation inside the assemble / finish kernels, the parts that need no GPU: the plain-torch restatement of the three
kernel contracts (tests/_impute_ref.py) against the vectors of the reference imputers, the ``Imputation`` value object, the
interface's route query, ``predict_step`` on the stand-ins against the reference interface
(tests/golden/make_golden_interface_imputers.py), and the argument checks of the new entry points through the C ABI."""

import os
import warnings

import numpy as np
import pytest
import torch

import _impute_ref as ir
from conftest import GOLDEN
from conftest import split_prefix
from test_host_logic import IMPUTER_CASES
from test_host_logic import NORMALIZER_METHODS
from test_host_logic import build_interface

from anemoi_models_amd.preprocessing import Processors
from anemoi_models_amd.preprocessing import imputer
from anemoi_models_amd.preprocessing.normalizer import InputNormalizer
from anemoi_models_amd.utils.indices import SimpleDataIndices


@pytest.fixture(scope="module")
def fix():
    return ir.fixture.load()


def reference_imputer(case):
    """(imputer, vectors) of one case of imputers.npz, as tests/test_host_logic.py::test_imputers_match_reference builds it."""
    with np.load(os.path.join(GOLDEN, "imputers.npz")) as z:
        gold = {k: torch.from_numpy(z[k]) for k in z.files}
    stats = None if "Constant" in case else {k: v.numpy() for k, v in split_prefix(gold, "stat.").items()}
    idx = SimpleDataIndices(n_prognostic=2, n_forcing=2, n_diagnostic=1, names=["x", "y", "z", "q", "other"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        imp = getattr(imputer, case.replace("Default", ""))(config=dict(IMPUTER_CASES[case]), data_indices=idx, statistics=stats)
    return imp, split_prefix(gold, case + ".")


@pytest.mark.parametrize("case", sorted(IMPUTER_CASES))
def test_restated_contract_is_the_reference_imputer(case):
    """select (no affine) of x_infer == the reference's transform, NaN restore of y_infer == its inverse_transform; a static
    imputer uses the map of x_train's first call (W = the training layout's width, the inference layout's columns)."""
    imp, g = reference_imputer(case)
    imp.transform(g["x_train"], in_place=False)
    obj = imp.imputation("cpu")
    dynamic = "Dynamic" in case
    assert (obj.nan_map is None) == dynamic and (obj.out_nan_src is None) == dynamic
    if not dynamic:
        assert obj.W == 5 and obj.nan_map.data_ptr() == imp.nan_locations.data_ptr()  # the imputer's own storage
    x = g["x_infer"][:, :, None]  # [B, T, Ens = 1, G, V]
    got = ir.select(x, obj.fill_val, obj.fill_src, obj.nan_map)[:, :, 0]
    torch.testing.assert_close(got, g["t_infer"], rtol=0, atol=0, equal_nan=True)
    back = ir.restore(g["y_infer"], obj.nan_map, obj.out_nan_src)
    torch.testing.assert_close(back, g["inv_infer"], rtol=0, atol=0, equal_nan=True)


def _chain(order):
    idx = SimpleDataIndices(n_prognostic=10, n_forcing=2, n_diagnostic=1)
    g = torch.Generator().manual_seed(3)
    mean = (torch.randn(13, generator=g) * 3.0).numpy()
    stdev = (0.5 + torch.rand(13, generator=g) * 2.0).numpy()
    stats = {"mean": mean, "stdev": stdev, "minimum": mean - 3.0 * stdev, "maximum": mean + 3.5 * stdev}
    norm = InputNormalizer(dict(NORMALIZER_METHODS), idx, stats)
    if order == "imputer_first":
        imp = imputer.InputImputer({"default": "none", "mean": ["prog_2"], "minimum": ["forc_1"], "maximum": ["prog_3"]}, idx, stats)
        return imp, norm, Processors([["imputer", imp], ["normalizer", norm]])
    imp = imputer.ConstantImputer({"default": "none", 0: ["prog_2"], 3.0: ["prog_5"], 22.7: ["forc_1"]}, idx)
    return imp, norm, Processors([["normalizer", norm], ["imputer", imp]])


@pytest.mark.parametrize("order", ["imputer_first", "normalizer_first"])
def test_fill_values_are_what_the_processor_chain_makes_of_a_nan(order):
    imp, norm, chain = _chain(order)
    x = torch.randn(1, 2, 9, 12, generator=torch.Generator().manual_seed(4)) * 5.0
    cols = [c for c in imp.index_inference_input if c is not None]
    x[..., cols] = float("nan")
    want = chain(x, in_place=False)[0, 0, 0]
    i_in = norm._input_idx.long()
    obj = imp.imputation("cpu", (norm._norm_mul[i_in], norm._norm_add[i_in]) if order == "imputer_first" else None)
    assert obj.fill_val.dtype == torch.float32 and obj.fill_src.dtype == torch.int32 and obj.out_nan_src.dtype == torch.int32
    assert [c for c, s in enumerate(obj.fill_src.tolist()) if s >= 0] == sorted(cols)
    assert obj.fill_src[cols].tolist() == [imp.index_training_input[i] for i, c in enumerate(imp.index_inference_input)
                                           if c is not None]
    if order == "normalizer_first":
        assert torch.equal(obj.fill_val[cols], want[cols])
    else:  # x * mul + add in f32, once by the chain and once by the builder: one ulp
        ulp = torch.finfo(torch.float32).eps * want[cols].abs().clamp_min(torch.finfo(torch.float32).tiny)
        assert bool(((obj.fill_val[cols] - want[cols]).abs() <= ulp).all())
    with pytest.raises(ValueError, match="outside the NaN map"):
        imputer.Imputation(obj.fill_val, obj.fill_src.tolist(), obj.nan_map[:, :3].contiguous(), obj.out_nan_src.tolist())


def _loaded(graph, gold, case, **kw):
    iface = ir.build_case_interface(graph, gold, case, **kw)
    iface.load_state_dict(split_prefix(gold, "sd."))
    return iface.eval()


@pytest.mark.parametrize("case", [1, 2, 3, 4])
def test_predict_step_on_the_stand_ins_matches_the_reference_interface(graph_o32, golden_interface, fix, case, monkeypatch):
    """Both calls against the reference: NaN maps identical, finite entries within the bounds of
    test_interface_predict_step_matches_golden; the first call is generic, the second one fused."""
    ir.install(monkeypatch)
    monkeypatch.setenv("ANEMOI_AMD_FUSE_NORMALIZER", "force")
    iface = _loaded(graph_o32, golden_interface, case)
    batch1 = ir.batch1_of(golden_interface, fix, case)

    def close(a, b):
        torch.testing.assert_close(a, b, atol=5e-4, rtol=5e-4)

    assert iface._fused_route(batch1) is None  # first run: the reference's one-off NaN check and the imputer's map
    ir.assert_matches(iface.predict_step(batch1), fix[f"case{case}.y1"], close)
    imp = iface.pre_processors.processors["imputer"]
    kept = (imp.nan_locations, imp.loss_mask_training)
    route = iface._fused_route(fix["batch2"])
    assert route is not None and isinstance(route[0], imputer.ImputedAffine) and len(route[0]) == 2
    assert iface._fused_route(fix["batch2"])[0].impute is route[0].impute  # built once, cached
    seen = []
    real = ir.assemble_nodes
    import anemoi_models_amd.ops as ops

    monkeypatch.setattr(ops, "assemble_nodes", lambda *a, **k: (seen.append(k.get("impute")), real(*a, **k))[1])
    ir.assert_matches(iface.predict_step(fix["batch2"]), fix[f"case{case}.y2"], close)
    assert route[0].impute in seen  # the second call took the fused route
    if "Dynamic" not in type(imp).__name__:  # the fused route never touches the two attributes of a static imputer
        assert imp.nan_locations is kept[0] and imp.loss_mask_training is kept[1]
    monkeypatch.setenv("ANEMOI_AMD_FUSE_NORMALIZER", "0")
    assert iface._fused_route(fix["batch2"]) is None
    ir.assert_matches(iface.predict_step(fix["batch2"]), fix[f"case{case}.y2"], close)


def test_route_query(graph_o32, golden_interface, fix, monkeypatch):
    ir.install(monkeypatch)
    monkeypatch.setenv("ANEMOI_AMD_FUSE_NORMALIZER", "force")
    gold = golden_interface
    # a normaliser-only interface: _normalizer_affines returns what it returned before, and is the route
    plain = build_interface(graph_o32, gold)
    plain.load_state_dict(split_prefix(gold, "sd."))
    plain.eval()
    assert plain._normalizer_affines(gold["batch"]) is None and plain._fused_route(gold["batch"]) is None
    plain.predict_step(gold["batch"])
    norm = plain.pre_processors.processors["normalizer"]
    i_in, i_out = norm._input_idx.long(), norm._output_idx.long()
    got = plain._normalizer_affines(gold["batch"])
    assert type(got) is tuple and type(got[0]) is tuple and type(got[1]) is tuple
    for a, b in zip(got[0] + got[1], (norm._norm_mul[i_in], norm._norm_add[i_in], norm._norm_mul[i_out], norm._norm_add[i_out])):
        assert torch.equal(a, b)
    route = plain._fused_route(gold["batch"])
    assert type(route[0]) is tuple and all(torch.equal(a, b) for a, b in zip(route[0] + route[1], got[0] + got[1]))

    # an imputer in the chain: _normalizer_affines stays None, the route opens after the first call
    iface = _loaded(graph_o32, gold, 1)
    batch1 = ir.batch1_of(gold, fix, 1)
    assert iface._fused_route(batch1) is None
    iface.predict_step(batch1)
    assert iface._normalizer_affines(batch1) is None and iface._fused_route(batch1) is not None
    assert iface._fused_route(batch1[0]) is None  # not 4-dimensional
    assert iface._fused_route(batch1[:, :, :100]) is None  # a static imputer's map is of another grid size
    monkeypatch.setenv("ANEMOI_AMD_FUSE_NORMALIZER", "1")
    assert iface._fused_route(batch1) is None  # a CPU tensor without "force"
    monkeypatch.setenv("ANEMOI_AMD_FUSE_NORMALIZER", "0")
    assert iface._fused_route(batch1) is None
    monkeypatch.setenv("ANEMOI_AMD_FUSE_NORMALIZER", "force")

    # two imputers
    procs, _ = ir.fixture.CASES[1]
    second = ("imputer2", ir.fixture.IMPUTER + "ConstantImputer", {"default": "none", 1.0: ["prog_5"]})
    two = _loaded(graph_o32, gold, 1, processors=[procs[0], second, procs[1]])
    b = gold["batch"].clone()
    two.predict_step(b)
    assert two._fused_route(b) is None

    # a dynamic imputer needs no map, so the grid size is free
    dyn = _loaded(graph_o32, gold, 3)
    dyn.predict_step(ir.batch1_of(gold, fix, 3))
    assert dyn._fused_route(batch1[:, :, :100]) is not None


def test_route_is_refused_for_a_truncated_model_and_the_model_refuses_an_imputation(graph_o32, golden_interface, fix, monkeypatch):
    from test_truncation_cpu import _matrices

    ir.install(monkeypatch)
    monkeypatch.setenv("ANEMOI_AMD_FUSE_NORMALIZER", "force")
    gold = golden_interface
    down, up = _matrices(graph_o32["data"].num_nodes, 50)
    trunc = _loaded(graph_o32, gold, 1, truncation_data={"down": down, "up": up})
    assert trunc.model._truncation is not None
    batch1 = ir.batch1_of(gold, fix, 1)
    trunc.pre_processors(batch1, in_place=False)  # the first run of the processors, without the model
    assert trunc._fused_route(batch1) is None
    # handed an imputation all the same, the truncated forward, the training forward and the sharded one refuse up front
    iface = _loaded(graph_o32, gold, 1)
    iface.predict_step(batch1)
    route = iface._fused_route(batch1)
    x = batch1[:, 0:2, None]
    with pytest.raises(NotImplementedError, match="imputation"), torch.no_grad():
        trunc.model(x, input_affine=route[0], output_affine=route[1])
    with pytest.raises(NotImplementedError, match="imputation"):
        iface.model._training_forward(x, route[0], route[1])
    from anemoi_models_amd.distributed.partition import sharded_forward

    with pytest.raises(NotImplementedError, match="imputation"), torch.no_grad():
        sharded_forward(iface.model, x, None, input_affine=route[0], output_affine=route[1])


def test_new_entry_points_validate_without_gpu():
    """Unpaired pointers and W <= 0 with a map come back as ANEMOI_ERR_INVALID, with a message, before anything is launched;
    the ops refuse rows= together with an imputation."""
    from anemoi_models_amd import _lib
    from anemoi_models_amd import ops

    lib = _lib.load()
    bad, p = _lib.ANEMOI_ERR_INVALID, 4096  # p: a non-null pointer value that the checks never dereference
    asm = lambda fv, fs, nm, w: lib.anemoi_assemble_nodes_imputed(_lib.F32, p, 1, 2, 1, 4, 3, p, 2, None, 0, p, 8, None, None,  # noqa: E731
                                                                  fv, fs, nm, w, None)
    assert asm(p, None, None, 0) == bad and b"anemoi_assemble_nodes_imputed: fill_val and fill_src come together" in lib.anemoi_last_error()
    assert asm(None, p, None, 0) == bad
    assert asm(None, None, p, 5) == bad and b"nan_map without" in lib.anemoi_last_error()
    assert asm(p, p, p, 0) == bad and b"W > 0" in lib.anemoi_last_error()
    assert asm(p, p, p, -1) == bad
    assert lib.anemoi_assemble_nodes_imputed(_lib.F32, p, 1, 2, 1, 4, 3, p, 2, None, 0, p, 8, p, None, p, p, None, 0, None) == bad
    assert b"in_mul and in_add come together" in lib.anemoi_last_error()
    fin = lambda fv, fs, nm, w, om=None: lib.anemoi_finalize_output_imputed(p, 2, p, 1, 2, 1, 4, 3, p, None, None, om, None,  # noqa: E731
                                                                            fv, fs, nm, w, None, None)
    assert fin(p, None, None, 0) == bad and b"anemoi_finalize_output_imputed: fill_val and fill_src" in lib.anemoi_last_error()
    assert fin(p, p, p, 0) == bad and b"W > 0" in lib.anemoi_last_error()
    assert fin(p, p, None, 0, om=p) == bad and b"mul and add come together" in lib.anemoi_last_error()
    bnd = lambda g, nm, w, fns, rows=8: lib.anemoi_bound_output_imputed(p, 3, rows, 0, None, None, None, None, 1, p, p, p,  # noqa: E731
                                                                         g, nm, w, fns, None)
    assert bnd(4, p, 0, p) == bad and b"anemoi_bound_output_imputed: nan_map needs W > 0" in lib.anemoi_last_error()
    assert bnd(4, p, 5, None) == bad and b"nan_map and fin_nan_src come together" in lib.anemoi_last_error()
    assert bnd(3, p, 5, p) == bad and b"not a multiple of the grid size" in lib.anemoi_last_error()
    assert lib.anemoi_bound_output_imputed(p, 3, 8, 0, None, None, None, None, 1, None, p, p, 4, p, 5, p, None) == bad
    assert b"null de-normalisation list" in lib.anemoi_last_error()

    obj = imputer.Imputation(torch.zeros(3), [-1, 0, -1], torch.zeros(4, 2, dtype=torch.bool), [0, -1])
    x, ll = torch.zeros(1, 2, 1, 4, 3), torch.zeros(4, 2)
    with pytest.raises(ValueError, match="rows= with impute="):
        ops.assemble_nodes(x, ll, None, 1, torch.float32, rows=torch.arange(2), impute=obj)
    with pytest.raises(ValueError, match="rows= with impute="):
        ops.finalize_output(torch.zeros(1, 1, 2, 2), x, torch.tensor([0, -1], dtype=torch.int32), rows=torch.arange(2), impute=obj)
    with pytest.raises(ValueError, match="rows= with impute="):
        ir.assemble_nodes(x, ll, None, 1, torch.float32, rows=torch.arange(2), impute=obj)
