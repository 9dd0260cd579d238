"""The bounding family without a GPU (layers/bounding.py): NormalizedReluBounding and the four Leaky* classes of current
anemoi-models -- values worked by hand from their formulas, constructor refusals, ``_target_`` instantiation, statistics reaching
them through the models and the interface -- the op list with slopes and its reverse walk against the module route and torch
autograd in f64 (tests/_bounding_ref.py), and the argument checks of the three new entry points through the library."""

import math

import pytest
import torch

import _bounding_ref as br
from conftest import split_prefix
from anemoi_models_amd.layers import bounding as B
from anemoi_models_amd.models.encoder_processor_decoder import instantiate
from anemoi_models_amd.utils.indices import SimpleDataIndices
from anemoi_models_amd.utils.presets import model_config

N2I = {"a": 0, "b": 1, "c": 2}
STATS = {"mean": [1.0, 2.0, 3.0], "stdev": [2.0, 4.0, 0.5], "minimum": [0.0, -2.0, 1.0], "maximum": [4.0, 2.0, 5.0]}
NORM_A = dict(variables=["c", "a", "b"], min_val=[3.5, 1.0, 1.0], normalizer=["mean-std", "min-max", "max"])  # t = 1, .25, .5
NORM_B = dict(variables=["b", "a"], min_val=[2.0, 0.0], normalizer=["std", "mean-std"])                       # t = .5, -.5
ST = dict(name_to_index=N2I, statistics=STATS, name_to_index_stats=N2I)


def x33():
    return torch.tensor([[-2.0, 0.5, 3.0], [1.0, -1.0, 0.25], [-0.5, 2.0, -4.0]])


def cases():
    """(module, expected) by hand: leaky_relu(v) = 0.01 v below 0; leaky hardtanh = bound + 0.01 (v - bound) outside;
    normalised: relu / leaky_relu of (v - t), plus t."""
    return [
        (B.LeakyReluBounding(variables=["c", "a"], name_to_index=N2I),
         [[-0.02, 0.5, 3.0], [1.0, -1.0, 0.25], [-0.005, 2.0, -0.04]]),
        (B.LeakyHardtanhBounding(variables=["b"], name_to_index=N2I, min_val=0.0, max_val=1.0),
         [[-2.0, 0.5, 3.0], [1.0, -0.01, 0.25], [-0.5, 1.01, -4.0]]),
        (B.LeakyFractionBounding(variables=["b"], name_to_index=N2I, min_val=0.0, max_val=1.0, total_var="c"),
         [[-2.0, 1.5, 3.0], [1.0, -0.0025, 0.25], [-0.5, -4.04, -4.0]]),
        (B.NormalizedReluBounding(**NORM_A, **ST), [[0.25, 0.5, 3.0], [1.0, 0.5, 1.0], [0.25, 2.0, 1.0]]),
        (B.NormalizedReluBounding(**NORM_B, **ST), [[-0.5, 0.5, 3.0], [1.0, 0.5, 0.25], [-0.5, 2.0, -4.0]]),
        (B.LeakyNormalizedReluBounding(**NORM_A, **ST), [[0.2275, 0.5, 3.0], [1.0, 0.485, 0.9925], [0.2425, 2.0, 0.95]]),
    ]


@pytest.mark.parametrize("case", range(6))
def test_exact_values_module_route_and_op_list(case):
    module, want = cases()[case]
    want = torch.tensor(want)
    torch.testing.assert_close(module(x33()), want, rtol=1e-6, atol=1e-8)
    got, _ = br.apply_ops(x33(), br.op_list([module]))
    torch.testing.assert_close(got, want, rtol=1e-6, atol=1e-8)
    assert len(module.state_dict()) == 0 and len(list(module.parameters())) == 0


def test_normalised_thresholds_belong_to_their_variables_by_name():
    b = B.NormalizedReluBounding(**NORM_A, **ST)
    assert b.data_index.tolist() == [2, 0, 1]  # ``variables`` order, not sorted
    assert b.norm_min_val.dtype == torch.float32 and b.norm_min_val.tolist() == [1.0, 0.25, 0.5]
    assert B.compile_boundings([b]) == [(2, 1.0, math.inf, -1), (0, 0.25, math.inf, -1), (1, 0.5, math.inf, -1)]
    assert B.bounding_slopes([b]) is None  # a hard op: no kernel change
    leaky = B.LeakyNormalizedReluBounding(**NORM_A, **ST)
    assert B.compile_boundings([leaky]) == B.compile_boundings([b])
    assert B.bounding_slopes([leaky]) == [B.LEAKY_SLOPE] * 3 and B.LEAKY_SLOPE == 0.01


def test_constructor_refusals():
    with pytest.raises(ValueError, match="normalizer"):
        B.NormalizedReluBounding(variables=["a"], min_val=[0.0], normalizer=["robust"], **ST)
    with pytest.raises(ValueError, match="one entry per variable"):
        B.NormalizedReluBounding(variables=["a", "b"], min_val=[0.0], normalizer=["max", "max"], **ST)
    with pytest.raises(ValueError, match="one entry per variable"):
        B.LeakyNormalizedReluBounding(variables=["a", "b"], min_val=[0.0, 1.0], normalizer=["max"], **ST)
    with pytest.raises(ValueError, match="twice"):
        B.NormalizedReluBounding(variables=["a", "a"], min_val=[0.0, 1.0], normalizer=["max", "std"], **ST)
    with pytest.raises(ValueError, match="statistics"):
        B.NormalizedReluBounding(variables=["a"], min_val=[0.0], normalizer=["max"], name_to_index=N2I)
    with pytest.raises(ValueError, match="statistics"):
        B.NormalizedReluBounding(variables=["a"], min_val=[0.0], normalizer=["max"], name_to_index=N2I, statistics=STATS)
    with pytest.raises(AssertionError):  # an unknown variable: the index builder asserts, as in the other classes
        B.NormalizedReluBounding(variables=["nope"], min_val=[0.0], normalizer=["max"], **ST)
    # the existing classes accept and ignore the two arguments
    for kind, kw in ((B.ReluBounding, {}), (B.HardtanhBounding, dict(min_val=0.0, max_val=1.0)),
                     (B.FractionBounding, dict(min_val=0.0, max_val=1.0, total_var="c"))):
        kind(variables=["a"], name_to_index=N2I, statistics=None, name_to_index_stats=None, **kw)


TARGETS = [
    ("LeakyReluBounding", {}),
    ("LeakyHardtanhBounding", {"min_val": 0.0, "max_val": 1.0}),
    ("LeakyFractionBounding", {"min_val": 0.0, "max_val": 1.0, "total_var": "c"}),
    ("NormalizedReluBounding", {"min_val": [0.0, 1.0], "normalizer": ["mean-std", "max"]}),
    ("LeakyNormalizedReluBounding", {"min_val": [0.0, 1.0], "normalizer": ["min-max", "std"]}),
]


@pytest.mark.parametrize("name,extra", TARGETS)
def test_instantiate_of_reference_targets(name, extra):
    cfg = {"_target_": f"anemoi.models.layers.bounding.{name}", "variables": ["a", "b"], **extra}
    b = instantiate(cfg, **ST)
    assert type(b) is getattr(B, name)
    b(x33())


class OldSignatureBounding(B.BaseBounding):
    """A user's own class written against the reference's signature: no ``statistics`` argument."""

    def __init__(self, *, variables: list, name_to_index: dict) -> None:
        B.BaseBounding.__init__(self, variables=variables, name_to_index=name_to_index)

    def forward(self, x):
        return x


def _config(bounding):
    cfg = model_config("GraphTransformer", 64, 2, 16)
    cfg["model"]["bounding"] = [dict(b) for b in bounding]
    cfg["data"] = {"forcing": ["forc_0", "forc_1"], "diagnostic": ["diag_0"],
                   "processors": {"normalizer": {"_target_": "anemoi.models.preprocessing.normalizer.InputNormalizer",
                                                 "config": {"default": "mean-std"}}}}
    cfg["model"]["model"] = {"_target_": "anemoi.models.models.encoder_processor_decoder.AnemoiModelEncProcDec"}
    return type(cfg)(cfg)


NORMALISED = {"_target_": "anemoi.models.layers.bounding.NormalizedReluBounding", "variables": ["diag_0", "prog_2"],
              "min_val": [0.0, 1.0], "normalizer": ["mean-std", "max"]}


def test_statistics_reach_the_boundings_through_model_and_interface(graph_o32, golden_interface):
    from anemoi_models_amd.interface import AnemoiModelInterface
    from anemoi_models_amd.models import AnemoiModelEncProcDec

    stats = {k: v.numpy() for k, v in split_prefix(golden_interface, "stat.").items()}
    idx = SimpleDataIndices(n_prognostic=10, n_forcing=2, n_diagnostic=1)
    old = {"_target_": "test_bounding_family_cpu.OldSignatureBounding", "variables": ["prog_0"]}
    cfg = _config([NORMALISED, old, {"_target_": "anemoi.models.layers.bounding.LeakyReluBounding", "variables": ["prog_1"]}])
    j_diag, j_p2 = idx.data.input.name_to_index["diag_0"], idx.data.input.name_to_index["prog_2"]
    want = [(0.0 - stats["mean"][j_diag]) / stats["stdev"][j_diag], 1.0 / stats["maximum"][j_p2]]
    model = AnemoiModelEncProcDec(model_config=cfg, data_indices=idx, graph_data=graph_o32, statistics=stats)
    iface = AnemoiModelInterface(config=cfg, graph_data=graph_o32, statistics=stats, data_indices=idx, metadata={})
    for m in (model, iface.model):
        assert [type(b).__name__ for b in m.boundings] == ["NormalizedReluBounding", "OldSignatureBounding", "LeakyReluBounding"]
        torch.testing.assert_close(m.boundings[0].norm_min_val, torch.tensor(want, dtype=torch.float32))
        assert m.boundings[0].data_index.tolist() == [10, 2]  # output columns of diag_0, prog_2 in ``variables`` order
        assert m._bounding_plan("cpu", None) is None  # the user's class: module route
    with pytest.raises(ValueError, match="statistics"):  # a model built without them cannot serve the class
        AnemoiModelEncProcDec(model_config=cfg, data_indices=idx, graph_data=graph_o32)
    # a list that compiles: the plan carries the slopes, the training plan the tape size
    known = AnemoiModelEncProcDec(model_config=_config([NORMALISED, {
        "_target_": "anemoi.models.layers.bounding.LeakyFractionBounding", "variables": ["prog_1"], "min_val": 0.0,
        "max_val": 1.0, "total_var": "prog_3"}]), data_indices=idx, graph_data=graph_o32, statistics=stats)
    lists, _, _, leaky = known._bounding_plan("cpu", None)
    assert lists[0].tolist() == [10, 2, 1, 1] and lists[3].tolist() == [-1, -1, -1, 3]
    assert leaky["slope"].tolist() == pytest.approx([0.0, 0.0, 0.01, 0.01])
    assert known._bounding_train_plan("cpu")[2] == 5
    hard = AnemoiModelEncProcDec(model_config=_config([NORMALISED]), data_indices=idx, graph_data=graph_o32, statistics=stats)
    assert hard._bounding_plan("cpu", None)[3] == {}  # hard ops only: ops.bound_output is called as it always was
    assert hard._bounding_train_plan("cpu")[1].tolist() == [0.0, 0.0]


def test_old_classes_compile_as_before():
    n2i = {f"v{i}": i for i in range(7)}
    chain = [
        B.ReluBounding(variables=["v5", "v0", "v5"], name_to_index=n2i),
        B.FractionBounding(variables=["v1", "v2", "v3"], name_to_index=n2i, min_val=0.0, max_val=1.0, total_var="v2"),
        B.HardtanhBounding(variables=["v0", "v3"], name_to_index=n2i, min_val=-0.25, max_val=0.5),
    ]
    inf = math.inf
    want = [(0, 0.0, inf, -1), (5, 0.0, inf, -1), (1, 0.0, 1.0, -1), (2, 0.0, 1.0, -1), (3, 0.0, 1.0, -1),
            (1, -inf, inf, 2), (3, -inf, inf, 2), (2, -inf, inf, 2), (0, -0.25, 0.5, -1), (3, -0.25, 0.5, -1)]
    got = B.compile_boundings(chain)
    assert got == want and type(got) is list and all(type(o) is tuple and len(o) == 4 for o in got)
    assert B.bounded_columns(got) == [0, 1, 2, 3, 5]
    assert B.bounding_slopes(chain) is None

    class Custom(B.LeakyReluBounding):
        pass

    custom = [Custom(variables=["v0"], name_to_index=n2i)]
    assert B.compile_boundings(custom) is None and B.bounding_slopes(custom) is None
    mixed = chain + [B.LeakyHardtanhBounding(variables=["v6"], name_to_index=n2i, min_val=0.0, max_val=2.0)]
    assert B.compile_boundings(mixed) == want + [(6, 0.0, 2.0, -1)]
    assert B.bounding_slopes(mixed) == [0.0] * 10 + [0.01]
    assert B.bounded_columns(B.compile_boundings(mixed)) == [0, 1, 2, 3, 5, 6]


def _single_class_chains(v_out):
    return [[m] for m in br.chain(v_out)]


@pytest.mark.parametrize("v_out", br.WIDTHS)
def test_op_list_with_slopes_equals_module_route_f64(v_out):
    """Every class alone, the 11-op chain (a fraction whose total is among its own variables, one whose total is bounded later)
    and the old-class chain: the sequential restatement of the op list in f64 equals the module route to 1e-15."""
    assert len(br.op_list(br.chain(v_out))) == 11
    x = br.inputs(1000, v_out)[0].double()
    x[3, 0] = float("nan")
    for modules in _single_class_chains(v_out) + [br.chain(v_out), br.old_chain(v_out)]:
        want = br.module_chain(modules, x)
        got, tape = br.apply_ops(x.clone(), br.op_list(modules, exact=True))
        ops = br.op_list(modules)
        assert tape.shape == (len(ops) + sum(o[3] >= 0 for o in ops), 1000)
        assert torch.equal(torch.isnan(got), torch.isnan(want)) and bool(torch.isnan(got[3]).any())
        assert float((torch.nan_to_num(got) - torch.nan_to_num(want)).abs().max()) <= 1e-15


@pytest.mark.parametrize("v_out", br.WIDTHS)
def test_reverse_walk_over_the_tape_equals_autograd_f64(v_out):
    x, g = (t.double() for t in br.inputs(1000, v_out))
    for modules in _single_class_chains(v_out) + [br.chain(v_out), br.old_chain(v_out)]:
        ops = br.op_list(modules, exact=True)
        leaf = x.clone().requires_grad_()
        br.module_chain(modules, leaf).backward(g)
        _, tape = br.apply_ops(x.clone(), ops)
        g_before = g.clone()
        dx = br.reverse_walk(g, tape, ops)
        assert torch.equal(g, g_before)
        assert float((dx - leaf.grad).abs().max()) <= 1e-15


def test_derivative_at_the_bounds_is_the_slope():
    """1 strictly inside (lo, hi), s elsewhere: at the kinks the module route (torch autograd) and the reverse walk agree."""
    n2i = {"v0": 0}
    for module in (B.ReluBounding(variables=["v0"], name_to_index=n2i),
                   B.HardtanhBounding(variables=["v0"], name_to_index=n2i, min_val=-1.0, max_val=2.0),
                   B.LeakyReluBounding(variables=["v0"], name_to_index=n2i),
                   B.LeakyHardtanhBounding(variables=["v0"], name_to_index=n2i, min_val=-1.0, max_val=2.0)):
        x = torch.tensor([[-1.0], [0.0], [2.0], [0.5]], dtype=torch.float64)
        leaf = x.clone().requires_grad_()
        module(leaf.clone()).backward(torch.ones_like(x))
        ops = br.op_list([module], exact=True)
        _, tape = br.apply_ops(x.clone(), ops)
        assert torch.equal(br.reverse_walk(torch.ones_like(x), tape, ops), leaf.grad), type(module).__name__


def test_f32_walk_stays_inside_the_f64_bounds():
    """The bounds of tests/_bounding_ref.py hold for the restatement evaluated in f32 on the CPU (what the kernels compute up to
    contraction), forward and backward; no row of these inputs is near a threshold."""
    for v_out in br.WIDTHS:
        modules = br.chain(v_out)
        x, g = br.inputs(1000, v_out)
        want, bound = br.forward_ref(x, modules)
        got, tape = br.apply_ops(x.clone(), br.op_list(modules))
        assert br.check(got, want, bound, "forward") <= 1.0
        want_dx, bound_dx, _ = br.backward_ref(x, g, modules)
        left_out = br.guarded_rows(x, modules)
        assert float(left_out.double().mean()) <= 0.01
        assert br.check(br.reverse_walk(g.clone(), tape, br.op_list(modules)), want_dx, bound_dx, "backward", ~left_out) <= 1.0


def test_argument_validation_of_the_new_entry_points_without_gpu():
    from anemoi_models_amd import _lib

    lib, bad, p = _lib.load(), _lib.ANEMOI_ERR_INVALID, 4096  # (a non-null address: nothing is dereferenced before a refusal)
    err = lambda: lib.anemoi_last_error()  # noqa: E731
    # anemoi_bound_output_leaky(y, V, rows, n_ops, col, lo, hi, mul, n_fin, fcol, fmul, fadd, G, nan_map, W, fin_nan_src, slope, st)
    assert lib.anemoi_bound_output_leaky(p, 3, 8, 2, p, p, p, p, 0, None, None, None, 0, None, 0, None, None, None) == bad
    assert b"anemoi_bound_output_leaky: null slope list" in err()
    assert lib.anemoi_bound_output_leaky(p, 3, 8, 2, None, p, p, p, 0, None, None, None, 0, None, 0, None, p, None) == bad
    assert b"null op list" in err()
    assert lib.anemoi_bound_output_leaky(p, 3, 8, -1, p, p, p, p, 0, None, None, None, 0, None, 0, None, p, None) == bad
    assert b"bad argument" in err()
    assert lib.anemoi_bound_output_leaky(p, 3, 8, 0, None, None, None, None, 1, p, p, p, 4, p, 0, p, p, None) == bad
    assert b"anemoi_bound_output_leaky: nan_map needs W > 0" in err()
    assert lib.anemoi_bound_output_leaky(p, 3, 0, 2, p, p, p, p, 0, None, None, None, 0, None, 0, None, p, None) == _lib.ANEMOI_OK
    # anemoi_bound_output_train(y, V, rows, n_ops, col, lo, hi, mul, slope, tape, n_tape, stream)
    assert lib.anemoi_bound_output_train(p, 3, 8, 2, None, p, p, p, p, p, 2, None) == bad
    assert b"anemoi_bound_output_train: null op list" in err()
    assert lib.anemoi_bound_output_train(p, 3, 8, 2, p, p, p, p, None, p, 2, None) == bad
    assert b"anemoi_bound_output_train: null slope list" in err()
    assert lib.anemoi_bound_output_train(p, 3, 8, -1, p, p, p, p, p, p, 0, None) == bad
    assert b"anemoi_bound_output_train: bad argument" in err()
    assert lib.anemoi_bound_output_train(p, 3, 8, 2, p, p, p, p, p, None, 2, None) == bad and b"null tape" in err()
    for n_tape in (1, 5):
        assert lib.anemoi_bound_output_train(p, 3, 8, 2, p, p, p, p, p, p, n_tape, None) == bad and b"n_tape" in err()
    assert lib.anemoi_bound_output_train(p, 3, 0, 2, p, p, p, p, p, p, 3, None) == _lib.ANEMOI_OK
    # anemoi_bound_output_backward(g, dx, V, rows, n_ops, col, lo, hi, mul, slope, tape, n_tape, stream)
    assert lib.anemoi_bound_output_backward(None, p, 3, 8, 2, p, p, p, p, p, p, 2, None) == bad
    assert b"anemoi_bound_output_backward: null gradient" in err()
    assert lib.anemoi_bound_output_backward(p, p + 4096, 3, 8, 2, p, p, None, p, p, p, 2, None) == bad
    assert b"anemoi_bound_output_backward: null op list" in err()
    assert lib.anemoi_bound_output_backward(p, p + 4096, 3, 8, -2, p, p, p, p, p, p, 2, None) == bad
    assert b"anemoi_bound_output_backward: bad argument" in err()
    assert lib.anemoi_bound_output_backward(p, p + 4096, 3, 8, 2, p, p, p, p, None, p, 2, None) == bad
    assert b"null slope list" in err()
    assert lib.anemoi_bound_output_backward(p, p + 8, 3, 8, 2, p, p, p, p, p, p, 2, None) == bad
    assert b"dx must not alias g" in err()
    assert lib.anemoi_bound_output_backward(p, p + 4096, 3, 0, 2, p, p, p, p, p, p, 2, None) == _lib.ANEMOI_OK
