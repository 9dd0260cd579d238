"""The remappers off the device: ``preprocessing.{remapper,monomapper,multimapper,mappings}`` and ``SimpleDataIndices(remapped=)``
against vectors recorded from the reference (tests/golden/make_golden_remappers.py), the error types, the table builder
(``preprocessing.remapper.remapping`` -> ``ops.Remapping``) against the processor chain itself, the bounds of tests/_remap_ref.py
(f32 torch inside, mutants outside) and the argument checks of the three entry points, which run before any launch."""

import sys

import pytest
import torch

import _remap_ref as rr
from conftest import GOLDEN
from conftest import split_prefix

sys.path.insert(0, GOLDEN)
import make_golden_remappers as fixture  # noqa: E402  (load() and the cases' configs; imports no reference at module level)

from anemoi_models_amd.preprocessing.monomapper import Monomapper  # noqa: E402
from anemoi_models_amd.preprocessing.multimapper import Multimapper  # noqa: E402
from anemoi_models_amd.preprocessing.normalizer import InputNormalizer  # noqa: E402
from anemoi_models_amd.preprocessing.remapper import Remapper  # noqa: E402
from anemoi_models_amd.preprocessing.remapper import remapping  # noqa: E402
from anemoi_models_amd.utils.indices import SimpleDataIndices  # noqa: E402


@pytest.fixture(scope="module")
def fix():
    return fixture.load()


def indices_of(remapped):
    return SimpleDataIndices(n_prognostic=10, n_forcing=2, n_diagnostic=1, remapped=remapped)


def mapper_of(case: int):
    processors, remapped, _ = fixture.CASES[case]
    config = next(c for _, target, c in processors if target == fixture.REMAPPER)
    return Remapper(config=config, data_indices=indices_of(remapped))


# ------------------------------------------------------------------------------------------------ modules
@pytest.mark.parametrize("case", sorted(fixture.CASES))
def test_modules_match_the_reference_vectors(fix, case):
    mapper = mapper_of(case)
    assert type(mapper) is (Multimapper if fixture.CASES[case][1] else Monomapper)
    for what in ("transform.training", "transform.inference", "inverse.training", "inverse.inference"):
        x, want = fix[f"case{case}.{what}.x"], fix[f"case{case}.{what}.y"]
        got = mapper.transform(x.clone(), in_place=False) if what.startswith("transform") else \
            mapper.inverse_transform(x.clone(), in_place=False)
        assert got.shape == want.shape and got.dtype == want.dtype, what
        torch.testing.assert_close(got, want, rtol=1e-6, atol=0, msg=lambda m: f"case {case} {what}: {m}")
        copies = [c for c in range(want.shape[-1]) if any(torch.equal(want[..., c], x[..., k]) for k in range(x.shape[-1]))]
        assert len(copies) >= want.shape[-1] - 4 and all(torch.equal(got[..., c], want[..., c]) for c in copies), what
    # the processors' forward() contract and, for a Monomapper, the in-place form
    x = fix[f"case{case}.transform.inference.x"]
    torch.testing.assert_close(mapper(x.clone(), in_place=False), fix[f"case{case}.transform.inference.y"], rtol=1e-6, atol=0)
    if type(mapper) is Monomapper:
        buf = x.clone()
        assert mapper.transform(buf) is buf
    with pytest.raises(ValueError, match="does not match the training"):
        mapper.transform(torch.zeros(2, 3))
    with pytest.raises(ValueError, match="does not match the training"):
        mapper.inverse_transform(torch.zeros(2, 3))


def test_loss_mask(fix):
    one = {"prog_7": fixture.REMAPPED["prog_7"]}
    mapper = Remapper(config={"default": "none", "cos_sin": one}, data_indices=indices_of(one))
    got = mapper.transform_loss_mask(fix["lossmask.x"])
    assert torch.equal(got, fix["lossmask.y"])
    with pytest.raises(NotImplementedError, match="forcing"):  # the reference fails on the shapes there
        mapper_of(1).transform_loss_mask(torch.ones(7, 11))


def test_error_types():
    idx = indices_of(fixture.REMAPPED)
    with pytest.raises(NotImplementedError, match="mix of monomapper and multimapper"):
        Remapper(config={"default": "none", "log1p": ["prog_2"], "cos_sin": fixture.COS_SIN["cos_sin"]}, data_indices=idx)
    with pytest.raises(ValueError, match="No valid remapping method"):
        Remapper(config={"default": "none", "tanh": ["prog_2"]}, data_indices=idx)
    with pytest.raises(AssertionError, match="not a variable"):  # cos_sin names that config.data.remapped does not list
        Remapper(config={"default": "none", "cos_sin": {"prog_7": ["c7", "s7"]}}, data_indices=idx)
    from anemoi_models_amd.preprocessing import mappings

    with pytest.raises(ValueError, match="0.5"):
        mappings.boxcox_converter(torch.ones(2), lambd=0.25)
    x = torch.rand(64) * 4
    assert torch.equal(mappings.boxcox_converter(x), (torch.pow(x, 0.5) - 1) / 0.5)
    assert torch.equal(mappings.inverse_boxcox_converter(x), torch.pow(x * 0.5 + 1, 2.0))


# ------------------------------------------------------------------------------------------------ indices
def _view(idx) -> dict:
    return {"name_to_index": dict(idx.name_to_index),
            **{k: getattr(idx, k).tolist() for k in ("full", "prognostic", "diagnostic", "forcing")}}


@pytest.mark.parametrize("which, remapped", [("views", fixture.REMAPPED), ("lossmask_views", {"prog_7": ["cos_p7", "sin_p7"]})])
def test_simple_data_indices_remapped_views(fix, which, remapped):
    idx = indices_of(remapped)
    for key, want in fix["indices"][which].items():
        view, side = key.split(".")
        got = _view(getattr(getattr(idx, view), side))
        if key in ("data.input", "data.output"):
            # the plain dataset view keeps the attributes it had before `remapped` existed: its list of the variables the side
            # leaves out (input.diagnostic / output.forcing) is empty
            left_out = "diagnostic" if side == "input" else "forcing"
            got.pop(left_out), want.pop(left_out)
        assert got == want, key
        assert len(getattr(getattr(idx, view), side)) == len(want["full"])
    assert idx.num_input == 12 and idx.num_output == 11


def test_simple_data_indices_assertions_and_default():
    with pytest.raises(AssertionError, match="diagnostic"):
        indices_of({"diag_0": ["a", "b"]})
    with pytest.raises(AssertionError, match="does not exist"):
        indices_of({"prog_77": ["a", "b"]})
    plain = SimpleDataIndices(n_prognostic=10, n_forcing=2, n_diagnostic=1)
    assert plain.internal_model is plain.model and plain.internal_data is plain.data and plain.remapped == {}


# ------------------------------------------------------------------------------------------------ table builder
def _statistics(gold):
    return {k: v.numpy() for k, v in split_prefix(gold, "stat.").items()}


@pytest.mark.parametrize("case", sorted(fixture.CASES))
def test_table_builder_against_the_processor_chain(fix, golden_interface, case):
    processors, remapped, _ = fixture.CASES[case]
    idx = indices_of(remapped)
    chain = []
    for _, target, config in processors:
        if target == fixture.REMAPPER:
            chain.append(Remapper(config=config, data_indices=idx))
        else:
            chain.append(InputNormalizer(config=fixture.normalizer_config(remapped), data_indices=idx,
                                         statistics=_statistics(golden_interface)))
    mapper_first = type(chain[1]) is InputNormalizer
    mapper, norm = (chain[0], chain[1]) if mapper_first else (chain[1], chain[0])
    i_in, i_out = norm._input_idx.long(), norm._output_idx.long()
    remap = remapping(mapper, (norm._norm_mul[i_in], norm._norm_add[i_in]), (norm._norm_mul[i_out], norm._norm_add[i_out]),
                      mapper_first, "cpu")
    t = rr.tables(remap)
    f32 = {k: None if t[k] is None else tuple(p.float() for p in t[k]) for k in ("pre", "post")}
    x = fix["batch"][:, :, :97]
    want = x.clone()
    for p in chain:
        want = p(want, in_place=False)
    got = rr.forward_f32(x[..., t["src"]], t["op"], f32["pre"], f32["post"])
    assert remap.v_raw == 12 and remap.v_int == want.shape[-1] == len(idx.internal_model.input)
    torch.testing.assert_close(got, want, rtol=1e-6, atol=1e-6)
    y = torch.randn((1, 1, 97, len(idx.internal_model.output)), generator=torch.Generator().manual_seed(case))
    want = y.clone()
    for p in chain[::-1]:
        want = p(want, in_place=False, inverse=True)
    got = rr.inverse_f32(y, t)
    assert remap.v_int_out == y.shape[-1] and remap.v_out == want.shape[-1] == 11
    err = (got - want).abs()
    names = t["inv_op"]
    for c in range(want.shape[-1]):  # directions on the circle
        col = torch.minimum(err[..., c], (360.0 - err[..., c]).abs()) if names[c] == "atan2deg" else err[..., c]
        assert float(col.max()) <= 1e-5 * max(1.0, float(want[..., c].abs().max())), (c, names[c])
    res = [-1] * remap.v_int_out
    for c, j in zip(idx.internal_model.output.prognostic.tolist(), idx.internal_model.input.prognostic.tolist()):
        res[c] = j
    assert remap.h_res.tolist() == res
    if remapped:  # a cos column's residual is the cosine of the raw direction
        out_names = list(idx.internal_model.output.name_to_index)
        j = res[out_names.index("cos_p7")]
        assert t["op"][j] == "cos" and int(t["src"][j]) == 7
        with pytest.raises(ValueError, match="refuses"):
            remapping(mapper, (norm._norm_mul[i_in], norm._norm_add[i_in]), None, True, "cpu")


def test_remapping_refuses_bad_tables():
    from anemoi_models_amd.ops import Remapping

    good = dict(device="cpu", v_raw=3, src=[0, 1, 2, 2], op=["copy", "log1p", "cos", "sin"], res=[0, 1, -1],
                s0=[0, 1, 2], s1=[-1, -1, 3], inv_op=["copy", "expm1", "copy"])
    Remapping(**good)
    for change in ({"src": [0, 1, 2, 3]}, {"op": ["copy", "log1p", "cos", "expm1"]}, {"res": [0, 1, 4]},
                   {"s0": [0, 1, 3]}, {"inv_op": ["copy", "expm1", "atan2deg"], "s1": [-1, -1, 3]},
                   {"inv_op": ["copy", "log1p", "copy"]}, {"pre": (torch.ones(3), torch.zeros(3))}):
        with pytest.raises(ValueError, match="Remapping"):
            Remapping(**{**good, **change})


# ------------------------------------------------------------------------------------------------ bounds
def _emulate(remap, x, y, mutant=""):
    """The three kernels' results in f32 torch, from the tables."""
    t = rr.tables(remap)
    pre, post = (None if t[k] is None else tuple(p.float() for p in t[k]) for k in ("pre", "post"))
    f = rr.forward_f32(x[..., t["src"]], t["op"], pre, post, mutant)
    b, nt, ens, g, v_int = f.shape
    feat = f.permute(0, 2, 3, 1, 4).reshape(b * ens * g, nt * v_int)
    last = x[:, -1][..., t["src"]] if mutant == "residual_from_raw" else f[:, -1]
    res = y.clone()
    for c, j in enumerate(t["res"].tolist()):
        if j >= 0:
            res[..., c] = y[..., c] + last[..., j]
    return feat, res, rr.inverse_f32(y, t, mutant)


CASES = [(shape, extra, affine) for shape in rr.SHAPES for extra in (1, 2) for affine in (False, True)]


@pytest.mark.parametrize("shape, extra, affine", CASES)
def test_f32_torch_stays_inside_the_bounds(shape, extra, affine):
    remap, x, y = rr.make_case(shape, extra, affine)
    feat, res, out = _emulate(remap, x, y)
    ldo = feat.shape[1]
    want, bound = rr.assemble_ref(x, None, None, remap, ldo, torch.float32)
    used = [rr.check(feat, want, bound, "assemble")]
    used.append(rr.check(feat.bfloat16(), *rr.assemble_ref(x, None, None, remap, ldo, torch.bfloat16), "assemble bf16"))
    used.append(rr.check(res, *rr.residual_ref(y, x, remap), "residual"))
    want, bound, period = rr.unmap_ref(y, remap)
    used.append(rr.check(out, want, bound, "unmap", period))
    assert int(torch.isnan(want).sum()) > 0 and int(torch.isnan(rr.residual_ref(y, x, remap)[0]).sum()) > 0
    print(f"{shape} +{extra} affine={affine}: largest fractions of a bound used {[f'{u:.3f}' for u in used]}")


@pytest.mark.parametrize("mutant, kernels", [("cos_sin_swapped", ("assemble", "residual", "unmap")),
                                             ("no_degree_factor", ("assemble", "residual", "unmap")),
                                             ("exp_for_expm1", ("unmap",)),
                                             ("pairs_exchanged", ("assemble", "residual", "unmap")),
                                             ("residual_from_raw", ("residual",))])
@pytest.mark.parametrize("affine", [False, True])
def test_mutants_fall_outside_the_bounds(mutant, kernels, affine):
    remap, x, y = rr.make_case(rr.SHAPES[0], 2, affine)
    feat, res, out = _emulate(remap, x, y, mutant)
    if "assemble" in kernels:
        with pytest.raises(AssertionError):
            rr.check(feat, *rr.assemble_ref(x, None, None, remap, feat.shape[1], torch.float32), "assemble")
    if "residual" in kernels:
        with pytest.raises(AssertionError):
            rr.check(res, *rr.residual_ref(y, x, remap), "residual")
    if "unmap" in kernels:
        want, bound, period = rr.unmap_ref(y, remap)
        with pytest.raises(AssertionError):
            rr.check(out, want, bound, "unmap", period)


# ------------------------------------------------------------------------------------------------ entry points' checks
def test_entry_points_refuse_bad_tables_before_any_launch():
    """Null tables, src outside [0, V_raw), op codes out of range and an ldo that is too small: ANEMOI_ERR_INVALID.  The checks
    read the HOST tables only, so they run here, without a device: the data pointers are never followed."""
    from anemoi_models_amd import _lib

    lib = _lib.load()
    remap, _, _ = rr.make_case(rr.SHAPES[0], 2, False)
    buf = torch.zeros(64)
    p, h = buf.data_ptr(), lambda t: t.data_ptr()
    v_raw, v_int, v_io, v_out = remap.v_raw, remap.v_int, remap.v_int_out, remap.v_out

    def assemble(src=p, op=p, h_src=None, h_op=None, ldo=24, pre=(None, None)):
        return lib.anemoi_assemble_nodes_remapped(_lib.F32, p, 2, 2, 2, 37, v_raw, v_int, None, 0, None, 0, p, ldo, src, op, pre[0],
                                                  pre[1], None, None, h(remap.h_src) if h_src is None else h(h_src),
                                                  h(remap.h_op) if h_op is None else h(h_op), None)

    def residual(h_res=None, h_src=None, res=p):
        return lib.anemoi_residual_remapped(p, v_io, p, 2, 2, 2, 37, v_raw, v_int, res, p, p, None, None, None, None,
                                            h(remap.h_res) if h_res is None else h(h_res),
                                            h(remap.h_src) if h_src is None else h(h_src), h(remap.h_op), None)

    def unmap(h_s0=None, h_s1=None, h_op=None, s0=p):
        return lib.anemoi_unmap_output(p, v_io, p + 4, v_out, 8, s0, p, p, None, None, None, None,
                                       h(remap.h_s0) if h_s0 is None else h(h_s0), h(remap.h_s1) if h_s1 is None else h(h_s1),
                                       h(remap.h_inv_op) if h_op is None else h(h_op), None)

    def changed(table, at, value):
        out = table.clone()
        out[at] = value
        return out

    bad = _lib.ANEMOI_ERR_INVALID
    assert assemble(ldo=2 * v_int - 1) == bad and b"ldo too small" in lib.anemoi_last_error()
    assert assemble(src=None) == bad and assemble(op=None) == bad
    assert assemble(pre=(p, None)) == bad
    assert assemble(h_src=changed(remap.h_src, 1, v_raw)) == bad and b"src[1]" in lib.anemoi_last_error()
    assert assemble(h_src=changed(remap.h_src, 0, -1)) == bad
    assert assemble(h_op=changed(remap.h_op, 2, 6)) == bad and b"op[2]" in lib.anemoi_last_error()  # an inverse op code
    assert assemble(h_op=changed(remap.h_op, 2, -1)) == bad
    assert residual(res=None) == bad
    assert residual(h_res=changed(remap.h_res, 0, v_int)) == bad and residual(h_res=changed(remap.h_res, 0, -2)) == bad
    assert residual(h_src=changed(remap.h_src, 3, v_raw)) == bad
    assert unmap(s0=None) == bad
    assert unmap(h_s0=changed(remap.h_s0, 0, v_io)) == bad
    atan = remap.h_inv_op.tolist().index(9)
    assert unmap(h_s1=changed(remap.h_s1, atan, v_io)) == bad and unmap(h_s1=changed(remap.h_s1, atan, -1)) == bad
    assert unmap(h_op=changed(remap.h_inv_op, 0, 1)) == bad and unmap(h_op=changed(remap.h_inv_op, 0, 10)) == bad


# ------------------------------------------------------------------------------------------------ interface, off the device
def test_rollout_refuses_a_multimapper(graph_o32, golden_interface):
    iface = rr.build_case_interface(graph_o32, golden_interface, 1)
    batch = fixture.load()["batch"]
    with pytest.raises(NotImplementedError, match="Multimapper"):
        iface.rollout(batch, 2)
    assert iface._fused_route(batch) is None  # a CPU tensor, and the first call
    assert len(iface.data_indices.internal_model.input) == 14 and iface.model.num_input_channels == 14
