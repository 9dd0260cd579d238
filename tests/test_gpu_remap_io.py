"""The remapper kernels on the device (csrc/remap.hip): the three entry points per element against the f64 contracts of
tests/_remap_ref.py, and ``AnemoiModelInterface.predict_step`` with a remapper next to the normaliser against the vectors
recorded from the reference (tests/golden/make_golden_remappers.py)."""

import os
import subprocess
import sys

import pytest
import torch

import _remap_ref as rr

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
N_LL, N_TR = 2, 1  # widest row: T * V_int + 3 = 21 = the element-form ldo


def on(remap):
    """The same remapping with its device tables on the GPU."""
    from anemoi_models_amd.ops import Remapping

    t = rr.tables(remap)
    f32 = {k: None if t[k] is None else tuple(p.float() for p in t[k]) for k in ("pre", "post", "inv_pre", "inv_post")}
    return Remapping(DEV, remap.v_raw, t["src"].tolist(), t["op"], t["res"].tolist(), t["s0"].tolist(), t["s1"].tolist(),
                     t["inv_op"], **f32)


def attributes(g, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn((g, N_LL), generator=gen), torch.randn((g, N_TR), generator=gen)


@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("extra", [1, 2])
@pytest.mark.parametrize("shape", rr.SHAPES)
def test_entry_points_against_the_f64_contracts(shape, extra, affine):
    from anemoi_models_amd import ops

    host, x, y = rr.make_case(shape, extra, affine, seed=shape[3] + extra)
    remap = on(host)
    b, t, ens, g, _ = shape
    ll, tr = attributes(g, 3)
    xd, lld, trd = x.to(DEV), ll.to(DEV), tr.to(DEV)
    used = {}
    for ldo in (24, 21):  # eight columns per thread / one
        for dtype in (F32, BF16):
            trainable = (tr, trd) if ldo == 24 else (None, None)
            got = ops.assemble_nodes(xd, lld, trainable[1], b, dtype, ld_out=ldo, remap=remap)
            want, bound = rr.assemble_ref(x, ll, trainable[0], host, ldo, dtype)
            used[f"assemble ldo {ldo} {dtype}"] = rr.check(got.float(), want, bound, f"assemble ldo {ldo} {dtype}")
            again = ops.assemble_nodes(xd, lld, trainable[1], b, dtype, ld_out=ldo, remap=remap)
            assert torch.equal(got.view(torch.int16 if dtype == BF16 else torch.int32),
                               again.view(torch.int16 if dtype == BF16 else torch.int32))
    got = ops.residual_remapped(y.to(DEV), xd, remap)
    used["residual"] = rr.check(got, *rr.residual_ref(y, x, host), "residual")
    assert torch.equal(got.view(torch.int32), ops.residual_remapped(y.to(DEV), xd, remap).view(torch.int32))
    yd = y.to(DEV)
    got = ops.unmap_output(yd, remap)
    want, bound, period = rr.unmap_ref(y, host)
    assert got.shape == want.shape and torch.equal(yd.cpu().view(torch.int32), y.view(torch.int32))  # y is read only
    used["unmap"] = rr.check(got, want, bound, "unmap", period)
    assert torch.equal(got.view(torch.int32), ops.unmap_output(yd, remap).view(torch.int32))
    print(f"{shape} +{extra} affine={affine}: largest fraction of a bound used", {k: round(v, 3) for k, v in used.items()})


def test_64_bit_index_instantiations(tmp_path):
    """``ANEMOI_AMD_IDX64=1`` (read once per process) forces the 64-bit index instantiations of the three kernels: a fresh
    process computes one case with them, this one with the 32-bit ones, bit for bit the same."""
    from anemoi_models_amd import ops

    here = os.path.dirname(os.path.abspath(__file__))
    script = tmp_path / "run.py"
    script.write_text(
        "import sys, torch\n"
        f"sys.path[:0] = [{os.path.dirname(here)!r}, {here!r}]\n"
        "import _remap_ref as rr\n"
        "from test_gpu_remap_io import attributes, on\n"
        "from anemoi_models_amd import ops\n"
        "host, x, y = rr.make_case(rr.SHAPES[0], 2, True, seed=5)\n"
        "remap, (ll, tr) = on(host), attributes(37, 3)\n"
        "out = {'a': ops.assemble_nodes(x.cuda(), ll.cuda(), tr.cuda(), 2, torch.bfloat16, ld_out=24, remap=remap),\n"
        "       'r': ops.residual_remapped(y.cuda(), x.cuda(), remap), 'u': ops.unmap_output(y.cuda(), remap)}\n"
        "torch.save({k: v.cpu() for k, v in out.items()}, sys.argv[1])\n")
    path = str(tmp_path / "out.pt")
    subprocess.run([sys.executable, str(script), path], check=True, env=dict(os.environ, ANEMOI_AMD_IDX64="1"), timeout=300)
    child = torch.load(path)
    host, x, y = rr.make_case(rr.SHAPES[0], 2, True, seed=5)
    remap, (ll, tr) = on(host), attributes(37, 3)
    mine = {"a": ops.assemble_nodes(x.to(DEV), ll.to(DEV), tr.to(DEV), 2, BF16, ld_out=24, remap=remap),
            "r": ops.residual_remapped(y.to(DEV), x.to(DEV), remap), "u": ops.unmap_output(y.to(DEV), remap)}
    for k, v in mine.items():
        bits = torch.int16 if v.dtype == BF16 else torch.int32
        assert torch.equal(v.cpu().view(bits), child[k].view(bits)), k
    rr.check(child["a"].float(), *rr.assemble_ref(x, ll, tr, host, 24, BF16), "assemble, 64-bit indices")


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("ldo", [24, 21])
@pytest.mark.parametrize("pairs", ["none", "identity"])
def test_all_copy_table_is_the_plain_assembly(ldo, dtype, pairs):
    from anemoi_models_amd import ops
    from anemoi_models_amd.ops import Remapping

    b, t, ens, g, v = 2, 2, 2, 37, 9
    gen = torch.Generator().manual_seed(2)
    x = torch.randn((b, t, ens, g, v), generator=gen).to(DEV)
    ll, tr = (a.to(DEV) for a in attributes(g, 4))
    one = (torch.ones(v), torch.zeros(v))
    kw = {} if pairs == "none" else {"pre": one, "post": one}
    remap = Remapping(DEV, v, list(range(v)), ["copy"] * v, [-1] * v, list(range(v)), [-1] * v, ["copy"] * v, **kw)
    got = ops.assemble_nodes(x, ll, tr, b, dtype, ld_out=ldo, remap=remap)
    want = ops.assemble_nodes(x, ll, tr, b, dtype, ld_out=ldo)
    bits = torch.int16 if dtype == BF16 else torch.int32
    assert torch.equal(got.view(bits), want.view(bits))


# ------------------------------------------------------------------------------------------------ predict_step
@pytest.fixture(scope="module")
def fix():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_remappers as fixture

    return fixture.load()


def report(case, what, errs, limit):
    print(f"case {case} {what}: per-column error over the column's magnitude {[f'{e:.2e}' for e in errs]}")
    assert max(errs) < limit, (what, errs)


@pytest.mark.parametrize("case", [1, 2, 3, 4])
def test_interface_predict_step_with_a_remapper_vs_reference(graph_o32, golden_interface, fix, case, monkeypatch):
    """Per output column: max error over the column's max magnitude below 1e-4 against the reference (the bound of the imputer
    interface tests), on the circle and against 360 for the direction column; fused against generic below 1e-5."""
    from anemoi_models_amd import trail

    iface = rr.build_case_interface(graph_o32, golden_interface, case, fix).to(DEV).eval()
    directions = (7,) if case in (1, 4) else ()  # prog_7 in the raw output layout
    batch1, batch2 = fix["batch"].to(DEV), fix["batch2"].to(DEV)
    assert iface._fused_route(batch1) is None
    y1 = iface.predict_step(batch1)
    assert y1.dtype == torch.float32 and tuple(y1.shape) == tuple(fix[f"case{case}.y1"].shape)
    report(case, "first call (generic)", rr.column_errors(y1, fix[f"case{case}.y1"], directions), 1e-4)
    assert iface._fused_route(batch2) is not None
    with trail.record() as launches:
        y2 = iface.predict_step(batch2)
    names = {n.split(":")[0] for n in launches.names()}
    assert {"anemoi_assemble_nodes_remapped", "anemoi_residual_remapped", "anemoi_unmap_output"} <= names
    assert ("anemoi_bound_output" in names) == (case == 4)
    report(case, "second call (fused)", rr.column_errors(y2, fix[f"case{case}.y2"], directions), 1e-4)
    monkeypatch.setenv("ANEMOI_AMD_FUSE_NORMALIZER", "0")
    assert iface._fused_route(batch2) is None
    y3 = iface.predict_step(batch2)
    report(case, "generic", rr.column_errors(y3, fix[f"case{case}.y2"], directions), 1e-4)
    report(case, "fused against generic", rr.column_errors(y2, y3, directions), 1e-5)


def test_chains_and_models_that_keep_the_generic_route(graph_o32, graph_hier, golden_interface, fix):
    import make_golden_remappers as fixture

    from anemoi_models_amd.utils.presets import hierarchical_model_config

    batch = fix["batch"].to(DEV)
    # an imputer in the same chain
    imputer = ("imputer", "anemoi.models.preprocessing.imputer.InputImputer", {"default": "none", "mean": ["prog_2"]})
    iface = rr.build_case_interface(graph_o32, golden_interface, 1, fix, processors=[imputer] + fixture.CASES[1][0]).to(DEV).eval()
    iface.predict_step(batch)
    assert iface._fused_route(batch) is None
    # the hierarchical model (the route's other conditions hold: not the first call, the width, the device)
    hier = rr.build_case_interface(graph_hier, golden_interface, 3, config=hierarchical_model_config(64, 16),
                                   model_target="anemoi.models.models.hierarchical.AnemoiModelEncProcDecHierarchical").to(DEV).eval()
    hier.pre_processors.first_run = False
    assert hier._fused_route(batch) is None
    flat = rr.build_case_interface(graph_o32, golden_interface, 3, fix).to(DEV).eval()
    flat.pre_processors.first_run = False
    assert flat._fused_route(batch) is not None
    # a Multimapper before the normaliser: generic, and it fails as the reference fails
    first = rr.build_case_interface(graph_o32, golden_interface, 1, fix, processors=fixture.MULTI_FIRST).to(DEV).eval()
    first.pre_processors.first_run = False
    assert first._fused_route(batch) is None
    error = {"RuntimeError": RuntimeError}[fix["indices"]["multimapper_first_error"]]
    with pytest.raises(error):
        first.predict_step(batch)
