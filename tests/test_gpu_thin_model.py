"""The thin-Linear route in the model (``ANEMOI_AMD_THIN``), on config 1's graph at 256 channels with 2 processor blocks --
the size at which the mapper folds its embedding and the raw-row route exists (tests/test_gpu_raw_rows.py) -- with 16 output
variables, so that the decoder's extraction (K = 256, N = 16) and the encoder's embedding-variance product (K = 128, N = 256)
are shapes of the thin kernel's table.  (The per-head products of the raw-row encoder need head width 64, i.e. 1024 channels:
tests/test_gpu_thin_linear.py checks ``ops.linear_heads`` with its residual at those shapes.)"""

import pytest
import torch

from oracle import reference_path as ref
from test_gpu_raw_rows import DEV, _model, rel_err
from test_oracle_golden import graph_tensors

pytestmark = pytest.mark.gpu

CHANNELS, N_PROG, N_FORC, N_DIAG = 256, 13, 2, 3


@pytest.fixture(scope="module")
def setup():
    model, x, graph, n_prog = _model("o32_ico2", CHANNELS, 2, n_prog=N_PROG, n_forc=N_FORC, n_diag=N_DIAG)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        want, stages = ref.model_forward(sd, graph_tensors(graph), x, num_heads=16, num_layers=2, num_chunks=2,
                                         prognostic_in=range(n_prog), prognostic_out=range(n_prog), return_stages=True)
    return model.to(DEV), x.to(DEV), graph, want, stages["x_latent"]


def test_error_against_the_f32_oracle_with_the_route_on_and_off(setup, monkeypatch):
    """The raw-row test's own rule: with the route on, latent and prediction are no further from the f32 CPU oracle than
    1.5 x the switch-off route's distance; either route repeats bit for bit and the switch restores the other's bits.  (All
    thin sites, the opt-in statistics site included.)"""
    import bench

    model, x, _, want, latent = setup
    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "bf16")
    monkeypatch.setenv("ANEMOI_AMD_THIN_STATS", "1")
    monkeypatch.setenv("ANEMOI_AMD_THIN", "0")
    y_off, lat_off = bench.device_forward_with_latent(model, x)
    monkeypatch.setenv("ANEMOI_AMD_THIN", "1")
    y_on, lat_on = bench.device_forward_with_latent(model, x)
    y_on2, lat_on2 = bench.device_forward_with_latent(model, x)
    monkeypatch.setenv("ANEMOI_AMD_THIN", "0")
    y_off2, lat_off2 = bench.device_forward_with_latent(model, x)
    e_off, e_on = rel_err(lat_off, latent), rel_err(lat_on, latent)
    p_off, p_on = rel_err(y_off, want), rel_err(y_on, want)
    print(f"thin route vs f32 oracle: latent off {e_off:.3e}, on {e_on:.3e}; prediction off {p_off:.3e}, on {p_on:.3e}; "
          f"on vs off: prediction {rel_err(y_on, y_off):.3e}")
    # (equal bits are possible -- the same MFMA chain over K = 256 in one wave -- so that the route RAN is test_launch_lists' job)
    assert torch.equal(y_on, y_on2) and torch.equal(lat_on, lat_on2)
    assert torch.equal(y_off, y_off2) and torch.equal(lat_off, lat_off2)
    assert e_on <= 1.5 * e_off and p_on <= 1.5 * p_off


def test_launch_lists(setup, monkeypatch):
    """Switch on: the extraction and the variance product are thin launches, no 128 x 128 extraction launch is left and no
    ``add`` launch is new.  Switch off: no thin launch, the fused family's extraction and variance launches are back."""
    from anemoi_models_amd import ops

    model, x, graph, _, _ = setup
    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "bf16")
    monkeypatch.setenv("ANEMOI_AMD_THIN_STATS", "1")  # the opt-in statistics site too
    n_data, n_out = graph["data"].num_nodes, N_PROG + N_DIAG

    def launches(flag):
        monkeypatch.setenv("ANEMOI_AMD_THIN", flag)
        with torch.no_grad():
            model(x)  # (packed weights, plans)
            ops.PROFILE = []
            try:
                model(x)
            finally:
                records, ops.PROFILE = ops.PROFILE, None
        torch.cuda.synchronize()
        lin = [(bool(w.get("thin")), w["m"], w["n"], w["k"]) for name, _, _, w in records if name == "linear"]
        return lin, [name for name, _, _, _ in records]

    lin_on, names_on = launches("1")
    lin_off, names_off = launches("0")
    extraction = [r for r in lin_on + lin_off if r[1:3] == (n_data, n_out)]
    variance = [r for r in lin_on + lin_off if r[1:3] == (n_data, 256) and r[3] < CHANNELS]
    print(f"extraction launches (thin, m, n, k): {extraction}; variance launches: {variance}; add launches on / off: "
          f"{names_on.count('add')} / {names_off.count('add')}")
    assert [r for r in lin_on if r[1:3] == (n_data, n_out)] == [(True, n_data, n_out, CHANNELS)]
    assert [r for r in lin_off if r[1:3] == (n_data, n_out)] == [(False, n_data, n_out, CHANNELS)]
    assert sum(r[0] for r in lin_on) == 2 and not any(r[0] for r in lin_off)  # extraction + variance product
    wide = [r for r in lin_off if r[1:3] == (n_data, 256) and r[3] < CHANNELS]  # the variance product and the decoder's embedding
    assert [r for r in lin_on if r[1:3] == (n_data, 256) and r[3] < CHANNELS] == [(True,) + wide[0][1:]] + wide[1:]
    assert names_on.count("add") == names_off.count("add")  # (the root's skip connection; no head-product add at this width)
    # the statistics-only launch replaces a Linear AND the finalize / row_stats pass behind it: everything else is the same list
    rest_on = [n for n in names_on if n not in ("linear", "row_stats")]
    rest_off = [n for n in names_off if n not in ("linear", "row_stats")]
    assert rest_on == rest_off and names_on.count("linear") == names_off.count("linear")


# ---------------------------------------------------------------------------------------------- head width 64: the head products
WIDE, W_PROG, W_FORC, W_DIAG = 1024, 88, 4, 0  # 2 x 92 input columns + attributes + the constant 1: raw rows 256 wide


@pytest.fixture(scope="module")
def wide():
    model, x, graph, n_prog = _model("o32_ico2", WIDE, 2, n_prog=W_PROG, n_forc=W_FORC, n_diag=W_DIAG)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        want, stages = ref.model_forward(sd, graph_tensors(graph), x, num_heads=16, num_layers=2, num_chunks=2,
                                         prognostic_in=range(n_prog), prognostic_out=range(n_prog), return_stages=True)
    return model.to(DEV), x.to(DEV), graph, want, stages["x_latent"]


def test_head_products_in_the_model(wide, monkeypatch):
    """1024 channels, 16 heads of 64, raw rows 256 wide: the shapes of config 3's encoder.  Switch on: ``q -> q~`` and
    ``g -> sum alpha v`` are thin launches on the block's own slices (``sq[:, c:2c]``, ``out=att[:, :c]``, ``residual=sq[:, :c]``)
    and the head product's ``add`` launch is gone (the extraction, 88 variables here, is test_launch_lists' subject) -- the one ``add`` left is the model
    root's skip connection around the processor.  Switch off: no thin launch, both ``add`` launches.  The 1.5 x rule against the
    f32 oracle holds with these sites active.  (The hoist is off here so that ``q -> q~`` runs on every forward.)"""
    import bench
    from anemoi_models_amd import ops

    model, x, graph, want, latent = wide
    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "bf16")
    monkeypatch.setenv("ANEMOI_AMD_ENC_HOIST", "0")
    n_mesh, c = graph["hidden"].num_nodes, WIDE

    def run(flag):
        monkeypatch.setenv("ANEMOI_AMD_THIN", flag)
        y, lat = bench.device_forward_with_latent(model, x)
        ops.PROFILE = []
        try:
            y2, lat2 = bench.device_forward_with_latent(model, x)
            records = ops.PROFILE
        finally:
            ops.PROFILE = None
        torch.cuda.synchronize()
        assert torch.equal(y, y2) and torch.equal(lat, lat2)
        lin = [(bool(w.get("thin")), w["m"], w["n"], w["k"]) for name, _, _, w in records if name == "linear"]
        return y, lat, lin, [name for name, _, _, _ in records]

    y_on, lat_on, lin_on, names_on = run("1")
    y_off, lat_off, lin_off, names_off = run("0")
    thin_on = [r[1:] for r in lin_on if r[0]]
    print(f"thin launches (m, n, k): {thin_on}; add launches on / off: {names_on.count('add')} / {names_off.count('add')}")
    assert thin_on == [(n_mesh, 16 * 256, 64), (n_mesh, c, 256)]
    assert not any(r[0] for r in lin_off) and [r[1:] for r in lin_off] == [r[1:] for r in lin_on]
    assert names_on.count("add") == 1 and names_off.count("add") == 2
    rest = [n for n in names_off if n != "add"]
    assert [n for n in names_on if n != "add"] == rest
    e_off, e_on = rel_err(lat_off, latent), rel_err(lat_on, latent)
    p_off, p_on = rel_err(y_off, want), rel_err(y_on, want)
    print(f"head width 64, thin vs f32 oracle: latent off {e_off:.3e}, on {e_on:.3e}; prediction off {p_off:.3e}, on {p_on:.3e}")
    # (equal bits happen: one wave's MFMA chain over K adds in the order the tiled kernels do; the launch list shows what ran)
    assert e_on <= 1.5 * e_off and p_on <= 1.5 * p_off
