"""The decoder fold in the model (``ANEMOI_AMD_DEC_FOLD``): config 1's graph at 256 channels, 2 processor
blocks, bf16 -- where the mappers fold their embeddings (tests/test_gpu_raw_rows.py) -- against the f32 CPU oracle and
against the switch-off route; launch coverage; rebuilds of the composed weight."""

import pytest
import torch

from oracle import reference_path as ref
from test_gpu_raw_rows import DEV, _model, rel_err
from test_oracle_golden import graph_tensors

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


def _build():
    model, x, graph, n_prog = _model("o32_ico2", 256, 2, n_prog=10, n_forc=2, n_diag=1)
    return model, x, graph, n_prog


def _forward(model, x, record=False):
    from anemoi_models_amd import ops

    if record:
        ops.PROFILE = []
    try:
        with torch.no_grad():
            y = model(x)
        recs = None if not record else [(name, w.get("m"), w.get("n"), w.get("k")) for name, _, _, w in ops.PROFILE]
    finally:
        ops.PROFILE = None
    torch.cuda.synchronize()
    return y, recs


def test_prediction_against_oracle_and_switch(monkeypatch):
    """Prediction error against the f32 CPU oracle with the route on within 1.5 x the error with it off; the latent (in front
    of the decoder) unchanged bit for bit; either route repeats bit for bit and the switch goes back and forth."""
    import bench

    model, x, graph, n_prog = _build()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        want = ref.model_forward(sd, graph_tensors(graph), x, num_heads=16, num_layers=2, num_chunks=2,
                                 prognostic_in=range(n_prog), prognostic_out=range(n_prog))
    model, x = model.to(DEV), x.to(DEV)
    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "bf16")
    monkeypatch.setenv("ANEMOI_AMD_DEC_FOLD", "0")
    y_off, lat_off = bench.device_forward_with_latent(model, x)
    monkeypatch.setenv("ANEMOI_AMD_DEC_FOLD", "1")
    y_on, lat_on = bench.device_forward_with_latent(model, x)
    y_on2, lat_on2 = bench.device_forward_with_latent(model, x)
    monkeypatch.setenv("ANEMOI_AMD_DEC_FOLD", "0")
    y_off2, lat_off2 = bench.device_forward_with_latent(model, x)
    p_off, p_on = rel_err(y_off, want), rel_err(y_on, want)
    print(f"config-1 graph, 256 channels, prediction vs f32 oracle: route off {p_off:.3e}, route on {p_on:.3e}")
    assert not torch.equal(y_on, y_off), "the switch changed nothing: the folded route did not run"
    assert torch.equal(lat_on, lat_off) and torch.equal(lat_on2, lat_off) and torch.equal(lat_off2, lat_off)
    assert torch.equal(y_on, y_on2) and torch.equal(y_off, y_off2)
    assert p_on <= 1.5 * p_off


def test_launch_coverage(monkeypatch):
    """Route on: one ``q | u`` product (N = C + H up) over the grid rows, one projection with K = C + H up + 2 K_s, no
    ``x_r | q | u`` product, and the embedding of the grid rows is never packed, let alone launched.  (At 256 channels the
    statistics side product of the rows' LayerNorm is an N = 256, K = K_s Linear too -- the encoder launches one on the same
    rows in either route -- so the embedding is told by its packed weight, not by its shape.)  Route off: the parent's list."""
    model, x, graph, _ = _build()
    model, x = model.to(DEV), x.to(DEV)
    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "bf16")
    n_grid, c, h = graph["data"].num_nodes, 256, 16
    up = model.decoder.proc.fold_width(BF16)

    def lists(flag):
        monkeypatch.setenv("ANEMOI_AMD_DEC_FOLD", flag)
        model.decoder._packed.clear()
        _forward(model, x)
        _, recs = _forward(model, x, record=True)
        emb_packed = [k for k in model.decoder._packed._store if k[:2] == ("emb_nodes_dst", "w")]
        lin = [r for r in recs if r[0] == "linear" and r[1] == n_grid]
        return recs, lin, emb_packed

    recs_on, lin_on, emb_on = lists("1")
    recs_off, lin_off, emb_off = lists("0")
    ks = [r for r in recs_on if r[0] == "row_scale"]
    assert len(ks) == 1, "one raw-row tail launch"
    k_s = next(r[3] for r in lin_off if r[2] == 2 * c + h * up)
    count = lambda lin, **kw: len([r for r in lin if all(r[{"n": 2, "k": 3}[key]] == val for key, val in kw.items())])  # noqa: E731
    print(f"grid rows {n_grid}, K_s {k_s}, up {up}: on {lin_on}; off {lin_off}")
    assert k_s in (64, 128, 256)
    assert emb_on == [] and emb_off != []
    assert count(lin_on, n=c + h * up, k=k_s) == 1 and count(lin_on, n=2 * c + h * up) == 0
    assert count(lin_on, n=c, k=c + h * up + 2 * k_s) == 1 and count(lin_on, n=c, k=c + h * up) == 0
    assert count(lin_off, n=c + h * up, k=k_s) == 0 and count(lin_off, n=2 * c + h * up, k=k_s) == 1
    assert count(lin_off, n=c, k=c + h * up + 2 * k_s) == 0 and count(lin_off, n=c, k=c + h * up) == 1
    assert count(lin_on, n=c, k=k_s) == count(lin_off, n=c, k=k_s)  # (statistics product in, embedding out)
    assert not [r for r in recs_off if r[0] == "row_scale"]
    edge = lambda recs: len([r for r in recs if r[0] == "gt_edge_attention"])  # noqa: E731
    assert edge(recs_on) == edge(recs_off)


@pytest.fixture(scope="module")
def shared_model():
    """One model for the tests below, which change switches only (never a parameter)."""
    model, x, _, _ = _build()
    return model.to(DEV), x.to(DEV)


def _refused_route_is_the_switch_off_route(monkeypatch, shared_model, switch, name, value):
    """Under ``name=value`` the route behind ``switch`` is refused: ``switch=1`` and ``switch=0`` then run the same launches
    and give the same bits (and the forward runs -- no rows are handed over without an embedding their route reads)."""
    model, x = shared_model
    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "bf16")
    monkeypatch.setenv(name, value)
    got = {}
    for flag in ("1", "0"):
        monkeypatch.setenv(switch, flag)
        _forward(model, x)  # packs and hoists what this setting needs: the recorded forward is a steady-state one
        got[flag] = _forward(model, x, record=True)
    (y_on, recs_on), (y_off, recs_off) = got["1"], got["0"]
    print(f"{name}={value}: {len(recs_on)} launches with {switch}=1, {len(recs_off)} with {switch}=0")
    assert recs_on and recs_on == recs_off
    assert torch.equal(y_on, y_off)


@pytest.mark.parametrize("name,value", [("ANEMOI_AMD_THIN_STATS", "1"), ("ANEMOI_AMD_MXFP8", "1"), ("ANEMOI_AMD_EDGE_FOLD", "0"),
                                        ("ANEMOI_AMD_EMBED_FOLD", "0"), ("ANEMOI_AMD_LN_FOLD", "0"),
                                        ("ANEMOI_INFERENCE_NUM_CHUNKS", "2")])
def test_a_setting_that_refuses_the_decoder_fold_gives_the_switch_off_route(monkeypatch, shared_model, name, value):
    _refused_route_is_the_switch_off_route(monkeypatch, shared_model, "ANEMOI_AMD_DEC_FOLD", name, value)


@pytest.mark.parametrize("name,value", [("ANEMOI_AMD_EDGE_FOLD", "0"), ("ANEMOI_INFERENCE_NUM_CHUNKS", "2"),
                                        ("ANEMOI_AMD_MXFP8", "1")])
def test_a_setting_that_refuses_the_raw_row_encoder_gives_the_switch_off_route(monkeypatch, shared_model, name, value):
    _refused_route_is_the_switch_off_route(monkeypatch, shared_model, "ANEMOI_AMD_EDGE_RAW", name, value)


@pytest.mark.parametrize("what", ["emb_nodes_dst", "lin_self", "projection", "load_state_dict"])
def test_a_changed_parameter_rebuilds_the_composed_weight(monkeypatch, what):
    """After an in-place update of a parameter that enters the composed weight (or ``load_state_dict``) the output changes and
    equals that of a fresh model with the same state (fresh caches)."""
    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "bf16")
    monkeypatch.setenv("ANEMOI_AMD_DEC_FOLD", "1")
    model, x, _, _ = _build()
    model, x = model.to(DEV), x.to(DEV)
    y_before, _ = _forward(model, x)
    _forward(model, x)
    key = next(k for k in model.decoder.proc._packed._store if k[:2] == ("projf", "decfold"))
    w_before = model.decoder.proc._packed._store[key][1][0]
    if what == "load_state_dict":
        other, _, _, _ = _build()
        with torch.no_grad():
            for p in other.parameters():
                p.mul_(1.25)
        model.load_state_dict(other.state_dict())
    else:
        with torch.no_grad():
            layer = model.decoder.emb_nodes_dst if what == "emb_nodes_dst" else getattr(model.decoder.proc, what)
            layer.weight.mul_(1.5)
    y_after, _ = _forward(model, x)
    y_after2, _ = _forward(model, x)
    w_after = model.decoder.proc._packed._store[key][1][0]
    fresh, _, _, _ = _build()
    fresh = fresh.to(DEV)
    fresh.load_state_dict(model.state_dict())
    y_fresh, _ = _forward(fresh, x)
    assert w_after is not w_before and not torch.equal(w_after, w_before), "the composed weight was not rebuilt"
    assert not torch.equal(y_after, y_before), "the parameter does not reach the output: the test shows nothing"
    assert torch.equal(y_after, y_after2) and torch.equal(y_after, y_fresh)
