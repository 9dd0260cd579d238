"""The encoder's hoisted destination side (``ANEMOI_AMD_ENC_HOIST``): on the inference path the mesh
rows, their embedding with its statistics, ``x_r | q | u`` and ``qt`` are built once per parameter state.  Config 1's graph at
256 channels, 2 processor blocks, bf16 -- where the raw-row route exists (tests/test_gpu_raw_rows.py)."""

import pytest
import torch

from test_gpu_raw_rows import DEV, _model

pytestmark = pytest.mark.gpu


def _build():
    model, x, graph, _ = _model("o32_ico2", 256, 2, n_prog=10, n_forc=2, n_diag=1)
    return model.to(DEV), x.to(DEV), graph


def _forward(model, x, record=False):
    from anemoi_models_amd import ops

    if record:
        ops.PROFILE = []
    try:
        with torch.no_grad():
            y = model(x)
        names = None if not record else [(name, w.get("m"), w.get("n"), w.get("k")) for name, _, _, w in ops.PROFILE]
    finally:
        ops.PROFILE = None
    torch.cuda.synchronize()
    return y, names


def test_bits_and_launches(monkeypatch):
    """Hoist on and off give the same bits; the first forward records the parent's launch list, the second and third record
    it without the hoisted launches (the mesh rows' assemble, their embedding, x_r | q | u, qt) and nothing else changes."""
    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "bf16")
    model, x, graph = _build()
    n_mesh = graph["hidden"].num_nodes
    monkeypatch.setenv("ANEMOI_AMD_ENC_HOIST", "0")
    y_off, names_off = _forward(model, x, record=True)
    y_off2, names_off2 = _forward(model, x, record=True)
    monkeypatch.setenv("ANEMOI_AMD_ENC_HOIST", "1")
    y1, names1 = _forward(model, x, record=True)
    y2, names2 = _forward(model, x, record=True)
    y3, names3 = _forward(model, x, record=True)
    assert torch.equal(y_off, y_off2) and torch.equal(y1, y_off) and torch.equal(y2, y_off) and torch.equal(y3, y_off)
    assert names_off == names_off2 == names1, "the filling forward launches what the switch-off forward launches"
    assert names2 == names3 and len(names2) < len(names1)
    gone = list(names1)
    for rec in names2:
        gone.remove(rec)  # (raises if the hoisted forward launched anything the full one did not)
    print(f"launches: {len(names1)} recomputing, {len(names2)} hoisted; gone: {gone}")
    linear_gone = [r for r in gone if r[0] == "linear"]
    assert len(linear_gone) == 3 and all(r[1] == n_mesh for r in linear_gone)  # embedding, x_r | q | u, qt: mesh rows only
    assert {r[0] for r in gone} <= {"linear", "assemble_nodes", "row_stats"}


@pytest.mark.parametrize("what", ["lin_query", "hidden_trainable"])
def test_a_changed_parameter_rebuilds(monkeypatch, what):
    """After an in-place update of a parameter that enters the hoisted side, the output changes and equals that of a model
    built with the changed parameter (a fresh model, fresh caches, same state)."""
    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "bf16")
    monkeypatch.setenv("ANEMOI_AMD_ENC_HOIST", "1")
    model, x, _ = _build()
    y_before, _ = _forward(model, x)
    _forward(model, x)
    with torch.no_grad():
        if what == "lin_query":
            model.encoder.proc.lin_query.weight.mul_(1.5)
        else:
            model.node_attributes.trainable_tensors[model._graph_name_hidden].trainable.mul_(-2.0)
    y_after, _ = _forward(model, x)
    y_after2, _ = _forward(model, x)
    fresh, _, _ = _build()
    fresh.load_state_dict(model.state_dict())
    y_fresh, _ = _forward(fresh, x)
    monkeypatch.setenv("ANEMOI_AMD_ENC_HOIST", "0")
    y_plain, _ = _forward(model, x)
    assert not torch.equal(y_after, y_before), "the parameter does not reach the output: the test shows nothing"
    assert torch.equal(y_after, y_after2) and torch.equal(y_after, y_fresh) and torch.equal(y_after, y_plain)


def test_load_state_dict_rebuilds_and_training_is_untouched(monkeypatch):
    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "bf16")
    monkeypatch.setenv("ANEMOI_AMD_ENC_HOIST", "1")
    model, x, _ = _build()
    _forward(model, x)
    other, _, _ = _build()
    with torch.no_grad():
        for p in other.parameters():
            p.mul_(1.25)
    model.load_state_dict(other.state_dict())
    y_loaded, _ = _forward(model, x)
    y_other, _ = _forward(other, x)
    assert torch.equal(y_loaded, y_other)
    # a training forward (autograd route) neither reads nor fills the cache
    monkeypatch.delenv("ANEMOI_AMD_DTYPE")
    trainee, _, _ = _build()
    trainee.train()
    y_train = trainee(x)
    assert y_train.requires_grad and trainee._hoisted._store == {}
    assert not any(k[0] == "hoist" for k in trainee.encoder._packed._store)
    assert not any(k[0] == "hoist" for k in trainee.encoder.proc._packed._store)
    monkeypatch.setenv("ANEMOI_AMD_ENC_HOIST", "0")
    again, _, _ = _build()
    again.train()
    assert torch.equal(again(x).detach(), y_train.detach())


def test_graphed_forward_captures_the_hoisted_path(monkeypatch):
    """``runtime.GraphedForward``: its warm-up forwards fill the cache outside the capture, the captured graph replays the
    hoisted forward, and its result is the eager one, bit for bit, also for a second input."""
    from anemoi_models_amd import runtime

    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "bf16")
    monkeypatch.setenv("ANEMOI_AMD_ENC_HOIST", "1")
    model, x, _ = _build()
    graphed = runtime.GraphedForward(model, x)
    kept = {k: v[1][1] for k, v in model.encoder.proc._packed._store.items() if k[0] == "hoist"}
    assert len(model._hoisted._store) == 1 and len(kept) == 1, "the warm-up did not fill the cache"
    y_eager, _ = _forward(model, x)
    assert torch.equal(graphed(x), y_eager)
    x2 = x * 0.5 + 0.25
    y2_eager, _ = _forward(model, x2)
    assert torch.equal(graphed(x2), y2_eager)
    after = {k: v[1][1] for k, v in model.encoder.proc._packed._store.items() if k[0] == "hoist"}
    assert all(after[k][0] is kept[k][0] for k in kept), "a replay or an eager forward rebuilt what was hoisted"
