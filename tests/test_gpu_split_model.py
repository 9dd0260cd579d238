"""``ANEMOI_AMD_F32_LINEAR=bf16x3`` at model level on the MI355X (``-m gpu``): the f32 inference route with its Linears on
the split-bf16 kernel.  Error against the exact f32 route (which tests/test_gpu_baseline_sizes.py pins to the CPU oracle) and
against the CPU oracle itself, with the oracle on split-bf16 Linears (tests/_split_ref.py) as the yardstick; launch coverage
by profile for the three processor families; and the switch's hygiene: off restores the exact route bit for bit, bf16 and
training ignore it, weight updates are picked up, a captured graph replays it."""

import numpy as np
import pytest
import torch

from _split_ref import Bf16x3Linears
from oracle import reference_path as ref
from test_oracle_golden import graph_tensors

pytestmark = pytest.mark.gpu

DEV = "cuda"
PARITY = 1e-3  # the project's parity target against fp32 (README / SURVEY)
N_PROG = 20


def _model(processor, channels, layers, graph_name, mappers="GraphTransformer", seed=1234):
    from anemoi_models_amd.graphs.synthetic import build_graph
    from anemoi_models_amd.models import AnemoiModelEncProcDec
    from anemoi_models_amd.utils.indices import SimpleDataIndices
    from anemoi_models_amd.utils.presets import model_config

    graph = build_graph(graph_name)
    idx = SimpleDataIndices(n_prognostic=N_PROG, n_forcing=4, n_diagnostic=2)
    torch.manual_seed(seed)
    model = AnemoiModelEncProcDec(model_config=model_config(processor, channels, layers, 16, mappers=mappers),
                                  data_indices=idx, graph_data=graph)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("trainable"):
                p.normal_(0.0, 0.1)
    x = torch.randn(1, 2, 1, graph["data"].num_nodes, idx.num_input, generator=torch.Generator().manual_seed(7))
    return model.eval(), x, graph


def _oracles(model, x, graph, layers, processor="GraphTransformer"):
    """``(f32 oracle, oracle with every F.linear as the split-bf16 product)`` on the CPU, from the model's own weights."""
    sd = {k: v.detach().clone().cpu() for k, v in model.state_dict().items()}
    kw = dict(num_heads=16, num_layers=layers, num_chunks=2, prognostic_in=range(N_PROG), prognostic_out=range(N_PROG),
              processor=processor)
    gt = graph_tensors(graph)
    with torch.no_grad():
        want = ref.model_forward(sd, gt, x.cpu(), **kw)
        with Bf16x3Linears():
            emu = ref.model_forward(sd, gt, x.cpu(), **kw)
    return want, emu


@pytest.fixture(scope="module")
def cfg2():
    model, x, graph = _model("GraphTransformer", 512, 16, "o96_ico5")  # the seeds of test_gpu_baseline_sizes._make
    want, emu = _oracles(model, x, graph, 16)
    return model.to(DEV), x.to(DEV), want, emu


@pytest.fixture(scope="module")
def small():
    model, x, graph = _model("GraphTransformer", 128, 8, "o32_ico2")
    want, emu = _oracles(model, x, graph, 8)
    return model.to(DEV), x.to(DEV), want, emu


def _run(model, x, monkeypatch, dtype, mode):
    monkeypatch.setenv("ANEMOI_AMD_DTYPE", dtype)
    if mode is None:
        monkeypatch.delenv("ANEMOI_AMD_F32_LINEAR", raising=False)
    else:
        monkeypatch.setenv("ANEMOI_AMD_F32_LINEAR", mode)
    with torch.no_grad():
        return model(x).float()


def _errors(got, want):
    got, want = got.float().cpu(), want.float().cpu()
    err = float((got - want).abs().max() / want.abs().max())
    num = (got - want).abs().flatten(0, -2).max(dim=0).values
    den = want.abs().flatten(0, -2).max(dim=0).values.clamp_min(1e-30)
    return err, float((num / den).max())


def test_config2_bf16x3_against_the_exact_f32_route(cfg2, monkeypatch):
    """Measured on the MI355X (profiles/r08_bf16x3.md): see the printed line."""
    model, x, _, _ = cfg2
    exact = _run(model, x, monkeypatch, "fp32", None)
    split = _run(model, x, monkeypatch, "fp32", "bf16x3")
    bf16 = _run(model, x, monkeypatch, "bf16", None)
    e_split, v_split = _errors(split, exact)
    e_bf16, v_bf16 = _errors(bf16, exact)
    print(f"config 2 vs the exact f32 route: bf16x3 max rel {e_split:.3e} / per variable {v_split:.3e}; "
          f"bf16 {e_bf16:.3e} / {v_bf16:.3e}; ratio {e_bf16 / max(e_split, 1e-30):.0f} / {v_bf16 / max(v_split, 1e-30):.0f}")
    assert not torch.equal(split, exact), "the switch changed nothing"
    assert e_split <= PARITY and v_split <= PARITY
    assert e_split <= e_bf16 / 20 and v_split <= v_bf16 / 20


def _against_oracle(fixture, monkeypatch, label):
    model, x, want, emu = fixture
    e_ref, v_ref = _errors(emu, want)
    e_exact, v_exact = _errors(_run(model, x, monkeypatch, "fp32", None), want)
    e_split, v_split = _errors(_run(model, x, monkeypatch, "fp32", "bf16x3"), want)
    print(f"{label} vs the f32 CPU oracle: device bf16x3 {e_split:.3e} / per variable {v_split:.3e}; oracle on split-bf16 "
          f"Linears {e_ref:.3e} / {v_ref:.3e}; device exact f32 {e_exact:.3e} / {v_exact:.3e}")
    assert e_split <= 2 * e_ref + e_exact and v_split <= 2 * v_ref + v_exact


def test_o32_bf16x3_against_the_oracle_on_split_linears(small, monkeypatch):
    _against_oracle(small, monkeypatch, "o32_ico2, 128 ch, 8 blocks")


def test_config2_bf16x3_against_the_oracle_on_split_linears(cfg2, monkeypatch):
    _against_oracle(cfg2, monkeypatch, "config 2")


def _profile(fn):
    from anemoi_models_amd import ops

    ops.PROFILE = []
    try:
        fn()
        return [(r[0], r[3]) for r in ops.PROFILE]
    finally:
        ops.PROFILE = None


def _check_coverage(run, monkeypatch):
    from anemoi_models_amd.runtime import split_route

    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "fp32")
    monkeypatch.delenv("ANEMOI_AMD_F32_LINEAR", raising=False)
    run()
    exact = _profile(run)
    monkeypatch.setenv("ANEMOI_AMD_F32_LINEAR", "bf16x3")
    run()  # planes made outside the profiled pass
    split = _profile(run)
    n_exact = sum(name == "linear" for name, _ in exact)
    assert n_exact > 0 and not any(name == "linear_split" for name, _ in exact)
    assert sum(name in ("linear", "linear_split") for name, _ in split) == n_exact
    assert not any(name == "split_weight" for name, _ in split), "planes rebuilt in a steady-state forward"
    shapes = lambda recs, which: [(w["m"], w["n"], w["k"]) for name, w in recs if name == which]  # noqa: E731
    assert sorted(shapes(split, "linear") + shapes(split, "linear_split")) == sorted(shapes(exact, "linear"))
    for m, n, k in shapes(split, "linear"):
        assert not split_route(m, n, k), f"[{m}, {k}] x [{n}, {k}] stayed on the exact kernel although the rule admits it"
    for m, n, k in shapes(split, "linear_split"):
        assert split_route(m, n, k)
    return split


@pytest.mark.parametrize("processor", ["GraphTransformer", "GNN", "Transformer"])
def test_profile_coverage_of_the_three_processor_families(processor, monkeypatch):
    model, x, _ = _model(processor, 128, 4, "o32_ico2", mappers="GNN" if processor == "GNN" else "GraphTransformer")
    model, x = model.to(DEV), x.to(DEV)

    def run():
        with torch.no_grad():
            model(x)

    split = _check_coverage(run, monkeypatch)
    routed = {(w["n"], w["k"]) for name, w in split if name == "linear_split"}
    assert (128, 128) in routed or any(n > 128 and k == 128 for n, k in routed)
    assert (512, 128) in routed or processor == "GNN"  # C -> hidden of the GraphTransformer / Transformer node MLPs
    assert any(n == 128 and k >= 128 for n, k in routed)  # hidden (or concatenated features) -> C


def test_profile_coverage_of_predict_step(monkeypatch):
    from anemoi_models_amd.graphs.synthetic import build_graph
    from anemoi_models_amd.interface import AnemoiModelInterface
    from anemoi_models_amd.utils.indices import SimpleDataIndices
    from anemoi_models_amd.utils.presets import model_config

    graph = build_graph("o32_ico2")
    n_prog, n_forc, n_diag = 10, 2, 1
    n_all = n_prog + n_forc + n_diag
    cfg = model_config("GraphTransformer", 128, 4, 16)
    cfg["data"] = {"forcing": [f"forc_{i}" for i in range(n_forc)], "diagnostic": ["diag_0"],
                   "processors": {"normalizer": {"_target_": "anemoi.models.preprocessing.normalizer.InputNormalizer",
                                                 "config": {"default": "mean-std"}}}}
    cfg["model"]["model"] = {"_target_": "anemoi.models.models.encoder_processor_decoder.AnemoiModelEncProcDec"}
    gen = torch.Generator().manual_seed(11)
    mean = (torch.randn(n_all, generator=gen) * 3.0).numpy().astype(np.float32)
    stdev = (0.5 + torch.rand(n_all, generator=gen) * 2.0).numpy().astype(np.float32)
    stats = {"mean": mean, "stdev": stdev, "minimum": mean - 3.0 * stdev, "maximum": mean + 3.5 * stdev}
    idx = SimpleDataIndices(n_prognostic=n_prog, n_forcing=n_forc, n_diagnostic=n_diag)
    torch.manual_seed(1234)
    iface = AnemoiModelInterface(config=type(cfg)(cfg), graph_data=graph, statistics=stats, data_indices=idx,
                                 metadata={}).eval().to(DEV)
    batch = torch.randn((1, 2, graph["data"].num_nodes, n_prog + n_forc), generator=torch.Generator().manual_seed(7)).to(DEV)
    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "fp32")
    monkeypatch.delenv("ANEMOI_AMD_F32_LINEAR", raising=False)
    exact = iface.predict_step(batch)
    _check_coverage(lambda: iface.predict_step(batch), monkeypatch)
    got = iface.predict_step(batch)
    assert not torch.equal(got, exact) and _errors(got, exact)[0] <= PARITY


def test_switch_off_and_bf16_are_bit_identical_to_never_having_seen_it(small, monkeypatch):
    model, x, _, _ = small
    exact = _run(model, x, monkeypatch, "fp32", None)
    bf16 = _run(model, x, monkeypatch, "bf16", None)
    on = _run(model, x, monkeypatch, "fp32", "bf16x3")
    assert not torch.equal(on, exact)
    assert torch.equal(_run(model, x, monkeypatch, "fp32", "bf16x3"), on)
    assert torch.equal(_run(model, x, monkeypatch, "fp32", "exact"), exact)
    assert torch.equal(_run(model, x, monkeypatch, "fp32", None), exact)
    assert torch.equal(_run(model, x, monkeypatch, "bf16", "bf16x3"), bf16)
    with pytest.raises(ValueError, match="ANEMOI_AMD_F32_LINEAR"):
        _run(model, x, monkeypatch, "fp32", "tf32")


def test_f32_training_step_is_bit_identical_with_the_switch(monkeypatch):
    model, x, _ = _model("GraphTransformer", 128, 2, "o32_ico2")
    model, x = model.to(DEV), x.to(DEV)
    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "fp32")
    steps = []
    for mode in ("exact", "bf16x3"):
        monkeypatch.setenv("ANEMOI_AMD_F32_LINEAR", mode)
        model.zero_grad(set_to_none=True)
        loss = model(x).float().square().mean()
        loss.backward()
        steps.append((loss.detach(), [p.grad.clone() for p in model.parameters() if p.grad is not None]))
    (l0, g0), (l1, g1) = steps
    assert torch.equal(l0, l1) and len(g0) == len(g1) and len(g0) > 0
    assert all(torch.equal(a, b) for a, b in zip(g0, g1))


def test_in_place_weight_update_is_picked_up(monkeypatch):
    model, x, _ = _model("GraphTransformer", 128, 4, "o32_ico2")
    fresh, _, _ = _model("GraphTransformer", 128, 4, "o32_ico2")  # the same seeded weights, never split before the update
    model, fresh, x = model.to(DEV), fresh.to(DEV), x.to(DEV)
    before = _run(model, x, monkeypatch, "fp32", "bf16x3")
    with torch.no_grad():
        model.processor.proc[0].blocks[0].node_dst_mlp[1].weight.mul_(0.5)
        fresh.processor.proc[0].blocks[0].node_dst_mlp[1].weight.mul_(0.5)
    after = _run(model, x, monkeypatch, "fp32", "bf16x3")
    want = _run(fresh, x, monkeypatch, "fp32", "bf16x3")
    assert not torch.equal(after, before)
    assert torch.equal(after, want)


def test_graphed_forward_replays_the_route(small, monkeypatch):
    from anemoi_models_amd.runtime import GraphedForward

    model, x, _, _ = small
    eager = _run(model, x, monkeypatch, "fp32", "bf16x3")
    graphed = GraphedForward(model, torch.zeros_like(x))
    with torch.no_grad():
        got = graphed(x).float()
    assert torch.equal(got, eager)
    assert not torch.equal(got, _run(model, x, monkeypatch, "fp32", None))
