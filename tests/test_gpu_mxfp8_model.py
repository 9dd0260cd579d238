"""``ANEMOI_AMD_MXFP8=1`` at model level on the MI355X (``-m gpu``): config 2 (O96 -> ico-5, 16 GraphTransformer blocks,
512 channels) with the switch on against the exact-f32 route, which tests/test_gpu_baseline_sizes.py pins to the CPU oracle
within 1e-3.  The switch's limits: f32 and training ignore it, the node-partitioned forward and widths that are not a
multiple of 128 refuse it, and turning it off restores the bf16 route bit for bit."""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
# The bench's bf16 parity bound is 1e-2.  The MXFP8 route does not meet it with any covered set (profiles/r07_mxfp8.md
# section 5), which is why it stays an experimental opt-in; these bounds hold the error measured with the default set on
# this model (max-rel 1.18e-2, per-variable max 1.99e-2) so that a regression shows.
BOUND, BOUND_PER_VARIABLE = 1.6e-2, 2.5e-2


def _model(channels, layers, graph_name, n_prog=20, seed=1234):
    from anemoi_models_amd.graphs.synthetic import build_graph
    from anemoi_models_amd.models import AnemoiModelEncProcDec
    from anemoi_models_amd.utils.indices import SimpleDataIndices
    from anemoi_models_amd.utils.presets import model_config

    graph = build_graph(graph_name)
    idx = SimpleDataIndices(n_prognostic=n_prog, n_forcing=4, n_diagnostic=2)
    torch.manual_seed(seed)
    model = AnemoiModelEncProcDec(model_config=model_config("GraphTransformer", channels, layers, 16), data_indices=idx,
                                  graph_data=graph)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("trainable"):
                p.normal_(0.0, 0.1)
    x = torch.randn(1, 2, 1, graph["data"].num_nodes, idx.num_input, generator=torch.Generator().manual_seed(7))
    return model.to(DEV).eval(), x.to(DEV)


@pytest.fixture(scope="module")
def cfg2():
    model, x = _model(512, 16, "o96_ico5")
    return model, x


def _run(model, x, monkeypatch, dtype, mx):
    monkeypatch.setenv("ANEMOI_AMD_DTYPE", dtype)
    if mx is None:
        monkeypatch.delenv("ANEMOI_AMD_MXFP8", raising=False)
    else:
        monkeypatch.setenv("ANEMOI_AMD_MXFP8", mx)
    with torch.no_grad():
        return model(x).float()


def _errors(got, want):
    got, want = got.cpu(), want.cpu()
    err = float((got - want).abs().max() / want.abs().max())
    num = (got - want).abs().flatten(0, -2).max(dim=0).values
    den = want.abs().flatten(0, -2).max(dim=0).values.clamp_min(1e-30)
    return err, num / den


def test_config2_mxfp8_error_repeat_and_switch_off(cfg2, monkeypatch):
    model, x = cfg2
    plain = _run(model, x, monkeypatch, "bf16", None)  # never saw the switch
    want = _run(model, x, monkeypatch, "fp32", None)
    got = _run(model, x, monkeypatch, "bf16", "1")
    again = _run(model, x, monkeypatch, "bf16", "1")
    off = _run(model, x, monkeypatch, "bf16", "0")
    err, per_var = _errors(got, want)
    err_bf16, _ = _errors(plain, want)
    msg = (f"config 2 with MXFP8: max rel {err:.3e} (bf16 route {err_bf16:.3e}); per-variable max {float(per_var.max()):.3e}, "
           f"per variable {[round(float(v), 5) for v in per_var]}")
    print(msg)
    assert err <= BOUND and float(per_var.max()) <= BOUND_PER_VARIABLE, msg
    assert not torch.equal(got, plain), "the switch changed nothing"
    assert torch.equal(got, again), "two MXFP8 runs differ"
    assert torch.equal(off, plain), "switching MXFP8 off did not restore the bf16 route bit for bit"


def test_config2_mxfp8_profile_covers_exactly_the_covered_linears(cfg2, monkeypatch):
    from anemoi_models_amd import ops
    from anemoi_models_amd.layers.block import GraphTransformerMapperBlock
    from anemoi_models_amd.layers.block import GraphTransformerProcessorBlock

    model, x = cfg2
    _run(model, x, monkeypatch, "bf16", "1")  # weights quantised outside the profiled pass
    ops.PROFILE = []
    try:
        _run(model, x, monkeypatch, "bf16", "1")
        names = [r[0] for r in ops.PROFILE]
    finally:
        ops.PROFILE = None
    n_proc = sum(isinstance(m, GraphTransformerProcessorBlock) for m in model.modules())
    n_map = sum(isinstance(m, GraphTransformerMapperBlock) for m in model.modules())
    n_map_mx = sum(isinstance(m, GraphTransformerMapperBlock) and m.mx_node_mlp for m in model.modules())
    assert n_proc == 16 and n_map == 2 and n_map_mx == 1  # the encoder's node MLP; the decoder's stays bf16
    assert not GraphTransformerProcessorBlock.mx_sqkvu
    # per processor block: projection, fc1, fc2 (x_r | q | k | v | u stays on the bf16 fold); per covered mapper: fc1, fc2
    assert names.count("linear_mx") == 3 * n_proc + 2 * n_map_mx
    assert names.count("mx_quantize") == 2 * n_proc + n_map_mx  # [out | t] and LayerNorm + y; the mapper's LayerNorm + y


def test_config2_mxfp8_wider_covered_set(cfg2, monkeypatch):
    """The x_r | q | k | v | u product on MXFP8 too (``mx_sqkvu``): one more launch per block, deterministic, and further
    from f32 than the default set (measured 1.1e-2 -> 1.7e-2 at config 2)."""
    from anemoi_models_amd import ops
    from anemoi_models_amd.layers.block import GraphTransformerProcessorBlock

    model, x = cfg2
    want = _run(model, x, monkeypatch, "fp32", None)
    procs = [m for m in model.modules() if isinstance(m, GraphTransformerProcessorBlock)]
    for b in procs:
        b.mx_sqkvu = True
    try:
        got = _run(model, x, monkeypatch, "bf16", "1")
        ops.PROFILE = []
        try:
            again = _run(model, x, monkeypatch, "bf16", "1")
            names = [r[0] for r in ops.PROFILE]
        finally:
            ops.PROFILE = None
    finally:
        for b in procs:
            del b.mx_sqkvu
    err, per_var = _errors(got, want)
    print(f"config 2 with MXFP8 incl. x_r|q|k|v|u: max rel {err:.3e}, per-variable max {float(per_var.max()):.3e}")
    assert torch.equal(got, again)
    assert names.count("linear_mx") == 4 * len(procs) + 2 and names.count("mx_quantize") == 3 * len(procs) + 1
    assert err <= 2.5e-2


def test_config2_mxfp8_graphed_forward_equals_eager(cfg2, monkeypatch):
    from anemoi_models_amd.runtime import GraphedForward

    model, x = cfg2
    eager = _run(model, x, monkeypatch, "bf16", "1")
    graphed = GraphedForward(model, torch.zeros_like(x))
    with torch.no_grad():
        got = graphed(x).float()
    assert torch.equal(got, eager)


def test_mxfp8_in_place_weight_update_is_picked_up(cfg2, monkeypatch):
    model, x = cfg2
    before = _run(model, x, monkeypatch, "bf16", "1")
    fc1 = model.processor.proc[0].blocks[0].node_dst_mlp[1]
    fresh, _ = _model(512, 16, "o96_ico5")  # the same seeded weights, never quantised before the update
    with torch.no_grad():
        fc1.weight.mul_(0.5)
        fresh.processor.proc[0].blocks[0].node_dst_mlp[1].weight.mul_(0.5)
    try:
        after = _run(model, x, monkeypatch, "bf16", "1")
        want = _run(fresh, x, monkeypatch, "bf16", "1")
    finally:
        with torch.no_grad():
            fc1.weight.mul_(2.0)  # exact: the module-scoped model is shared
    assert not torch.equal(after, before)
    assert torch.equal(after, want)


def test_mxfp8_is_ignored_by_the_f32_route(monkeypatch):
    model, x = _model(64, 4, "o32_ico2", n_prog=10)
    assert torch.equal(_run(model, x, monkeypatch, "fp32", "1"), _run(model, x, monkeypatch, "fp32", None))


def test_mxfp8_refuses_widths_off_128(monkeypatch):
    model, x = _model(64, 4, "o32_ico2", n_prog=10)
    with pytest.raises(NotImplementedError, match="64"):
        _run(model, x, monkeypatch, "bf16", "1")


def test_mxfp8_refuses_the_node_partitioned_forward(cfg2, monkeypatch):
    from anemoi_models_amd.layers.block import GraphTransformerProcessorBlock

    model, _ = cfg2
    blk = next(m for m in model.modules() if isinstance(m, GraphTransformerProcessorBlock))
    monkeypatch.setenv("ANEMOI_AMD_MXFP8", "1")
    x = torch.zeros(8, 512, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(NotImplementedError, match="node-partitioned"):
        blk.native(x, None, None, halo=object())


def test_mxfp8_training_step_unchanged(monkeypatch):
    """Autograd never reaches the native blocks: a bf16 training step's loss and gradients are identical with the switch."""
    model, x = _model(512, 2, "o32_ico2", n_prog=10)  # eval(): no dropout, so the two steps can be compared bit for bit
    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "bf16")
    grads = []
    for mx in ("0", "1"):
        monkeypatch.setenv("ANEMOI_AMD_MXFP8", mx)
        model.zero_grad(set_to_none=True)
        loss = model(x).float().square().mean()
        loss.backward()
        grads.append((loss.detach(), [p.grad.clone() for p in model.parameters() if p.grad is not None]))
    (l0, g0), (l1, g1) = grads
    assert torch.equal(l0, l1) and len(g0) == len(g1) and len(g0) > 0
    assert all(torch.equal(a, b) for a, b in zip(g0, g1))
