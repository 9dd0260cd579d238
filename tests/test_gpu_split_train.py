"""``ANEMOI_AMD_F32_TRAIN_LINEAR=bf16x3`` at model level on the MI355X (``-m gpu``): an f32 training step with its Linear
products (forward, dX, dW) on the split-bf16 kernels.  Gradient accuracy against the f64 CPU oracle under torch autograd,
bounded by the two routes that exist without the switch (exact f32 and bf16); launch coverage by profile for the three
processor families; and the switch's hygiene: unset / exact / bf16 are bit-identical to never having seen it, weight updates
are picked up, both switches together, and a captured training step replays the route."""

import math

import pytest
import torch

from oracle import reference_path as ref
from test_gpu_split_model import N_PROG
from test_gpu_split_model import _model
from test_oracle_golden import graph_tensors

pytestmark = pytest.mark.gpu

DEV = "cuda"
SWITCH = "ANEMOI_AMD_F32_TRAIN_LINEAR"


def _step(model, x, dy, monkeypatch, dtype="fp32", mode=None, infer_mode=None):
    """One training step ``loss = sum(y * dy)``: ``(y, loss, {name: grad})`` on the CPU."""
    monkeypatch.setenv("ANEMOI_AMD_DTYPE", dtype)
    for var, val in ((SWITCH, mode), ("ANEMOI_AMD_F32_LINEAR", infer_mode)):
        if val is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, val)
    model.zero_grad(set_to_none=True)
    y = model(x).float()
    loss = (y * dy).sum()
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    return y.detach(), loss.detach(), grads


def _oracle_step(model, x, graph, layers, processor, dy, n_prog=N_PROG):
    sd = {k: v.detach().clone().cpu() for k, v in model.state_dict().items()}
    rsd = {k: (v.double().requires_grad_() if v.is_floating_point() else v) for k, v in sd.items()}
    gt = {k: (v.double() if v.is_floating_point() else v) for k, v in graph_tensors(graph).items()}
    y = ref.model_forward(rsd, gt, x.cpu().double(), num_heads=16, num_layers=layers, num_chunks=2,
                          prognostic_in=range(n_prog), prognostic_out=range(n_prog), processor=processor)
    loss = (y * dy.cpu().double()).sum()
    loss.backward()
    return y.detach(), loss.detach(), {k: v.grad for k, v in rsd.items() if v.is_floating_point() and v.grad is not None}


def _err(got, want):
    return float((got.cpu().double() - want).abs().max() / want.abs().max())


def _accuracy(label, model, x, graph, layers, processor, dy, monkeypatch, n_prog=N_PROG, assert_loss=True):
    y_o, l_o, g_o = _oracle_step(model, x, graph, layers, processor, dy, n_prog)
    model, x, dy = model.to(DEV), x.to(DEV), dy.to(DEV)
    runs = {"exact": _step(model, x, dy, monkeypatch, "fp32", None), "split": _step(model, x, dy, monkeypatch, "fp32", "bf16x3"),
            "bf16": _step(model, x, dy, monkeypatch, "bf16", None)}
    names = [k for k, _ in model.named_parameters()]
    compared = [k for k in names if k in g_o and float(g_o[k].abs().max()) > 0]
    print(f"{label}: {len(compared)} of {len(names)} parameters compared")
    assert len(compared) >= 0.9 * len(names)
    rows = [("output", *(_err(runs[r][0], y_o) for r in ("exact", "split", "bf16"))),
            ("loss", *(abs(float(runs[r][1]) - float(l_o)) / abs(float(l_o)) for r in ("exact", "split", "bf16")))]
    for k in compared:
        assert all(k in runs[r][2] for r in runs), k
        rows.append((k, *(_err(runs[r][2][k], g_o[k]) for r in ("exact", "split", "bf16"))))
    worst, failed = max(rows[2:], key=lambda r: r[2] / math.sqrt(r[1] * r[3])), []
    for name, e_exact, e_split, e_bf16 in rows:
        bound = math.sqrt(e_exact * e_bf16)
        print(f"  {name}: exact {e_exact:.3e}  bf16x3 {e_split:.3e}  bf16 {e_bf16:.3e}  bound {bound:.3e}")
        if not e_split <= bound and (assert_loss or name != "loss"):
            failed.append(name)
    print(f"  worst gradient against its bound: {worst[0]} exact {worst[1]:.3e} bf16x3 {worst[2]:.3e} bf16 {worst[3]:.3e}; "
          f"largest bf16x3 gradient error {max(r[2] for r in rows[2:]):.3e}")
    assert not failed, failed


def _preset(processor, channels, layers, graph_name, monkeypatch, assert_loss=True):
    model, x, graph = _model(processor, channels, layers, graph_name)
    dy = torch.randn(model_out_shape(model, x), generator=torch.Generator().manual_seed(2))
    _accuracy(f"{processor} {graph_name} {channels} ch {layers} blocks", model, x, graph, layers, processor, dy, monkeypatch,
              assert_loss=assert_loss)


def model_out_shape(model, x):
    return (x.shape[0], x.shape[2], x.shape[3], N_PROG + 2)


def test_the_golden_training_step_against_the_f64_oracle_between_exact_and_bf16(golden_cfg1_gt, graph_o32, monkeypatch):
    """The step of ``test_gpu_parity.test_whole_model_training_step_vs_oracle_autograd`` -- the golden config-1 weights
    (GraphTransformer, O32 -> ico-2, 4 blocks, 64 channels), the golden batch, ``dy = randn(seed 2)`` as the output gradient,
    i.e. the loss ``sum(y * dy)`` -- with the switch on: ``e_split(p) <= sqrt(e_exact(p) * e_bf16(p))`` for the output, the
    loss and every parameter whose oracle gradient is not identically zero (at least 90 % of them), all three errors against
    the f64 oracle under torch autograd and normalised by ``max |g_oracle|``.  The bound comes from the two routes that
    exist without the switch; a dropped correction product in any of the three GEMMs lands at the bf16 level.
    Measured: profiles/r10_bf16x3_train.md."""
    from conftest import split_prefix
    from test_gpu_parity import _build

    gold = golden_cfg1_gt
    model, _ = _build(graph_o32, 64, 4)
    model.load_state_dict(split_prefix(gold, "sd."))
    dy = torch.randn(gold["y"].shape, generator=torch.Generator().manual_seed(2))
    _accuracy("golden config 1 (GraphTransformer O32, 64 ch, 4 blocks)", model.eval(), gold["x"], graph_o32, 4,
              "GraphTransformer", dy, monkeypatch, n_prog=10)


@pytest.mark.parametrize("processor", ["GNN", "Transformer"])
def test_o32_gradients_against_the_f64_oracle_between_exact_and_bf16(processor, monkeypatch):
    """The same rule for the other two processor families on the O32 preset of tests/test_gpu_split_model.py (128 channels,
    4 blocks, seeded weights).  Measured (profiles/r10_bf16x3_train.md), exact / bf16x3 / bf16: output 3.0e-7 / 4.6e-6 /
    3.3e-3 (GNN), 2.8e-7 / 4.4e-6 / 3.1e-3 (Transformer); worst gradient 3.1e-7 / 2.3e-5 / 8.3e-3, 3.9e-7 / 2.0e-5 / 9.4e-3.
    The GraphTransformer family is the golden step above (the step the rule is stated for) and, on this preset, the test
    below."""
    _preset(processor, 128, 4, "o32_ico2", monkeypatch)


def test_o32_preset_graph_transformer_output_and_gradients(monkeypatch):
    """The GraphTransformer on the same 128-channel preset: output and every gradient under the same rule; the LOSS is
    printed, not asserted.  ``sqrt(e_exact * e_bf16)`` of a single scalar is only as good as that one sample of ``e_exact``:
    here the exact route's ``sum(y * dy)`` lands at 7.6e-10 of the oracle's -- 80 x below one f32 rounding, the rounding
    errors of its 115 456 terms cancel for this seed -- which puts the bound (8.9e-7) under a bf16x3 loss error (1.49e-6) that
    is itself below the bf16x3 output error (4.2e-6) and below the loss errors the other cases pass with.  The loss IS asserted
    on the golden step, the GNN, the Transformer and the config-2-size model, where ``e_exact(loss)`` is 4e-8 ... 3e-6."""
    _preset("GraphTransformer", 128, 4, "o32_ico2", monkeypatch, assert_loss=False)


def test_config2_gradients_against_the_f64_oracle_between_exact_and_bf16(monkeypatch):
    """The same at config 2's size (O96 -> ico-5, 512 channels, 16 blocks)."""
    _preset("GraphTransformer", 512, 16, "o96_ico5", monkeypatch)


def _profiled_step(model, x, dy, monkeypatch, mode):
    """``(PROFILE records, f32 calls of the exact ops.weight_grad as (m, n, k, x columns))`` of one f32 training step."""
    from anemoi_models_amd import ops

    calls, real = [], ops.weight_grad

    def spy(dpre, xx, k, *a, **kw):
        if dpre.dtype == torch.float32:
            calls.append((dpre.shape[0], dpre.shape[1], k, xx.shape[1]))
        return real(dpre, xx, k, *a, **kw)

    _step(model, x, dy, monkeypatch, "fp32", mode)  # plans and planes made outside the profiled pass
    monkeypatch.setattr(ops, "weight_grad", spy)
    ops.PROFILE = []
    try:
        _step(model, x, dy, monkeypatch, "fp32", mode)
        return [(r[0], r[3]) for r in ops.PROFILE], calls
    finally:
        ops.PROFILE = None
        monkeypatch.setattr(ops, "weight_grad", real)


@pytest.mark.parametrize("processor", ["GraphTransformer", "GNN", "Transformer"])
def test_profile_coverage_of_a_training_step(processor, monkeypatch):
    """Every Linear-type product of the exact step has its counterpart in the split step: forward and dX on ``linear_split``
    and dW on ``weight_grad_split`` for every shape the routing rules admit, the exact kernels only for the rest."""
    from anemoi_models_amd import ops
    from anemoi_models_amd.runtime import split_grad_route, train_split_route

    model, x, _ = _model(processor, 128, 4, "o32_ico2", mappers="GNN" if processor == "GNN" else "GraphTransformer")
    model, x = model.to(DEV), x.to(DEV)
    dy = torch.randn(model_out_shape(model, x), generator=torch.Generator().manual_seed(2)).to(DEV)
    exact, wg_exact = _profiled_step(model, x, dy, monkeypatch, None)
    split, wg_split = _profiled_step(model, x, dy, monkeypatch, "bf16x3")
    shapes = lambda recs, which: sorted((w["m"], w["n"], w["k"]) for name, w in recs if name == which)  # noqa: E731
    assert shapes(exact, "linear") and not shapes(exact, "linear_split") and not shapes(exact, "weight_grad_split")
    assert sorted(shapes(split, "linear") + shapes(split, "linear_split")) == shapes(exact, "linear")
    for m, n, k in shapes(split, "linear"):
        assert not train_split_route(m, n, k), f"[{m}, {k}] x [{n}, {k}] stayed on the exact kernel although the rule admits it"
    # "one linear_split and one weight_grad_split per Linear layer" follows from the equalities, not from a count of
    # nn.Linear modules (a GraphTransformer block runs its four input Linears and the folded lin_edge as ONE product, the GNN
    # splits one Linear into three): every product of the exact step -- forward, dX and dW of every layer -- reappears in the
    # split step (multiset equality above, count equality below), and whatever stayed on an exact kernel is a shape the
    # routing rules refuse.  The module count is a floor on top of that.
    n_lin = sum(isinstance(mod, torch.nn.Linear) for mod in model.modules())
    assert len(shapes(split, "linear_split")) >= n_lin // 2
    # dW: the exact route (transposes + anemoi_linear_batched) only where the rule refuses the shape
    assert len(wg_exact) > 0 and len(shapes(split, "weight_grad_split")) + len(wg_split) == len(wg_exact)
    assert len(shapes(split, "weight_grad_split")) > 0
    for m, n, k, cols in wg_split:
        k4 = ops.round_up(k, 4)
        assert k4 > cols or not split_grad_route(m, n, k4), f"dW [{n}, {k}] over {m} rows stayed on the exact route"
    # planes: weights the step assembles from parameters (torch.cat, column slices) are split per step, a parameter that did
    # not change is not split again -- two planes (W, W^T) per product at the most, none on the exact route
    assert sum(name == "split_weight" for name, _ in split) <= 2 * len(shapes(split, "linear_split"))
    assert not any(name == "split_weight" for name, _ in exact)


def _small(monkeypatch, layers=2):
    model, x, _ = _model("GraphTransformer", 128, layers, "o32_ico2")
    model, x = model.to(DEV), x.to(DEV)
    dy = torch.randn(model_out_shape(model, x), generator=torch.Generator().manual_seed(2)).to(DEV)
    return model, x, dy


def _same(a, b):
    return (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2].keys() == b[2].keys()
            and all(torch.equal(a[2][k], b[2][k]) for k in a[2]))


def test_unset_exact_and_bf16_are_bit_identical_to_never_having_seen_it(monkeypatch):
    model, x, dy = _small(monkeypatch)
    unset = _step(model, x, dy, monkeypatch, "fp32", None)
    on = _step(model, x, dy, monkeypatch, "fp32", "bf16x3")
    assert not _same(on, unset) and len(unset[2]) > 0
    assert _same(_step(model, x, dy, monkeypatch, "fp32", "bf16x3"), on)  # run to run
    assert _same(_step(model, x, dy, monkeypatch, "fp32", "exact"), unset)
    assert _same(_step(model, x, dy, monkeypatch, "fp32", None), unset)
    bf16 = _step(model, x, dy, monkeypatch, "bf16", None)
    assert _same(_step(model, x, dy, monkeypatch, "bf16", "bf16x3"), bf16)
    with pytest.raises(ValueError, match=SWITCH):
        _step(model, x, dy, monkeypatch, "fp32", "tf32")


def test_both_switches_training_takes_the_new_route_and_inference_the_old_one(monkeypatch):
    from anemoi_models_amd import ops

    model, x, dy = _small(monkeypatch)
    train_only = _step(model, x, dy, monkeypatch, "fp32", "bf16x3", None)
    ops.PROFILE = []
    try:
        both = _step(model, x, dy, monkeypatch, "fp32", "bf16x3", "bf16x3")
        names = {r[0] for r in ops.PROFILE}
    finally:
        ops.PROFILE = None
    assert _same(both, train_only) and {"linear_split", "weight_grad_split"} <= names
    monkeypatch.setenv(SWITCH, "exact")
    with torch.no_grad():
        infer_only = model(x).float()
    monkeypatch.setenv(SWITCH, "bf16x3")
    ops.PROFILE = []
    try:
        with torch.no_grad():
            got = model(x).float()
        names = {r[0] for r in ops.PROFILE}
    finally:
        ops.PROFILE = None
    assert torch.equal(got, infer_only) and "linear_split" in names and "weight_grad_split" not in names


def test_an_optimiser_step_is_picked_up(monkeypatch):
    model, x, dy = _small(monkeypatch)
    first = _step(model, x, dy, monkeypatch, "fp32", "bf16x3")
    torch.optim.SGD(model.parameters(), lr=1e-2).step()
    second = _step(model, x, dy, monkeypatch, "fp32", "bf16x3")
    fresh, _, _ = _model("GraphTransformer", 128, 2, "o32_ico2", seed=99)  # other weights, never split before
    fresh.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    want = _step(fresh.to(DEV), x, dy, monkeypatch, "fp32", "bf16x3")
    assert not _same(second, first)
    assert _same(second, want)
    params = {k for k, _ in model.named_parameters()}  # (buffers stay as they are)
    fresh.load_state_dict({k: v.detach().cpu() * 0.5 if k in params else v.detach().cpu() for k, v in model.state_dict().items()})
    halved = _step(fresh, x, dy, monkeypatch, "fp32", "bf16x3")  # load_state_dict into a model whose planes exist
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(0.5)
    assert _same(_step(model, x, dy, monkeypatch, "fp32", "bf16x3"), halved)


def test_graphed_train_step_replays_the_route(monkeypatch):
    from anemoi_models_amd.runtime import GraphedTrainStep

    model, x, dy = _small(monkeypatch)
    eager = _step(model, x, dy, monkeypatch, "fp32", "bf16x3")
    exact = _step(model, x, dy, monkeypatch, "fp32", None)
    monkeypatch.setenv(SWITCH, "bf16x3")
    model.zero_grad(set_to_none=True)
    graphed = GraphedTrainStep(model, lambda y, t: (y.float() * t).sum(), torch.zeros_like(x), torch.zeros_like(dy), warmup=2)
    loss = graphed(x, dy)
    grads = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    assert torch.equal(loss, eager[1]) and not torch.equal(loss, exact[1])
    assert grads.keys() == eager[2].keys() and all(torch.equal(grads[k], eager[2][k]) for k in grads)
    with torch.no_grad():  # an update between replays (no optimiser inside the graph) is seen by the next replay
        for p in model.parameters():
            p.mul_(0.5)
    loss2 = graphed(x, dy)
    got = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    del graphed
    want = _step(model, x, dy, monkeypatch, "fp32", "bf16x3")
    assert torch.equal(loss2, want[1]) and all(torch.equal(got[k], want[2][k]) for k in got)
