"""Rollout training, the parts that need no GPU: the restatements the GPU tests compare against (tests/_rollout_ref.py), the
host-side inverse column map, and the argument checks of the new entry points through the C ABI."""

import pytest
import torch

import _rollout_ref as rr
from conftest import split_prefix
from oracle import reference_path as ref


def test_restated_advance_on_a_hand_written_case():
    """colmap semantics of include/anemoi_amd.h (anemoi_advance_input) on x [1, 2, 1, 2, 3], y [1, 1, 2, 2], forcing [1, 1, 2, 1]:
    column 0 <- y column 1, column 1 persists, column 2 <- forcing column 0."""
    x = torch.tensor([[[1., 2., 3.], [4., 5., 6.]], [[7., 8., 9.], [10., 11., 12.]]]).reshape(1, 2, 1, 2, 3)
    y = torch.tensor([[20., 21.], [22., 23.]]).reshape(1, 1, 2, 2)
    f = torch.tensor([[30.], [31.]]).reshape(1, 1, 2, 1)
    colmap = [1, -1, -2]
    got = rr.advance(x, y, colmap, f)
    want = torch.tensor([[[7., 8., 9.], [10., 11., 12.]], [[21., 8., 30.], [23., 11., 31.]]]).reshape(1, 2, 1, 2, 3)
    assert torch.equal(got, want)
    got = rr.advance(x, y, colmap, None)  # without forcing the forcing column persists too
    want[0, 1, 0, :, 2] = torch.tensor([9., 12.])
    assert torch.equal(got, want)
    one = rr.advance(x[:, 1:], y, colmap, f)  # T = 1: only the last slice
    assert torch.equal(one, want.new_tensor([[21., 8., 30.], [23., 11., 31.]]).reshape(1, 1, 1, 2, 3))
    xg, yg = x.clone().requires_grad_(), y.clone().requires_grad_()  # gradients: shifted copy, persist term, scatter into y
    rr.advance(xg, yg, colmap, f).backward(torch.arange(12.).reshape(1, 2, 1, 2, 3))
    assert torch.equal(xg.grad.reshape(2, 2, 3), torch.tensor([[[0., 0., 0.], [0., 0., 0.]], [[0., 1. + 7., 2.], [3., 4. + 10., 5.]]]))
    assert torch.equal(yg.grad.reshape(2, 2), torch.tensor([[0., 6.], [0., 9.]]))


def test_restated_advance_is_the_oracle_rollouts(golden_interface, graph_o32):
    """tests/_rollout_ref.py::rollout (normalised space, colmap from the package's shared helper) gives the steps of
    oracle.reference_path.rollout (physical space, its own roll + index writes) on the golden interface fixture."""
    from test_oracle_golden import graph_tensors

    from anemoi_models_amd.utils.indices import SimpleDataIndices, advance_colmap

    gold = golden_interface
    sd = split_prefix(gold, "sd.")
    graph = graph_tensors(graph_o32)
    kw = dict(num_heads=16, num_layers=4, num_chunks=2, prognostic_in=list(range(10)), prognostic_out=list(range(10)))
    want = ref.rollout(sd, graph, gold["batch"], 2, gold["rollout_forcings"], multi_step=2, forcing_in=[10, 11], **kw)
    p = "pre_processors.processors.normalizer."
    mul, add = sd[p + "_norm_mul"], sd[p + "_norm_add"]
    i_in, i_out = sd[p + "_input_idx"].long(), sd[p + "_output_idx"].long()
    colmap = advance_colmap(SimpleDataIndices(n_prognostic=10, n_forcing=2, n_diagnostic=1))
    assert colmap.tolist() == list(range(10)) + [-2, -3]
    x = (gold["batch"] * mul[i_in] + add[i_in])[:, 0:2, None]
    forc = (gold["rollout_forcings"] * mul[i_in][[10, 11]] + add[i_in][[10, 11]])[:, :, None]
    model_sd = {k[len("model."):]: v for k, v in sd.items() if k.startswith("model.")}
    got = rr.rollout(model_sd, graph, x, 2, colmap, forc, **kw)
    got = (got - add[i_out]) / mul[i_out]
    torch.testing.assert_close(got, want, atol=1e-5, rtol=1e-5)


def test_inverse_colmap_builder_refuses_repeats():
    from anemoi_models_amd import ops

    inv = ops.inverse_colmap(torch.tensor([2, -1, 0, -2, -3], dtype=torch.int32), 4)
    assert inv.dtype == torch.int32 and inv.tolist() == [2, -1, 0, -1]
    with pytest.raises(ValueError, match="feeds input columns 0 and 2"):
        ops.inverse_colmap(torch.tensor([1, -1, 1], dtype=torch.int32), 2)
    with pytest.raises(ValueError, match="not one of the 2 output columns"):
        ops.inverse_colmap(torch.tensor([2, -1], dtype=torch.int32), 2)


def test_new_entry_points_validate_without_gpu():
    """Null pointers, bad shapes and rows % G != 0 come back as ANEMOI_ERR_INVALID with a message before anything is launched."""
    from anemoi_models_amd import _lib

    lib = _lib.load()
    bad, p = _lib.ANEMOI_ERR_INVALID, 4096  # p: a non-null pointer value that is never dereferenced by the checks
    assert lib.anemoi_advance_state(None, None, 1, 2, 1, 4, 3, None, 2, None, 0, None, None) == bad
    assert b"anemoi_advance_state: null pointer" in lib.anemoi_last_error()
    assert lib.anemoi_advance_state(p, p + (1 << 20), 1, 0, 1, 4, 3, p, 2, None, 0, p, None) == bad
    assert b"bad shape" in lib.anemoi_last_error()
    assert lib.anemoi_advance_state(p, p + 16, 1, 2, 1, 4, 3, p, 2, None, 0, p, None) == bad  # overlapping in and out
    assert b"alias" in lib.anemoi_last_error()
    assert lib.anemoi_advance_state_backward(None, None, None, 1, 2, 1, 4, 3, 2, None, None, 0, None) == bad
    assert b"anemoi_advance_state_backward: null pointer" in lib.anemoi_last_error()
    assert lib.anemoi_advance_state_backward(p, p + (1 << 20), p, 1, 2, 1, -1, 3, 2, p, p, 0, None) == bad
    assert lib.anemoi_assemble_nodes_backward(_lib.F32, None, 8, None, 1, 2, 1, 4, 3, None) == bad
    assert b"anemoi_assemble_nodes_backward: null pointer" in lib.anemoi_last_error()
    assert lib.anemoi_assemble_nodes_backward(_lib.BF16, p, 5, p, 1, 2, 1, 4, 3, None) == bad  # ldg 5 < T * V = 6
    assert b"ldg 5 < T * V = 6" in lib.anemoi_last_error()
    assert lib.anemoi_prognostic_residual_backward(None, 2, None, 1, 2, 1, 4, 3, None, None) == bad
    assert b"anemoi_prognostic_residual_backward: null pointer" in lib.anemoi_last_error()
    assert lib.anemoi_prognostic_residual_backward(p, 2, p, 1, 2, 1, 4, 0, p, None) == bad
    assert lib.anemoi_weighted_mse(None, None, 8, 3, 4, None, None, None, 1.0, None, None, 0, None) == bad
    assert b"anemoi_weighted_mse: null pointer" in lib.anemoi_last_error()
    assert lib.anemoi_weighted_mse(p, p, 9, 3, 4, p, p, None, 1.0, p, p, 1, None) == bad
    assert b"rows 9 is not a multiple of the grid size G = 4" in lib.anemoi_last_error()
    assert lib.anemoi_weighted_mse(p, p, -4, 3, 4, p, p, None, 1.0, p, p, 1, None) == bad
    assert lib.anemoi_weighted_mse(p, p, 8, 3, 4, p, p, None, 1.0, p, p, 0, None) == bad  # workspace too small
    assert b"workspace" in lib.anemoi_last_error()
    assert lib.anemoi_weighted_mse_backward(None, None, 8, 3, 4, None, None, None, 1.0, None, None, None) == bad
    assert b"anemoi_weighted_mse_backward: null pointer" in lib.anemoi_last_error()
    assert lib.anemoi_weighted_mse_backward(p, p, 9, 3, 4, p, p, None, 1.0, p, p, None) == bad
    assert b"not a multiple" in lib.anemoi_last_error()
    assert lib.anemoi_weighted_mse_backward(p, p, 8, 3, 4, p, p, None, 1.0, None, p, None) == bad


def test_weighted_mse_workspace_is_a_function_of_the_element_count():
    """The workgroup count of stage 1 (= the partials) depends on rows * V alone: the reduction order cannot change with the
    device, the occupancy or the split of the element count into rows and columns."""
    from anemoi_models_amd import _lib

    lib = _lib.load()
    ws = lib.anemoi_weighted_mse_workspace_floats
    assert ws(0, 5) == 0 and ws(1, 1) == 1
    for rows, v in [(2062, 5), (257, 80), (4096, 1), (542080 * 3, 80)]:
        n = rows * v
        same = {ws(r, n // r) for r in (1, 2, 5, 10) if n % r == 0} | {ws(rows, v), ws(v, rows)}
        assert len(same) == 1 and 1 <= next(iter(same)) <= n
    counts = [ws(r, 80) for r in (1, 52, 1031, 542080, 4 * 542080)]
    assert counts == sorted(counts) and counts[0] == 1 and counts[-1] == counts[-2]  # grows with the size, then saturates
