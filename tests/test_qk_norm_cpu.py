"""qk_norm without a GPU: the restatement and its bound (tests/_qk_norm_ref.py), the entry points' argument checks, the
workspace geometry, the state-dict keys of every class that takes the switch, the config plumbing, the refusals and the route
switch of the GraphTransformer blocks."""

import pytest
import torch

import _qk_norm_ref as R


# ------------------------------------------------------------------------------------------------ restatement and bound
@pytest.mark.parametrize("rows,groups,h,d", R.F32_CASES)
def test_restatement_equals_torch_layer_norm_on_the_head_view(rows, groups, h, d):
    x, w, _ = R.inputs(torch.float32, rows, groups, h, d)
    x, w = x.double(), w.double()
    got = R.head_norm(x, w, h, groups)
    for g in range(groups):
        cols = slice(g * h * d, (g + 1) * h * d)
        want = torch.nn.functional.layer_norm(x[:, cols].reshape(rows, h, d), (d,), w[g], None, R.EPS).reshape(rows, h * d)
        assert float((got[:, cols] - want).abs().max()) < 1e-12
    st = R.stats(x, h, groups)
    xhat = x.reshape(rows, groups * h, d) * st[..., :1] + st[..., 1:]
    assert float((xhat.reshape(rows, -1) * w.repeat_interleave(h, 0).reshape(1, -1) - got).abs().max()) < 1e-12


@pytest.mark.parametrize("dtype,rows,groups,h,d", R.CASES, ids=lambda v: R.name(v) if isinstance(v, torch.dtype) else str(v))
def test_f32_emulation_stays_inside_the_bound_and_every_forward_fault_leaves_it(dtype, rows, groups, h, d):
    x, w, _ = R.inputs(dtype, rows, groups, h, d)
    assert R.rel_err(R.emulate(x, w, h, groups, dtype=dtype), R.reference(dtype, rows, groups, h, d)[0]) < R.FWD_TOL[dtype]
    lone = rows * groups * h == 1  # a single head: it stays as drawn (the faults have nothing else to show on)
    if not lone:
        x = x.clone()
        x[0, :d] = x[0, 0]  # one constant head: its variance is 0, the result 0 (eps keeps rstd finite)
    want, bound = R.forward_bound(x, w, h, groups, dtype)
    used = R.used_fraction(R.emulate(x, w, h, groups, dtype=dtype), want, bound)
    print(f"{R.name(dtype)} {(rows, groups, h, d)}: plain f32 evaluation uses {used:.2f} of the bound (K = {R.bound_k(d)})")
    assert used <= 1.0
    for fault in R.FAULTS_FORWARD:
        # (one group has no other weight to take; a row of one head keeps its statistics under a rotation; no constant head)
        if (fault == "k_with_q_weight" and groups == 1) or (fault == "offset_one" and groups * h == 1) or (fault == "no_eps" and lone):
            continue
        f = R.used_fraction(R.emulate(x, w, h, groups, fault=fault, dtype=dtype), want, bound)
        assert f > 1.0, (fault, f)


def test_bound_constant_counts_roundings_and_does_not_grow_like_d():
    assert R.bound_k(4) == 9.0 and R.bound_k(5) == 9.5 and R.bound_k(64) == 11.0 and R.bound_k(128) == 11.5
    assert all(2.1 < R.bound_k(d) <= 11.5 for d in range(1, 129))


def test_backward_faults_leave_the_aggregate_gradient_bound():
    caught = {f: {torch.float32: [], torch.bfloat16: []} for f in R.FAULTS_BACKWARD}
    for dtype, rows, groups, h, d in R.CASES:
        x, w, dy = R.inputs(dtype, rows, groups, h, d)
        _, dx, dw, _ = R.reference(dtype, rows, groups, h, d)
        gx, gw = R.emulate_backward(x, w, dy, h, groups, dtype=dtype)
        assert R.rel_err(gx, dx) < R.GRAD_TOL[dtype] and R.rel_err(gw, dw) < R.GRAD_TOL[dtype], (dtype, rows, groups, h, d)
        for fault in R.FAULTS_BACKWARD:
            if (fault == "dw_both_groups" and groups == 1) or (fault == "dw_row_dropped" and rows == 1):
                continue
            fx, fw = R.emulate_backward(x, w, dy, h, groups, fault=fault, dtype=dtype)
            caught[fault][dtype].append(max(R.rel_err(fx, dx), R.rel_err(fw, dw)) >= R.GRAD_TOL[dtype])
    for fault, by_dtype in caught.items():
        assert all(by_dtype[torch.float32]), fault  # every f32 case sees it
        # bf16: one row of 4100 x 16 terms is below the storage rounding of the others; the small cases see it
        assert any(by_dtype[torch.bfloat16]), fault
        if fault != "dw_row_dropped":
            assert all(by_dtype[torch.bfloat16]), fault


# ------------------------------------------------------------------------------------------------ entry points, no GPU
def test_head_norm_entry_points_validate_without_gpu():
    from anemoi_models_amd import _lib

    lib = _lib.load()
    bad, unsupported = _lib.ANEMOI_ERR_INVALID, _lib.ANEMOI_ERR_UNSUPPORTED
    p = 4096  # (never dereferenced: every call below is refused before a launch)

    def fwd(**kw):
        a = dict(dtype=0, x=p, ldx=64, w=p, y=p, ldy=64, stats=None, rows=8, groups=2, h=4, d=8, eps=1e-5)
        a.update(kw)
        return lib.anemoi_head_norm(a["dtype"], a["x"], a["ldx"], a["w"], a["y"], a["ldy"], a["stats"], a["rows"], a["groups"],
                                    a["h"], a["d"], a["eps"], None)

    for name in ("x", "w", "y"):
        assert fwd(**{name: None}) == bad and b"anemoi_head_norm: null pointer" in lib.anemoi_last_error()
    assert fwd(ldx=63) == bad and b"leading dimension 63 < groups * H * D = 64" in lib.anemoi_last_error()
    assert fwd(ldy=10) == bad and b"leading dimension" in lib.anemoi_last_error()
    assert fwd(d=0) == bad and b"bad shape" in lib.anemoi_last_error()
    assert fwd(d=129, ldx=2048, ldy=2048) == unsupported and b"D = 129, at most 128" in lib.anemoi_last_error()
    assert fwd(groups=0) == bad and fwd(h=0) == bad and fwd(rows=-1) == bad
    assert fwd(stats=p + 4) == bad and b"8-byte aligned" in lib.anemoi_last_error()
    assert fwd(dtype=7) == unsupported and b"dtype 7" in lib.anemoi_last_error()
    assert fwd(rows=0) == _lib.ANEMOI_OK  # nothing to do, nothing launched

    n_ws = lib.anemoi_head_norm_backward_workspace_floats(8, 2, 4, 8)

    def bwd(**kw):
        a = dict(dtype=1, dy=p, ldd=64, x=p, ldx=64, stats=p, w=p, dx=p, ldo=64, dw=p, rows=8, groups=2, h=4, d=8, ws=p, n_ws=n_ws)
        a.update(kw)
        return lib.anemoi_head_norm_backward(a["dtype"], a["dy"], a["ldd"], a["x"], a["ldx"], a["stats"], a["w"], a["dx"],
                                             a["ldo"], a["dw"], a["rows"], a["groups"], a["h"], a["d"], a["ws"], a["n_ws"], None)

    for name in ("dy", "x", "stats", "w", "dx", "dw"):
        assert bwd(**{name: None}) == bad and b"anemoi_head_norm_backward: null pointer" in lib.anemoi_last_error()
    for name in ("ldd", "ldx", "ldo"):
        assert bwd(**{name: 63}) == bad and b"leading dimension 63" in lib.anemoi_last_error()
    assert bwd(d=0) == bad
    assert bwd(d=129, ldd=2048, ldx=2048, ldo=2048) == unsupported and b"at most 128" in lib.anemoi_last_error()
    assert bwd(ws=None) == bad and b"workspace" in lib.anemoi_last_error()
    assert bwd(n_ws=n_ws - 1) == bad and b"workspace of" in lib.anemoi_last_error()
    assert bwd(rows=0) == bad


def test_head_norm_backward_workspace_is_a_function_of_its_arguments():
    from anemoi_models_amd import _lib

    ws = _lib.load().anemoi_head_norm_backward_workspace_floats
    assert ws(0, 2, 16, 64) == 0 and ws(8, 0, 16, 64) == 0 and ws(8, 2, 16, 129) == 0
    for rows, groups, h, d in [(1, 1, 1, 4), (64, 2, 16, 64), (65, 2, 16, 64), (8192, 1, 16, 64), (40962, 2, 16, 64),
                               (542080, 1, 16, 64)]:
        chunk = max((rows + 127) // 128, 64)  # at most 128 chunks of at least 64 rows
        chunks = (rows + chunk - 1) // chunk
        assert ws(rows, groups, h, d) == (chunks + 1) * groups * h * d == ws(rows, groups, h, d)
        assert chunks <= 128


# ------------------------------------------------------------------------------------------------ state dicts
def _classes():
    from anemoi_models_amd.layers.attention import MultiHeadSelfAttention
    from anemoi_models_amd.layers.block import (GraphTransformerMapperBlock, GraphTransformerProcessorBlock,
                                                TransformerProcessorBlock)
    from anemoi_models_amd.layers.chunk import GraphTransformerProcessorChunk, TransformerProcessorChunk
    from anemoi_models_amd.layers.processor import TransformerProcessor

    gt = dict(in_channels=64, hidden_dim=128, out_channels=64, edge_dim=3, num_heads=16)
    return [
        (MultiHeadSelfAttention, dict(num_heads=4, embed_dim=64), [""], 16),
        (TransformerProcessorBlock, dict(num_channels=64, hidden_dim=128, num_heads=4, activation="GELU", window_size=8),
         ["attention."], 16),
        (TransformerProcessorChunk, dict(num_channels=64, num_layers=2, window_size=8, num_heads=4),
         ["blocks.0.attention.", "blocks.1.attention."], 16),
        (TransformerProcessor, dict(num_layers=2, num_channels=64, num_chunks=2, num_heads=4, window_size=8),
         ["proc.0.blocks.0.attention.", "proc.1.blocks.0.attention."], 16),
        (GraphTransformerProcessorBlock, gt, [""], 4),
        (GraphTransformerMapperBlock, gt, [""], 4),
        (GraphTransformerProcessorChunk, dict(num_channels=64, num_layers=2, num_heads=16, edge_dim=3), ["blocks.0.", "blocks.1."], 4),
    ]


def _keys_from_submodules(module, skip=("q_norm", "k_norm")):
    """The state-dict keys a module has without the norms, from its own parameters / buffers and its other sub-modules."""
    keys = [k for k, _ in module.named_parameters(recurse=False)] + [k for k, _ in module.named_buffers(recurse=False)
                                                                     if k not in module._non_persistent_buffers_set]
    for name, child in module.named_children():
        if name not in skip:
            keys += [f"{name}.{k}" for k in _keys_from_submodules(child, skip)]
    return keys


@pytest.mark.parametrize("case", range(7))
def test_state_dict_keys_with_and_without_qk_norm(case):
    cls, kw, prefixes, d = _classes()[case]
    today, off, on = cls(**kw), cls(**kw, qk_norm=False), cls(**kw, qk_norm=True)
    assert list(off.state_dict()) == list(today.state_dict())
    assert sorted(off.state_dict()) == sorted(_keys_from_submodules(off)) == sorted(_keys_from_submodules(on))
    extra = {p + n for p in prefixes for n in ("q_norm.weight", "k_norm.weight")}
    assert set(on.state_dict()) - set(off.state_dict()) == extra and set(off.state_dict()) <= set(on.state_dict())
    for k in extra:
        v = on.state_dict()[k]
        assert tuple(v.shape) == (d,) and v.dtype == torch.float32 and bool((v == 1).all())
    assert not any(k.endswith("norm.bias") and ("q_norm" in k or "k_norm" in k) for k in on.state_dict())


# ------------------------------------------------------------------------------------------------ config plumbing
def _model(graph, processor, qk_norm=True, channels=64, layers=2):
    from anemoi_models_amd.models import AnemoiModelEncProcDec
    from anemoi_models_amd.utils.indices import SimpleDataIndices
    from anemoi_models_amd.utils.presets import model_config

    cfg = model_config(processor, channels, layers, 16)
    if qk_norm:
        for part in ("encoder", "processor", "decoder"):
            cfg.model[part]["qk_norm"] = True
    idx = SimpleDataIndices(n_prognostic=10, n_forcing=2, n_diagnostic=1)
    return AnemoiModelEncProcDec(model_config=cfg, data_indices=idx, graph_data=graph)


@pytest.mark.parametrize("processor", ["GraphTransformer", "Transformer"])
def test_a_config_with_qk_norm_builds_the_norms_in_encoder_processor_and_decoder(graph_o32, processor):
    torch.manual_seed(0)
    plain, model = _model(graph_o32, processor, qk_norm=False), _model(graph_o32, processor)
    att = "attention." if processor == "Transformer" else ""
    want = {f"{p}.{n}_norm.weight" for n in "qk"
            for p in ["encoder.proc", "decoder.proc"] + [f"processor.proc.{c}.blocks.0.{att}".rstrip(".") for c in range(2)]}
    sd = model.state_dict()
    assert set(sd) - set(plain.state_dict()) == want and set(plain.state_dict()) <= set(sd)
    assert model.encoder.proc.qk_norm and model.decoder.proc.qk_norm and model.processor.qk_norm
    assert all(tuple(sd[k].shape) == (64 // 16,) for k in want)
    # a checkpoint of such a model round-trips, and is refused by a model built without the switch
    with torch.no_grad():
        for k in want:
            sd[k].normal_()
    other = _model(graph_o32, processor)
    other.load_state_dict(sd, strict=True)
    assert all(torch.equal(other.state_dict()[k], sd[k]) for k in sd)
    with pytest.raises(RuntimeError, match="q_norm"):
        plain.load_state_dict(sd, strict=True)


# ------------------------------------------------------------------------------------------------ refusals and routes
def test_graph_transformer_blocks_with_qk_norm_leave_every_folded_route():
    from anemoi_models_amd.layers.block import GraphTransformerMapperBlock, GraphTransformerProcessorBlock, Rows

    kw = dict(in_channels=128, hidden_dim=256, out_channels=128, edge_dim=3, num_heads=16)
    for dtype in (torch.float32, torch.bfloat16):
        for cls in (GraphTransformerProcessorBlock, GraphTransformerMapperBlock):
            assert cls(**kw).fold_width(dtype) == 4 and cls(**kw, qk_norm=True).fold_width(dtype) is None
    plain, normed = GraphTransformerMapperBlock(**kw), GraphTransformerMapperBlock(**kw, qk_norm=True)
    raw = Rows("raw", 64, 40, 40, on_gpu=True)
    for src, dst in ((Rows(on_gpu=True), Rows(on_gpu=True)), (raw, Rows("embedded", 64, 40, 40, True)), (Rows(on_gpu=True), raw)):
        r = normed.route(torch.bfloat16, src, dst)
        assert r.name == "unfolded" and r.up is None and not r.block_tail and r.dst_h
        assert plain.route(torch.bfloat16, src, dst).name != "unfolded"
    assert normed.edge_layout(torch.bfloat16) == (4, -1) and plain.edge_layout(torch.bfloat16) == (4, 3)
    assert GraphTransformerProcessorBlock(**kw, qk_norm=True).block_abi_operands(torch.bfloat16, [], "sqkvu") is None


def test_qk_norm_refusals_are_raised_before_anything_is_launched(graph_o32, monkeypatch):
    from anemoi_models_amd.layers.block import GraphTransformerMapperBlock, GraphTransformerProcessorBlock

    kw = dict(in_channels=128, hidden_dim=256, out_channels=128, edge_dim=3, num_heads=16)
    x = torch.zeros(8, 128, dtype=torch.bfloat16)  # CPU tensors: a launch would raise RuntimeError ("no CPU fallback") instead
    proc, mapper = GraphTransformerProcessorBlock(**kw, qk_norm=True), GraphTransformerMapperBlock(**kw, qk_norm=True)
    with pytest.raises(NotImplementedError, match="qk_norm"):
        proc.native(x, None, None, halo=object())
    with pytest.raises(NotImplementedError, match="qk_norm"):
        mapper.native(x, x, None, None, halo=object())
    monkeypatch.setenv("ANEMOI_AMD_MXFP8", "1")
    with pytest.raises(NotImplementedError, match="qk_norm"):
        proc.native(x, None, None)
    with pytest.raises(NotImplementedError, match="qk_norm"):
        mapper.native(x, x, None, None)
    monkeypatch.delenv("ANEMOI_AMD_MXFP8")
    model = _model(graph_o32, "GraphTransformer")
    with pytest.raises(NotImplementedError, match="qk_norm"):
        model.processor.native_local(x, None)
    with pytest.raises(NotImplementedError, match="qk_norm"):
        model.encoder.native_local(x, x, None)
    with pytest.raises(NotImplementedError, match="qk_norm"):
        model.decoder.native_local(x, x, None)
    # the node-partitioned model routes, forward and training: refused before a shard plan is built (no process group here)
    from anemoi_models_amd.distributed import partition

    xin = torch.zeros(1, 2, 1, graph_o32["data"].num_nodes, 12)
    for fn in (partition.sharded_forward, partition.sharded_training_forward):
        with pytest.raises(NotImplementedError, match="qk_norm"):
            fn(model, xin, None)
    for part in ("encoder", "decoder"):  # one GraphTransformer part with the switch is enough
        cfg_model = _model(graph_o32, "Transformer", qk_norm=False)
        getattr(cfg_model, part).qk_norm = True
        with pytest.raises(NotImplementedError, match="qk_norm"):
            partition.sharded_training_forward(cfg_model, xin, None)


def test_prepared_processor_weights_are_not_built_for_qk_norm_blocks():
    from anemoi_models_amd import autograd

    sd = {"b.q_norm.weight": torch.ones(4)}
    assert autograd.has_qk_norm(sd, "b") and not autograd.has_qk_norm({}, "b")
    assert autograd.gt_processor_weights([sd, sd], "b", 64, 16, 4, torch.bfloat16, "cpu") is None


def test_ops_head_norm_has_no_cpu_fallback():
    from anemoi_models_amd import autograd, ops

    x, w = torch.zeros(4, 64), torch.ones(2, 8)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.head_norm(x, w, 4, 2)
    with pytest.raises(RuntimeError, match="MI355X"):
        autograd.head_norm(x.requires_grad_(), w, 4, 2)
