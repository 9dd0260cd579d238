"""Launch trail on the GPU: the digest kernel against the host references (integers and bits: exact), and the trail of
whole forwards and training steps -- it changes no output bit, repeats, sees every kernel behind a block-level call, and
names the first launch whose output differs between two runs."""

import pytest
import torch

from _trail_ref import numpy_record
from _trail_ref import torch_record
from conftest import split_prefix

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _fields(e):
    return (e.digest, e.nonfinite, e.absmax)


def _seeded(dtype, rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype in (torch.float32, torch.bfloat16):
        return (torch.randn(rows, cols, generator=g) * 3).to(dtype)
    if dtype == torch.int32:
        return torch.randint(-2**31, 2**31 - 1, (rows, cols), generator=g, dtype=torch.int64).to(torch.int32)
    return torch.randint(0, 256, (rows, cols), generator=g, dtype=torch.int64).to(torch.uint8)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows,cols", [(1, 1), (7, 3), (257, 1000), (0, 64)])
def test_digest_against_the_numpy_reference(dtype, rows, cols):
    from anemoi_models_amd import trail

    x = _seeded(dtype, rows, cols, 3 * rows + cols)
    e = trail.digest(x.to(DEV))
    assert (e.rows, e.cols, e.dtype) == (rows, cols, "f32" if dtype == torch.float32 else "bf16")
    assert _fields(e) == numpy_record(x)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_digest_of_slices_never_reads_the_padding_and_takes_odd_starts(dtype):
    from anemoi_models_amd import trail

    wide = _seeded(dtype, 129, 200, 9)
    wide[:, 77:] = float("nan")  # the padding of the slice below
    d = wide.to(DEV)
    e = trail.digest(d[:, :77])
    assert _fields(e) == numpy_record(wide[:, :77]) and e.nonfinite == 0
    # a view that starts at an odd element (not 16-byte aligned), rows of an odd pitch
    e = trail.digest(d[:, 1:76])
    assert _fields(e) == numpy_record(wide[:, 1:76]) and e.nonfinite == 0
    flat = _seeded(dtype, 1, 5003, 4)
    e = trail.digest(flat.to(DEV)[:, 3:])
    assert _fields(e) == numpy_record(flat[:, 3:])
    # long rows with padding: the rows are cut into units
    big = _seeded(dtype, 3, 40000, 6)
    big[:, 33333:] = float("inf")
    e = trail.digest(big.to(DEV)[:, 5:33333])
    assert _fields(e) == numpy_record(big[:, 5:33333])


@pytest.mark.parametrize("dtype", [torch.int32, torch.uint8])
def test_digest_of_integer_dtypes(dtype):
    from anemoi_models_amd import trail

    for rows, cols in [(1, 1), (65, 131), (4, 5000)]:
        x = _seeded(dtype, rows, cols + 2, rows)
        e = trail.digest(x.to(DEV)[:, 1 : cols + 1])
        assert _fields(e) == numpy_record(x[:, 1 : cols + 1]) and e.nonfinite == 0 and e.absmax == 0.0


def test_digest_indexes_in_64_bits():
    """More than 2^32 elements (9 GB of bf16): the digest equals the torch-int64 reference computed on the device in chunks."""
    from anemoi_models_amd import trail

    rows, cols = 1_100_000, 4096
    assert rows * cols > 2**32
    x = torch.empty(rows, cols, dtype=torch.bfloat16, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(5)
    for r0 in range(0, rows, 100_000):
        x[r0 : r0 + 100_000].normal_(generator=g)
    e = trail.digest(x)
    want = torch_record(x)
    print(f"64-bit case: digest {e.digest:016x}, reference {want[0]:016x}")
    assert _fields(e) == want and e.nonfinite == 0
    x[rows - 2, cols - 5] = float("inf")
    e2 = trail.digest(x)
    assert e2.nonfinite == 1 and e2.digest != e.digest
    assert e2.digest == torch_record(x)[0]
    del x


def test_nonfinite_and_absmax_against_torch():
    from anemoi_models_amd import trail

    for dtype in (torch.float32, torch.bfloat16):
        x = _seeded(dtype, 300, 70, 8).clamp(-50, 50)
        x[3, 5], x[17, 0], x[299, 69], x[100, 33] = float("nan"), float("inf"), -float("inf"), -1024.0
        e = trail.digest(x.to(DEV))
        f = x.float()
        assert e.nonfinite == int((~torch.isfinite(f)).sum()) == 3
        assert e.absmax == float(f[torch.isfinite(f)].abs().max()) == 1024.0
        assert e.digest == numpy_record(x)[0]


def _model(graph, gold, sd=None, layers=4):
    from test_gpu_parity import _build

    model, _ = _build(graph, 64, layers)
    model.load_state_dict(sd if sd is not None else split_prefix(gold, "sd."))
    return model.to(DEV).eval()


def _forward(model, x, capacity=4096):
    from anemoi_models_amd import trail

    with torch.no_grad(), trail.record(capacity=capacity) as t:
        y = model(x)
    return y, t


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_trail_changes_nothing_and_repeats(graph_o32, golden_cfg1_gt, monkeypatch, dtype):
    from anemoi_models_amd import trail

    monkeypatch.setenv("ANEMOI_AMD_DTYPE", dtype)
    model = _model(graph_o32, golden_cfg1_gt)
    x = golden_cfg1_gt["x"].to(DEV)
    with torch.no_grad():
        model(x)  # (the first forward also packs weights and builds the edge plans)
        plain = model(x)
    y1, t1 = _forward(model, x)
    y2, t2 = _forward(model, x)
    assert torch.equal(y1, plain) and torch.equal(y2, plain)
    assert trail.first_difference(t1, t2) is None
    assert len(t1.entries) > 0 and t1.dropped == 0
    names = t1.names()
    print(f"{dtype}: {len(names)} records; entry points: {sorted({n.split(':')[0] for n in names})}")
    assert any(n.startswith("anemoi_linear") for n in names)
    assert any(n.startswith("anemoi_gt_edge_attention") for n in names)
    assert any(n.startswith(("anemoi_assemble_node", "anemoi_finalize_output")) for n in names)
    assert t1.first_nonfinite() is None


def test_kernel_granularity_inside_one_block_level_call():
    """anemoi_transformer_block_forward runs seven kernels behind one C call: each leaves its own record, in order."""
    from anemoi_models_amd import trail
    from anemoi_models_amd.layers.block import TransformerProcessorBlock

    torch.manual_seed(3)
    blk = TransformerProcessorBlock(512, 2048, 16, "GELU", window_size=16, dropout_p=0.0).to(DEV).eval()
    x = (torch.randn(1300, 512, generator=torch.Generator().manual_seed(1)) * 0.8).to(torch.bfloat16).to(DEV)
    with torch.no_grad():
        assert blk._block_abi(x, 1) is not None  # (packs the weights; the route is taken)
        with trail.record() as t:
            y = blk._block_abi(x, 1)  # ONE Python-visible library call
    assert y is not None and len(t.entries) >= 7
    main = [e.name.split(":")[0] for e in t.entries if e.name.endswith(":out")]
    assert main == ["anemoi_layer_norm", "anemoi_linear", "anemoi_mhsa", "anemoi_linear", "anemoi_layer_norm", "anemoi_linear",
                    "anemoi_linear"], t.names()
    assert (t.entries[-1].rows, t.entries[-1].cols) == (1300, 512)
    assert t.entries[-1].digest == trail.digest(y).digest


def _changed(sd, key, index, delta=0.25):
    sd2 = {k: v.clone() for k, v in sd.items()}
    sd2[key].view(-1)[index] += delta
    assert int((sd2[key] != sd[key]).sum()) == 1
    return sd2


def test_localisation_of_a_changed_weight(graph_o32, golden_cfg1_gt):
    from anemoi_models_amd import trail

    sd = split_prefix(golden_cfg1_gt, "sd.")
    x = golden_cfg1_gt["x"].to(DEV)

    def run(state):
        model = _model(graph_o32, golden_cfg1_gt, state)  # a model of its own: no packed-weight cache is shared
        with torch.no_grad():
            model(x)
        return _forward(model, x)[1]

    base = run(sd)
    linears = [e.index for e in base.entries if e.name.startswith("anemoi_linear") and e.name.endswith(":out")]
    edges = [e.index for e in base.entries if e.name.startswith("anemoi_gt_edge_attention")]

    # the last Linear of the forward: the decoder's final extractor
    other = run(_changed(sd, "decoder.node_data_extractor.1.bias", 4))
    diff = trail.first_difference(base, other)
    assert diff is not None
    i, ea, eb = diff
    assert i == linears[-1] and ea.name == eb.name and ea.digest != eb.digest, (i, ea, eb, linears[-1])
    assert all(a.same_as(b) for a, b in zip(base.entries[:i], other.entries[:i]))

    # a Linear in the middle of the processor
    other = run(_changed(sd, "processor.proc.0.blocks.1.projection.bias", 7))
    i, ea, eb = trail.first_difference(base, other)
    assert all(a.same_as(b) for a, b in zip(base.entries[:i], other.entries[:i]))
    assert ea.name.startswith("anemoi_linear") and ea.name == eb.name, (i, ea, eb)
    assert edges[0] < i < edges[-1], (edges[0], i, edges[-1])


def test_nonfinite_input_is_named_at_the_first_record(graph_o32, golden_cfg1_gt):
    model = _model(graph_o32, golden_cfg1_gt)
    x = golden_cfg1_gt["x"].to(DEV)
    with torch.no_grad():
        model(x)
    _, clean = _forward(model, x)
    assert clean.first_nonfinite() is None
    bad = x.clone()
    bad[0, 1, 0, 1234, 3] = float("nan")
    _, t = _forward(model, bad)
    first = t.first_nonfinite()
    assert first is not None and first.nonfinite >= 1
    assert first.index == 0, (first, t.names()[:4])
    assert first.name.startswith(("anemoi_assemble_node", "anemoi_linear")), first


def test_capacity_drops_the_rest_and_changes_nothing(graph_o32, golden_cfg1_gt):
    model = _model(graph_o32, golden_cfg1_gt)
    x = golden_cfg1_gt["x"].to(DEV)
    with torch.no_grad():
        model(x)
        plain = model(x)
    _, full = _forward(model, x)
    y, t = _forward(model, x, capacity=2)
    assert torch.equal(y, plain)
    assert len(t.entries) == 2 and t.dropped == len(full.entries) - 2 > 0
    assert all(a.same_as(b) and a.nonfinite == b.nonfinite and a.absmax == b.absmax for a, b in zip(t.entries, full.entries))


def test_training_step_is_recorded_and_repeats(graph_o32, golden_cfg1_gt, monkeypatch):
    from anemoi_models_amd import trail
    from test_gpu_parity import _build

    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "bf16")
    gold = golden_cfg1_gt
    model, _ = _build(graph_o32, 64, 4)
    model.load_state_dict(split_prefix(gold, "sd."))
    model = model.to(DEV)
    x = gold["x"].to(DEV)
    dy = torch.randn(gold["y"].shape, generator=torch.Generator().manual_seed(2)).to(DEV)

    def step(armed):
        for p in model.parameters():
            p.grad = None
        if not armed:
            model(x).backward(dy)
            return None
        with trail.record(capacity=16384) as t:
            model(x).backward(dy)
        return t

    step(False)
    grads = {k: p.grad.clone() for k, p in model.named_parameters()}
    t1, t2 = step(True), step(True)
    assert all(torch.equal(p.grad, grads[k]) for k, p in model.named_parameters())  # the trail changes no gradient bit
    names = {n.split(":")[0] for n in t1.names()}
    print(f"training step: {len(t1.entries)} records; entry points: {sorted(names)}")
    assert t1.dropped == 0
    assert any("backward" in n for n in names), names
    assert names & {"anemoi_weight_grad_tn", "anemoi_linear_batched", "anemoi_col_sum"}, names
    assert trail.first_difference(t1, t2) is None
    assert t1.first_nonfinite() is None


def test_mark_adds_a_torch_side_tensor():
    from anemoi_models_amd import trail

    a = _seeded(torch.float32, 40, 24, 2).to(DEV)
    with trail.record(capacity=8) as t:
        b = torch.relu(a)  # an ATen op: invisible to the trail by itself
        trail.mark("relu(a)", b)
        trail.mark("a, 4-D", a.view(2, 20, 4, 6))
    assert [e.name for e in t.entries] == ["relu(a)", "a, 4-D"]
    assert t.entries[0].digest == trail.digest(b).digest == numpy_record(b.cpu())[0]
    assert (t.entries[1].rows, t.entries[1].cols) == (1, 960) and t.entries[1].digest == trail.digest(a).digest
    trail.mark("nothing armed", a)  # a no-op


def test_save_and_load_round_trip(tmp_path):
    from anemoi_models_amd import trail

    with trail.record(capacity=4) as t:
        trail.mark("x", _seeded(torch.bfloat16, 9, 9, 1).to(DEV))
    t.save(str(tmp_path / "t.json"))
    back = trail.load(str(tmp_path / "t.json"))
    assert back.entries == t.entries and back.dropped == 0 and trail.first_difference(t, back) is None


def test_record_under_graph_capture_is_refused_and_leaves_nothing_armed():
    from anemoi_models_amd import _lib, trail

    a = torch.ones(8, 8, device=DEV)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            with pytest.raises(NotImplementedError):
                with trail.record():
                    pass
            b = a * 2  # (something to capture)
    torch.cuda.current_stream().wait_stream(s)
    assert _lib.load().anemoi_trail_end(None, None) == _lib.ANEMOI_ERR_INVALID  # nothing was armed
    with trail.record(capacity=2) as t:  # and a trail can be armed afterwards
        trail.mark("a", a)
    assert len(t.entries) == 1
    del b


def test_record_disarms_on_an_exception():
    from anemoi_models_amd import _lib, trail

    with pytest.raises(ZeroDivisionError):
        with trail.record(capacity=2):
            1 / 0
    assert _lib.load().anemoi_trail_end(None, None) == _lib.ANEMOI_ERR_INVALID
