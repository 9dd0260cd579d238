"""The conditional LayerNorm, the device noise and the ensemble model on the HIP kernels (csrc/cond_layer_norm.hip):
anemoi_cond_layer_norm / _backward and anemoi_gaussian_noise against the restatements of tests/_cond_ln_ref.py, the
conditional Transformer block against an f64 torch restatement, and AnemoiEnsModelEncProcDec end to end."""

import numpy as np
import pytest
import torch

import _cond_ln_ref as cr
from test_gpu_parity import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"

F32_CASES = [(1, 64, 1), (5, 100, 5), (257, 512, 16), (33, 2048, 32), (7, 4096, 4)]
BF16_CASES = [(5, 100, 5), (257, 1024, 16), (33, 4096, 32), (4, 4104, 8)]
CASES = [(torch.float32, *c) for c in F32_CASES] + [(torch.bfloat16, *c) for c in BF16_CASES]
FWD_TOL = {torch.float32: 1e-5, torch.bfloat16: 1e-2}  # the project's LayerNorm bounds
GRAD_TOL = {torch.float32: 1e-4, torch.bfloat16: 3e-2}
NAMES = ("x", "cond", "ws", "bs", "wb", "bb")


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from anemoi_models_amd import _lib

    _lib.load()


def _inputs(dtype, rows, c, k, seed=0):
    """x and dy rounded to ``dtype`` (the reference sees what the kernel sees), weights of order 1 / sqrt K."""
    g = torch.Generator().manual_seed(1000 * seed + rows + c + k)
    t = {"x": (2.0 * torch.randn(rows, c, generator=g) + 0.5).to(dtype).float(), "cond": torch.randn(rows, k, generator=g),
         "ws": torch.randn(c, k, generator=g) / k**0.5, "bs": 0.1 * torch.randn(c, generator=g),
         "wb": torch.randn(c, k, generator=g) / k**0.5, "bb": 0.1 * torch.randn(c, generator=g)}
    dy = torch.randn(rows, c, generator=g).to(dtype).float()
    return t, dy


_REF = {}


def _reference(dtype, rows, c, k):
    """f64 forward and autograd gradients of the restatement, computed once per case."""
    key = (dtype, rows, c, k)
    if key not in _REF:
        t, dy = _inputs(dtype, rows, c, k)
        leaf = {n: v.double().requires_grad_() for n, v in t.items()}
        y = cr.cond_layer_norm(*(leaf[n] for n in NAMES))
        y.backward(dy.double())
        _REF[key] = (y.detach(), {n: leaf[n].grad for n in NAMES})
    return _REF[key]


def _device_args(dtype, t):
    return [t["x"].to(DEV, dtype)] + [t[n].to(DEV) for n in NAMES[1:]]


@pytest.mark.parametrize("dtype,rows,c,k", CASES)
def test_cond_layer_norm_forward_and_backward_vs_f64(dtype, rows, c, k):
    from anemoi_models_amd import autograd, ops

    t, dy = _inputs(dtype, rows, c, k)
    want_y, want_g = _reference(dtype, rows, c, k)
    args = [a.requires_grad_() for a in _device_args(dtype, t)]
    y = autograd.cond_layer_norm(*args, 1e-5)
    assert y.dtype == dtype and tuple(y.shape) == (rows, c)
    y.backward(dy.to(DEV, dtype))
    errs = {"y": rel_err(y.detach(), want_y)}
    errs.update({n: rel_err(a.grad, want_g[n]) for n, a in zip(NAMES, args)})
    print(f"cond_layer_norm {dtype} rows={rows} C={c} K={k}: " + ", ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    assert errs.pop("y") < FWD_TOL[dtype]
    for n, e in errs.items():
        assert e < GRAD_TOL[dtype], n
    # the no-grad kernel route gives the same bits, and the statistics are those of row_stats
    with torch.no_grad():
        y2, stats = ops.cond_layer_norm(*[a.detach() for a in args], 1e-5, with_stats=True)
        assert torch.equal(y2, y.detach())
        assert torch.equal(stats, ops.row_stats(args[0].detach().clone(), 1e-5))


@pytest.mark.parametrize("dtype,rows,c,k", CASES)
def test_zero_weights_are_the_plain_layer_norm_bit_for_bit(dtype, rows, c, k):
    from anemoi_models_amd import ops

    t, _ = _inputs(dtype, rows, c, k, seed=1)
    x, cond = t["x"].to(DEV, dtype), t["cond"].to(DEV)
    zw, zb = torch.zeros(c, k, device=DEV), torch.zeros(c, device=DEV)
    y, stats = ops.cond_layer_norm(x, cond, zw, zb, zw, zb, 1e-5, with_stats=True)
    assert torch.equal(y, ops.layer_norm(x, torch.ones(c, device=DEV), zb, 1e-5))
    assert torch.equal(stats, ops.row_stats(x.clone(), 1e-5))
    # a row-strided input (a column slice of a wider matrix) takes the same values
    wide = torch.zeros(rows, c + 8, dtype=dtype, device=DEV)
    wide[:, :c] = x
    assert torch.equal(ops.cond_layer_norm(wide[:, :c], cond, zw, zb, zw, zb, 1e-5), y)


@pytest.mark.parametrize("dtype,rows,c,k", [(torch.float32, 257, 512, 16), (torch.float32, 5, 100, 5),
                                            (torch.bfloat16, 257, 1024, 16)])
def test_fused_and_composed_routes_agree(dtype, rows, c, k):
    from anemoi_models_amd import autograd

    t, _ = _inputs(dtype, rows, c, k)
    want_y, _ = _reference(dtype, rows, c, k)
    args = _device_args(dtype, t)
    with torch.no_grad():
        fused, composed = autograd.cond_layer_norm(*args, 1e-5), autograd.cond_layer_norm_composed(*args, 1e-5)
    print(f"fused vs composed {dtype}: {rel_err(fused, composed):.2e}; composed vs f64 {rel_err(composed, want_y):.2e}")
    assert rel_err(fused, composed) < FWD_TOL[dtype]


def test_backward_is_deterministic():
    from anemoi_models_amd import ops

    for dtype, rows, c, k in [(torch.float32, 257, 512, 16), (torch.bfloat16, 257, 1024, 16), (torch.float32, 5, 100, 5)]:
        t, dy = _inputs(dtype, rows, c, k)
        x, cond, ws, bs, wb, bb = _device_args(dtype, t)
        _, stats = ops.cond_layer_norm(x, cond, ws, bs, wb, bb, 1e-5, with_stats=True)
        runs = [ops.cond_layer_norm_backward(dy.to(DEV, dtype), x, stats, cond, ws, bs, wb) for _ in range(2)]
        for a, b in zip(*runs):
            assert torch.equal(a, b)


def test_wide_condition_takes_the_composed_route():
    from anemoi_models_amd import autograd, ops

    rows, c, k = 40, 128, 33
    t, dy = _inputs(torch.float32, rows, c, k)
    leaf = {n: v.double().requires_grad_() for n, v in t.items()}
    want = cr.cond_layer_norm(*(leaf[n] for n in NAMES))
    want.backward(dy.double())
    args = [a.requires_grad_() for a in _device_args(torch.float32, t)]
    with pytest.raises(NotImplementedError, match="at most 32"):
        ops.cond_layer_norm(*[a.detach() for a in args], 1e-5)
    y = autograd.cond_layer_norm(*args, 1e-5)
    y.backward(dy.to(DEV))
    assert rel_err(y.detach(), want.detach()) < 1e-5
    for n, a in zip(NAMES, args):
        assert rel_err(a.grad, leaf[n].grad) < 1e-4, n


# ------------------------------------------------------------------------------------------------------------------ noise
def test_noise_is_a_function_of_seed_word_and_index():
    from anemoi_models_amd import ops
    from anemoi_models_amd.runtime import DeviceDropout

    n, k = 1000, 5
    a = ops.gaussian_noise(n, k, seed=7, device=DEV)
    assert a.dtype == torch.float32 and tuple(a.shape) == (n, k)
    assert torch.equal(a, ops.gaussian_noise(n, k, seed=7, device=DEV))
    assert torch.equal(ops.gaussian_noise(2 * n, k, seed=7, device=DEV)[:n], a)
    assert not torch.equal(ops.gaussian_noise(n, k, seed=8, device=DEV), a)
    assert torch.equal(ops.gaussian_noise(n, k, 0.25, seed=7, device=DEV), 0.25 * a)
    dd = DeviceDropout(DEV, start=3)
    b = ops.gaussian_noise(n, k, seed=7, seed_dev=dd.word)
    assert torch.equal(b, ops.gaussian_noise(n, k, seed=7, seed_dev=dd.word)) and not torch.equal(b, a)
    word = int(dd.word.item()) & 0xFFFFFFFF
    assert torch.equal(b, ops.gaussian_noise(n, k, seed=(7 + word) & 0xFFFFFFFF, device=DEV))
    dd.advance()
    assert not torch.equal(ops.gaussian_noise(n, k, seed=7, seed_dev=dd.word), b)
    want = cr.gaussian_noise(n, k, seed=7, word=word)
    err = float(np.abs(b.double().cpu().numpy() - want).max())
    print(f"noise vs f64 restatement: max abs err {err:.2e}")
    assert err < 1e-5


@pytest.mark.parametrize("seed", cr.NOISE_SEEDS)
def test_noise_values_and_moments(seed):
    """2^20 values at the seeds of the CPU test: every value within 1e-5 of the f64 restatement (accurate logf, sqrtf and
    sincospif are within a few ulp: about 1e-6 at |z| <= 5.77), and the 6 sigma moment bounds."""
    from anemoi_models_amd import ops

    z = ops.gaussian_noise(65536, 16, seed=seed, device=DEV).double().cpu().numpy()
    err = float(np.abs(z - cr.gaussian_noise(65536, 16, seed=seed)).max())
    print(f"noise seed {seed}: max abs err vs f64 {err:.2e}")
    assert err < 1e-5
    cr.check_moments(z, f"device, seed {seed}")


# ------------------------------------------------------------------------------------------------------------------ block
def _block_reference(sd, x, cond, heads):
    """The conditional Transformer block in f64 torch (attention: scaled_dot_product_attention on the CPU)."""
    def cln(h, p):
        return cr.cond_layer_norm(h, cond, sd[p + ".scale.weight"], sd[p + ".scale.bias"], sd[p + ".bias.weight"], sd[p + ".bias.bias"])

    s, c = x.shape
    qkv = cln(x, "layer_norm1") @ sd["attention.lin_qkv.weight"].T
    q, k, v = (t.reshape(s, heads, c // heads).transpose(0, 1) for t in qkv.chunk(3, dim=-1))
    a = torch.nn.functional.scaled_dot_product_attention(q[None], k[None], v[None])[0].transpose(0, 1).reshape(s, c)
    x = x + a @ sd["attention.projection.weight"].T + sd["attention.projection.bias"]
    h = torch.nn.functional.gelu(cln(x, "layer_norm2") @ sd["mlp.0.weight"].T + sd["mlp.0.bias"])
    return x + h @ sd["mlp.2.weight"].T + sd["mlp.2.bias"]


def test_conditional_transformer_block_vs_f64(monkeypatch):
    from anemoi_models_amd.layers.block import TransformerProcessorBlock

    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "fp32")
    torch.manual_seed(11)
    rows, c, heads, k = 96, 64, 4, 8
    block = TransformerProcessorBlock(c, 4 * c, heads, "GELU", 512, cond_dim=k)
    g = torch.Generator().manual_seed(12)
    with torch.no_grad():
        for ln in (block.layer_norm1, block.layer_norm2):
            for lin in (ln.scale, ln.bias):
                lin.weight.copy_(torch.randn(c, k, generator=g) / k**0.5)
                lin.bias.copy_(0.1 * torch.randn(c, generator=g))
    x, cond, dy = torch.randn(rows, c, generator=g), torch.randn(rows, k, generator=g), torch.randn(rows, c, generator=g)
    sd = {n: p.detach().double().requires_grad_() for n, p in block.named_parameters()}
    xr, cr_ = x.double().requires_grad_(), cond.double().requires_grad_()
    want = _block_reference(sd, xr, cr_, heads)
    want.backward(dy.double())
    block = block.to(DEV).train()
    xd, cd = x.to(DEV).requires_grad_(), cond.to(DEV).requires_grad_()
    y = block(xd, None, 1, cond=cd)
    y.backward(dy.to(DEV))
    errs = {"y": rel_err(y.detach(), want.detach()), "dx": rel_err(xd.grad, xr.grad), "dcond": rel_err(cd.grad, cr_.grad)}
    errs.update({n: rel_err(p.grad, sd[n].grad) for n, p in block.named_parameters()})
    print("conditional block f32: " + ", ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    assert errs.pop("y") < 1e-4 and errs.pop("dx") < 1e-4 and errs.pop("dcond") < 2e-4
    assert len(errs) == 15
    for n, e in errs.items():
        assert e < 2e-4, n
    with torch.no_grad():
        y2 = block.eval()(x.to(DEV), None, 1, cond=cond.to(DEV))
    assert rel_err(y2, want.detach()) < 1e-4


# ------------------------------------------------------------------------------------------------------------------ model
NOISE = {"noise_std": 1.0, "noise_channels_dim": 8, "noise_mlp_hidden_dim": 16}
N_MEMBERS = 3


def _ens_model(graph, seed=5, warm=True):
    from anemoi_models_amd.models import AnemoiEnsModelEncProcDec
    from anemoi_models_amd.utils.indices import SimpleDataIndices
    from anemoi_models_amd.utils.presets import model_config

    torch.manual_seed(seed)
    idx = SimpleDataIndices(n_prognostic=10, n_forcing=2, n_diagnostic=1)
    model = AnemoiEnsModelEncProcDec(model_config=model_config("Transformer", 64, 2, noise_injector=NOISE), data_indices=idx,
                                     graph_data=graph)
    if warm:  # non-zero conditional weights: a fresh model has zero ones and its members would stay equal
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            for n, p in model.named_parameters():
                if ".scale." in n or (".bias." in n and "layer_norm" in n):
                    p.copy_(0.3 * torch.randn(p.shape, generator=g))
    n = graph["data"].num_nodes
    x = torch.randn(1, 2, 1, n, idx.num_input, generator=torch.Generator().manual_seed(seed + 2)).repeat(1, 1, N_MEMBERS, 1, 1)
    return model.to(DEV), idx, x.to(DEV)


def test_ensemble_model_members_differ_and_repeat_with_the_seed(graph_o32, monkeypatch):
    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "fp32")
    model, idx, x = _ens_model(graph_o32)
    model.eval()
    with torch.no_grad():
        torch.manual_seed(77)
        y = model(x)
        torch.manual_seed(77)
        again = model(x)
        other = model(x)
    assert tuple(y.shape) == (1, N_MEMBERS, x.shape[3], model.num_output_channels) and bool(torch.isfinite(y).all())
    for a in range(N_MEMBERS):
        for b in range(a + 1, N_MEMBERS):
            assert not torch.equal(y[0, a], y[0, b]) and rel_err(y[0, a], y[0, b]) > 1e-3
    assert torch.equal(y, again) and not torch.equal(y, other)
    # the training route draws members that differ as well
    model.train()
    torch.manual_seed(77)
    yt = model(x)
    assert not torch.equal(yt[0, 0], yt[0, 1]) and not torch.equal(yt[0, 1], yt[0, 2])


def test_ensemble_model_with_zero_conditional_weights_is_the_base_model(graph_o32, monkeypatch):
    from anemoi_models_amd.models import AnemoiModelEncProcDec
    from anemoi_models_amd.utils.presets import model_config

    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "fp32")
    model, idx, x = _ens_model(graph_o32, warm=False)
    base = AnemoiModelEncProcDec(model_config=model_config("Transformer", 64, 2), data_indices=idx, graph_data=graph_o32)
    shared = {k: v for k, v in model.state_dict().items() if not k.startswith("noise_injector.") and "layer_norm" not in k}
    missing, unexpected = base.load_state_dict(shared, strict=False)
    assert not unexpected and missing and all("layer_norm" in k for k in missing)  # the default LayerNorms: gamma 1, beta 0
    base = base.to(DEV).eval()
    model.eval()
    with torch.no_grad():
        y = model(x)
        want = base(x.transpose(0, 2)).transpose(0, 1)  # (the members as the batch of the deterministic model)
        single = torch.cat([base(x[:, :, m:m + 1]) for m in range(N_MEMBERS)], dim=1)  # and member by member, one at a time
    assert torch.equal(y[0, 0], y[0, 1])  # zero conditional weights: the noise reaches nothing
    print(f"zero conditional weights vs the base model: {rel_err(y, want):.2e}, member by member {rel_err(y, single):.2e}")
    assert rel_err(y, want) < 1e-5 and rel_err(y, single) < 1e-5
    # the training route of the base model takes [1, T, E, G, V] as it is: the same members in the same places
    base.train()
    model.train()
    yt, wt = model(x).detach(), base(x).detach()
    assert tuple(yt.shape) == tuple(wt.shape) == tuple(y.shape)
    print(f"training route, zero conditional weights vs base(x): {rel_err(yt, wt):.2e}; vs the inference route {rel_err(yt, y):.2e}")
    assert rel_err(yt, wt) < 1e-5 and rel_err(yt, y) < 1e-4
    # distinct members stay where they are put (a transposed or re-ordered ensemble axis would show here)
    xd = x.clone()
    xd[:, :, 1] += 0.5
    xd[:, :, 2] -= 0.25
    model.eval()
    base.eval()
    with torch.no_grad():
        yd = model(xd)
        for m in range(N_MEMBERS):
            assert rel_err(yd[:, m:m + 1], base(xd[:, :, m:m + 1])) < 1e-5, m


def test_ensemble_model_noise_is_reproducible_from_the_seed(graph_o32, monkeypatch):
    from anemoi_models_amd import ops

    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "fp32")
    model, idx, x = _ens_model(graph_o32)
    model.train()
    seen = {}
    handle = model.processor.register_forward_pre_hook(lambda m, a, kw: seen.update(cond=kw["cond"].detach().clone()),
                                                       with_kwargs=True)
    torch.manual_seed(123)
    model(x)
    handle.remove()
    torch.manual_seed(123)
    seed = model.noise_injector.next_seed()
    n_mesh = graph_o32["hidden"].num_nodes
    z = ops.gaussian_noise(N_MEMBERS * n_mesh, NOISE["noise_channels_dim"], NOISE["noise_std"], seed=seed, device=DEV)
    mlp = model.noise_injector.noise_mlp
    with torch.no_grad():
        want = torch.nn.functional.linear(torch.nn.functional.gelu(torch.nn.functional.linear(
            z.double(), mlp[0].weight.double(), mlp[0].bias.double())), mlp[2].weight.double(), mlp[2].bias.double())
    assert tuple(seen["cond"].shape) == (N_MEMBERS * n_mesh, NOISE["noise_channels_dim"]) and seen["cond"].dtype == torch.float32
    assert rel_err(seen["cond"], want) < 1e-4
    assert np.abs(z.double().cpu().numpy() - cr.gaussian_noise(N_MEMBERS * n_mesh, 8, seed=seed)).max() < 1e-5


def _crps(graph, model):
    from anemoi_models_amd import AlmostFairKernelCRPS

    g = torch.Generator().manual_seed(3)
    return AlmostFairKernelCRPS(torch.rand(graph["data"].num_nodes, generator=g) + 0.1,
                                torch.rand(model.num_output_channels, generator=g) + 0.5, alpha=0.95).to(DEV)


def test_ensemble_training_step_reaches_the_noise_parameters(graph_o32, monkeypatch):
    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "fp32")
    model, idx, x = _ens_model(graph_o32)
    model.train()
    loss_fn = _crps(graph_o32, model)
    target = torch.randn(1, x.shape[3], model.num_output_channels, generator=torch.Generator().manual_seed(4)).to(DEV)
    torch.manual_seed(9)
    loss = loss_fn(model(x), target)
    loss.backward()
    assert bool(torch.isfinite(loss.detach())) and float(loss.detach()) > 0
    checked = 0
    for n, p in model.named_parameters():
        if n.startswith("noise_injector.") or ("layer_norm" in n and (".scale." in n or ".bias." in n)):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, n
            checked += 1
    assert checked == 4 + 2 * 2 * 4  # noise_mlp, and scale / bias Linears of the two LayerNorms of the two blocks


def test_graphed_ensemble_train_step_draws_new_noise_and_equals_eager(graph_o32, monkeypatch):
    """GraphedTrainStep opens its DeviceDropout context for the noise (the model has no dropout): two replays on the same batch
    give different losses, and equal, bit for bit, the two eager steps inside a DeviceDropout context started at the same
    counter (the pattern of test_graphed_train_step_with_attention_dropout_equals_eager)."""
    from anemoi_models_amd.runtime import DeviceDropout, GraphedTrainStep

    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "fp32")
    model, idx, x = _ens_model(graph_o32)
    model.train()
    loss_fn = _crps(graph_o32, model)
    target = torch.randn(1, x.shape[3], model.num_output_channels, generator=torch.Generator().manual_seed(4)).to(DEV)
    step = GraphedTrainStep(model, loss_fn, x, target)
    assert step.dropout is not None
    params = [p for p in model.parameters() if p.requires_grad]
    step.dropout.counter.fill_(100)
    graphed = []
    for _ in range(2):
        loss = step(x, target)
        graphed.append((loss.clone(), [p.grad.clone() for p in params]))
    assert int(step.dropout.counter.item()) == 102
    assert not torch.equal(graphed[0][0], graphed[1][0])
    with DeviceDropout(DEV, start=100) as dd:
        for g_loss, g_grads in graphed:
            for p in params:
                p.grad = None
            dd.advance()
            loss = loss_fn(model(x), target)
            loss.backward()
            assert torch.equal(loss.detach(), g_loss)
            for p, gg in zip(params, g_grads):
                assert torch.equal(p.grad, gg)


def test_capturing_a_forward_without_device_dropout_raises(graph_o32, monkeypatch):
    """A captured forward would replay the seed it was captured with: the noise refuses to be drawn while a stream is capturing
    and no DeviceDropout context is active (the error is caught inside the capture, which then ends in order)."""
    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "fp32")
    model, idx, x = _ens_model(graph_o32)
    model.eval()
    caught = []
    with torch.no_grad():
        model(x)  # (plans, packed weights: nothing is built for the first time inside the capture)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            try:
                model(x)
            except RuntimeError as e:
                caught.append(str(e))
    assert len(caught) == 1 and "DeviceDropout" in caught[0]
