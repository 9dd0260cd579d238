"""The conditional LayerNorm, the noise generator and the ensemble model, the parts that need no GPU: the f64 restatement
(tests/_cond_ln_ref.py) against the composed torch form, the argument checks of the three entry points through the C ABI, the
backward workspace as a function of its arguments, the state dicts of the new modules, what the ensemble model refuses, and the
moments of the restated generator at the seeds the GPU test uses."""

import numpy as np
import pytest
import torch

import _cond_ln_ref as cr


def test_restatement_against_the_composed_torch_form():
    g = torch.Generator().manual_seed(3)
    for rows, c, k in [(1, 64, 1), (5, 100, 5), (33, 256, 32)]:
        x = (2.0 * torch.randn(rows, c, generator=g) + 0.5).double()
        cond = torch.randn(rows, k, generator=g).double()
        ws, wb = (torch.randn(c, k, generator=g).double() / k**0.5 for _ in range(2))
        bs, bb = (0.1 * torch.randn(c, generator=g).double() for _ in range(2))
        want = torch.nn.functional.layer_norm(x, (c,), None, None, 1e-5) * (1 + torch.nn.functional.linear(cond, ws, bs)) \
            + torch.nn.functional.linear(cond, wb, bb)
        got = cr.cond_layer_norm(x, cond, ws, bs, wb, bb, 1e-5)
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
        zero = torch.zeros_like(ws)
        plain = cr.cond_layer_norm(x, cond, zero, torch.zeros_like(bs), zero, torch.zeros_like(bb), 1e-5)
        assert float((plain - torch.nn.functional.layer_norm(x, (c,), None, None, 1e-5)).abs().max()) <= 1e-13


def test_cond_layer_norm_entry_points_validate_without_gpu():
    """Null pointers, K = 0, K = 33, leading dimensions below C, a condition or weights not padded to 4 / 8 / 16 / 32 columns,
    misaligned pointers, a short workspace, and the shapes of the
    noise come back as status codes with a message before anything is launched."""
    from anemoi_models_amd import _lib

    lib = _lib.load()
    bad, unsup, ok, p = _lib.ANEMOI_ERR_INVALID, _lib.ANEMOI_ERR_UNSUPPORTED, _lib.ANEMOI_OK, 4096  # p: never dereferenced here
    assert _lib.ABI_VERSION >= 51 and _lib.COND_LN_MAX_K == 32
    fwd, bwd, noise = lib.anemoi_cond_layer_norm, lib.anemoi_cond_layer_norm_backward, lib.anemoi_gaussian_noise
    assert [_lib.cond_ln_padded_k(k) for k in (1, 4, 5, 8, 9, 16, 17, 32)] == [4, 4, 8, 8, 16, 16, 32, 32]

    def f(x=p, ldx=64, cond=p, ldc=4, k=4, ws=p, ldw=4, bs=p, wb=p, bb=p, y=p, ldy=64, stats=p, rows=8, c=64, dtype=0):
        return fwd(dtype, x, ldx, cond, ldc, k, ws, ldw, bs, wb, bb, y, ldy, stats, rows, c, 1e-5, None)

    assert f(x=None) == bad and b"anemoi_cond_layer_norm: null pointer" in lib.anemoi_last_error()
    for name in ("cond", "ws", "bs", "wb", "bb", "y"):
        assert f(**{name: None}) == bad
    for k in (0, -1):
        assert f(k=k) == bad and b"at least one column" in lib.anemoi_last_error()
    assert f(k=33, ldc=64, ldw=64) == unsup and b"K = 33 condition columns, at most 32" in lib.anemoi_last_error()
    assert f(ldx=63) == bad and b"bad shape" in lib.anemoi_last_error()
    assert f(ldy=63) == bad and f(c=0) == bad and f(rows=-1) == bad
    assert f(stats=p + 4) == bad and b"8-byte aligned" in lib.anemoi_last_error()
    # K is padded to 4, 8, 16 or 32 columns by the caller: leading dimensions below that, odd ones, misaligned pointers
    assert f(k=5, ldc=5, ldw=8) == bad and b"padded to 8 columns" in lib.anemoi_last_error()
    assert f(k=5, ldc=8, ldw=5) == bad and f(k=17, ldc=32, ldw=24) == bad and f(k=3, ldc=6, ldw=4) == bad
    assert f(cond=p + 4) == bad and b"16-byte aligned" in lib.anemoi_last_error()
    assert f(ws=p + 8) == bad and f(wb=p + 4) == bad
    assert f(dtype=7) == unsup and b"dtype 7" in lib.anemoi_last_error()
    assert f(stats=None, rows=0) == ok and f(k=5, ldc=8, ldw=12, rows=0) == ok  # no rows: nothing to do (stats optional)
    ws_n = lib.anemoi_cond_layer_norm_backward_workspace_floats(8, 64, 4)

    def g(dy=p, ldd=64, x=p, ldx=64, stats=p, cond=p, ldc=4, k=4, ws=p, ldw=4, bs=p, wb=p, dx=p, ldo=64, dcond=p, dws=p, dbs=p,
          dwb=p, dbb=p, rows=8, c=64, work=p, n=ws_n, dtype=0):
        return bwd(dtype, dy, ldd, x, ldx, stats, cond, ldc, k, ws, ldw, bs, wb, dx, ldo, dcond, dws, dbs, dwb, dbb, rows, c, work,
                   n, None)

    assert g(dy=None) == bad and b"anemoi_cond_layer_norm_backward: null pointer" in lib.anemoi_last_error()
    assert g(dws=None) == bad and b"gradient outputs" in lib.anemoi_last_error()
    assert g(k=0) == bad and g(k=33, ldc=64, ldw=64, n=1 << 30) == unsup
    assert g(ldd=63) == bad and g(ldx=63) == bad and g(ldo=63) == bad and b"bad shape" in lib.anemoi_last_error()
    assert g(stats=p + 4) == bad
    assert g(k=5, ldc=5, ldw=8, n=1 << 20) == bad and b"padded to 8 columns" in lib.anemoi_last_error()
    assert g(ws=p + 4) == bad and b"16-byte aligned" in lib.anemoi_last_error()
    assert g(n=ws_n - 1) == bad and b"workspace" in lib.anemoi_last_error()
    assert g(work=None) == bad and g(dtype=7) == unsup
    #            out rows K std seed seed_dev stream
    assert noise(None, 8, 4, 1.0, 1, None, None) == bad and b"anemoi_gaussian_noise: null pointer" in lib.anemoi_last_error()
    assert noise(p, -1, 4, 1.0, 1, None, None) == bad and noise(p, 8, 0, 1.0, 1, None, None) == bad
    assert noise(p, 8, 4, -1.0, 1, None, None) == bad and b"std" in lib.anemoi_last_error()
    assert noise(p, 8, 4, 1.0, 1, p + 2, None) == bad and b"4-byte aligned" in lib.anemoi_last_error()
    assert noise(p, 0, 4, 1.0, 1, None, None) == ok


def test_cond_layer_norm_backward_workspace_is_a_function_of_its_arguments():
    """One [2 K + 2, C] partial per chunk of rows; the number of chunks depends on ``rows`` alone, is 1 for few rows and
    saturates at 128: the order of the column sums cannot change with the device or the occupancy."""
    from anemoi_models_amd import _lib

    ws = _lib.load().anemoi_cond_layer_norm_backward_workspace_floats
    assert ws(0, 64, 4) == 0 and ws(8, 0, 4) == 0 and ws(8, 64, 0) == 0 and ws(8, 64, 33) == 0
    assert ws(1, 64, 1) == 4 * 64 and ws(64, 100, 5) == 12 * 100 and ws(65, 100, 5) == 2 * 12 * 100
    for rows in (1, 64, 65, 257, 40962, 4 * 40962, 10**7):
        chunks = ws(rows, 1, 1) // 4
        assert 1 <= chunks <= 128 and chunks <= max(1, (rows + 63) // 64)
        for c, k in [(64, 1), (1024, 16), (4104, 32)]:
            assert ws(rows, c, k) == chunks * (2 * k + 2) * c
    # chunks of max(64, ceil(rows / 128)) rows, rounded up to a multiple of 8: 257 -> 64 -> 5 chunks; 40 962 -> 321 -> 328 -> 125
    assert ws(257, 1, 1) // 4 == 5 and ws(40962, 1, 1) // 4 == 125 and ws(10**7, 1, 1) // 4 == 128


def test_conditional_layer_norm_state_dict_and_zero_init():
    from anemoi_models_amd.layers.normalization import ConditionalLayerNorm

    ln = ConditionalLayerNorm(48, 6)
    assert list(ln.state_dict()) == ["scale.weight", "scale.bias", "bias.weight", "bias.bias"]
    assert tuple(ln.scale.weight.shape) == (48, 6) and tuple(ln.bias.bias.shape) == (48,) and ln.eps == 1e-5
    assert all(float(t.abs().max()) == 0.0 for t in ln.state_dict().values())
    warm = ConditionalLayerNorm(48, 6, zero_init=False, eps=1e-6)
    assert float(warm.scale.weight.detach().abs().max()) > 0 and warm.eps == 1e-6
    with pytest.raises(ValueError):
        ln(torch.zeros(4, 48), torch.zeros(4, 5))


def test_transformer_block_without_cond_dim_keeps_its_state_dict():
    from anemoi_models_amd.layers.block import TransformerProcessorBlock
    from anemoi_models_amd.layers.chunk import TransformerProcessorChunk
    from anemoi_models_amd.layers.normalization import ConditionalLayerNorm
    from anemoi_models_amd.layers.processor import TransformerProcessor

    before = ["layer_norm1.weight", "layer_norm1.bias", "attention.lin_qkv.weight", "attention.projection.weight",
              "attention.projection.bias", "mlp.0.weight", "mlp.0.bias", "mlp.2.weight", "mlp.2.bias", "layer_norm2.weight",
              "layer_norm2.bias"]
    plain = TransformerProcessorBlock(64, 256, 4, "GELU", 512)
    assert list(plain.state_dict()) == before and plain.cond_dim is None and type(plain.layer_norm1) is torch.nn.LayerNorm
    cond = TransformerProcessorBlock(64, 256, 4, "GELU", 512, cond_dim=8)
    assert isinstance(cond.layer_norm1, ConditionalLayerNorm) and isinstance(cond.layer_norm2, ConditionalLayerNorm)
    want = [k for k in before if not k.startswith("layer_norm")]
    for ln in ("layer_norm1", "layer_norm2"):
        want += [f"{ln}.{p}" for p in ("scale.weight", "scale.bias", "bias.weight", "bias.bias")]
    assert sorted(cond.state_dict()) == sorted(want)
    assert cond._block_abi(torch.zeros(8, 64), 1) is None  # op by op: the block-level entry point has no conditional LayerNorm
    with pytest.raises(ValueError, match="cond_dim"):
        cond(torch.zeros(8, 64), None, 1)
    with pytest.raises(ValueError, match="cond_dim"):
        plain(torch.zeros(8, 64), None, 1, cond=torch.zeros(8, 8))

    class Group:
        def size(self):
            return 2

    with pytest.raises(NotImplementedError, match="model communication group"):
        cond(torch.zeros(8, 64), None, 1, Group(), cond=torch.zeros(8, 8))
    chunk = TransformerProcessorChunk(64, 2, 512, num_heads=4)
    assert list(chunk.state_dict()) == [f"blocks.{i}.{k}" for i in range(2) for k in before]
    proc = TransformerProcessor(2, num_channels=64, num_chunks=1, num_heads=4, window_size=512, cond_dim=8)
    assert all(isinstance(b.layer_norm2, ConditionalLayerNorm) for ch in proc.proc for b in ch.blocks)
    with pytest.raises(NotImplementedError, match="model communication group"):
        proc(torch.zeros(8, 64), 1, None, Group(), cond=torch.zeros(8, 8))


NOISE = {"noise_std": 1.0, "noise_channels_dim": 8, "noise_mlp_hidden_dim": 16}


def test_ensemble_model_construction_and_refusals(graph_o32):
    import anemoi_models_amd.models as models
    from anemoi_models_amd.layers.ensemble import NoiseConditioning
    from anemoi_models_amd.utils.indices import SimpleDataIndices
    from anemoi_models_amd.utils.presets import model_config

    assert "AnemoiEnsModelEncProcDec" in models.__all__
    idx = SimpleDataIndices(n_prognostic=10, n_forcing=2, n_diagnostic=1)
    assert "noise_injector" not in model_config("Transformer", 64, 2)["model"]  # every existing call: unchanged
    for proc in ("GraphTransformer", "GNN"):
        with pytest.raises(NotImplementedError, match="Transformer processor"):
            models.AnemoiEnsModelEncProcDec(model_config=model_config(proc, 64, 2, noise_injector=NOISE), data_indices=idx,
                                            graph_data=graph_o32)
    with pytest.raises(ValueError, match="noise_injector"):
        models.AnemoiEnsModelEncProcDec(model_config=model_config("Transformer", 64, 2), data_indices=idx, graph_data=graph_o32)
    model = models.AnemoiEnsModelEncProcDec(model_config=model_config("Transformer", 64, 2, noise_injector=NOISE),
                                            data_indices=idx, graph_data=graph_o32)
    assert isinstance(model, models.AnemoiModelEncProcDec) and isinstance(model.noise_injector, NoiseConditioning)
    keys = list(model.state_dict())
    assert [k for k in keys if k.startswith("noise_injector.")] == [
        f"noise_injector.noise_mlp.{i}.{p}" for i in (0, 2) for p in ("weight", "bias")]
    assert tuple(model.noise_injector.noise_mlp[0].weight.shape) == (16, 8)
    assert tuple(model.noise_injector.noise_mlp[2].weight.shape) == (8, 16)
    assert sum(k.endswith("scale.weight") for k in keys) == 4 and "processor.proc.0.blocks.0.layer_norm1.bias.bias" in keys
    assert NoiseConditioning(1.0, 8, 16, inject_noise=False)(10, "cpu", torch.float32) is None

    class Group:
        def size(self):
            return 2

    with pytest.raises(NotImplementedError, match="model communication group"):
        model(torch.zeros(1, 2, 3, graph_o32["data"].num_nodes, idx.num_input), Group())
    with pytest.raises(NotImplementedError, match="batch size 1"):
        model(torch.zeros(2, 2, 3, graph_o32["data"].num_nodes, idx.num_input))


def test_philox_restatement_on_the_published_vectors():
    """Random123's known-answer tests of philox4x32-10: the zero counter and key, all ones, and the digits of pi."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF, 0xFFFFFFFF), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
            (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in kat:
        got = cr.philox4x32_10(*(np.array([c], dtype=np.uint64) for c in ctr), *key)
        assert tuple(int(w[0]) for w in got) == want


@pytest.mark.parametrize("seed", cr.NOISE_SEEDS)
def test_restated_generator_moments(seed):
    """2^20 values (rows = 65 536, K = 16) of the restated generator inside the 6 sigma bounds of iid normals; the first rows of
    a longer draw are the shorter draw; another seed or device word gives another draw."""
    z = cr.gaussian_noise(65536, 16, seed=seed)
    cr.check_moments(z, f"restatement, seed {seed}")
    assert np.array_equal(cr.gaussian_noise(100, 16, seed=seed), z[:100])
    assert np.array_equal(cr.gaussian_noise(7, 5, seed=seed).reshape(-1), cr.gaussian_noise(35, 1, seed=seed).reshape(-1))
    assert not np.array_equal(cr.gaussian_noise(100, 16, seed=seed + 1), z[:100])
    assert np.array_equal(cr.gaussian_noise(100, 16, seed=seed, word=5), cr.gaussian_noise(100, 16, seed=seed + 5))
    assert np.array_equal(cr.gaussian_noise(4, 4, 0.5, seed=seed), 0.5 * z[:1].reshape(4, 4))
