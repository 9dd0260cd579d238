"""The raw-row encoder route on the GPU: ``anemoi_gt_edge_attention_raw`` against the torch
restatement (tests/_raw_rows_ref.py), with the existing folded kernel on the same problem as the yardstick of the error;
the route in the model against the switch-off route and the CPU oracle; launch coverage."""

import pytest
import torch

from _raw_rows_ref import degree_graph, kernel_reference
from oracle import reference_path as ref
from test_oracle_golden import graph_tensors

pytestmark = pytest.mark.gpu

DEV = "cuda"


def rel_err(got, want):
    got, want = got.double().cpu(), want.double().cpu()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("ks,d,up", [(256, 64, 4), (128, 64, 4), (64, 32, 8), (256, 64, 16)])
def test_raw_row_kernel_against_restatement_and_folded_kernel(ks, d, up):
    """One attention problem, two routes, one reference.  Inputs: bf16 q, raw rows x, f32 rstd, f32 operators A_k, A_v.
    Reference (f64 on those inputs): sum_j alpha_ij v_j and t.  Old route: k | v = bf16(rstd A x + b) as the k|v GEMM leaves
    them, the folded kernel.  New route: qt = bf16(A_k^T q), the raw-row kernel, bf16(A_v g).  The new route rounds qt and
    g where the old one rounds k and v: its error must stay within 2 x the old route's, measured here on the same inputs
    (in-degrees 0 / 1 / 104 among them)."""
    from anemoi_models_amd import ops

    h, c = 16, 16 * d
    gen = torch.Generator().manual_seed(ks + up)
    degrees = [0, 1, 104, 16, 17, 3, 0, 32, 15, 1, 64, 9] + [int(v) for v in torch.randint(0, 40, (53,), generator=gen)]
    n_src, k_in, sum_col = 301, ks - 9, ks - 1
    rowptr, col, _ = degree_graph(degrees, n_src, ks)
    n_dst, e = len(degrees), int(rowptr[-1])
    rnd = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    x = torch.zeros(n_src, ks)
    x[:, :k_in], x[:, k_in] = rnd(n_src, k_in), 1.0
    x = x.bfloat16()
    rstd = (0.5 + torch.rand(n_src, generator=gen)) / k_in**0.5
    a_k, a_v = rnd(h, d, ks), rnd(h, d, ks)
    a_k[:, :, k_in + 1:], a_v[:, :, k_in + 1:] = 0.0, 0.0
    b_v = rnd(h, d)
    q = rnd(n_dst, h, d).bfloat16()
    u = rnd(n_dst, h, up).bfloat16()
    attr = rnd(e, up)
    attr[:, up - 1] = 1.0
    stats = torch.stack([rstd, torch.zeros(n_src)], dim=1).contiguous()

    # reference in f64 on the same inputs
    xd, qd = x.double(), q.double()
    qt64 = torch.einsum("hdk,nhd->nhk", a_k.double(), qd)
    g64, t64 = kernel_reference(qt64, xd, rstd.double(), u.double(), attr.double(), rowptr, col, d, sum_col)
    av1 = a_v.double().clone()
    av1[:, :, sum_col] = b_v.double()
    want = torch.einsum("hdk,nhk->nhd", av1, g64).reshape(n_dst, c)

    # old route: k | v as the GEMM leaves them (f32 accumulate, one rounding), the folded kernel
    kk = (rstd[:, None, None] * torch.einsum("hdk,nk->nhd", a_k, x.float())).reshape(n_src, c).bfloat16()
    vv = (rstd[:, None, None] * torch.einsum("hdk,nk->nhd", a_v, x.float()) + b_v[None]).reshape(n_src, c).bfloat16()
    dev = lambda t: t.to(DEV).contiguous()  # noqa: E731
    old = ops.gt_edge_attention_folded(dev(q.reshape(n_dst, c)), dev(kk), dev(vv), None, dev(u.reshape(n_dst, h * up)),
                                       dev(attr), dev(rowptr), dev(col), h, up)
    err_old, err_old_t = rel_err(old[:, :c], want), rel_err(old[:, c:c + h * up], t64.reshape(n_dst, h * up))

    # new route
    qt = torch.einsum("hdk,nhd->nhk", a_k, q.float()).reshape(n_dst, h * ks).bfloat16()
    t_new = torch.zeros(n_dst, h * up, dtype=torch.bfloat16, device=DEV)
    g = ops.gt_edge_attention_raw(dev(qt), dev(x), dev(stats), dev(u.reshape(n_dst, h * up)), dev(attr), dev(rowptr),
                                  dev(col), h, d, up, sum_col, t_new)
    g2 = ops.gt_edge_attention_raw(dev(qt), dev(x), dev(stats), dev(u.reshape(n_dst, h * up)), dev(attr), dev(rowptr),
                                   dev(col), h, d, up, sum_col, torch.zeros_like(t_new))
    assert torch.equal(g, g2)  # run-to-run bit-identical
    # the kernel itself against its restatement on ITS inputs (the rounded qt)
    gk, tk = kernel_reference(qt.double().view(n_dst, h, ks), xd, rstd.double(), u.double(), attr.double(), rowptr, col, d,
                              sum_col)
    err_kernel = rel_err(g, gk.reshape(n_dst, h * ks))
    av1f = a_v.clone()
    av1f[:, :, sum_col] = b_v
    new = torch.einsum("hdk,nhk->nhd", av1f, g.float().cpu().view(n_dst, h, ks)).reshape(n_dst, c).bfloat16()
    err_new, err_new_t = rel_err(new, want), rel_err(t_new, t64.reshape(n_dst, h * up))
    print(f"Ks={ks} D={d} up={up}: sum alpha v -- folded kernel {err_old:.3e}, raw-row route {err_new:.3e}; "
          f"t -- folded {err_old_t:.3e}, raw-row {err_new_t:.3e}; raw-row kernel vs its own restatement (g) {err_kernel:.3e}")
    iso = [i for i, dg in enumerate(degrees) if dg == 0]
    assert not g[iso].any() and not t_new[iso].any()
    assert err_new <= 2 * err_old and err_new_t <= 2 * err_old_t


def _model(graph_name, channels, layers, n_prog=20, n_forc=4, n_diag=2):
    from anemoi_models_amd.graphs.synthetic import build_graph
    from anemoi_models_amd.models import AnemoiModelEncProcDec
    from anemoi_models_amd.utils.indices import SimpleDataIndices
    from anemoi_models_amd.utils.presets import model_config

    graph = build_graph(graph_name)
    idx = SimpleDataIndices(n_prognostic=n_prog, n_forcing=n_forc, n_diagnostic=n_diag)
    torch.manual_seed(1234)
    model = AnemoiModelEncProcDec(model_config=model_config("GraphTransformer", channels, layers, 16), data_indices=idx,
                                  graph_data=graph)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("trainable"):
                p.normal_(0.0, 0.1)
    model.eval()
    x = torch.randn(1, 2, 1, graph["data"].num_nodes, idx.num_input, generator=torch.Generator().manual_seed(7))
    return model, x, graph, n_prog


def test_config2_encoder_latent_route_on_vs_off_vs_oracle(monkeypatch):
    """Config 2 (O96 -> ico-5, 512 channels; 2 processor blocks: the latent is taken in front of them).  The encoder latent
    with the route on must be no further from the f32 CPU oracle than 1.5 x the switch-off route's own distance; two
    identical forwards are bit-identical; the switch restores the other route's bits."""
    import bench

    model, x, graph, n_prog = _model("o96_ico5", 512, 2)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        want, stages = ref.model_forward(sd, graph_tensors(graph), x, num_heads=16, num_layers=2, num_chunks=2,
                                         prognostic_in=range(n_prog), prognostic_out=range(n_prog), return_stages=True)
    model, x = model.to(DEV), x.to(DEV)
    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "bf16")
    monkeypatch.setenv("ANEMOI_AMD_EDGE_RAW", "0")
    y_off, lat_off = bench.device_forward_with_latent(model, x)
    monkeypatch.setenv("ANEMOI_AMD_EDGE_RAW", "1")
    y_on, lat_on = bench.device_forward_with_latent(model, x)
    y_on2, lat_on2 = bench.device_forward_with_latent(model, x)
    monkeypatch.setenv("ANEMOI_AMD_EDGE_RAW", "0")
    y_off2, lat_off2 = bench.device_forward_with_latent(model, x)
    e_off, e_on = rel_err(lat_off, stages["x_latent"]), rel_err(lat_on, stages["x_latent"])
    p_off, p_on = rel_err(y_off, want), rel_err(y_on, want)
    print(f"config-2 encoder latent vs f32 oracle: route off {e_off:.3e}, route on {e_on:.3e}; prediction: off {p_off:.3e}, "
          f"on {p_on:.3e}")
    assert not torch.equal(lat_on, lat_off), "the switch changed nothing: the raw-row route did not run"
    assert torch.equal(lat_on, lat_on2) and torch.equal(y_on, y_on2)
    assert torch.equal(lat_off, lat_off2) and torch.equal(y_off, y_off2)
    assert e_on <= 1.5 * e_off


def test_config1_graph_launch_coverage(monkeypatch):
    """With the route on, a forward on config 1's graph records no k | v Linear over the encoder's source rows (the
    statistics product of their LayerNorm stays) and exactly one raw-row edge launch; with it off, the k | v product is
    back.  256 channels instead of config 1's 64: at 64 the mapper does not fold the embedding of its 2 x 12 + ... input
    columns (``2 (k_in + 1) > channels``), the sources are no ``EmbeddedRows`` and neither route exists."""
    from anemoi_models_amd import ops

    channels = 256
    model, x, graph, _ = _model("o32_ico2", channels, 2, n_prog=10, n_forc=2, n_diag=1)
    model, x = model.to(DEV), x.to(DEV)
    monkeypatch.setenv("ANEMOI_AMD_DTYPE", "bf16")
    n_src = graph["data"].num_nodes

    def launches(flag):
        monkeypatch.setenv("ANEMOI_AMD_EDGE_RAW", flag)
        with torch.no_grad():
            model(x)  # (packed weights, plans)
            ops.PROFILE = []
            try:
                model(x)
            finally:
                records, ops.PROFILE = ops.PROFILE, None
        torch.cuda.synchronize()
        kv = [w for name, _, _, w in records if name == "linear" and w.get("m") == n_src and w.get("n") == 2 * channels]
        raw = [w for name, _, _, w in records if name == "gt_edge_attention" and "raw_rows" in w]
        return kv, raw

    kv_on, raw_on = launches("1")
    kv_off, raw_off = launches("0")
    print(f"config 1: route on -- k|v launches {len(kv_on)}, raw-row edge launches {len(raw_on)}; off -- {len(kv_off)}, {len(raw_off)}")
    assert len(kv_on) == 0 and len(raw_on) == 1 and raw_on[0]["n_src"] == n_src
    assert len(kv_off) == 1 and len(raw_off) == 0
