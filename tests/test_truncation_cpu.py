"""Host side of the truncated residual connection (no GPU): CSR transpose, the numpy-only ``.npz`` reader, canonicalisation, the
``state_dict`` of a model with ``truncation_data``, the f64 restatement against the upstream-style composition, and the argument
validation of ``anemoi_csr_project``."""

import ctypes

import numpy as np
import pytest
import torch

import _truncation_ref as tr


def _random_dense(rng, rows, cols, density=0.2):
    d = (rng.random((rows, cols)) < density) * rng.standard_normal((rows, cols))
    d[rows // 2] = 0.0      # an empty row
    d[:, cols // 3] = 0.0   # an empty column
    d[0] = 0.0
    d[:, cols - 1] = 0.0
    return d


def _csr_of(d):
    r, c = np.nonzero(d)
    indptr = np.zeros(d.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=d.shape[0]), out=indptr[1:])
    return indptr, c.astype(np.int32), d[r, c].astype(np.float32)


@pytest.mark.parametrize("rows,cols,seed", [(5, 9, 0), (40, 17, 1), (1, 6, 2), (33, 33, 3), (7, 1, 4)])
def test_csr_transpose_vs_dense_and_keeps_source_row_order(rows, cols, seed):
    from anemoi_models_amd import ops

    d = _random_dense(np.random.default_rng(seed), rows, cols) if min(rows, cols) > 1 else np.random.default_rng(seed).standard_normal((rows, cols))
    indptr, idx, val = _csr_of(d)
    t_indptr, t_idx, t_val = ops.csr_transpose(torch.from_numpy(indptr), torch.from_numpy(idx), torch.from_numpy(val), cols)
    assert t_indptr.dtype == torch.int64 and t_idx.dtype == torch.int32 and t_indptr.numel() == cols + 1
    assert torch.equal(tr.dense(t_indptr, t_idx, t_val, rows), torch.from_numpy(d.astype(np.float32).T).double())
    for j in range(cols):  # ascending source rows within every transposed row
        seg = t_idx[t_indptr[j]:t_indptr[j + 1]]
        assert bool((seg[1:] > seg[:-1]).all())


def test_csr_transpose_is_stable_for_repeated_entries():
    from anemoi_models_amd import ops

    # row 0 holds column 2 twice (values 1, 2), row 1 once (3): the transposed row 2 keeps the order 1, 2, 3
    t = ops.csr_transpose(torch.tensor([0, 2, 3]), torch.tensor([2, 2, 2], dtype=torch.int32), torch.tensor([1.0, 2.0, 3.0]), 4)
    assert t[0].tolist() == [0, 0, 0, 3, 3] and t[1].tolist() == [0, 0, 1] and t[2].tolist() == [1.0, 2.0, 3.0]
    with pytest.raises(ValueError):
        ops.csr_transpose(torch.tensor([0, 1]), torch.tensor([4], dtype=torch.int32), torch.tensor([1.0]), 4)


def _save_like_scipy(path, fmt, d):
    r, c = np.nonzero(d)
    if fmt == "coo":
        np.savez(path, row=r.astype(np.int32), col=c.astype(np.int32), format=np.array(b"coo"), shape=np.array(d.shape), data=d[r, c])
        return
    m = d if fmt == "csr" else d.T
    indptr, idx, _ = _csr_of(m)
    rr, cc = np.nonzero(m)
    np.savez(path, indices=idx, indptr=indptr.astype(np.int32), format=np.array(fmt.encode()), shape=np.array(d.shape), data=m[rr, cc])


@pytest.mark.parametrize("fmt", ["csr", "csc", "coo"])
def test_npz_reader_with_numpy_only(tmp_path, fmt):
    from anemoi_models_amd.layers.truncation import canonical_csr

    d = _random_dense(np.random.default_rng(7), 12, 19)
    path = tmp_path / f"m_{fmt}.npz"
    _save_like_scipy(path, fmt, d)
    for p in (path, str(path)):
        m = canonical_csr(p, "down")
        assert m.shape == (12, 19) and m.idx.dtype == torch.int32 and m.val.dtype == torch.float32
        assert torch.equal(tr.dense(m.indptr, m.idx, m.val, 19), torch.from_numpy(d.astype(np.float32)).double())


@pytest.mark.parametrize("fmt", ["csr", "csc", "coo"])
def test_npz_reader_reads_scipy_files(tmp_path, fmt):
    sp = pytest.importorskip("scipy.sparse")
    from anemoi_models_amd.layers.truncation import canonical_csr

    d = _random_dense(np.random.default_rng(8), 12, 19)
    m_sp = getattr(sp, fmt + "_matrix")(d)
    sp.save_npz(tmp_path / "m.npz", m_sp)
    for src in (tmp_path / "m.npz", m_sp):  # the file and the matrix object itself (duck-typed through .tocsr())
        m = canonical_csr(src)
        assert torch.equal(tr.dense(m.indptr, m.idx, m.val, 19), torch.from_numpy(d.astype(np.float32)).double())


def test_canonicalisation_sums_duplicates_sorts_columns_and_checks_ranges():
    from anemoi_models_amd.layers.truncation import TruncationPlan, canonical_csr

    coo = torch.sparse_coo_tensor(torch.tensor([[1, 0, 1, 1, 0], [3, 2, 0, 3, 2]]), torch.tensor([1.0, 2.0, 3.0, 4.0, 0.5]), (3, 4))
    m = canonical_csr(coo)
    assert m.indptr.tolist() == [0, 1, 3, 3] and m.idx.tolist() == [2, 0, 3] and m.val.tolist() == [2.5, 3.0, 5.0]
    same = canonical_csr(coo.coalesce().to_sparse_csr())
    assert same.indptr.tolist() == m.indptr.tolist() and same.idx.tolist() == m.idx.tolist() and same.val.tolist() == m.val.tolist()
    # unsorted columns and a duplicate inside an (indptr, indices, values, shape) tuple
    tup = canonical_csr((torch.tensor([0, 3, 3]), torch.tensor([2, 0, 2]), torch.tensor([1.0, 2.0, 3.0]), (2, 3)))
    assert tup.indptr.tolist() == [0, 2, 2] and tup.idx.tolist() == [0, 2] and tup.val.tolist() == [2.0, 4.0]
    with pytest.raises(ValueError, match="out of range"):
        canonical_csr((torch.tensor([0, 1]), torch.tensor([3]), torch.tensor([1.0]), (1, 3)), "down")
    with pytest.raises(ValueError, match="out of range"):
        canonical_csr((torch.tensor([0, 1]), torch.tensor([-1]), torch.tensor([1.0]), (1, 3)), "down")
    down = (torch.tensor([0, 1, 2]), torch.tensor([0, 4]), torch.tensor([1.0, 1.0]), (2, 5))
    up = (torch.tensor([0, 1, 1, 2, 2, 2]), torch.tensor([0, 1]), torch.tensor([1.0, 1.0]), (5, 2))
    plan = TruncationPlan({"down": down, "up": up})
    assert plan and plan.grid_size == 5 and len(plan.stages) == 2
    assert not TruncationPlan(None) and not TruncationPlan({})
    with pytest.raises(ValueError, match=r"\(2, 5\).*\(2, 5\)|\(2, 5\)"):
        TruncationPlan({"down": down, "up": down})          # up does not take what down gives
    with pytest.raises(ValueError, match=r"\(2, 5\)"):
        TruncationPlan({"down": down})                      # one matrix alone must be G x G
    with pytest.raises(ValueError, match="G = 6"):
        TruncationPlan({"down": down, "up": up}, grid_size=6)
    square = (torch.tensor([0, 1, 2]), torch.tensor([1, 0]), torch.tensor([1.0, 1.0]), (2, 2))
    assert TruncationPlan({"up": square}).grid_size == 2 and TruncationPlan({"down": square}, grid_size=2)
    with pytest.raises(ValueError, match="unknown keys"):
        TruncationPlan({"dwn": square})


def _matrices(g, g_c, seed=0):
    rng = np.random.default_rng(seed)
    down = tr.random_csr(rng, g_c, g, rng.integers(0, 6, size=g_c), 0.5)
    up = tr.random_csr(rng, g, g_c, rng.integers(0, 4, size=g), 0.5)
    return (*down, (g_c, g)), (*up, (g, g_c))


def test_state_dict_is_that_of_the_model_without_truncation(graph_o32):
    from anemoi_models_amd.interface import AnemoiModelInterface  # noqa: F401  (importable with the new argument)
    from anemoi_models_amd.models import AnemoiModelEncProcDec
    from anemoi_models_amd.utils.indices import SimpleDataIndices
    from anemoi_models_amd.utils.presets import model_config

    idx = SimpleDataIndices(n_prognostic=10, n_forcing=2, n_diagnostic=1)
    g = graph_o32["data"].num_nodes
    down, up = _matrices(g, 50)
    kw = dict(model_config=model_config("GraphTransformer", 64, 2, 16), data_indices=idx, graph_data=graph_o32)
    plain = AnemoiModelEncProcDec(**kw)
    trunc = AnemoiModelEncProcDec(**kw, truncation_data={"down": down, "up": up})
    assert list(plain.state_dict()) == list(trunc.state_dict())
    assert {k: tuple(v.shape) for k, v in plain.state_dict().items()} == {k: tuple(v.shape) for k, v in trunc.state_dict().items()}
    assert trunc._truncation is not None and plain._truncation is None
    assert AnemoiModelEncProcDec(**kw, truncation_data={})._truncation is None
    with pytest.raises(TypeError):
        AnemoiModelEncProcDec(kw["model_config"], idx, graph_o32, {"down": down, "up": up})  # keyword-only, as upstream
    with pytest.raises(ValueError, match="must map"):
        AnemoiModelEncProcDec(**kw, truncation_data={"down": _matrices(g + 1, 50)[0], "up": _matrices(g + 1, 50)[1]})


def test_model_with_truncation_refuses_a_model_group_before_any_launch(graph_o32):
    from anemoi_models_amd.models import AnemoiModelEncProcDec
    from anemoi_models_amd.utils.indices import SimpleDataIndices
    from anemoi_models_amd.utils.presets import model_config

    class Group:
        def size(self):
            return 2

    idx = SimpleDataIndices(n_prognostic=10, n_forcing=2, n_diagnostic=1)
    g = graph_o32["data"].num_nodes
    down, up = _matrices(g, 50)
    model = AnemoiModelEncProcDec(model_config=model_config("GraphTransformer", 64, 2, 16), data_indices=idx, graph_data=graph_o32,
                                  truncation_data={"down": down, "up": up})
    x = torch.zeros(1, 2, 1, g, idx.num_input)
    for grad in (False, True):
        with torch.set_grad_enabled(grad), pytest.raises(NotImplementedError, match="single-device"):
            model(x, Group())


def test_restatement_equals_the_upstream_style_composition():
    """Projecting only the prognostic columns equals projecting every variable and selecting, to f64 rounding."""
    from anemoi_models_amd.layers.truncation import TruncationPlan

    g, g_c, v_in, v_out = 60, 13, 9, 7
    down, up = _matrices(g, g_c, seed=3)
    plan = TruncationPlan({"down": down, "up": up})
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(2, 2, 3, g, v_in, generator=gen, dtype=torch.float64)
    out = torch.randn(2, 3, g, v_out, generator=gen, dtype=torch.float64)
    out_idx, in_idx = torch.tensor([5, 0, 3, 2]), torch.tensor([1, 8, 4, 6])
    mats = [tr.dense(m.indptr, m.idx, m.val, m.shape[1]) for m in plan.stages]
    sparse = [m.to_sparse_coo(dtype=torch.float64) for m in plan.stages]
    got = tr.truncated_residual(out, x, mats, out_idx, in_idx)
    want = tr.upstream_style(out, x, sparse, out_idx, in_idx)
    assert float((got - want).abs().max()) <= 64 * 2.0 ** -53 * float(want.abs().max())
    untouched = [c for c in range(v_out) if c not in out_idx.tolist()]
    assert torch.equal(got[..., untouched], out[..., untouched])


def test_csr_project_argument_validation_without_gpu():
    """Status codes and messages come back through the ABI before anything is launched."""
    from anemoi_models_amd import _lib

    lib = _lib.load()
    bad, unsup = _lib.ANEMOI_ERR_INVALID, _lib.ANEMOI_ERR_UNSUPPORTED
    assert _lib.ABI_VERSION >= 52
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)  # never dereferenced: every call below is refused, or has nothing to do, before a launch

    def call(x=p, ldx=4, xso=0, xsi=0, out=p, ldo=4, oso=0, osi=0, n_outer=1, n_inner=1, n_in=2, n_out=2, indptr=p, idx=p,
             val=p, cols_in=None, cols_out=None, n_p=4, mul=None, add=None, acc=0):
        return lib.anemoi_csr_project(x, ldx, xso, xsi, out, ldo, oso, osi, n_outer, n_inner, n_in, n_out, indptr, idx, val,
                                      cols_in, cols_out, n_p, mul, add, acc, None)

    for missing in ("x", "out", "indptr", "idx", "val"):
        assert call(**{missing: None}) == bad and b"anemoi_csr_project: null pointer" in lib.anemoi_last_error()
    assert call(n_p=0) == bad and b"P = 0" in lib.anemoi_last_error()
    assert call(n_p=-3) == bad
    for name in ("n_outer", "n_inner", "n_in", "n_out"):
        assert call(**{name: -1}) == bad and b"negative size" in lib.anemoi_last_error()
    assert call(mul=p) == bad and b"come together" in lib.anemoi_last_error()
    assert call(acc=2) == bad
    assert call(ldx=3) == bad and b"row pitch" in lib.anemoi_last_error()      # identity columns need ldx >= P
    assert call(ldo=3) == bad
    assert call(ldx=-1, cols_in=p) == bad
    assert call(xso=-8) == bad and b"negative slab stride" in lib.anemoi_last_error()
    assert call(n_inner=3, osi=4) == bad and b"overlap" in lib.anemoi_last_error()  # slabs of 2 rows x 4 are 8 apart at least
    assert call(n_outer=2, n_inner=3, oso=16, osi=8) == bad and b"overlap" in lib.anemoi_last_error()
    assert call(n_outer=70000, oso=8) == unsup
    # nothing to do: no launch, OK
    assert call(n_out=0) == _lib.ANEMOI_OK and call(n_outer=0) == _lib.ANEMOI_OK
