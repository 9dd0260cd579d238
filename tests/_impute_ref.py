"""NaN imputation inside the I/O kernels, restated in plain torch straight from the contracts of include/anemoi_amd.h
(anemoi_assemble_nodes_imputed / anemoi_finalize_output_imputed / anemoi_bound_output_imputed), plus stand-ins for the extended
``ops`` functions (installed on top of ``_cpu_ops.install``) and the interface builder the CPU and the GPU tests share.  The
package never imports this file."""

from __future__ import annotations

import os
import sys
import warnings

import torch

import _cpu_ops
from conftest import GOLDEN
from conftest import split_prefix

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import make_golden_interface_imputers as fixture  # noqa: E402  (CASES, load(); imports the reference only to generate)

NAN = float("nan")


# ------------------------------------------------------------------------------------------------ the three contracts
def select(x, fill_val, fill_src, nan_map, in_affine=None):
    """``x [..., G, V]`` -> ``pick ? fill_val[v] : (affine ? raw * mul[v] + add[v] : raw)`` with
    ``pick = fill_src[v] >= 0 && (nan_map ? nan_map[g, fill_src[v]] : isnan(raw))``; the map row serves every leading index."""
    src = fill_src.long()
    has = src >= 0
    if nan_map is not None:
        pick = (nan_map.bool()[:, src.clamp_min(0)] & has).expand(x.shape)
    else:
        pick = torch.isnan(x) & has
    val = x if in_affine is None else torch.addcmul(in_affine[1].float(), x, in_affine[0].float())
    return torch.where(pick, fill_val.to(val.dtype), val)


def restore(y, nan_map, nan_src, cols=None):
    """``y [..., G, C]``: NaN where ``nan_map[g, nan_src[j]]`` is set, ``j`` over ``cols`` (default: every column)."""
    if nan_map is None or nan_src is None:
        return y
    src = nan_src.long()
    mask = nan_map.bool()[:, src.clamp_min(0)] & (src >= 0)
    if cols is None:
        return torch.where(mask.expand(y.shape), torch.full_like(y, NAN), y)
    y = y.clone()
    y[..., cols.long()] = torch.where(mask.expand(y[..., cols.long()].shape), torch.full_like(y[..., cols.long()], NAN),
                                      y[..., cols.long()])
    return y


def assemble_nodes(x, latlons, trainable, batch_size, dtype, ld_out=None, ensemble=1, in_affine=None, rows=None, impute=None):
    if impute is None:
        return _cpu_ops.assemble_nodes(x, latlons, trainable, batch_size, dtype, ld_out, ensemble, in_affine, rows)
    if rows is not None:
        raise ValueError("assemble_nodes: the row-list kernel takes no imputation (rows= with impute=)")
    x = select(x.float(), impute.fill_val, impute.fill_src, impute.nan_map, in_affine)
    b, t, ens, g, v = x.shape  # rows (b, ens, g); the node attributes repeat per batch entry AND member
    parts = [x.permute(0, 2, 3, 1, 4).reshape(b * ens * g, t * v), latlons.float().repeat(b * ens, 1)]
    if trainable is not None:
        parts.append(trainable.detach().float().repeat(b * ens, 1))
    out = torch.cat(parts, dim=1)
    return torch.nn.functional.pad(out, (0, (out.shape[1] if ld_out is None else ld_out) - out.shape[1])).to(dtype)


def finalize_output(y, x, src, in_affine=None, out_affine=None, rows=None, impute=None):
    if impute is None:
        return _cpu_ops.finalize_output(y, x, src, in_affine, out_affine, rows)
    if rows is not None:
        raise ValueError("finalize_output: the row-list kernel takes no imputation (rows= with impute=)")
    last = select(x[:, -1:].float(), impute.fill_val, impute.fill_src, impute.nan_map, in_affine)
    _cpu_ops.finalize_output(y, last, src, None, out_affine)
    y.copy_(restore(y, impute.nan_map, impute.out_nan_src))
    return y


def bound_output(y, op_col, op_lo, op_hi, op_mul, fin=None, impute=None):
    _cpu_ops.bound_output(y, op_col, op_lo, op_hi, op_mul, fin)
    if impute is not None and fin is not None:
        y.copy_(restore(y, impute.nan_map, impute.out_nan_src, fin[0]))
    return y


def install(monkeypatch):
    import anemoi_models_amd.ops as ops

    _cpu_ops.install(monkeypatch)
    for name in ("assemble_nodes", "finalize_output", "bound_output"):
        monkeypatch.setattr(ops, name, globals()[name])


# ------------------------------------------------------------------------------------------------ shared builders
def build_case_interface(graph, gold, case, model_target="anemoi.models.models.encoder_processor_decoder.AnemoiModelEncProcDec",
                         processors=None, **model_kw):
    """The interface of ``tests/golden/make_golden_interface_imputers.py`` case ``case`` on config 1 (``gold``:
    interface_gt.npz, whose statistics and weights the fixture shares); ``processors`` overrides the case's list."""
    from test_host_logic import NORMALIZER_METHODS

    from anemoi_models_amd.interface import AnemoiModelInterface
    from anemoi_models_amd.utils.indices import SimpleDataIndices
    from anemoi_models_amd.utils.presets import model_config

    procs, bounding = fixture.CASES[case]
    cfg = model_config("GraphTransformer", 64, 4, 16) if "config" not in model_kw else model_kw.pop("config")
    cfg["data"] = {"forcing": ["forc_0", "forc_1"], "diagnostic": ["diag_0"],
                   "processors": {name: {"_target_": target, "config": dict(NORMALIZER_METHODS) if c is None else dict(c)}
                                  for name, target, c in (processors or procs)}}
    cfg["model"]["model"] = {"_target_": model_target}
    if bounding is not None:
        cfg["model"]["bounding"] = [dict(b) for b in bounding]
    cfg = type(cfg)(cfg)
    stats = {k: v.numpy() for k, v in split_prefix(gold, "stat.").items()}
    idx = SimpleDataIndices(n_prognostic=10, n_forcing=2, n_diagnostic=1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (the dynamic imputers warn when they are built)
        return AnemoiModelInterface(config=cfg, graph_data=graph, statistics=stats, data_indices=idx, metadata={}, **model_kw)


def batch1_of(gold, fix, case):
    b = gold["batch"].clone()
    b[:, :, fix[f"case{case}.map"]] = NAN
    return b


def assert_matches(got, want, check_finite):
    """NaN maps identical; ``check_finite(got, want)`` on copies whose NaN entries are zeroed."""
    got = got.detach().cpu()
    assert got.shape == want.shape
    assert torch.equal(torch.isnan(got), torch.isnan(want)), (int(torch.isnan(got).sum()), int(torch.isnan(want).sum()))
    check_finite(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(want, nan=0.0))


assert os.path.isdir(GOLDEN)
