"""Generate ``tests/golden/interface_imputers*.npz`` from the REAL reference sources: ``AnemoiModelInterface.predict_step``
with a NaN imputer next to the ``InputNormalizer`` in ``config.data.processors``.

Run in the build container only (needs the reference checkout, see ``make_golden.py``)::

    python tests/golden/make_golden_interface_imputers.py            # writes the files
    python tests/golden/make_golden_interface_imputers.py --check    # regenerates in memory, compares with the files

Config 1 exactly as ``make_golden.golden_interface``: same seeds, weights, statistics and ``NORMALIZER_METHODS`` -- the
``sd.*`` and ``stat.*`` arrays are asserted to equal those of ``interface_gt.npz`` and are not stored again.  Per case a
fresh reference interface runs ``y1 = predict_step(batch1)`` (the first call fixes a static imputer's NaN map) and then
``y2 = predict_step(batch2)``.  ``batch1`` is ``interface_gt.npz``'s ``batch`` with NaNs at the case's stored boolean map (both
time steps); ``batch2`` is stored once and shared.  Only data is written: the maps, ``batch2`` and ``y1`` / ``y2`` per case.

Files (each below the size limit of a committed file): ``interface_imputers.npz`` holds the maps and ``batch2``,
``interface_imputers_case<N>.npz`` holds ``y1`` / ``y2`` of case N.  ``load()`` merges them into one dictionary with the keys
``batch2``, ``case<N>.map``, ``case<N>.y1``, ``case<N>.y2``.
"""

from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

MAIN = "interface_imputers.npz"
IMPUTER = "anemoi.models.preprocessing.imputer."
NORMALIZER = "anemoi.models.preprocessing.normalizer.InputNormalizer"
CASES = {  # case -> (processors in order, bounding list or None); the normaliser's config is make_golden.NORMALIZER_METHODS
    1: ([("imputer", IMPUTER + "InputImputer", {"default": "none", "mean": ["prog_2"], "minimum": ["forc_1"]}),
         ("normalizer", NORMALIZER, None)], None),
    2: ([("normalizer", NORMALIZER, None),
         ("imputer", IMPUTER + "ConstantImputer", {"default": "none", 0: ["prog_2"], 3.0: ["prog_5"]})], None),
    3: ([("imputer", IMPUTER + "DynamicInputImputer", {"default": "none", "mean": ["prog_2"], "maximum": ["forc_1"]}),
         ("normalizer", NORMALIZER, None)], None),
    4: ([("imputer", IMPUTER + "InputImputer", {"default": "none", "mean": ["prog_2"], "minimum": ["forc_1"]}),
         ("normalizer", NORMALIZER, None)],
        [{"_target_": "anemoi.models.layers.bounding.HardtanhBounding", "variables": ["prog_2"], "min_val": 0.0, "max_val": 1.0},
         {"_target_": "anemoi.models.layers.bounding.FractionBounding", "variables": ["prog_3"], "min_val": 0.0,
          "max_val": 1.0, "total_var": "prog_2"}]),
}
NAMES = [f"prog_{i}" for i in range(10)] + [f"forc_{i}" for i in range(2)] + ["diag_0"]
INPUT_NAMES = NAMES[:12]  # the inference input layout of config 1: prognostic, then forcing


def case_file(case: int) -> str:
    return f"interface_imputers_case{case}.npz"


def load(golden_dir: str = HERE) -> dict:
    """Every array of the fixture as torch tensors (the tests' entry point; needs no reference)."""
    out = {}
    for name in [MAIN] + [case_file(c) for c in CASES]:
        with np.load(os.path.join(golden_dir, name)) as z:
            out.update({k: torch.from_numpy(z[k]) for k in z.files})
    return out


def imputed_columns(case: int) -> list:
    cfg = next(c for _, target, c in CASES[case][0] if target.startswith(IMPUTER))
    return sorted(INPUT_NAMES.index(v) for k, vs in cfg.items() if k != "default" for v in vs)


def nan_inputs(batch: torch.Tensor) -> dict:
    """The stored maps and ``batch2``.  One pattern per input column that some case imputes (about 30 % of the grid, grid point
    3 in every one of them); a case's map holds the patterns of ITS imputed columns.  ``batch2`` is ``batch`` with its grid rows
    rolled by one, NaN in prog_2 -- imputed by every case -- at one random half of that column's pattern on the first time
    step and at another half on the second: inside every static map (other mapped points hold finite values that must be
    overwritten, nothing is NaN outside a map) and a pattern the dynamic case has not seen in ``batch1``."""
    gen = torch.Generator().manual_seed(31)
    grid, n_in = batch.shape[-2], batch.shape[-1]
    pattern = torch.rand((grid, n_in), generator=gen) < 0.3
    pattern[3, :] = True
    pattern[5, :] = False  # ... and one that is NaN in none
    out = {}
    for case in CASES:
        m = torch.zeros((grid, n_in), dtype=torch.bool)
        cols = imputed_columns(case)
        m[:, cols] = pattern[:, cols]
        out[f"case{case}.map"] = m
    batch2 = batch.roll(1, dims=-2).clone()
    col = INPUT_NAMES.index("prog_2")
    for t in range(batch2.shape[1]):
        half = pattern[:, col] & (torch.rand(grid, generator=gen) < 0.5)
        batch2[:, t, half, col] = float("nan")
    out["batch2"] = batch2
    return out


def generate() -> dict:
    import warnings

    import make_golden as mg  # installs the stand-ins and imports the real reference
    from _ref_stubs import DotDict

    g = mg.build_graph("o32_ico2")
    with np.load(os.path.join(HERE, "interface_gt.npz")) as z:
        gt = {k: z[k] for k in z.files}
    batch = torch.from_numpy(gt["batch"])
    out = nan_inputs(batch)
    for case, (processors, bounding) in CASES.items():
        cfg = mg.model_config("GraphTransformer", 64, 4, 16)
        cfg["data"] = {
            "forcing": ["forc_0", "forc_1"], "diagnostic": ["diag_0"],
            "processors": {name: {"_target_": target, "config": dict(mg.NORMALIZER_METHODS) if c is None else dict(c)}
                           for name, target, c in processors},
        }
        cfg["model"]["model"] = {"_target_": "anemoi.models.models.encoder_processor_decoder.AnemoiModelEncProcDec"}
        if bounding is not None:
            cfg["model"]["bounding"] = [dict(b) for b in bounding]
        cfg = DotDict(cfg)
        indices = mg.IndexCollection(cfg, {n: i for i, n in enumerate(NAMES)})
        # the f32 statistics of interface_gt.npz as f64 arrays (same values): the reference imputer assigns statistics[...][i]
        # to a tensor element, which torch refuses for a numpy.float32 scalar; the normaliser's buffers are asserted below to
        # come out bit-identical to those built from the f32 arrays
        statistics = {k: gt["stat." + k].astype(np.float64) for k in ("mean", "stdev", "minimum", "maximum")}
        torch.manual_seed(1234)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            iface = mg.AnemoiModelInterface(config=cfg, graph_data=mg.to_ref_graph(g), statistics=statistics,
                                            data_indices=indices, metadata={})
        mg.randomise(iface.model, 4321)
        iface.eval()
        sd = iface.state_dict()
        assert sorted("sd." + k for k in sd) == sorted(k for k in gt if k.startswith("sd.")), "state_dict keys differ"
        for k, v in sd.items():
            assert np.array_equal(gt["sd." + k], v.numpy()), k
        assert len(iface.model.boundings) == (0 if bounding is None else len(bounding))
        batch1 = batch.clone()
        batch1[:, :, out[f"case{case}.map"]] = float("nan")
        with torch.no_grad():
            y1 = iface.predict_step(batch1)
            y2 = iface.predict_step(out["batch2"])
        out[f"case{case}.y1"], out[f"case{case}.y2"] = y1, y2
        print(f"case {case}: NaN in batch1 {int(torch.isnan(batch1).sum())}, in y1 {int(torch.isnan(y1).sum())}, in batch2 "
              f"{int(torch.isnan(out['batch2']).sum())}, in y2 {int(torch.isnan(y2).sum())}, |y2|max "
              f"{float(y2[~torch.isnan(y2)].abs().max()):.3f}")
    return {k: v.numpy() for k, v in out.items()}


if __name__ == "__main__":
    arrays = generate()
    if "--check" in sys.argv:
        have = {k: v.numpy() for k, v in load().items()}
        assert sorted(have) == sorted(arrays), (sorted(have), sorted(arrays))
        for k, v in arrays.items():
            assert have[k].dtype == v.dtype and np.array_equal(have[k], v, equal_nan=v.dtype.kind == "f"), k
        print("the committed fixture regenerates bit-identically:", len(arrays), "arrays")
        sys.exit(0)
    np.savez_compressed(os.path.join(HERE, MAIN), **{k: v for k, v in arrays.items() if k == "batch2" or k.endswith(".map")})
    for c in CASES:
        np.savez_compressed(os.path.join(HERE, case_file(c)), **{k: v for k, v in arrays.items()
                                                                 if k in (f"case{c}.y1", f"case{c}.y2")})
    sizes = {n: os.path.getsize(os.path.join(HERE, n)) for n in [MAIN] + [case_file(c) for c in CASES]}
    print(sizes, "total", sum(sizes.values()), "interface_gt.npz", os.path.getsize(os.path.join(HERE, "interface_gt.npz")))
    assert max(sizes.values()) < (1 << 20) and sum(sizes.values()) < os.path.getsize(os.path.join(HERE, "interface_gt.npz"))
