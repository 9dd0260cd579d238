"""Generate ``tests/golden/remappers*.npz`` and ``remappers_indices.json`` from the REAL reference sources: the ``Remapper``
pre/post-processors (``Monomapper``, ``Multimapper``) alone and next to the ``InputNormalizer`` in
``AnemoiModelInterface.predict_step``, and ``IndexCollection`` with ``config.data.remapped``.

Run in the build container only (needs the reference checkout, see ``make_golden.py``)::

    python tests/golden/make_golden_remappers.py            # writes the files
    python tests/golden/make_golden_remappers.py --check    # regenerates in memory, compares with the files

Config 1 as ``make_golden.golden_interface``: same graph, seeds, statistics and, wherever the shape allows, weights -- every
state-dict tensor whose shape equals that of ``interface_gt.npz`` is asserted (mono cases) or set (multi cases) equal to it and
not stored again; the multi cases widen the two input embeddings and the output head, whose four tensors are stored once
(``sd_multi.*``).  ``batch`` is ``interface_gt.npz``'s ``batch`` with the two direction columns (prog_7, forc_1) replaced by the
stored ``directions``, uniform in [0, 360), and the three columns of the mono case (prog_2, forc_0, prog_8) by their
magnitudes; ``batch2`` is ``batch`` rolled by one grid row.  Neither is stored: ``load()`` rebuilds them.  Per case a fresh
reference interface runs ``y1 = predict_step(batch)`` and ``y2 = predict_step(batch2)``.

Only data is written.  ``remappers.npz``: ``directions``, ``sd_multi.*``, and per case the module vectors
``case<N>.<transform|inverse>.<training|inference>.<x|y>`` (the processor alone on small random tensors) plus ``lossmask.x`` /
``lossmask.y`` (``Multimapper.transform_loss_mask`` with prog_7 alone remapped).  ``remappers_case<N>.npz``: ``y1`` / ``y2``.
``remappers_indices.json``: the four views of the multi cases' ``IndexCollection`` (names and index lists) and the error a
``Multimapper`` in front of the normaliser ends in.  ``load()`` merges the arrays into one dictionary.
"""

from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

MAIN = "remappers.npz"
INDICES = "remappers_indices.json"
REMAPPER = "anemoi.models.preprocessing.remapper.Remapper"
NORMALIZER = "anemoi.models.preprocessing.normalizer.InputNormalizer"
NAMES = [f"prog_{i}" for i in range(10)] + [f"forc_{i}" for i in range(2)] + ["diag_0"]
INPUT_NAMES = NAMES[:12]
DIRECTIONS = ["prog_7", "forc_1"]
NON_NEGATIVE = ["prog_2", "forc_0", "prog_8"]
REMAPPED = {"prog_7": ["cos_p7", "sin_p7"], "forc_1": ["cos_f1", "sin_f1"]}
COS_SIN = {"default": "none", "cos_sin": {k: list(v) for k, v in REMAPPED.items()}}
MONO = {"default": "none", "log1p": ["prog_2"], "sqrt": ["forc_0"], "boxcox": ["prog_8"]}
BOUNDING = [
    {"_target_": "anemoi.models.layers.bounding.ReluBounding", "variables": ["prog_0", "diag_0"]},
    {"_target_": "anemoi.models.layers.bounding.HardtanhBounding", "variables": ["cos_p7", "sin_p7"], "min_val": -1.0,
     "max_val": 1.0},
]
# case -> (processors in order as (name, target, config), config.data.remapped, bounding list); "normalizer" stands for
# normalizer_config(case)
CASES = {
    1: ([("normalizer", NORMALIZER, None), ("remapper", REMAPPER, COS_SIN)], REMAPPED, None),
    2: ([("remapper", REMAPPER, MONO), ("normalizer", NORMALIZER, None)], None, None),
    3: ([("normalizer", NORMALIZER, None), ("remapper", REMAPPER, {"default": "none", "log1p": ["prog_3"]})], None, None),
    4: ([("normalizer", NORMALIZER, None), ("remapper", REMAPPER, COS_SIN)], REMAPPED, BOUNDING),
}
MULTI_FIRST = [("remapper", REMAPPER, COS_SIN), ("normalizer", NORMALIZER, None)]  # fails in the reference normaliser


def normalizer_config(remapped) -> dict:
    """``make_golden.NORMALIZER_METHODS``; the directions of a cos_sin case are not normalised."""
    methods = {"default": "mean-std", "min-max": ["prog_3"], "max": ["prog_4"], "std": ["prog_5"], "none": ["forc_0"],
               "remap": {"prog_7": "prog_6"}}
    if remapped:
        methods["none"] = ["forc_0"] + list(remapped)
    return methods


def case_file(case: int) -> str:
    return f"remappers_case{case}.npz"


def batches(gt_batch: torch.Tensor, directions: torch.Tensor):
    batch = gt_batch.clone()
    for k, name in enumerate(DIRECTIONS):
        batch[..., INPUT_NAMES.index(name)] = directions[..., k]
    for name in NON_NEGATIVE:
        batch[..., INPUT_NAMES.index(name)] = batch[..., INPUT_NAMES.index(name)].abs()
    return batch, batch.roll(1, dims=-2).clone()


def load(golden_dir: str = HERE) -> dict:
    """Every array of the fixture as torch tensors, ``batch`` / ``batch2`` rebuilt, and ``indices`` = the JSON document
    (the tests' entry point; needs no reference)."""
    out = {}
    for name in [MAIN] + [case_file(c) for c in CASES]:
        with np.load(os.path.join(golden_dir, name)) as z:
            out.update({k: torch.from_numpy(z[k]) for k in z.files})
    with np.load(os.path.join(golden_dir, "interface_gt.npz")) as z:
        out["batch"], out["batch2"] = batches(torch.from_numpy(z["batch"]), out["directions"])
    with open(os.path.join(golden_dir, INDICES)) as f:
        out["indices"] = json.load(f)
    return out


def data_config(processors, remapped) -> dict:
    cfg = {"forcing": ["forc_0", "forc_1"], "diagnostic": ["diag_0"],
           "processors": {name: {"_target_": target, "config": normalizer_config(remapped) if c is None else c}
                          for name, target, c in processors}}
    if remapped:
        cfg["remapped"] = {k: list(v) for k, v in remapped.items()}
    return cfg


def views(indices) -> dict:
    doc = {}
    for view in ("data", "internal_data", "model", "internal_model"):
        for side in ("input", "output"):
            idx = getattr(getattr(indices, view), side)
            doc[f"{view}.{side}"] = {"name_to_index": dict(idx.name_to_index),
                                     **{k: getattr(idx, k).tolist() for k in ("full", "prognostic", "diagnostic", "forcing")}}
    return doc


def generate():
    import warnings

    import make_golden as mg  # installs the stand-ins and imports the real reference
    from _ref_stubs import DotDict
    from anemoi.models.preprocessing.remapper import Remapper

    g = mg.build_graph("o32_ico2")
    with np.load(os.path.join(HERE, "interface_gt.npz")) as z:
        gt = {k: z[k] for k in z.files}
    gt_batch = torch.from_numpy(gt["batch"])
    gen = torch.Generator().manual_seed(53)
    out = {"directions": torch.rand(gt_batch.shape[:-1] + (len(DIRECTIONS),), generator=gen) * 360.0}
    batch, batch2 = batches(gt_batch, out["directions"])
    statistics = {k: gt["stat." + k].astype(np.float64) for k in ("mean", "stdev", "minimum", "maximum")}
    name_to_index = {n: i for i, n in enumerate(NAMES)}
    doc = {}

    def interface(processors, remapped, bounding):
        cfg = mg.model_config("GraphTransformer", 64, 4, 16)
        cfg["data"] = data_config(processors, remapped)
        cfg["model"]["model"] = {"_target_": "anemoi.models.models.encoder_processor_decoder.AnemoiModelEncProcDec"}
        if bounding is not None:
            cfg["model"]["bounding"] = [dict(b) for b in bounding]
        cfg = DotDict(cfg)
        indices = mg.IndexCollection(cfg, name_to_index)
        torch.manual_seed(1234)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            iface = mg.AnemoiModelInterface(config=cfg, graph_data=mg.to_ref_graph(g), statistics=statistics,
                                            data_indices=indices, metadata={})
        mg.randomise(iface.model, 4321)
        return iface.eval(), indices

    for case, (processors, remapped, bounding) in CASES.items():
        iface, indices = interface(processors, remapped, bounding)
        sd = iface.state_dict()
        assert sorted("sd." + k for k in sd) == sorted(k for k in gt if k.startswith("sd.")), "state_dict keys differ"
        widened = [k for k, v in sd.items() if tuple(v.shape) != gt["sd." + k].shape]
        if remapped:
            assert len(widened) == 4, widened
            iface.load_state_dict({k: torch.from_numpy(gt["sd." + k]) for k in sd if k not in widened}, strict=False)
            for k in widened:
                stored = out.setdefault("sd_multi." + k, sd[k].clone())
                assert torch.equal(stored, iface.state_dict()[k]), k
            doc.setdefault("views", views(indices))
        else:
            assert not widened, widened
        for k, v in iface.state_dict().items():
            assert k in widened or np.array_equal(gt["sd." + k], v.numpy()), k
        assert len(iface.model.boundings) == (0 if bounding is None else len(bounding))
        with torch.no_grad():
            y1 = iface.predict_step(batch)
            y2 = iface.predict_step(batch2)
        out[f"case{case}.y1"], out[f"case{case}.y2"] = y1, y2
        # the processor alone, on both layouts, fresh instance (a Multimapper never works in place)
        mapper = Remapper(config=DotDict(dict(next(c for _, t, c in processors if t == REMAPPER))), data_indices=indices,
                          statistics=statistics)
        multi = bool(remapped)
        widths = {"transform.training": len(indices.data.input.name_to_index),
                  "transform.inference": len(indices.model.input.name_to_index),
                  "inverse.training": len((indices.internal_data if multi else indices.data).output.name_to_index),
                  "inverse.inference": len((indices.internal_model if multi else indices.model).output.name_to_index)}
        for what, width in widths.items():
            x = torch.rand((2, 5, width), generator=gen)
            x = x * 360.0 if what.startswith("transform") else x * 2.0 - 1.0
            y = mapper.transform(x.clone(), in_place=False) if what.startswith("transform") else \
                mapper.inverse_transform(x.clone(), in_place=False)
            out[f"case{case}.{what}.x"], out[f"case{case}.{what}.y"] = x, y
        print(f"case {case}: y1 {tuple(y1.shape)} |y2|max {float(y2.abs().max()):.3f} NaN {int(torch.isnan(y2).sum())}")

    # transform_loss_mask: defined in the reference without a remapped forcing only
    one = {"prog_7": REMAPPED["prog_7"]}
    cfg = DotDict({"data": data_config([("remapper", REMAPPER, {"default": "none", "cos_sin": one})], one)})
    indices = mg.IndexCollection(cfg, name_to_index)
    mapper = Remapper(config=DotDict({"default": "none", "cos_sin": one}), data_indices=indices, statistics=statistics)
    out["lossmask.x"] = (torch.rand((7, len(indices.model.output.name_to_index)), generator=gen) < 0.5).float()
    out["lossmask.y"] = mapper.transform_loss_mask(out["lossmask.x"])
    doc["lossmask_views"] = views(indices)

    iface, _ = interface(MULTI_FIRST, REMAPPED, None)
    try:
        with torch.no_grad():
            iface.predict_step(batch)
        raise AssertionError("a Multimapper before the normaliser ran in the reference")
    except RuntimeError as e:
        doc["multimapper_first_error"] = type(e).__name__
    return {k: v.numpy() for k, v in out.items()}, doc


if __name__ == "__main__":
    arrays, document = generate()
    if "--check" in sys.argv:
        have = {k: v.numpy() for k, v in load().items() if k not in ("batch", "batch2", "indices")}
        assert sorted(have) == sorted(arrays), (sorted(have), sorted(arrays))
        for k, v in arrays.items():
            assert have[k].dtype == v.dtype and np.array_equal(have[k], v, equal_nan=v.dtype.kind == "f"), k
        assert load()["indices"] == json.loads(json.dumps(document))
        print("the committed fixture regenerates bit-identically:", len(arrays), "arrays")
        sys.exit(0)
    per_case = {c: (f"case{c}.y1", f"case{c}.y2") for c in CASES}
    in_case = {k for keys in per_case.values() for k in keys}
    np.savez_compressed(os.path.join(HERE, MAIN), **{k: v for k, v in arrays.items() if k not in in_case})
    for c, keys in per_case.items():
        np.savez_compressed(os.path.join(HERE, case_file(c)), **{k: arrays[k] for k in keys})
    with open(os.path.join(HERE, INDICES), "w") as f:
        json.dump(document, f, indent=1, sort_keys=True)
        f.write("\n")
    sizes = {n: os.path.getsize(os.path.join(HERE, n)) for n in [MAIN, INDICES] + [case_file(c) for c in CASES]}
    print(sizes, "total", sum(sizes.values()))
    assert max(sizes.values()) < (1 << 20)
