__all__ = ["WeightedMSELoss"]


def __getattr__(name):
    import importlib

    if name == "trail":  # anemoi_models_amd.trail: the launch trail (per-launch output digests), imported on first use
        return importlib.import_module(".trail", __name__)
    if name == "WeightedMSELoss":  # anemoi_models_amd.losses: the rollout training loss, imported on first use
        return importlib.import_module(".losses", __name__).WeightedMSELoss
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
