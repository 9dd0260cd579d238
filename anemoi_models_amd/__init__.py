_LOSSES = ("WeightedMSELoss", "WeightedMAELoss", "WeightedHuberLoss", "WeightedLogCoshLoss", "WeightedRMSELoss",
           "ValidationMetrics", "AlmostFairKernelCRPS", "KernelCRPS", "EnsembleMetrics")
__all__ = list(_LOSSES)


def __getattr__(name):
    import importlib

    if name == "trail":  # anemoi_models_amd.trail: the launch trail (per-launch output digests), imported on first use
        return importlib.import_module(".trail", __name__)
    if name in _LOSSES:  # anemoi_models_amd.losses: the training losses and validation metrics, imported on first use
        return getattr(importlib.import_module(".losses", __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
