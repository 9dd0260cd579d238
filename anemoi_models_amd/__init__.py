def __getattr__(name):
    if name == "trail":  # anemoi_models_amd.trail: the launch trail (per-launch output digests), imported on first use
        import importlib

        return importlib.import_module(".trail", __name__)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
