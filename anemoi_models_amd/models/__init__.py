from .encoder_processor_decoder import AnemoiModelEncProcDec
from .ensemble import AnemoiEnsModelEncProcDec
from .hierarchical import AnemoiModelEncProcDecHierarchical

__all__ = ["AnemoiModelEncProcDec", "AnemoiEnsModelEncProcDec", "AnemoiModelEncProcDecHierarchical"]
