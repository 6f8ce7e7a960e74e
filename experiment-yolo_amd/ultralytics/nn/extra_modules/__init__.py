from .block import CARAFE, Add, DySample, ScalSeq, SPDConv, Zoom_cat

__all__ = ("CARAFE", "Add", "DySample", "ScalSeq", "SPDConv", "Zoom_cat")
