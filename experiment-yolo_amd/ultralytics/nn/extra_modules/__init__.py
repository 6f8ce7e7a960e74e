from .block import CARAFE, ADown, Add, DySample, ScalSeq, SPDConv, Zoom_cat

__all__ = ("ADown", "CARAFE", "Add", "DySample", "ScalSeq", "SPDConv", "Zoom_cat")
