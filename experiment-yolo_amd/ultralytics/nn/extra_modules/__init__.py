from .block import CARAFE, ADown, Add, DySample, Fusion, ScalSeq, SPDConv, Zoom_cat

__all__ = ("ADown", "CARAFE", "Add", "DySample", "Fusion", "ScalSeq", "SPDConv", "Zoom_cat")
