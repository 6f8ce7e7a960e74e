from .block import Add, DySample, ScalSeq, SPDConv, Zoom_cat

__all__ = ("Add", "DySample", "ScalSeq", "SPDConv", "Zoom_cat")
