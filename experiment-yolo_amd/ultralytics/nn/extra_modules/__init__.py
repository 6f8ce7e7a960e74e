from .block import Add, ScalSeq, SPDConv, Zoom_cat

__all__ = ("Add", "ScalSeq", "SPDConv", "Zoom_cat")
