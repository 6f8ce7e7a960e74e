from .block import CARAFE, ADown, Add, DySample, Fusion, GSBottleneck, GSConv, ScalSeq, SPDConv, VoVGSCSP, Zoom_cat

__all__ = ("ADown", "CARAFE", "Add", "DySample", "Fusion", "GSBottleneck", "GSConv", "ScalSeq", "SPDConv", "VoVGSCSP", "Zoom_cat")
