from .attention import SimAM
from .block import CARAFE, ADown, Add, DySample, Fusion, GSBottleneck, GSConv, ScalSeq, SPDConv, VoVGSCSP, Zoom_cat

__all__ = ("ADown", "CARAFE", "Add", "DySample", "Fusion", "GSBottleneck", "GSConv", "ScalSeq", "SimAM", "SPDConv", "VoVGSCSP", "Zoom_cat")
